// artn_unity.hip -- the whole library as ONE translation unit (make single / stamps / phases / ablate / asan): the
// __device__ stamp and phase buffers of the diagnostic builds are shared by all kernels, and the sanitizer recipe stands in
// for exactly one device fat binary.  artn_api.hip comes first: it is the unit that asks artn_kernels.hip for both sections.
#include "artn_api.hip"
#include "units/bits_k1.hip"
#include "units/bits_k2.hip"
#include "units/bits_k3.hip"
#include "units/bits_k4.hip"
#include "units/bits_k5h0.hip"
#include "units/bits_k5h1.hip"
#include "units/bits_k6h0.hip"
#include "units/bits_k6h1.hip"
#include "units/b128.hip"
#include "units/b128a.hip"
#include "units/wide.hip"
#ifdef ARTN_DEV_BITS3
#include "units/bits3_k3.hip"
#include "units/bits3_k4.hip"
#include "units/bits3_k5.hip"
#endif
#include "artn_born.hip"
#include "artn_rdm.hip"
#include "artn_pauli.hip" // (artn_pauli_kernel.h, artn_pauli_apply_kernel.h, artn_pauli_evolve_kernel.h, artn_pauli_adjoint_kernel.h)
#include "artn_gates.hip" // (artn_gates_kernel.h, artn_gates_adjoint_kernel.h)
#include "artn_wgate.hip" // (artn_wgate_kernel.h)
#include "artn_mgate.hip" // (artn_mgate_kernel.h)
#include "artn_cgate.hip" // (artn_cgate_kernel.h)
#include "artn_krylov.hip" // (artn_krylov_kernel.h)
#include "artn_measure.hip" // (artn_measure_kernel.h)
#include "artn_channel.hip" // (artn_channel_kernel.h)
#include "artn_batch.hip" // (artn_batch_kernel.h)
#include "artn_cgate_batch.hip" // (artn_cgate_batch_kernel.h)
#include "artn_pauli_batch.hip" // (artn_pauli_batch_kernel.h)
#include "artn_sample_batch.hip" // (artn_sample_batch_kernel.h)
#include "artn_diag.hip" // (artn_diag_kernel.h)
#include "artn_bitperm.hip" // (artn_bitperm_kernel.h)
