// artn_launch_bits128.h -- launcher of the complex128 state-streaming kernel (units/b128.hip, units/b128a.hip).
#pragma once
#include "artn_host.h"
#include "artn_kernels.hip"
#include "artn_bits128_kernel.h"

// complex128 plans of make_bits: artn_k_bits128<KB1, KB2, ACC> (ACC: ArtnBitsPlan::accumulate: a translation unit each)
template <bool ACC>
static hipError_t launch_bits128_t(const ArtnPlan &p, const void *A, const void *B1, const void *B2, void *C, hipStream_t st) {
  dim3 grid(p.info.grid), block(ARTN_WG_THREADS);
  const size_t lds = (size_t)p.info.lds_bytes;
  const int k1 = p.bits.st[0].k, k2 = p.bits.n_stages == 2 ? p.bits.st[1].k : 0;
  const double2 *a = (const double2 *)A, *b1 = (const double2 *)B1, *b2 = (const double2 *)B2;
  double2 *c = (double2 *)C;
#define ARTN_B128_GO(K1, K2)                                                                        \
  {                                                                                                 \
    auto kern = artn_k_bits128<K1, K2, ACC>;                                                        \
    if (hipError_t e = ensure_lds<artn_k_bits128<K1, K2, ACC>>(lds); e != hipSuccess) return e;     \
    hipLaunchKernelGGL(kern, grid, block, lds, st, a, b1, b2, c, p.bits);                           \
    return hipGetLastError();                                                                       \
  }
#define ARTN_B128_K2(K1)                                                                            \
  case K1:                                                                                          \
    switch (k2) {                                                                                   \
      case 0: ARTN_B128_GO(K1, 0)                                                                   \
      case 1: ARTN_B128_GO(K1, 1)                                                                   \
      case 2: ARTN_B128_GO(K1, 2)                                                                   \
      case 3: ARTN_B128_GO(K1, 3)                                                                   \
      case 4: ARTN_B128_GO(K1, 4)                                                                   \
      case 5: ARTN_B128_GO(K1, 5)                                                                   \
      case 6: ARTN_B128_GO(K1, 6)                                                                   \
      default: return hipErrorInvalidValue;                                                         \
    }
  switch (k1) {
    ARTN_B128_K2(1)
    ARTN_B128_K2(2)
    ARTN_B128_K2(3)
    ARTN_B128_K2(4)
    ARTN_B128_K2(5)
    ARTN_B128_K2(6)
    default: return hipErrorInvalidValue;
  }
#undef ARTN_B128_K2
#undef ARTN_B128_GO
}
