// artn_k_bits128<*, *, true>: the accumulating instantiations (ArtnBitsPlan::accumulate)
#include "artn_launch_bits128.h"
hipError_t artn_launch_bits128_acc(ARTN_VOID_ARGS) { return launch_bits128_t<true>(p, A, B1, B2, C, st); }
