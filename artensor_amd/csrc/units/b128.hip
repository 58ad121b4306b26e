// artn_k_bits128<*, *, false>
#include "artn_launch_bits128.h"
hipError_t artn_launch_bits128(ARTN_VOID_ARGS) { return launch_bits128_t<false>(p, A, B1, B2, C, st); }
