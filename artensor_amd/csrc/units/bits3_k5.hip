// artn_k_bits3<5, *, *> (make dev)
#include "artn_launch_bits3.h"
hipError_t artn_launch_bits3_k5(ARTN_BITS3_ARGS) { return launch_bits3_k<5>(p, A, B1, B2, B3, C, st); }
