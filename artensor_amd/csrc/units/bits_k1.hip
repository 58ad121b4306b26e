// artn_k_bits<1, *>
#include "artn_launch_bits.h"
hipError_t artn_launch_bits_k1(ARTN_BITS_ARGS) { return launch_bits_k2<1>(p, A, B1, B2, C, st); }
