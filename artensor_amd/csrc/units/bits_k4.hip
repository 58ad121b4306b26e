// artn_k_bits<4, *> and artn_k_alt<4, *>
#include "artn_launch_bits.h"
hipError_t artn_launch_bits_k4(ARTN_BITS_ARGS) { return launch_bits_k2<4>(p, A, B1, B2, C, st); }
