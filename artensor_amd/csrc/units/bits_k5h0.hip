// artn_k_bits<5, *> and artn_k_alt<5, *>, second-stage counts 0..3
#include "artn_launch_bits.h"
hipError_t artn_launch_bits_k5h0(ARTN_BITS_ARGS) { return launch_bits_k2<5, 0>(p, A, B1, B2, C, st); }
