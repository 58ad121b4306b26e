// artn_k_bits<6, *> and artn_k_alt<6, *>, second-stage counts 0..3
#include "artn_launch_bits.h"
hipError_t artn_launch_bits_k6h0(ARTN_BITS_ARGS) { return launch_bits_k2<6, 0>(p, A, B1, B2, C, st); }
