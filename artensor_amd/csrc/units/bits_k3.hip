// artn_k_bits<3, *> and artn_k_alt<3, *>
#include "artn_launch_bits.h"
hipError_t artn_launch_bits_k3(ARTN_BITS_ARGS) { return launch_bits_k2<3>(p, A, B1, B2, C, st); }
