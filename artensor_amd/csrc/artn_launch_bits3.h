// artn_launch_bits3.h -- launcher of the three-step kernel (units/bits3_k*.hip; development builds only).
#pragma once
#include "artn_host.h"
#include "artn_kernels.hip"
#include "artn_bits3_kernel.h"

// fused triples (make_bits3): artn_k_bits3<KB1, KB2, KB3, M3>, 3..5 contracted bits per stage, fragments of at most 80 registers;
// M3 exactly when a stage contracts 5 bits
template <int KB1>
static hipError_t launch_bits3_k(const ArtnPlan &p, const float2 *A, const float2 *B1, const float2 *B2, const float2 *B3, float2 *C,
                                 hipStream_t st) {
  dim3 grid(p.info.grid), block(ARTN_WG_THREADS);
  const size_t lds = (size_t)p.info.lds_bytes;
  const int k2 = p.bits.st[1].k, k3 = p.bits.st[2].k;
#define ARTN_B3_GO(K2, K3)                                                                                \
  if (k2 == K2 && k3 == K3) {                                                                             \
    if constexpr ((1 << KB1) + (1 << K2) + (1 << K3) <= 80) {                                             \
      constexpr bool M3V = KB1 == 5 || K2 == 5 || K3 == 5;                                                \
      if ((p.bits.m3 != 0) != M3V) return hipErrorInvalidValue;                                           \
      if (p.bits.nt_loads) {                                                                              \
        auto kern = artn_k_bits3<KB1, K2, K3, M3V, true>;                                                 \
        if (hipError_t e = ensure_lds<artn_k_bits3<KB1, K2, K3, M3V, true>>(lds); e != hipSuccess) return e; \
        hipLaunchKernelGGL(kern, grid, block, lds, st, A, B1, B2, B3, C, p.bits);                         \
      } else {                                                                                            \
        auto kern = artn_k_bits3<KB1, K2, K3, M3V, false>;                                                \
        if (hipError_t e = ensure_lds<artn_k_bits3<KB1, K2, K3, M3V, false>>(lds); e != hipSuccess) return e; \
        hipLaunchKernelGGL(kern, grid, block, lds, st, A, B1, B2, B3, C, p.bits);                         \
      }                                                                                                   \
      return hipGetLastError();                                                                           \
    }                                                                                                     \
  }
  ARTN_B3_GO(3, 3) ARTN_B3_GO(3, 4) ARTN_B3_GO(3, 5)
  ARTN_B3_GO(4, 3) ARTN_B3_GO(4, 4) ARTN_B3_GO(4, 5)
  ARTN_B3_GO(5, 3) ARTN_B3_GO(5, 4) ARTN_B3_GO(5, 5)
#undef ARTN_B3_GO
  return hipErrorInvalidValue;
}
