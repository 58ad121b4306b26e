// artn_k_wide<*, *> (artn_wide_kernel.h, which artn_kernels.hip includes: artn_k_bits borrows its stage)
#include "artn_host.h"
#include "artn_kernels.hip"

// fused pairs of 2^12-element tiles (ArtnBitsPlan::wide8): artn_k_wide<KB1, KB2>, 3..6 contracted bits per stage
hipError_t artn_launch_wide(ARTN_VOID_ARGS) {
  dim3 grid(p.info.grid), block(ARTN_WIDE_THREADS);
  const size_t lds = (size_t)p.info.lds_bytes;
  const int k1 = p.bits.st[0].k, k2 = p.bits.st[1].k;
  const float2 *a = (const float2 *)A, *b1 = (const float2 *)B1, *b2 = (const float2 *)B2;
  float2 *c = (float2 *)C;
#define ARTN_WIDE_GO(K1, K2)                                                                        \
  if (k1 == K1 && k2 == K2) {                                                                       \
    auto kern = artn_k_wide<K1, K2>;                                                                \
    if (hipError_t e = ensure_lds<artn_k_wide<K1, K2>>(lds); e != hipSuccess) return e;             \
    hipLaunchKernelGGL(kern, grid, block, lds, st, a, b1, b2, c, p.bits);                           \
    return hipGetLastError();                                                                       \
  }
#define ARTN_WIDE_ROW(K1) ARTN_WIDE_GO(K1, 3) ARTN_WIDE_GO(K1, 4) ARTN_WIDE_GO(K1, 5) ARTN_WIDE_GO(K1, 6)
  ARTN_WIDE_ROW(3) ARTN_WIDE_ROW(4) ARTN_WIDE_ROW(5) ARTN_WIDE_ROW(6)
#undef ARTN_WIDE_ROW
#undef ARTN_WIDE_GO
  return hipErrorInvalidValue;
}
