// artn_launch_bits.h -- launcher of the complex64 state-streaming kernels artn_k_bits / artn_k_alt (artn_kernels.hip).
// launch_bits_k2<KB1, HALF> instantiates every kernel of the family with KB1 first-stage contracted bits that the planner
// can select; the units/bits_k*.hip sources wrap one instantiation each in an exported artn_launch_bits_*().
#pragma once
#include "artn_host.h"
#include "artn_kernels.hip"

// (HALF = 0 / 1: only the second-stage counts 0..3 / 4..6 of the family, everything else answers hipErrorInvalidValue -- the
//  families of 5 and 6 contracted bits took a minute each to compile and were the long pole of `make -j8`; -1: all of it)
template <int KB1, int HALF = -1>
static hipError_t launch_bits_k2(const ArtnPlan &p, const float2 *A, const float2 *B1, const float2 *B2, float2 *C,
                                 hipStream_t st) {
  dim3 grid(p.info.grid), block(ARTN_WG_THREADS);
  const size_t lds = (size_t)p.info.lds_bytes;
  const int k2 = p.bits.n_stages == 2 ? p.bits.st[1].k : 0;
  const int split = p.bits.split;
  const bool full = p.bits.T_in == 12 && p.bits.T_out == 12; // (the FULL instantiations)
  constexpr bool LO = HALF != 1, HI = HALF != 0;
#define ARTN_K2_HERE(K2) ((K2) >= 4 ? HI : LO)
#define ARTN_LAUNCH_NP(K2, NPV)                                                                           \
  {                                                                                                       \
    auto kern = artn_k_bits<KB1, K2, false, NPV>;                                                         \
    if (hipError_t e = ensure_lds<artn_k_bits<KB1, K2, false, NPV>>(lds); e != hipSuccess) return e;      \
    hipLaunchKernelGGL(kern, grid, block, lds, st, A, B1, B2, C, p.bits);                                 \
  }
  // split-bf16 instantiations exist only where a stage has the >= 3 contracted bits they need -- and only in development
  // builds (-DARTN_DEV_SPLIT3): fp32-grade results from three bfloat16 pieces, parity-green, no faster on any workload
  // (DESIGN.md 4.1); the product never plans split = 3
#ifdef ARTN_DEV_SPLIT3
#define ARTN_SPLIT3_CASE(K2) if (split == 3) { ARTN_LAUNCH_NP(K2, 3) break; }
#else
#define ARTN_SPLIT3_CASE(K2) if (split == 3) return hipErrorInvalidValue;
#endif
#define ARTN_LAUNCH(K2)                                                                                   \
  case K2: if constexpr (!ARTN_K2_HERE(K2)) return hipErrorInvalidValue; else {                           \
    if constexpr (KB1 >= 3 || K2 >= 3) {                                                                  \
      ARTN_SPLIT3_CASE(K2)                                                                                \
      if constexpr (KB1 >= 3 && (K2 == 0 || K2 >= 3)) {                                                   \
        if (split == 1 && p.bits.nt_loads) { /* bf16 operands: every big launch is HBM-bound */           \
          auto kern = artn_k_bits<KB1, K2, false, 1, false, true>;                                        \
          if (hipError_t e = ensure_lds<artn_k_bits<KB1, K2, false, 1, false, true>>(lds); e != hipSuccess) return e; \
          hipLaunchKernelGGL(kern, grid, block, lds, st, A, B1, B2, C, p.bits);                           \
          break;                                                                                          \
        }                                                                                                 \
      }                                                                                                   \
      if (split == 1) { ARTN_LAUNCH_NP(K2, 1) break; }                                                    \
    }                                                                                                     \
    if constexpr ((KB1 == 5 || KB1 == 6 || K2 == 5 || K2 == 6) && !((KB1 >= 5 && K2 >= 5) && KB1 + K2 > 11)) {      \
      if (p.bits.m3 && p.bits.nt_loads && full) { /* three real products per complex product in the 5-bit stages */ \
        auto kern = artn_k_bits<KB1, K2, false, 0, false, true, true, true>;                              \
        if (hipError_t e = ensure_lds<artn_k_bits<KB1, K2, false, 0, false, true, true, true>>(lds); e != hipSuccess) return e; \
        hipLaunchKernelGGL(kern, grid, block, lds, st, A, B1, B2, C, p.bits);                             \
        break;                                                                                            \
      }                                                                                                   \
      if (p.bits.m3 && full) {                                                                            \
        auto kern = artn_k_bits<KB1, K2, false, 0, false, false, true, true>;                             \
        if (hipError_t e = ensure_lds<artn_k_bits<KB1, K2, false, 0, false, false, true, true>>(lds); e != hipSuccess) return e; \
        hipLaunchKernelGGL(kern, grid, block, lds, st, A, B1, B2, C, p.bits);                             \
        break;                                                                                            \
      }                                                                                                   \
      if (p.bits.m3 && p.bits.nt_loads) {                                                                 \
        auto kern = artn_k_bits<KB1, K2, false, 0, false, true, true>;                                    \
        if (hipError_t e = ensure_lds<artn_k_bits<KB1, K2, false, 0, false, true, true>>(lds); e != hipSuccess) return e; \
        hipLaunchKernelGGL(kern, grid, block, lds, st, A, B1, B2, C, p.bits);                             \
        break;                                                                                            \
      }                                                                                                   \
      if (p.bits.m3) {                                                                                    \
        auto kern = artn_k_bits<KB1, K2, false, 0, false, false, true>;                                   \
        if (hipError_t e = ensure_lds<artn_k_bits<KB1, K2, false, 0, false, false, true>>(lds); e != hipSuccess) return e; \
        hipLaunchKernelGGL(kern, grid, block, lds, st, A, B1, B2, C, p.bits);                             \
        break;                                                                                            \
      }                                                                                                   \
    }                                                                                                     \
    if constexpr (KB1 >= 3 && (K2 == 0 || K2 >= 3)) {                                                     \
      if (p.bits.nt_loads && full) { /* the big steps: non-temporal loads of A, 2^12-element tiles */     \
        auto kern = artn_k_bits<KB1, K2, false, 0, false, true, false, true>;                             \
        if (hipError_t e = ensure_lds<artn_k_bits<KB1, K2, false, 0, false, true, false, true>>(lds); e != hipSuccess) return e; \
        hipLaunchKernelGGL(kern, grid, block, lds, st, A, B1, B2, C, p.bits);                             \
        break;                                                                                            \
      }                                                                                                   \
      if (p.bits.nt_loads) { /* non-temporal loads of A */                                                \
        auto kern = artn_k_bits<KB1, K2, false, 0, false, true>;                                          \
        if (hipError_t e = ensure_lds<artn_k_bits<KB1, K2, false, 0, false, true>>(lds); e != hipSuccess) return e; \
        hipLaunchKernelGGL(kern, grid, block, lds, st, A, B1, B2, C, p.bits);                             \
        break;                                                                                            \
      }                                                                                                   \
    }                                                                                                     \
    ARTN_LAUNCH_NP(K2, 0)                                                                                 \
    break;                                                                                                \
  }
  // the big launches (2^12-element tiles, fp32 chains, grid-stride tiles): one 8-wave workgroup per CU whose two
  // groups alternate between the MFMA stages and the copy phases (artn_k_alt)
  if constexpr (KB1 >= 3) {
    if (full && p.bits.T_mid == 12 && split == 0 && p.bits.gather_dim < 0 && !p.bits.blocked && p.bits.st[0].k <= 6 && !p.bits.accumulate &&
        (artn::tuning().alt == 1 || (artn::tuning().alt == 2 && p.bits.run_out < 4)) &&
        p.bits.n_tiles >= 64 && (k2 == 0 || k2 >= 3)) {
      const long half_tiles = (long)((p.bits.n_tiles + 1) / 2);
      dim3 agrid((unsigned)std::min<long>((long)p.n_cu, half_tiles)), ablock(2 * ARTN_WG_THREADS);
      const size_t alds = lds + 65536;
#define ARTN_ALT_GO(K2, NTV, M3V)                                                                           \
  {                                                                                                       \
    auto kern = artn_k_alt<KB1, K2, NTV, M3V>;                                                            \
    if (hipError_t e = ensure_lds<artn_k_alt<KB1, K2, NTV, M3V>>(alds); e != hipSuccess) return e;        \
    hipLaunchKernelGGL(kern, agrid, ablock, alds, st, A, B1, B2, C, p.bits);                              \
    return hipGetLastError();                                                                             \
  }
#define ARTN_ALT_CASE(K2)                                                                                 \
  case K2: {                                                                                              \
    if constexpr (ARTN_K2_HERE(K2)) {                                                                     \
      if constexpr ((KB1 == 5 || KB1 == 6 || K2 == 5 || K2 == 6) && !((KB1 >= 5 && K2 >= 5) && KB1 + K2 > 11)) { \
        if (p.bits.m3) {                                                                                  \
          if (p.bits.nt_loads) ARTN_ALT_GO(K2, true, true) else ARTN_ALT_GO(K2, false, true)              \
        }                                                                                                 \
      }                                                                                                   \
      if (!p.bits.m3) {                                                                                   \
        if (p.bits.nt_loads) ARTN_ALT_GO(K2, true, false) else ARTN_ALT_GO(K2, false, false)              \
      }                                                                                                   \
    }                                                                                                     \
    break;                                                                                                \
  }
      switch (k2) {
        ARTN_ALT_CASE(0)
        ARTN_ALT_CASE(3)
        ARTN_ALT_CASE(4)
        ARTN_ALT_CASE(5)
        ARTN_ALT_CASE(6)
        default: break;
      }
#undef ARTN_ALT_CASE
#undef ARTN_ALT_GO
    }
  }
  if constexpr (LO && (KB1 == 5 || KB1 == 6)) { // single steps that keep at most 4 result bits in the tile: 16 x 16 x 4 blocks, three products
    if (p.bits.narrow3 == 1 && k2 == 0 && split == 0 && p.bits.gather_dim < 0 && p.bits.st[0].k <= 6 && !full) {
      if (p.bits.nt_loads) {
        auto kern = artn_k_bits<KB1, 0, false, 0, false, true, false, false, 1>;
        if (hipError_t e = ensure_lds<artn_k_bits<KB1, 0, false, 0, false, true, false, false, 1>>(lds); e != hipSuccess) return e;
        hipLaunchKernelGGL(kern, grid, block, lds, st, A, B1, B2, C, p.bits);
      } else {
        auto kern = artn_k_bits<KB1, 0, false, 0, false, false, false, false, 1>;
        if (hipError_t e = ensure_lds<artn_k_bits<KB1, 0, false, 0, false, false, false, false, 1>>(lds); e != hipSuccess) return e;
        hipLaunchKernelGGL(kern, grid, block, lds, st, A, B1, B2, C, p.bits);
      }
      return hipGetLastError();
    }
  }
  if constexpr (HI && KB1 >= 2) { // 3M pairs whose SECOND stage keeps at most 4 result bits in the tile (ArtnBitsPlan::narrow3 = 2)
    if (p.bits.narrow3 == 2 && p.bits.m3 && (k2 == 5 || k2 == 6) && split == 0 && p.bits.gather_dim < 0 && p.bits.st[0].k <= 6 && !full) {
#define ARTN_N3_GO(K2, NTV)                                                                               \
  {                                                                                                       \
    auto kern = artn_k_bits<KB1, K2, false, 0, false, NTV, true, false, 2>;                               \
    if (hipError_t e = ensure_lds<artn_k_bits<KB1, K2, false, 0, false, NTV, true, false, 2>>(lds); e != hipSuccess) return e; \
    hipLaunchKernelGGL(kern, grid, block, lds, st, A, B1, B2, C, p.bits);                                 \
    return hipGetLastError();                                                                             \
  }
      if (k2 == 5) { if (p.bits.nt_loads) ARTN_N3_GO(5, true) else ARTN_N3_GO(5, false) }
      else { if (p.bits.nt_loads) ARTN_N3_GO(6, true) else ARTN_N3_GO(6, false) }
#undef ARTN_N3_GO
    }
  }
  if constexpr (LO) { // single stages (k2 == 0): the row gather and the steps of more than 6 contracted bits
    if (p.bits.gather_dim >= 0) { // fused row gather: single stage, fp32 chains
      if (k2 != 0) return hipErrorInvalidValue;
      if (KB1 == 6 && p.bits.st[0].k > 6) {
        auto kern = artn_k_bits<(KB1 == 6 ? 6 : 1), 0, true, 0, true>;
        if (hipError_t e = ensure_lds<artn_k_bits<(KB1 == 6 ? 6 : 1), 0, true, 0, true>>(lds); e != hipSuccess) return e;
        hipLaunchKernelGGL(kern, grid, block, lds, st, A, B1, B2, C, p.bits);
      } else {
        auto kern = artn_k_bits<KB1, 0, false, 0, true>;
        if (hipError_t e = ensure_lds<artn_k_bits<KB1, 0, false, 0, true>>(lds); e != hipSuccess) return e;
        hipLaunchKernelGGL(kern, grid, block, lds, st, A, B1, B2, C, p.bits);
      }
      return hipGetLastError();
    }
    if (KB1 == 6 && k2 == 0 && p.bits.st[0].k > 6 && split == 1) { // bf16 operands
      auto kern = artn_k_bits<(KB1 == 6 ? 6 : 1), 0, true, 1>;
      if (hipError_t e = ensure_lds<artn_k_bits<(KB1 == 6 ? 6 : 1), 0, true, 1>>(lds); e != hipSuccess) return e;
      hipLaunchKernelGGL(kern, grid, block, lds, st, A, B1, B2, C, p.bits);
      return hipGetLastError();
    }
    if (KB1 == 6 && k2 == 0 && p.bits.st[0].k > 6) {
      auto kern = artn_k_bits<(KB1 == 6 ? 6 : 1), 0, true>;
      if (hipError_t e = ensure_lds<artn_k_bits<(KB1 == 6 ? 6 : 1), 0, true>>(lds); e != hipSuccess) return e;
      hipLaunchKernelGGL(kern, grid, block, lds, st, A, B1, B2, C, p.bits);
      return hipGetLastError();
    }
  }
  switch (k2) {
    ARTN_LAUNCH(0)
    ARTN_LAUNCH(1)
    ARTN_LAUNCH(2)
    ARTN_LAUNCH(3)
    ARTN_LAUNCH(4)
    ARTN_LAUNCH(5)
    ARTN_LAUNCH(6)
    default: return hipErrorInvalidValue;
  }
#undef ARTN_LAUNCH
#undef ARTN_K2_HERE
#undef ARTN_LAUNCH_NP
  return hipGetLastError();
}
