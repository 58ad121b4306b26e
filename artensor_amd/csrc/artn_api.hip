// artn_api.hip -- the main translation unit of libartn_hip.so: dispatch from a plan to its launcher, the launchers of the
// two-operand GEMMs and of the small kernels, the small-step program builder, and every extern "C" entry point of
// include/artn.h except the Born-statistics and reduced-density-matrix ones (artn_born.hip, artn_rdm.hip).  It emits every
// kernel of artn_kernels.hip that no unit under units/ emits.
#include <map>
#include <mutex>
#include <stdio.h>

#include "artn_host.h"
#define ARTN_KERNELS_REST 1
#include "artn_kernels.hip"

ArtnHostState &artn_host_state() {
  static thread_local ArtnHostState s;
  return s;
}

static int g_ndev = -1, g_ncu = 256;
static std::once_flag g_once;
static void probe_devices() {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
  int good = 0;
  for (int d = 0; d < n; ++d) {
    hipDeviceProp_t pr;
    if (hipGetDeviceProperties(&pr, d) != hipSuccess) continue;
    if (strncmp(pr.gcnArchName, "gfx950", 6) == 0) {
      ++good;
      g_ncu = pr.multiProcessorCount;
    }
  }
  (void)hipGetLastError();
  g_ndev = good;
}

// Three-step fusion (artn_k_bits3 / artn_contract3, round 4) was built, is parity-green and shortens no committed workload
// (DESIGN.md 4.1c): it is compiled only into development builds (make dev: -DARTN_DEV_BITS3).
#if defined(ARTN_DEV_BITS3)
static hipError_t launch_bits3(const ArtnPlan &p, const void *A, const void *B1, const void *B2, const void *B3, void *C, hipStream_t st) {
  const float2 *a = (const float2 *)A, *b1 = (const float2 *)B1, *b2 = (const float2 *)B2, *b3 = (const float2 *)B3;
  float2 *c = (float2 *)C;
  switch (p.bits.st[0].k) {
    case 3: return artn_launch_bits3_k3(p, a, b1, b2, b3, c, st);
    case 4: return artn_launch_bits3_k4(p, a, b1, b2, b3, c, st);
    case 5: return artn_launch_bits3_k5(p, a, b1, b2, b3, c, st);
  }
  return hipErrorInvalidValue;
}
#endif // ARTN_DEV_BITS3

static hipError_t launch_bits(const ArtnPlan &p, const void *A, const void *B1, const void *B2, void *C,
                              hipStream_t st) {
  if (p.bits.c128) return p.bits.accumulate ? artn_launch_bits128_acc(p, A, B1, B2, C, st) : artn_launch_bits128(p, A, B1, B2, C, st);
  if (p.bits.wide8) return artn_launch_wide(p, A, B1, B2, C, st);
  const float2 *a = (const float2 *)A, *b1 = (const float2 *)B1, *b2 = (const float2 *)B2;
  float2 *c = (float2 *)C;
  const bool hi = p.bits.n_stages == 2 && p.bits.st[1].k >= 4; // (the families of 5 and 6 bits: two objects each)
  switch (std::min(p.bits.st[0].k, 6)) {
    case 1: return artn_launch_bits_k1(p, a, b1, b2, c, st);
    case 2: return artn_launch_bits_k2(p, a, b1, b2, c, st);
    case 3: return artn_launch_bits_k3(p, a, b1, b2, c, st);
    case 4: return artn_launch_bits_k4(p, a, b1, b2, c, st);
    case 5: return (hi ? artn_launch_bits_k5h1 : artn_launch_bits_k5h0)(p, a, b1, b2, c, st);
    case 6: return (hi ? artn_launch_bits_k6h1 : artn_launch_bits_k6h0)(p, a, b1, b2, c, st);
  }
  return hipErrorInvalidValue;
}

static hipError_t launch_pgemm(const ArtnPlan &p, const void *A, const void *B, void *C, void *ws, hipStream_t st) {
  const ArtnPackPlan &g = p.pack;
  const float2 *a = (const float2 *)(g.swapped ? B : A), *b = (const float2 *)(g.swapped ? A : B);
  // 16-byte units of the packed copies: bf16 -- 4 chunk values of one row; fp32 -- one chunk value of a row pair
  const int unit_bits = g.arith == 0 ? g.kc_bits - 2 : g.kc_bits - 1;
  const long a_units = 1L << (g.n_mo + g.n_ko + unit_bits + ARTN_PG_MT), b_units = 1L << (g.n_no + g.n_ko + unit_bits + ARTN_PG_NT);
  unsigned char *Ap = (unsigned char *)ws, *Bp = Ap + a_units * 16;
  auto blocks = [&](long units) { return dim3((unsigned)std::min<long>((units + ARTN_WG_THREADS - 1) / ARTN_WG_THREADS, (long)p.n_cu * 16)); };
  const size_t lds = (size_t)p.info.lds_bytes;
  if (g.arith == 0) {
    hipLaunchKernelGGL(artn_k_pack_bf16, blocks(a_units), dim3(ARTN_WG_THREADS), 0, st, a, (u32x4_t *)Ap, g.a, g.n_ko, a_units);
    hipLaunchKernelGGL(artn_k_pack_bf16, blocks(b_units), dim3(ARTN_WG_THREADS), 0, st, b, (u32x4_t *)Bp, g.b, g.n_ko, b_units);
    if (artn::tuning().pgemm16 >= 2) {
      if (hipError_t e = ensure_lds<artn_k_pgemm<2>>(lds); e != hipSuccess) return e;
      hipLaunchKernelGGL(artn_k_pgemm<2>, dim3(p.info.grid), dim3(ARTN_PG_THREADS), lds, st, Ap, Bp, (float2 *)C, g);
    } else if (artn::tuning().pgemm16 == 1) {
      if (hipError_t e = ensure_lds<artn_k_pgemm<1>>(lds); e != hipSuccess) return e;
      hipLaunchKernelGGL(artn_k_pgemm<1>, dim3(p.info.grid), dim3(ARTN_PG_THREADS), lds, st, Ap, Bp, (float2 *)C, g);
    } else {
      if (hipError_t e = ensure_lds<artn_k_pgemm<0>>(lds); e != hipSuccess) return e;
      hipLaunchKernelGGL(artn_k_pgemm<0>, dim3(p.info.grid), dim3(ARTN_PG_THREADS), lds, st, Ap, Bp, (float2 *)C, g);
    }
  } else {
    hipLaunchKernelGGL(artn_k_pack_f32, blocks(a_units), dim3(ARTN_WG_THREADS), 0, st, a, (f32x4 *)Ap, g.a, g.n_ko, a_units);
    hipLaunchKernelGGL(artn_k_pack_f32, blocks(b_units), dim3(ARTN_WG_THREADS), 0, st, b, (f32x4 *)Bp, g.b, g.n_ko, b_units);
    if (hipError_t e = ensure_lds<artn_k_pgemm3m>(lds); e != hipSuccess) return e;
    hipLaunchKernelGGL(artn_k_pgemm3m, dim3(p.info.grid), dim3(ARTN_PG_THREADS), lds, st, Ap, Bp, (float2 *)C, g);
  }
  return hipGetLastError();
}

static hipError_t launch_xgemm128(const ArtnPlan &p, const void *A, const void *B, void *C, hipStream_t st) {
  const ArtnXGemmPlan &g = p.xg;
  const double2 *a = (const double2 *)(g.swapped ? B : A), *b = (const double2 *)(g.swapped ? A : B);
  dim3 grid(p.info.grid), block(ARTN_WG_THREADS);
  const size_t lds = (size_t)p.info.lds_bytes;
  if (g.kc != ARTN_XG128_KC || g.pc) return hipErrorInvalidValue;
  if (g.nb == 1) {
    if (hipError_t e = ensure_lds<artn_k_xgemm128<1>>(lds); e != hipSuccess) return e;
    hipLaunchKernelGGL(artn_k_xgemm128<1>, grid, block, lds, st, a, b, (double2 *)C, g);
  } else {
    return hipErrorInvalidValue;
  }
  return hipGetLastError();
}
// chunks of 16 contracted values: one of the six (blocks per tile, operand roles) instantiations
static hipError_t launch_xgemm16(const ArtnXGemmPlan &g, int n_wg, size_t lds, const float2 *a, const float2 *b, float2 *c, hipStream_t st) {
  dim3 grid(n_wg), block(ARTN_WG_THREADS);
#define ARTN_XGEMM_LAUNCH(NBV, TRV)                                                                  \
  {                                                                                                  \
    auto kern = artn_k_xgemm<NBV, TRV>;                                                              \
    if (hipError_t e = ensure_lds<artn_k_xgemm<NBV, TRV>>(lds); e != hipSuccess) return e;           \
    hipLaunchKernelGGL(kern, grid, block, lds, st, a, b, c, g);                                      \
    return hipGetLastError();                                                                        \
  }
  switch (g.nb * 2 + (g.trans ? 1 : 0)) {
    case 2: ARTN_XGEMM_LAUNCH(1, false)
    case 3: ARTN_XGEMM_LAUNCH(1, true)
    case 4: ARTN_XGEMM_LAUNCH(2, false)
    case 5: ARTN_XGEMM_LAUNCH(2, true)
    case 6: ARTN_XGEMM_LAUNCH(3, false)
    case 7: ARTN_XGEMM_LAUNCH(3, true)
  }
#undef ARTN_XGEMM_LAUNCH
  return hipErrorInvalidValue;
}
static hipError_t launch_xgemm(const ArtnPlan &p, const void *A, const void *B, void *C, hipStream_t st) {
  const ArtnXGemmPlan &g = p.xg;
  if (g.c128) return launch_xgemm128(p, A, B, C, st);
  const float2 *a = (const float2 *)(g.swapped ? B : A), *b = (const float2 *)(g.swapped ? A : B);
  float2 *c = (float2 *)C;
  dim3 grid(p.info.grid), block(ARTN_WG_THREADS);
  const size_t lds = (size_t)p.info.lds_bytes;
  if (g.rowmode == 2) { // the row-streaming form with a lane per row (64-row superblocks)
#define ARTN_XROW64_LAUNCH(SV)                                                                       \
  case SV:                                                                                           \
    if (artn_xrow_nbk(g.n.total) == 1) hipLaunchKernelGGL((artn_k_xrow64<SV, 1>), grid, block, lds, st, a, b, c, g); \
    else hipLaunchKernelGGL((artn_k_xrow64<SV, 2>), grid, block, lds, st, a, b, c, g);                 \
    break;
    if (artn_xrow_nbk(g.n.total) > 2) return hipErrorInvalidValue;
    switch (artn_xrow_steps(g.k.total)) {
      ARTN_XROW64_LAUNCH(1) ARTN_XROW64_LAUNCH(2) ARTN_XROW64_LAUNCH(3) ARTN_XROW64_LAUNCH(4)
      ARTN_XROW64_LAUNCH(5) ARTN_XROW64_LAUNCH(6) ARTN_XROW64_LAUNCH(7) ARTN_XROW64_LAUNCH(8)
      default: return hipErrorInvalidValue;
    }
#undef ARTN_XROW64_LAUNCH
    return hipGetLastError();
  }
  if (g.rowmode) { // the row-streaming form: the small operand in registers (1..8 MFMA steps of four contracted values, 1 or 2 column blocks)
#define ARTN_XROW_LAUNCH(SV)                                                                         \
  case SV:                                                                                           \
    switch (artn_xrow_nbk(g.n.total)) {                                                              \
      case 1: hipLaunchKernelGGL((artn_k_xrow<SV, 1>), grid, block, lds, st, a, b, c, g); break;     \
      case 2: hipLaunchKernelGGL((artn_k_xrow<SV, 2>), grid, block, lds, st, a, b, c, g); break;     \
      case 3: hipLaunchKernelGGL((artn_k_xrow<SV, 3>), grid, block, lds, st, a, b, c, g); break;     \
      default: return hipErrorInvalidValue;                                                          \
    }                                                                                                \
    break;
    switch (artn_xrow_steps(g.k.total)) {
      ARTN_XROW_LAUNCH(1) ARTN_XROW_LAUNCH(2) ARTN_XROW_LAUNCH(3) ARTN_XROW_LAUNCH(4)
      ARTN_XROW_LAUNCH(5) ARTN_XROW_LAUNCH(6) ARTN_XROW_LAUNCH(7) ARTN_XROW_LAUNCH(8)
      ARTN_XROW_LAUNCH(9) ARTN_XROW_LAUNCH(10) ARTN_XROW_LAUNCH(11) ARTN_XROW_LAUNCH(12)
      default: return hipErrorInvalidValue;
    }
#undef ARTN_XROW_LAUNCH
    return hipGetLastError();
  }
#ifdef ARTN_DEV_XGPC
  if (g.pc) { // one 8-wave workgroup per CU: four consumer waves (MFMAs, epilogue), four producer waves (tables, loads, LDS fills)
    dim3 pblock(ARTN_XGPC_THREADS);
#define ARTN_XGPC_LAUNCH(NBV, TRV)                                                                   \
  {                                                                                                  \
    auto kern = artn_k_xgemm_pc<NBV, TRV>;                                                           \
    if (hipError_t e = ensure_lds<artn_k_xgemm_pc<NBV, TRV>>(lds); e != hipSuccess) return e;        \
    hipLaunchKernelGGL(kern, grid, pblock, lds, st, a, b, c, g);                                     \
    return hipGetLastError();                                                                        \
  }
    switch (g.nb * 2 + (g.trans ? 1 : 0)) {
      case 2: ARTN_XGPC_LAUNCH(1, false)
      case 3: ARTN_XGPC_LAUNCH(1, true)
      case 4: ARTN_XGPC_LAUNCH(2, false)
      case 5: ARTN_XGPC_LAUNCH(2, true)
      case 6: ARTN_XGPC_LAUNCH(3, false)
      case 7: ARTN_XGPC_LAUNCH(3, true)
    }
#undef ARTN_XGPC_LAUNCH
    return hipErrorInvalidValue;
  }
#else
  if (g.pc) return hipErrorInvalidValue; // (development builds only)
#endif
  if (g.kc == 8) { // few contracted values, one block of columns: chunks of 8, four workgroups per CU
    if (g.nb != 1) return hipErrorInvalidValue;
    if (g.trans) {
      auto kern = artn_k_xgemm<1, true, 8>;
      if (hipError_t e = ensure_lds<artn_k_xgemm<1, true, 8>>(lds); e != hipSuccess) return e;
      hipLaunchKernelGGL(kern, grid, block, lds, st, a, b, c, g);
    } else {
      auto kern = artn_k_xgemm<1, false, 8>;
      if (hipError_t e = ensure_lds<artn_k_xgemm<1, false, 8>>(lds); e != hipSuccess) return e;
      hipLaunchKernelGGL(kern, grid, block, lds, st, a, b, c, g);
    }
    return hipGetLastError();
  }
  if (hipError_t e = launch_xgemm16(g, p.info.grid, lds, a, b, c, st); e != hipSuccess) return e;
  if (g.tail_nb) { // the columns behind the full column tiles: a second launch of the instantiation they need (artn_xg_tail_plan)
    const ArtnXGemmPlan t = artn_xg_tail_plan(g);
    return launch_xgemm16(t, g.tail_grid, (size_t)g.tail_lds, a, b, c, st);
  }
  return hipSuccess;
}

static hipError_t launch_gemm(const ArtnPlan &p, const void *A, const void *B, void *C, hipStream_t st) {
  const ArtnGemmPlan &g = p.gemm;
  const float2 *a = (const float2 *)(g.swapped ? B : A), *b = (const float2 *)(g.swapped ? A : B);
  float2 *c = (float2 *)C;
  dim3 grid(p.info.grid), block(ARTN_WG_THREADS);
  const size_t lds = (size_t)p.info.lds_bytes;
#define ARTN_GEMM_LAUNCH(MBV, NBV)                                                                   \
  {                                                                                                  \
    auto kern = artn_k_gemm<MBV, NBV>;                                                               \
    if (hipError_t e = ensure_lds<artn_k_gemm<MBV, NBV>>(lds); e != hipSuccess) return e;            \
    hipLaunchKernelGGL(kern, grid, block, lds, st, a, b, c, g);                                      \
    return hipGetLastError();                                                                        \
  }
#define ARTN_GEMM_LAUNCH_BF(MBV, NBV)                                                                \
  {                                                                                                  \
    auto kern = artn_k_gemm<MBV, NBV, true>;                                                         \
    if (hipError_t e = ensure_lds<artn_k_gemm<MBV, NBV, true>>(lds); e != hipSuccess) return e;      \
    hipLaunchKernelGGL(kern, grid, block, lds, st, a, b, c, g);                                      \
    return hipGetLastError();                                                                        \
  }
#define ARTN_GEMM_LAUNCH_M3(MBV, NBV)                                                                \
  {                                                                                                  \
    auto kern = artn_k_gemm<MBV, NBV, false, true>;                                                  \
    if (hipError_t e = ensure_lds<artn_k_gemm<MBV, NBV, false, true>>(lds); e != hipSuccess) return e; \
    hipLaunchKernelGGL(kern, grid, block, lds, st, a, b, c, g);                                      \
    return hipGetLastError();                                                                        \
  }
  if (g.split == 2) { // complex128 on v_mfma_f64_16x16x4_f64
    const double2 *a2 = (const double2 *)(g.swapped ? B : A), *b2 = (const double2 *)(g.swapped ? A : B);
    double2 *c2 = (double2 *)C;
#define ARTN_GEMM128_LAUNCH(NBV)                                                                     \
  {                                                                                                  \
    auto kern = artn_k_gemm128<NBV>;                                                                 \
    if (hipError_t e = ensure_lds<artn_k_gemm128<NBV>>(lds); e != hipSuccess) return e;              \
    hipLaunchKernelGGL(kern, grid, block, lds, st, a2, b2, c2, g);                                   \
    return hipGetLastError();                                                                        \
  }
#define ARTN_GEMM128_LAUNCH_G(NBV)                                                                   \
  {                                                                                                  \
    auto kern = artn_k_gemm128<NBV, true>;                                                           \
    if (hipError_t e = ensure_lds<artn_k_gemm128<NBV, true>>(lds); e != hipSuccess) return e;        \
    hipLaunchKernelGGL(kern, grid, block, lds, st, a2, b2, c2, g);                                   \
    return hipGetLastError();                                                                        \
  }
    if (g.gather_dim >= 0) { // row gather (artn_contract_gather) in complex128
      switch (g.nb_log2) {
        case 0: ARTN_GEMM128_LAUNCH_G(1)
        case 1: ARTN_GEMM128_LAUNCH_G(2)
        case 2: ARTN_GEMM128_LAUNCH_G(4)
      }
      return hipErrorInvalidValue;
    }
    switch (g.nb_log2) {
      case 0: ARTN_GEMM128_LAUNCH(1)
      case 1: ARTN_GEMM128_LAUNCH(2)
      case 2: ARTN_GEMM128_LAUNCH(4)
    }
#undef ARTN_GEMM128_LAUNCH_G
#undef ARTN_GEMM128_LAUNCH
    return hipErrorInvalidValue;
  }
  const int key = g.mb_log2 * 4 + g.nb_log2;
  if (g.gather_dim >= 0) { // row gather (artn_contract_gather): fp32, chunks of 2^4
    if (g.split || g.kc != ARTN_GEMM_KC || g.pitch_log2 != ARTN_GEMM_PITCH_LOG2) return hipErrorInvalidValue;
#define ARTN_GEMM_LAUNCH_G(MBV, NBV, M3V)                                                            \
  {                                                                                                  \
    auto kern = artn_k_gemm<MBV, NBV, false, M3V, false, true>;                                      \
    if (hipError_t e = ensure_lds<artn_k_gemm<MBV, NBV, false, M3V, false, true>>(lds); e != hipSuccess) return e; \
    hipLaunchKernelGGL(kern, grid, block, lds, st, a, b, c, g);                                      \
    return hipGetLastError();                                                                        \
  }
#define ARTN_GEMM_LAUNCH_DEEP_G(MBV, NBIV)                                                           \
  {                                                                                                  \
    auto kern = artn_k_gemm_deep<MBV, 1, 4, NBIV, true>;                                             \
    if (hipError_t e = ensure_lds<artn_k_gemm_deep<MBV, 1, 4, NBIV, true>>(lds); e != hipSuccess) return e; \
    hipLaunchKernelGGL(kern, grid, block, lds, st, a, b, c, g);                                      \
    return hipGetLastError();                                                                        \
  }
    if (g.m3) {
      if (g.nb_log2 == 0 && g.wk_log2 == 0 && g.n_ko >= 1 && g.n_ko <= 8 && g.ta_bits == 11 && artn::tuning().gemm_deep) {
        if (g.mb_log2 == 0 && g.tb_bits == 9) ARTN_GEMM_LAUNCH_DEEP_G(1, 1)
        if (g.mb_log2 == 1 && g.tb_bits == 10 && artn::tuning().gemm_deep >= 2) ARTN_GEMM_LAUNCH_DEEP_G(2, 2)
      }
      switch (key) {
        case 0: ARTN_GEMM_LAUNCH_G(1, 1, true)
        case 1: ARTN_GEMM_LAUNCH_G(1, 2, true)
        case 4: ARTN_GEMM_LAUNCH_G(2, 1, true)
      }
      return hipErrorInvalidValue;
    }
    if (key == 0 && g.wk_log2 == 0 && g.n_ko >= 1 && g.n_ko <= 8 && g.ta_bits == 11 && g.tb_bits <= 9 && artn::tuning().gemm_deep) {
      // 4M, 16 columns or fewer: the chunk steps of the sparse executor
      auto kern = artn_k_gemm_deep<1, 1, 4, 1, true, false>;
      if (hipError_t e = ensure_lds<artn_k_gemm_deep<1, 1, 4, 1, true, false>>(lds); e != hipSuccess) return e;
      hipLaunchKernelGGL(kern, grid, block, lds, st, a, b, c, g);
      return hipGetLastError();
    }
    switch (key) {
      case 0: ARTN_GEMM_LAUNCH_G(1, 1, false)
      case 1: ARTN_GEMM_LAUNCH_G(1, 2, false)
      case 2: ARTN_GEMM_LAUNCH_G(1, 4, false)
      case 5: ARTN_GEMM_LAUNCH_G(2, 2, false)
      case 6: ARTN_GEMM_LAUNCH_G(2, 4, false)
    }
#undef ARTN_GEMM_LAUNCH_G
#undef ARTN_GEMM_LAUNCH_DEEP_G
    return hipErrorInvalidValue;
  }
  if (g.kc == ARTN_GEMM_KC_TALL && !g.split) { // 32 x 32 tiles, chunks of 2^6 contracted values
    if (key != 0) return hipErrorInvalidValue;
    if (g.m3) {
      auto kern = artn_k_gemm<1, 1, false, true, true>;
      if (hipError_t e = ensure_lds<artn_k_gemm<1, 1, false, true, true>>(lds); e != hipSuccess) return e;
      hipLaunchKernelGGL(kern, grid, block, lds, st, a, b, c, g);
    } else {
      auto kern = artn_k_gemm<1, 1, false, false, true>;
      if (hipError_t e = ensure_lds<artn_k_gemm<1, 1, false, false, true>>(lds); e != hipSuccess) return e;
      hipLaunchKernelGGL(kern, grid, block, lds, st, a, b, c, g);
    }
    return hipGetLastError();
  }
  // memory-bound 3M steps (few free bits in the second operand: one block column per wave): operand loads two chunks ahead
  if (g.m3 && g.nb_log2 == 0 && g.wk_log2 == 0 && g.n_ko >= 1 && g.n_ko <= 8 && g.ta_bits == 11 &&
      g.pitch_log2 == ARTN_GEMM_PITCH_LOG2 && g.kc == ARTN_GEMM_KC && artn::tuning().gemm_deep) {
#define ARTN_GEMM_LAUNCH_DEEP(MBV, NBIV)                                                             \
  {                                                                                                  \
    auto kern = artn_k_gemm_deep<MBV, 1, 4, NBIV>;                                                   \
    if (hipError_t e = ensure_lds<artn_k_gemm_deep<MBV, 1, 4, NBIV>>(lds); e != hipSuccess) return e; \
    hipLaunchKernelGGL(kern, grid, block, lds, st, a, b, c, g);                                      \
    return hipGetLastError();                                                                        \
  }
    if (g.mb_log2 == 0 && g.tb_bits == 9) ARTN_GEMM_LAUNCH_DEEP(1, 1)
    if (g.mb_log2 == 1 && g.tb_bits == 10 && artn::tuning().gemm_deep >= 2) ARTN_GEMM_LAUNCH_DEEP(2, 2)
#undef ARTN_GEMM_LAUNCH_DEEP
  }
  if (g.m3) {
    switch (key) {
      case 0: ARTN_GEMM_LAUNCH_M3(1, 1)
      case 1: ARTN_GEMM_LAUNCH_M3(1, 2)
      case 4: ARTN_GEMM_LAUNCH_M3(2, 1)
    }
    return hipErrorInvalidValue;
  }
  if (g.split) {
    switch (key) {
      case 0: ARTN_GEMM_LAUNCH_BF(1, 1)
      case 1: ARTN_GEMM_LAUNCH_BF(1, 2)
      case 5: ARTN_GEMM_LAUNCH_BF(2, 2)
    }
    return hipErrorInvalidValue;
  }
  if (key == 0 && g.wk_log2 == 0 && g.n_ko >= 1 && g.n_ko <= 8 && g.ta_bits == 11 && g.tb_bits <= 9 &&
      g.pitch_log2 == ARTN_GEMM_PITCH_LOG2 && g.kc == ARTN_GEMM_KC && artn::tuning().gemm_deep) {
    // 4M, memory-bound: operand loads two chunks ahead
    auto kern = artn_k_gemm_deep<1, 1, 4, 1, false, false>;
    if (hipError_t e = ensure_lds<artn_k_gemm_deep<1, 1, 4, 1, false, false>>(lds); e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, grid, block, lds, st, a, b, c, g);
    return hipGetLastError();
  }
  switch (key) {
    case 0: ARTN_GEMM_LAUNCH(1, 1)
    case 1: ARTN_GEMM_LAUNCH(1, 2)
    case 2: ARTN_GEMM_LAUNCH(1, 4)
    case 5: ARTN_GEMM_LAUNCH(2, 2)
    case 6: ARTN_GEMM_LAUNCH(2, 4)
  }
#undef ARTN_GEMM_LAUNCH
#undef ARTN_GEMM_LAUNCH_BF
#undef ARTN_GEMM_LAUNCH_M3
  return hipErrorInvalidValue;
}

extern "C" {

int artn_abi_version(void) { return ARTN_ABI_VERSION; }
const char *artn_last_error(void) { return artn_host_state().err.c_str(); }

int artn_device_count(void) {
  std::call_once(g_once, probe_devices);
  return g_ndev;
}

int artn_contract_query(const ArtnStepDesc *d, ArtnStepInfo *info) {
  if (!info) return fail(ARTN_E_INVALID, "null info");
  ArtnPlan p;
  std::string err;
  const bool no_bits = env_flag("ARTN_FORCE_GENERIC");
  const int64_t min_tiles = env_flag("ARTN_FORCE_BITS") ? 1 : 32;
  int rc = artn::make_plan(d, p, err, g_ncu, !no_bits, min_tiles, -1, true, true);
  if (rc) return fail(rc, err);
  *info = p.info;
  artn_host_state().note = p.kernel == ARTN_KERNEL_GENERIC ? p.why_generic : std::string();
  return ARTN_OK;
}

const char *artn_last_plan_note(void) { return artn_host_state().note.c_str(); }

int artn_contract(const ArtnStepDesc *d, const void *A, const void *B, void *C, void *stream) {
  if (artn_device_count() < 1) return fail(ARTN_E_NODEVICE, "no gfx950 device visible");
  if (!A || !B || !C) return fail(ARTN_E_INVALID, "null operand pointer");
  ArtnPlan p;
  std::string err;
  const bool aligned = (((uintptr_t)A | (uintptr_t)C) & 15) == 0;
  const bool no_bits = env_flag("ARTN_FORCE_GENERIC") || !aligned;
  const int64_t min_tiles = env_flag("ARTN_FORCE_BITS") ? 1 : 32;
  int rc = artn::make_plan(d, p, err, g_ncu, !no_bits, min_tiles);
  if (rc) return fail(rc, err);
  if (p.kernel == ARTN_KERNEL_GEMM_MFMA && (((uintptr_t)B) & 15) != 0) { // the GEMM kernel moves both operands in 16-byte lanes
    rc = artn::make_plan(d, p, err, g_ncu, !no_bits, min_tiles, -1, false);
    if (rc) return fail(rc, err);
  }
  hipStream_t st = (hipStream_t)stream;
  if (p.kernel == ARTN_KERNEL_BITS_MFMA) {
    HIP_TRY(launch_bits(p, A, B, nullptr, C, st));
    return ARTN_OK;
  }
  if (p.kernel == ARTN_KERNEL_GEMM_MFMA) {
    HIP_TRY(launch_gemm(p, A, B, C, st));
    return ARTN_OK;
  }
  if (p.kernel == ARTN_KERNEL_XGEMM) {
    HIP_TRY(launch_xgemm(p, A, B, C, st));
    return ARTN_OK;
  }
  dim3 grid(p.info.grid), block(ARTN_WG_THREADS);
  if (p.gen.out_numel == 0) return ARTN_OK;
  if (p.gen.out_numel <= 4096 && p.gen.red_numel >= 64) { // few results of sums: a workgroup per result
    dim3 rgrid((unsigned)p.gen.out_numel);
    if (d->dtype != ARTN_C128)
      hipLaunchKernelGGL((artn_k_generic_red<float2, float>), rgrid, block, 0, st, (const float2 *)A, (const float2 *)B, (float2 *)C, p.gen);
    else
      hipLaunchKernelGGL((artn_k_generic_red<double2, double>), rgrid, block, 0, st, (const double2 *)A, (const double2 *)B, (double2 *)C, p.gen);
    HIP_TRY(hipGetLastError());
    return ARTN_OK;
  }
  if (d->dtype != ARTN_C128) // (small steps of the reduced-precision mode run in fp32: they are launch-bound)
    hipLaunchKernelGGL((artn_k_generic<float2, float>), grid, block, 0, st, (const float2 *)A,
                       (const float2 *)B, (float2 *)C, p.gen);
  else
    hipLaunchKernelGGL((artn_k_generic<double2, double>), grid, block, 0, st, (const double2 *)A,
                       (const double2 *)B, (double2 *)C, p.gen);
  HIP_TRY(hipGetLastError());
  return ARTN_OK;
}

int artn_contract_ws(const ArtnStepDesc *d, const void *A, const void *B, void *C, void *ws, int64_t ws_bytes, void *stream) {
  if (artn_device_count() < 1) return fail(ARTN_E_NODEVICE, "no gfx950 device visible");
  if (!A || !B || !C) return fail(ARTN_E_INVALID, "null operand pointer");
  if (ws && ws_bytes > 0 && (((uintptr_t)A | (uintptr_t)B | (uintptr_t)C | (uintptr_t)ws) & 15) == 0 && !env_flag("ARTN_FORCE_GENERIC")) {
    ArtnPlan p;
    std::string err;
    const int64_t min_tiles = env_flag("ARTN_FORCE_BITS") ? 1 : 32; // (the same switches as artn_contract / artn_contract_query)
    int rc = artn::make_plan(d, p, err, g_ncu, true, min_tiles, -1, true, true);
    if (rc) return fail(rc, err);
    if (p.kernel == ARTN_KERNEL_PGEMM && p.info.workspace_bytes <= ws_bytes) {
      HIP_TRY(launch_pgemm(p, A, B, C, ws, (hipStream_t)stream));
      return ARTN_OK;
    }
  }
  return artn_contract(d, A, B, C, stream);
}

int artn_contract_gather(const ArtnStepDesc *d, const void *A, const void *B, void *C, int label,
                         const int64_t *rows_a, int64_t src_rows_a, const int64_t *rows_b, int64_t src_rows_b,
                         int32_t *err_flag, void *stream) {
  if (artn_device_count() < 1) return fail(ARTN_E_NODEVICE, "no gfx950 device visible");
  if (!d || !A || !B || !C) return fail(ARTN_E_INVALID, "null pointer");
  if (label < 0 || label >= d->n_labels) return fail(ARTN_E_INVALID, "gather label out of range");
  if (d->stride_c[label] < 0) return fail(ARTN_E_INVALID, "the gathered label must be an output label");
  if ((rows_a && (d->stride_a[label] < 0 || src_rows_a < 1)) || (rows_b && (d->stride_b[label] < 0 || src_rows_b < 1)))
    return fail(ARTN_E_INVALID, "row indices for an operand that does not carry the label");
  // the tiled kernel moves 16-byte lanes (artn_contract falls back to the strided kernel instead;
  // there is no strided gather, so the caller gathers explicitly)
  if ((((uintptr_t)A | (uintptr_t)C) & 15) != 0) return fail(ARTN_E_UNSUPPORTED, "row gather needs 16-byte aligned operands");
  ArtnPlan p;
  std::string err;
  int rc = artn::make_plan(d, p, err, g_ncu, true, 1, label);
  if (rc) return fail(rc, err);
  if (p.kernel == ARTN_KERNEL_GEMM_MFMA) { // (the kernel's first operand is the caller's B when the plan swapped them)
    if ((((uintptr_t)B) & 15) != 0) return fail(ARTN_E_UNSUPPORTED, "row gather needs 16-byte aligned operands");
    const bool sw = p.gemm.swapped != 0;
    p.gemm.rows_a = sw ? rows_b : rows_a;
    p.gemm.rows_b = sw ? rows_a : rows_b;
    p.gemm.src_rows_a = sw ? src_rows_b : src_rows_a;
    p.gemm.src_rows_b = sw ? src_rows_a : src_rows_b;
    p.gemm.gather_err = err_flag;
    if (hipError_t e = launch_gemm(p, A, B, C, (hipStream_t)stream); e != hipSuccess) {
      const ArtnGemmPlan &g = p.gemm;
      return fail(ARTN_E_LAUNCH, std::string("row gather on the GEMM kernel (tile 2^") + std::to_string(g.mt) + " x 2^" + std::to_string(g.nt) +
                                  ", chunk 2^" + std::to_string(g.kc) + ", blocks " + std::to_string(1 << g.mb_log2) + " x " +
                                  std::to_string(1 << g.nb_log2) + (g.m3 ? ", 3M" : "") + ", lds " + std::to_string(p.info.lds_bytes) +
                                  ", grid " + std::to_string(p.info.grid) + "): " + hipGetErrorString(e));
    }
    return ARTN_OK;
  }
  p.bits.rows_a = rows_a;
  p.bits.rows_b = rows_b;
  p.bits.src_rows_a = src_rows_a;
  p.bits.src_rows_b = src_rows_b;
  p.bits.gather_err = err_flag;
  HIP_TRY(launch_bits(p, A, B, nullptr, C, (hipStream_t)stream));
  return ARTN_OK;
}

int artn_contract2_query(const ArtnStepDesc *d1, const ArtnStepDesc *d2, ArtnStepInfo *info) {
  if (!info) return fail(ARTN_E_INVALID, "null info");
  ArtnPlan p;
  std::string err;
  if (env_flag("ARTN_NO_FUSE")) return fail(ARTN_E_UNSUPPORTED, "not fusable: ARTN_NO_FUSE is set");
  const int64_t min_tiles = env_flag("ARTN_FORCE_BITS") ? 1 : 32;
  int rc = artn::make_plan_fused(d1, d2, p, err, g_ncu, min_tiles);
  if (rc) return fail(rc, err);
  *info = p.info;
  return ARTN_OK;
}

int artn_contract2(const ArtnStepDesc *d1, const ArtnStepDesc *d2, const void *A, const void *B1, const void *B2,
                   void *C, void *stream) {
  if (artn_device_count() < 1) return fail(ARTN_E_NODEVICE, "no gfx950 device visible");
  if (!A || !B1 || !B2 || !C) return fail(ARTN_E_INVALID, "null operand pointer");
  if ((((uintptr_t)A | (uintptr_t)C) & 15) != 0) return fail(ARTN_E_UNSUPPORTED, "not fusable: operands not 16-byte aligned");
  if (env_flag("ARTN_NO_FUSE")) return fail(ARTN_E_UNSUPPORTED, "not fusable: ARTN_NO_FUSE is set");
  ArtnPlan p;
  std::string err;
  const int64_t min_tiles = env_flag("ARTN_FORCE_BITS") ? 1 : 32;
  int rc = artn::make_plan_fused(d1, d2, p, err, g_ncu, min_tiles);
  if (rc) return fail(rc, err);
  HIP_TRY(launch_bits(p, A, B1, B2, C, (hipStream_t)stream));
  return ARTN_OK;
}

int artn_contract2_acc(const ArtnStepDesc *d1, const ArtnStepDesc *d2, const void *A, const void *B1, const void *B2,
                       void *C, void *stream) {
  if (artn_device_count() < 1) return fail(ARTN_E_NODEVICE, "no gfx950 device visible");
  if (!A || !B1 || !B2 || !C) return fail(ARTN_E_INVALID, "null operand pointer");
  if ((((uintptr_t)A | (uintptr_t)C) & 15) != 0) return fail(ARTN_E_UNSUPPORTED, "not fusable: operands not 16-byte aligned");
  if (env_flag("ARTN_NO_FUSE") || env_flag("ARTN_NO_ACC")) return fail(ARTN_E_UNSUPPORTED, "not fusable: ARTN_NO_FUSE / ARTN_NO_ACC is set");
  ArtnPlan p;
  std::string err;
  const int64_t min_tiles = env_flag("ARTN_FORCE_BITS") ? 1 : 32;
  int rc = artn::make_plan_fused(d1, d2, p, err, g_ncu, min_tiles);
  if (rc) return fail(rc, err);
  if (p.bits.wide8) return fail(ARTN_E_UNSUPPORTED, "accumulate: not in artn_k_wide");
  if (!artn::bits_can_accumulate(p)) return fail(ARTN_E_UNSUPPORTED, "accumulate: this pair's store phase cannot add");
  p.bits.accumulate = 1;
  HIP_TRY(launch_bits(p, A, B1, B2, C, (hipStream_t)stream));
  return ARTN_OK;
}

int artn_contract_acc(const ArtnStepDesc *d, const void *A, const void *B, void *C, void *stream) {
  if (artn_device_count() < 1) return fail(ARTN_E_NODEVICE, "no gfx950 device visible");
  if (!A || !B || !C) return fail(ARTN_E_INVALID, "null operand pointer");
  if (env_flag("ARTN_NO_ACC")) return fail(ARTN_E_UNSUPPORTED, "accumulate: ARTN_NO_ACC is set");
  ArtnPlan p;
  std::string err;
  const bool aligned = (((uintptr_t)A | (uintptr_t)C) & 15) == 0;
  const int64_t min_tiles = env_flag("ARTN_FORCE_BITS") ? 1 : 32;
  int rc = artn::make_plan(d, p, err, g_ncu, aligned && !env_flag("ARTN_FORCE_GENERIC"), min_tiles);
  if (rc) return fail(rc, err);
  if (!artn::bits_can_accumulate(p)) return fail(ARTN_E_UNSUPPORTED, "accumulate: this step's kernel cannot add in its store phase");
  p.bits.accumulate = 1;
  HIP_TRY(launch_bits(p, A, B, nullptr, C, (hipStream_t)stream));
  return ARTN_OK;
}

#if defined(ARTN_DEV_BITS3)
int artn_contract3_query(const ArtnStepDesc *d1, const ArtnStepDesc *d2, const ArtnStepDesc *d3, ArtnStepInfo *info) {
  if (!info || !d1 || !d2 || !d3) return fail(ARTN_E_INVALID, "null argument");
  if (env_flag("ARTN_NO_FUSE")) return fail(ARTN_E_UNSUPPORTED, "not fusable: ARTN_NO_FUSE is set");
  ArtnPlan p;
  std::string err;
  int rc = artn::make_plan_fused3(d1, d2, d3, p, err, g_ncu);
  if (rc) return fail(rc, err);
  *info = p.info;
  return ARTN_OK;
}

int artn_contract3(const ArtnStepDesc *d1, const ArtnStepDesc *d2, const ArtnStepDesc *d3, const void *A, const void *B1,
                   const void *B2, const void *B3, void *C, void *stream) {
  if (artn_device_count() < 1) return fail(ARTN_E_NODEVICE, "no gfx950 device visible");
  if (!d1 || !d2 || !d3 || !A || !B1 || !B2 || !B3 || !C) return fail(ARTN_E_INVALID, "null pointer");
  if ((((uintptr_t)A | (uintptr_t)C) & 15) != 0) return fail(ARTN_E_UNSUPPORTED, "not fusable: operands not 16-byte aligned");
  if (env_flag("ARTN_NO_FUSE")) return fail(ARTN_E_UNSUPPORTED, "not fusable: ARTN_NO_FUSE is set");
  ArtnPlan p;
  std::string err;
  int rc = artn::make_plan_fused3(d1, d2, d3, p, err, g_ncu);
  if (rc) return fail(rc, err);
  HIP_TRY(launch_bits3(p, A, B1, B2, B3, C, (hipStream_t)stream));
  return ARTN_OK;
}
#endif // ARTN_DEV_BITS3

#if defined(ARTN_STAMPS) || defined(ARTN_PHASES)
// diagnostic builds only
int artn_debug_read_phases(unsigned long long *host) {
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpyFromSymbol(host, HIP_SYMBOL(artn_phase_buf), sizeof(unsigned long long) * 1024 * 20));
  return ARTN_OK;
}
#endif
#ifdef ARTN_STAMPS
int artn_debug_read_stamps(unsigned long long *host, int n_waves) {
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpyFromSymbol(host, HIP_SYMBOL(artn_stamp_buf), sizeof(unsigned long long) * ARTN_N_STAMPS * n_waves));
  return ARTN_OK;
}
#endif

int64_t artn_program_record_bytes(void) { return (int64_t)sizeof(ArtnProgStep); }

static int64_t prog_image_layout(int32_t n_steps, int32_t n_groups, int64_t n_levels, int64_t n_wtasks, int64_t n_terms, ArtnProgHeader *h) {
  int64_t off = sizeof(ArtnProgHeader);
  auto take = [&](int64_t bytes) { const int64_t o = off; off += (bytes + 15) / 16 * 16; return o; };
  const int64_t g = take((int64_t)n_groups * sizeof(ArtnProgGroup)), l = take(n_levels * sizeof(ArtnProgLevel));
  const int64_t w = take(n_wtasks * sizeof(ArtnProgWTask)), r = take((int64_t)n_steps * sizeof(ArtnProgStep));
  const int64_t t = take(n_terms * 8 + 64); // (+64: the 8-entry table loads of the last step may run past its end)
  if (h) { h->off_groups = g; h->off_levels = l; h->off_wtasks = w; h->off_records = r; h->off_tables = t; }
  return off;
}

int64_t artn_program_image_bytes(int32_t n_steps, const ArtnStepDesc *const *descs, int32_t n_groups) {
  if (n_steps < 0 || n_groups < 0 || (n_steps && !descs)) return -1;
  int64_t wt = 0, terms = 0;
  for (int s = 0; s < n_steps; ++s) {
    double f, na, nb, nc;
    artn::step_cost(descs[s], f, na, nb, nc);
    // wave tasks per step as artn_program_build cuts them: ceil(out / 128) for a general step, 2^(m bits - 5) *
    // max(1, 2^(n bits - 4)) blocks for a matrix-core step -- out / 32 when the second operand is fully contracted
    wt += (int64_t)((nc + 31.0) / 32.0) + 1;
    ArtnPlan p;
    std::string err;
    if (artn::validate(descs[s], err) || !artn::make_generic(descs[s], p, err)) return -1;
    terms += p.gen.red_numel;
  }
  return prog_image_layout(n_steps, n_groups, n_steps, wt, terms, nullptr); // (at most one level per step)
}

int artn_program_build(int32_t n_steps, const ArtnStepDesc *const *descs, const int64_t *loc_a, const int64_t *loc_b,
                       const int64_t *loc_c, const uint8_t *keep, int32_t n_groups, const int32_t *group_start,
                       void *host_image, int64_t image_bytes) {
  if (n_steps < 0 || n_groups < 0 || !descs || !loc_a || !loc_b || !loc_c || !group_start || !host_image)
    return fail(ARTN_E_INVALID, "null argument");
  if (group_start[0] != 0 || group_start[n_groups] != n_steps) return fail(ARTN_E_INVALID, "group_start must cover the steps");
  std::vector<ArtnProgStep> rec(n_steps);
  const bool c128 = n_steps > 0 && descs[0]->dtype == ARTN_C128;
  const int64_t esz = c128 ? 16 : 8; // bytes per element in the LDS arena (workspace offsets are the caller's)
  for (int s = 0; s < n_steps; ++s) {
    const ArtnStepDesc *d = descs[s];
    std::string err;
    int rc = artn::validate(d, err);
    if (rc) return fail(rc, err);
    if ((d->dtype == ARTN_C128) != (descs[0]->dtype == ARTN_C128)) return fail(ARTN_E_INVALID, "the steps of a program share one element type");
    ArtnPlan p;
    if (!artn::make_generic(d, p, err)) return fail(ARTN_E_UNSUPPORTED, err);
    const ArtnGenericPlan &g = p.gen;
    if (g.n_out > ARTN_PROG_MAX_OUT || g.n_red > ARTN_PROG_MAX_RED || g.red_numel > ARTN_PROG_MAX_REDN ||
        g.out_numel >= (1LL << 30) || loc_c[s] < 0)
      return fail(ARTN_E_UNSUPPORTED, "step does not fit a small-step record");
    ArtnProgStep &r = rec[s];
    memset(&r, 0, sizeof(r));
    r.n_out = g.n_out; r.n_red = g.n_red; r.out_numel = (int32_t)g.out_numel; r.red_numel = (int32_t)g.red_numel;
    r.loc_a = loc_a[s]; r.loc_b = loc_b[s]; r.loc_c = loc_c[s];
    r.lds_a = r.lds_b = r.lds_c = -1;
    {
      double f, na, nb, nc;
      artn::step_cost(d, f, na, nb, nc);
      if (na >= (double)(1 << 30) || nb >= (double)(1 << 30)) return fail(ARTN_E_UNSUPPORTED, "operand too large for a small-step record");
      r.a_numel = (int32_t)na; r.b_numel = (int32_t)nb;
      // operands are addressed as dense arrays of that many elements
      for (int which = 0; which < 2; ++which) {
        std::vector<std::pair<int64_t, int64_t>> v;
        for (int l = 0; l < d->n_labels; ++l) {
          const int64_t st = which ? d->stride_b[l] : d->stride_a[l];
          if (st >= 0 && d->extent[l] > 1) v.push_back({st, d->extent[l]});
        }
        std::sort(v.begin(), v.end());
        int64_t expect = 1;
        for (auto &pr : v) {
          if (pr.first != expect) return fail(ARTN_E_UNSUPPORTED, "small-step programs take dense operands");
          expect *= pr.second;
        }
      }
    }
    {
      // the generic plan lists the output axes fastest-in-C first: C strides are the running product; then the axes
      // are put in first-operand order (see ArtnProgStep)
      std::vector<int> ax(g.n_out);
      std::vector<int64_t> sc(g.n_out);
      int64_t run = 1;
      for (int i = 0; i < g.n_out; ++i) {
        if (g.out_sA[i] >= (1LL << 30) || g.out_sB[i] >= (1LL << 30)) return fail(ARTN_E_UNSUPPORTED, "stride too large for a small-step record");
        ax[i] = i; sc[i] = run; run *= g.out_ext[i];
      }
      std::stable_sort(ax.begin(), ax.end(), [&](int x, int y) {
        const bool nx = g.out_sA[x] == 0, ny = g.out_sA[y] == 0;
        return nx != ny ? ny : (!nx && g.out_sA[x] < g.out_sA[y]);
      });
      for (int q = 0; q < g.n_out; ++q) {
        const int i = ax[q];
        r.out_ext[q] = (int32_t)g.out_ext[i]; r.out_sA[q] = (int32_t)g.out_sA[i]; r.out_sB[q] = (int32_t)g.out_sB[i]; r.out_sC[q] = (int32_t)sc[i];
        r.out_lg[q] = artn::ilog2_exact(g.out_ext[i]);
      }
    }
    for (int i = 0; i < g.n_red; ++i) {
      if (g.red_sA[i] >= (1LL << 30) || g.red_sB[i] >= (1LL << 30)) return fail(ARTN_E_UNSUPPORTED, "stride too large for a small-step record");
      r.red_ext[i] = (int32_t)g.red_ext[i]; r.red_sA[i] = (int32_t)g.red_sA[i]; r.red_sB[i] = (int32_t)g.red_sB[i];
      r.red_lg[i] = artn::ilog2_exact(g.red_ext[i]);
    }
  }
  // ---- dependencies (a workspace offset names one result), levels, order by level inside each group
  std::map<int64_t, int> producer; // workspace offset -> step
  std::vector<int> level(n_steps, 1), last_use(n_steps, 0), group_of(n_steps, 0);
  for (int g = 0; g < n_groups; ++g)
    for (int s = group_start[g]; s < group_start[g + 1]; ++s) group_of[s] = g;
  for (int s = 0; s < n_steps; ++s) {
    for (int64_t loc : {loc_a[s], loc_b[s]}) {
      if (loc < 0) continue;
      auto it = producer.find(loc);
      if (it == producer.end()) return fail(ARTN_E_INVALID, "a step reads a workspace offset no earlier step wrote");
      if (group_of[it->second] != group_of[s]) return fail(ARTN_E_INVALID, "steps of different groups must be independent");
      level[s] = std::max(level[s], level[it->second] + 1);
    }
    if (producer.count(loc_c[s])) return fail(ARTN_E_INVALID, "two steps write the same workspace offset");
    producer[loc_c[s]] = s;
  }
  // fast steps (prog_mfma_task): every extent a power of two, no output axis in both operands, 5+ output bits in the
  // first operand, 2+ contracted values; a stride per output bit
  for (int s = 0; s < n_steps; ++s) {
    ArtnProgStep &r = rec[s];
    bool ok = r.red_numel >= 2 && (r.red_numel & (r.red_numel - 1)) == 0;
    for (int d = 0; d < r.n_red && ok; ++d) ok = r.red_lg[d] >= 0;
    int mb = 0, nb = 0;
    for (int d = 0; d < r.n_out && ok; ++d) {
      const int lg = r.out_lg[d];
      if (lg < 0 || (r.out_sA[d] != 0 && r.out_sB[d] != 0) || (r.out_sA[d] == 0 && r.out_sB[d] == 0)) { ok = false; break; }
      for (int b = 0; b < lg && ok; ++b) {
        if (r.out_sB[d] == 0) {
          if (mb >= 14) { ok = false; break; }
          r.mbit_sA[mb] = r.out_sA[d] << b; r.mbit_sC[mb] = r.out_sC[d] << b; ++mb;
        } else {
          if (nb >= 10) { ok = false; break; }
          r.nbit_sB[nb] = r.out_sB[d] << b; r.nbit_sC[nb] = r.out_sC[d] << b; ++nb;
        }
      }
    }
    r.fast = (ok && mb >= 5 && !c128) ? 1 : 0; // (complex128: the general path only)
    r.n_mbits = r.fast ? mb : 0; r.n_nbits = r.fast ? nb : 0;
  }
  for (int s = 0; s < n_steps; ++s)
    for (int which = 0; which < 2; ++which) {
      const int64_t loc = which ? loc_b[s] : loc_a[s];
      if (loc >= 0) last_use[producer[loc]] = std::max(last_use[producer[loc]], level[s]);
    }
  std::vector<int> order(n_steps), where(n_steps);
  for (int s = 0; s < n_steps; ++s) order[s] = s;
  std::stable_sort(order.begin(), order.end(), [&](int x, int y) {
    return group_of[x] != group_of[y] ? group_of[x] < group_of[y] : level[x] < level[y];
  });
  for (int q = 0; q < n_steps; ++q) where[order[q]] = q;
  // ---- per group: reduction tables, the LDS arena (first fit; a block is freed after its last consumer's level)
  struct Block { int off, size; };
  std::vector<ArtnProgGroup> groups(n_groups);
  std::vector<ArtnProgLevel> levels;
  std::vector<ArtnProgWTask> wtasks;
  for (int g = 0; g < n_groups; ++g) {
    const int b = group_start[g], e = group_start[g + 1];
    std::vector<int> steps(order.begin() + b, order.begin() + e); // by level
    int red = 0;
    int n_fast = 0;
    for (int s : steps) {
      rec[s].red_base = red; red += rec[s].red_numel; rec[s].level = level[s];
      if (rec[s].fast) {
        if (n_fast < ARTN_PROG_FAST_MAX) rec[s].fast_index = n_fast++;
        else rec[s].fast = 0; // (the general path takes what the bit-stride area cannot hold)
      }
    }
    if (red > ARTN_PROG_RED_ENTRIES) return fail(ARTN_E_UNSUPPORTED, "reduction tables of a group exceed their LDS share");
    std::vector<Block> free_list = {{0, ARTN_PROG_ARENA_BYTES}};
    // (two-ended: blocks of 16 KiB and more from the top of the arena, the many small ones from the bottom -- with
    //  one first-fit list the long-lived leaves of n12 left no room for the second 32 KiB buffer of its stem)
    auto alloc = [&](int bytes) {
      bytes = (bytes + 15) / 16 * 16;
      if (bytes >= 16384) {
        for (size_t i = free_list.size(); i-- > 0;)
          if (free_list[i].size >= bytes) {
            free_list[i].size -= bytes;
            const int off = free_list[i].off + free_list[i].size;
            if (free_list[i].size == 0) free_list.erase(free_list.begin() + i);
            return off;
          }
        return -1;
      }
      for (size_t i = 0; i < free_list.size(); ++i)
        if (free_list[i].size >= bytes) {
          const int off = free_list[i].off;
          free_list[i].off += bytes; free_list[i].size -= bytes;
          if (free_list[i].size == 0) free_list.erase(free_list.begin() + i);
          return off;
        }
      return -1;
    };
    auto release = [&](int off, int bytes) {
      bytes = (bytes + 15) / 16 * 16;
      size_t i = 0;
      while (i < free_list.size() && free_list[i].off < off) ++i;
      free_list.insert(free_list.begin() + i, {off, bytes});
      for (size_t k = 0; k + 1 < free_list.size();)
        if (free_list[k].off + free_list[k].size == free_list[k + 1].off) { free_list[k].size += free_list[k + 1].size; free_list.erase(free_list.begin() + k + 1); }
        else ++k;
    };
    const int max_level = steps.empty() ? 0 : level[steps.back()];
    // external operands (live from the start to their last reader)
    struct Ext { int lds, numel, last; };
    std::map<int64_t, Ext> exts;
    for (int s : steps)
      for (int which = 0; which < 2; ++which) {
        const int64_t loc = which ? loc_b[s] : loc_a[s];
        if (loc >= 0) continue;
        const int numel = which ? rec[s].b_numel : rec[s].a_numel;
        auto it = exts.find(loc);
        if (it == exts.end()) {
          Ext x = {-1, numel, level[s]};
          if (numel <= ARTN_PROG_PRELOAD_MAX) x.lds = alloc(numel * (int)esz);
          if (x.lds >= 0) (which ? rec[s].pre_b : rec[s].pre_a) = 1;
          it = exts.insert({loc, x}).first;
        } else if (it->second.numel != numel) {
          return fail(ARTN_E_INVALID, "an external operand is used with two sizes");
        }
        it->second.last = std::max(it->second.last, level[s]);
        (which ? rec[s].lds_b : rec[s].lds_a) = it->second.lds;
      }
    groups[g].step_begin = b; groups[g].step_end = e;
    groups[g].level_begin = (int)levels.size();
    size_t q = 0;
    for (int L = 1; L <= max_level; ++L) {
      ArtnProgLevel lv = {(int)wtasks.size(), 0, 0, 0};
      const size_t q0 = q;
      for (; q < steps.size() && level[steps[q]] == L; ++q) {
        const int s = steps[q];
        ArtnProgStep &r = rec[s];
        const bool read_inside = last_use[s] > 0; // (through the arena)
        r.to_ws = (!keep || keep[s] || !read_inside) ? 1 : 0;
        if (read_inside) r.lds_c = alloc(r.out_numel * (int)esz);
        if (r.lds_c < 0) r.to_ws = 1;
        if (r.fast) { // 32 x 16 blocks: first-operand sub-tile fastest
          const int n_tasks = (1 << (r.n_mbits - 5)) * (r.n_nbits > 4 ? 1 << (r.n_nbits - 4) : 1);
          for (int t = 0; t < n_tasks; ++t) wtasks.push_back({where[s], t});
        } else {
          for (int first = 0; first < r.out_numel; first += ARTN_PROG_TASK_ELEMS) wtasks.push_back({where[s], first});
        }
      }
      lv.wt_count = (int)wtasks.size() - lv.wt_begin;
      lv.first_step = lv.wt_count ? wtasks[lv.wt_begin].step : 0;
      levels.push_back(lv);
      // operands whose last reader ran at this level
      for (size_t k = q0; k < q; ++k) {
        const int s = steps[k];
        for (int which = 0; which < 2; ++which) {
          const int64_t loc = which ? loc_b[s] : loc_a[s];
          if (loc < 0) {
            Ext &x = exts[loc];
            if (x.lds >= 0 && x.last == L) { release(x.lds, x.numel * (int)esz); x.last = -1; }
          } else {
            const int p = producer[loc];
            (which ? rec[s].lds_b : rec[s].lds_a) = rec[p].lds_c;
            if (rec[p].lds_c >= 0 && last_use[p] == L) { release(rec[p].lds_c, rec[p].out_numel * (int)esz); last_use[p] = -1; }
          }
        }
      }
    }
    groups[g].level_end = (int)levels.size();
  }
  ArtnProgHeader h;
  memset(&h, 0, sizeof(h));
  h.magic = ARTN_PROG_MAGIC; h.n_groups = n_groups; h.n_steps = n_steps; h.n_levels = (int32_t)levels.size(); h.n_wtasks = (int32_t)wtasks.size();
  int64_t n_terms = 0;
  for (int s = 0; s < n_steps; ++s) n_terms += rec[s].red_numel;
  const int64_t need = prog_image_layout(n_steps, n_groups, (int64_t)levels.size(), (int64_t)wtasks.size(), n_terms, &h);
  if (need > image_bytes) return fail(ARTN_E_INVALID, "image buffer too small (artn_program_image_bytes)");
  char *img = (char *)host_image;
  memset(img, 0, (size_t)need);
  memcpy(img, &h, sizeof(h));
  if (n_groups) memcpy(img + h.off_groups, groups.data(), groups.size() * sizeof(ArtnProgGroup));
  if (!levels.empty()) memcpy(img + h.off_levels, levels.data(), levels.size() * sizeof(ArtnProgLevel));
  if (!wtasks.empty()) memcpy(img + h.off_wtasks, wtasks.data(), wtasks.size() * sizeof(ArtnProgWTask));
  {
    int64_t toff = h.off_tables;
    for (int s = 0; s < n_steps; ++s) {
      ArtnProgStep &r = rec[s];
      r.tab_off = toff;
      int32_t *tab = (int32_t *)(img + toff);
      for (int q = 0; q < r.red_numel; ++q) {
        int rr = q, ka = 0, kb = 0;
        for (int d = 0; d < r.n_red; ++d) {
          const int x = rr % r.red_ext[d];
          rr /= r.red_ext[d];
          ka += x * r.red_sA[d];
          kb += x * r.red_sB[d];
        }
        tab[2 * q] = ka; tab[2 * q + 1] = kb;
      }
      toff += (int64_t)r.red_numel * 8;
    }
  }
  for (int q = 0; q < n_steps; ++q) memcpy(img + h.off_records + (int64_t)q * sizeof(ArtnProgStep), &rec[order[q]], sizeof(ArtnProgStep));
  return ARTN_OK;
}

int artn_program_run(const void *dev_image, int32_t n_groups, const void *const *ext, int32_t n_ext, void *workspace, int32_t dtype,
                     void *stream) {
  if (artn_device_count() < 1) return fail(ARTN_E_NODEVICE, "no gfx950 device visible");
  if (n_groups < 0 || n_ext < 0 || n_ext > ARTN_PROGRAM_MAX_EXT) return fail(ARTN_E_INVALID, "bad group or pointer count");
  if (n_groups == 0) return ARTN_OK;
  if (!dev_image || !workspace || (n_ext && !ext)) return fail(ARTN_E_INVALID, "null pointer");
  ArtnExtPtrs e;
  memset(&e, 0, sizeof(e));
  for (int i = 0; i < n_ext; ++i) e.p[i] = ext[i];
  if (dtype == ARTN_C128) {
    HIP_TRY(ensure_lds<artn_k_program<double>>(ARTN_PROG_LDS_BYTES));
    hipLaunchKernelGGL(artn_k_program<double>, dim3(n_groups), dim3(1024), ARTN_PROG_LDS_BYTES, (hipStream_t)stream, (const char *)dev_image, e,
                       (char *)workspace);
  } else if (dtype == ARTN_C64 || dtype == ARTN_C64_BF16) {
    HIP_TRY(ensure_lds<artn_k_program<float>>(ARTN_PROG_LDS_BYTES));
    hipLaunchKernelGGL(artn_k_program<float>, dim3(n_groups), dim3(1024), ARTN_PROG_LDS_BYTES, (hipStream_t)stream, (const char *)dev_image, e,
                       (char *)workspace);
  } else {
    return fail(ARTN_E_INVALID, "dtype must be ARTN_C64, ARTN_C64_BF16 or ARTN_C128");
  }
  HIP_TRY(hipGetLastError());
  return ARTN_OK;
}

int artn_gather_rows(const void *src, const int64_t *idx, void *dst, int64_t nrows, int64_t row_bytes,
                     int64_t src_rows, int32_t *err_flag, void *stream) {
  if (artn_device_count() < 1) return fail(ARTN_E_NODEVICE, "no gfx950 device visible");
  if (nrows < 0 || row_bytes <= 0 || (row_bytes & 7)) return fail(ARTN_E_INVALID, "row_bytes must be a positive multiple of 8");
  if (nrows == 0) return ARTN_OK;
  if (!src || !idx || !dst) return fail(ARTN_E_INVALID, "null pointer");
  hipStream_t st = (hipStream_t)stream;
  const bool v16 = (row_bytes % 16 == 0) && ((((uintptr_t)src | (uintptr_t)dst) & 15) == 0);
  const long vecs = v16 ? row_bytes / 16 : row_bytes / 8;
  const long total = nrows * vecs;
  const int grid = (int)std::min<long>((total + ARTN_WG_THREADS - 1) / ARTN_WG_THREADS, 256L * 8);
  if (v16)
    hipLaunchKernelGGL((artn_k_gather_rows<float4>), dim3(grid), dim3(ARTN_WG_THREADS), 0, st,
                       (const float4 *)src, idx, (float4 *)dst, (long)nrows, vecs, (long)src_rows, err_flag);
  else
    hipLaunchKernelGGL((artn_k_gather_rows<float2>), dim3(grid), dim3(ARTN_WG_THREADS), 0, st,
                       (const float2 *)src, idx, (float2 *)dst, (long)nrows, vecs, (long)src_rows, err_flag);
  HIP_TRY(hipGetLastError());
  return ARTN_OK;
}

int artn_axpy_c64(void *acc, const void *x, int64_t n, void *stream) {
  if (artn_device_count() < 1) return fail(ARTN_E_NODEVICE, "no gfx950 device visible");
  if (n < 0) return fail(ARTN_E_INVALID, "negative length");
  if (n == 0) return ARTN_OK;
  if (!acc || !x) return fail(ARTN_E_INVALID, "null pointer");
  hipStream_t st = (hipStream_t)stream;
  const bool v16 = (n % 2 == 0) && ((((uintptr_t)acc | (uintptr_t)x) & 15) == 0);
  if (v16) {
    const long n4 = n / 2;
    const int grid = (int)std::min<long>((n4 + ARTN_WG_THREADS - 1) / ARTN_WG_THREADS, 256L * 8);
    hipLaunchKernelGGL(artn_k_axpy4, dim3(grid), dim3(ARTN_WG_THREADS), 0, st, (float4 *)acc, (const float4 *)x, n4);
  } else {
    const long n1 = n * 2;
    const int grid = (int)std::min<long>((n1 + ARTN_WG_THREADS - 1) / ARTN_WG_THREADS, 256L * 8);
    hipLaunchKernelGGL(artn_k_axpy1, dim3(grid), dim3(ARTN_WG_THREADS), 0, st, (float *)acc, (const float *)x, n1);
  }
  HIP_TRY(hipGetLastError());
  return ARTN_OK;
}

int artn_sum_axis_c64(const void *in, void *out, int64_t n_groups, int64_t n_rows, int64_t n_cols, void *stream) {
  if (artn_device_count() < 1) return fail(ARTN_E_NODEVICE, "no gfx950 device visible");
  if (n_groups < 0 || n_rows < 1 || n_cols < 0) return fail(ARTN_E_INVALID, "bad extent");
  if (n_groups == 0 || n_cols == 0) return ARTN_OK;
  if (!in || !out) return fail(ARTN_E_INVALID, "null pointer");
  if ((((uintptr_t)in | (uintptr_t)out) & 7) != 0) return fail(ARTN_E_UNSUPPORTED, "artn_sum_axis_c64 needs 8-byte aligned buffers");
  if ((n_cols & 1) || ((((uintptr_t)in | (uintptr_t)out) & 15) != 0)) {
    // an odd column count (3^12 amplitudes of a bond-dimension-3 network) or buffers that are only 8-byte aligned: one element per lane
    const long col_tiles = (n_cols + 63) / 64;
    if (n_groups * col_tiles > (1L << 30)) return fail(ARTN_E_UNSUPPORTED, "too many workgroups");
    hipLaunchKernelGGL(artn_k_sum_axis<v2f_t>, dim3((unsigned)(n_groups * col_tiles)), dim3(ARTN_WG_THREADS), 0, (hipStream_t)stream,
                       (const v2f_t *)in, (v2f_t *)out, (long)n_rows, (long)n_cols, col_tiles);
    HIP_TRY(hipGetLastError());
    return ARTN_OK;
  }
  const long n4 = n_cols / 2, col_tiles = (n4 + 63) / 64;
  if (n_groups * col_tiles > (1L << 30)) return fail(ARTN_E_UNSUPPORTED, "too many workgroups");
  hipLaunchKernelGGL(artn_k_sum_axis<f32x4>, dim3((unsigned)(n_groups * col_tiles)), dim3(ARTN_WG_THREADS), 0, (hipStream_t)stream,
                     (const f32x4 *)in, (f32x4 *)out, (long)n_rows, n4, col_tiles);
  HIP_TRY(hipGetLastError());
  return ARTN_OK;
}

int artn_sum_axis_c128(const void *in, void *out, int64_t n_groups, int64_t n_rows, int64_t n_cols, void *stream) {
  if (artn_device_count() < 1) return fail(ARTN_E_NODEVICE, "no gfx950 device visible");
  if (n_groups < 0 || n_rows < 1 || n_cols < 0) return fail(ARTN_E_INVALID, "bad extent");
  if (n_groups == 0 || n_cols == 0) return ARTN_OK;
  if (!in || !out) return fail(ARTN_E_INVALID, "null pointer");
  if ((((uintptr_t)in | (uintptr_t)out) & 15) != 0) return fail(ARTN_E_UNSUPPORTED, "artn_sum_axis_c128 needs 16-byte aligned buffers");
  const long col_tiles = (n_cols + 63) / 64;
  if (n_groups * col_tiles > (1L << 30)) return fail(ARTN_E_UNSUPPORTED, "too many workgroups");
  hipLaunchKernelGGL(artn_k_sum_axis<f64x2>, dim3((unsigned)(n_groups * col_tiles)), dim3(ARTN_WG_THREADS), 0, (hipStream_t)stream,
                     (const f64x2 *)in, (f64x2 *)out, (long)n_rows, (long)n_cols, col_tiles);
  HIP_TRY(hipGetLastError());
  return ARTN_OK;
}

int artn_axpy_c128(void *acc, const void *x, int64_t n, void *stream) {
  if (artn_device_count() < 1) return fail(ARTN_E_NODEVICE, "no gfx950 device visible");
  if (n < 0) return fail(ARTN_E_INVALID, "negative length");
  if (n == 0) return ARTN_OK;
  if (!acc || !x) return fail(ARTN_E_INVALID, "null pointer");
  if ((((uintptr_t)acc | (uintptr_t)x) & 15) != 0) return fail(ARTN_E_UNSUPPORTED, "artn_axpy_c128 needs 16-byte aligned buffers");
  const int grid = (int)std::min<long>((n + ARTN_WG_THREADS - 1) / ARTN_WG_THREADS, 256L * 8);
  hipLaunchKernelGGL(artn_k_axpy_v<f64x2>, dim3(grid), dim3(ARTN_WG_THREADS), 0, (hipStream_t)stream, (f64x2 *)acc, (const f64x2 *)x, (long)n);
  HIP_TRY(hipGetLastError());
  return ARTN_OK;
}

int artn_probe_mfma_rate(int kind, void *scratch4, double *tflops) {
  if (artn_device_count() < 1) return fail(ARTN_E_NODEVICE, "no gfx950 device visible");
  if (kind < 0 || kind > 2 || !scratch4 || !tflops) return fail(ARTN_E_INVALID, "bad argument");
  const int iters = 20000, waves_per_cu = 8;
  const double flop_per_mfma[3] = {4096.0, 32768.0, 2048.0}, per_iter[3] = {2.0, 2.0, 4.0};
  dim3 grid((unsigned)(g_ncu * waves_per_cu / 4)), block(ARTN_WG_THREADS);
  hipEvent_t e0, e1;
  HIP_TRY(hipEventCreate(&e0));
  HIP_TRY(hipEventCreate(&e1));
  float ms = 0.f;
  for (int rep = 0; rep < 2; ++rep) { // (the first launch warms the clocks up)
    HIP_TRY(hipEventRecord(e0, nullptr));
    if (kind == 0) hipLaunchKernelGGL(artn_k_mfma_probe<0>, grid, block, 0, nullptr, (float *)scratch4, iters);
    else if (kind == 1) hipLaunchKernelGGL(artn_k_mfma_probe<1>, grid, block, 0, nullptr, (float *)scratch4, iters);
    else hipLaunchKernelGGL(artn_k_mfma_probe<2>, grid, block, 0, nullptr, (float *)scratch4, iters);
    HIP_TRY(hipEventRecord(e1, nullptr));
    HIP_TRY(hipEventSynchronize(e1));
    HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
  }
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  const double mfmas = (double)g_ncu * waves_per_cu * iters * per_iter[kind];
  *tflops = mfmas * flop_per_mfma[kind] / (ms * 1e-3) / 1e12;
  return ARTN_OK;
}

int artn_absmax_normalize_c64(void *x, int64_t n, float *out_absmax, void *stream) {
  if (artn_device_count() < 1) return fail(ARTN_E_NODEVICE, "no gfx950 device visible");
  if (n <= 0 || !x || !out_absmax) return fail(ARTN_E_INVALID, "bad argument");
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(hipMemsetAsync(out_absmax, 0, sizeof(float), st));
  const int grid = (int)std::min<long>((n + ARTN_WG_THREADS - 1) / ARTN_WG_THREADS, 256L * 8);
  hipLaunchKernelGGL(artn_k_absmax, dim3(grid), dim3(ARTN_WG_THREADS), 0, st, (const float2 *)x, (long)n,
                     (unsigned int *)out_absmax);
  hipLaunchKernelGGL(artn_k_divide, dim3(grid), dim3(ARTN_WG_THREADS), 0, st, (float2 *)x, (long)n,
                     (const float *)out_absmax);
  HIP_TRY(hipGetLastError());
  return ARTN_OK;
}

int artn_absmax_normalize_c128(void *x, int64_t n, double *out_absmax, void *stream) {
  if (artn_device_count() < 1) return fail(ARTN_E_NODEVICE, "no gfx950 device visible");
  if (n <= 0 || !x || !out_absmax) return fail(ARTN_E_INVALID, "bad argument");
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(hipMemsetAsync(out_absmax, 0, sizeof(double), st));
  const int grid = (int)std::min<long>((n + ARTN_WG_THREADS - 1) / ARTN_WG_THREADS, 256L * 8);
  hipLaunchKernelGGL(artn_k_absmax128, dim3(grid), dim3(ARTN_WG_THREADS), 0, st, (const double2 *)x, (long)n,
                     (unsigned long long *)out_absmax);
  hipLaunchKernelGGL(artn_k_divide128, dim3(grid), dim3(ARTN_WG_THREADS), 0, st, (double2 *)x, (long)n,
                     (const double *)out_absmax);
  HIP_TRY(hipGetLastError());
  return ARTN_OK;
}

} // extern "C"
