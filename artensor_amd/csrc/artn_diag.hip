// artn_diag.hip -- host half of the diagonal-operator entry points artn_diag_* of include/artn.h (kernels: artn_diag_kernel.h).
//
// A translation unit of its own (build/obj/diag.o).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <string>
#include <unordered_map>
#include <vector>

#include "artn_host.h"
#include "artn_state_host.h"
#include "artn_diag_kernel.h"

static_assert(sizeof(ArtnDiagTable) == 64 && sizeof(ArtnDiagGroup) == 32 && sizeof(ArtnDiagTerm) == 16, "the table's records");
static_assert(ARTN_DIAG_MAX_GROUPS * 4 <= ARTN_BORN_THREADS, "thread 4g forms w_g");

struct DiagPlan {
  int64_t n = 1;
  int tb = 0;
  std::vector<uint64_t> zm;
  std::vector<int32_t> group;                // -1: static
  std::vector<uint64_t> group_lo;            // in the order the groups first appear
  std::vector<std::vector<int64_t>> members; // group -> its terms, in the caller's order
  ArtnDiagInfo info = {};
};

// The layout checks of artn_pauli_query, then every term's mask, static or dynamic, and the groups of equal lo.
static int diag_plan(const ArtnMarginalDesc *d, const uint8_t *ops, int64_t n_terms, DiagPlan &dp) {
  const char *who = "diagonal operators take";
  if (int rc = state_desc(d, who, ARTN_MARG_MAX_DIMS, false)) return rc;
  if (n_terms < 1) return fail(ARTN_E_INVALID, "at least one term is needed");
  if (n_terms > ARTN_DIAG_MAX_TERMS)
    return fail(ARTN_E_UNSUPPORTED, std::string(who) + " at most " + std::to_string(ARTN_DIAG_MAX_TERMS) + " terms, not " + std::to_string((long long)n_terms));
  if (!ops) return fail(ARTN_E_INVALID, "null pointer");
  StateLayout l;
  if (int rc = state_layout(d, l)) return rc;
  if (int rc = state_bits_only(l, who)) return rc;
  const int64_t n = dp.n = l.n;
  const int n_bits = __builtin_ctzll((uint64_t)n);
  const int tb = dp.tb = std::min(ARTN_DIAG_TILE_BITS, n_bits);
  const uint64_t in = ((uint64_t)1 << tb) - 1;
  dp.zm.assign(n_terms, 0), dp.group.assign(n_terms, -1);
  int bit[ARTN_MARG_MAX_DIMS];
  state_dim_bits(d, bit);
  std::unordered_map<uint64_t, int32_t> group_of;
  int64_t n_dynamic = 0;
  for (int64_t t = 0; t < n_terms; ++t) {
    uint64_t x = 0, z = 0;
    int32_t y = 0;
    if (int rc = state_string_masks(d, bit, ops + t * d->n_dims, t, x, z, y)) return rc;
    if (x) return fail(ARTN_E_INVALID, "term " + std::to_string(t) + ": a diagonal operator holds I and Z only, not X or Y");
    dp.zm[t] = z;
    if ((z >> tb) == 0) continue;
    ++n_dynamic;
    auto it = group_of.find(z & in);
    if (it == group_of.end()) {
      it = group_of.emplace(z & in, (int32_t)dp.members.size()).first;
      dp.members.emplace_back();
      dp.group_lo.push_back(z & in);
    }
    dp.group[t] = it->second;
    dp.members[it->second].push_back(t);
  }
  const int64_t ng = (int64_t)dp.members.size();
  if (ng > ARTN_DIAG_MAX_GROUPS)
    return fail(ARTN_E_UNSUPPORTED, "the terms above the tile form " + std::to_string((long long)ng) + " groups of equal low bits; " + who +
                                        " at most " + std::to_string(ARTN_DIAG_MAX_GROUPS));
  const int64_t elem = d->dtype == ARTN_C64 ? 8 : 16, tiles = n >> tb;
  ArtnDiagInfo &di = dp.info;
  di.n_terms = (int32_t)n_terms, di.n_dynamic = (int32_t)n_dynamic, di.n_static = (int32_t)(n_terms - n_dynamic), di.n_groups = (int32_t)ng;
  di.tile_bits = tb, di.n_tiles = tiles;
  di.table_bytes = (int64_t)sizeof(ArtnDiagTable) + ((int64_t)8 << tb) + ng * (int64_t)sizeof(ArtnDiagGroup) + n_dynamic * (int64_t)sizeof(ArtnDiagTerm);
  di.workspace_bytes = std::min<int64_t>(tiles, ARTN_BORN_MAX_GRID) * 4 * (int64_t)sizeof(double);
  const int64_t state = n * elem;
  di.bytes_read[ARTN_DIAG_OP_VALUES] = 0, di.bytes_written[ARTN_DIAG_OP_VALUES] = n * 8;
  di.bytes_read[ARTN_DIAG_OP_EXPECT] = state, di.bytes_written[ARTN_DIAG_OP_EXPECT] = 0;
  di.bytes_read[ARTN_DIAG_OP_PHASE] = di.bytes_written[ARTN_DIAG_OP_PHASE] = state;
  di.bytes_read[ARTN_DIAG_OP_MULTIPLY] = di.bytes_written[ARTN_DIAG_OP_MULTIPLY] = state;
  di.bytes_read[ARTN_DIAG_OP_PAIR] = di.bytes_written[ARTN_DIAG_OP_PAIR] = 2 * state;
  return ARTN_OK;
}

template <typename T, int OP>
static void diag_launch_op(const DiagPlan &dp, T *a, T *b, const void *table, double gamma, double *out, hipStream_t st) {
  const dim3 grid((unsigned)std::min<int64_t>(dp.info.n_tiles, ARTN_BORN_MAX_GRID)), block(ARTN_BORN_THREADS);
  hipLaunchKernelGGL((artn_k_diag<T, OP>), grid, block, 0, st, a, b, (const ArtnDiagTable *)table, dp.tb, (long)dp.info.n_tiles,
                     (int)dp.info.n_groups, gamma, out);
}

template <typename T>
static void diag_launch(int op, const DiagPlan &dp, void *a, void *b, const void *table, double gamma, double *out, hipStream_t st) {
  switch (op) {
  case DIAG_VALUES: diag_launch_op<T, DIAG_VALUES>(dp, (T *)a, (T *)b, table, gamma, out, st); break;
  case DIAG_EXPECT: diag_launch_op<T, DIAG_EXPECT>(dp, (T *)a, (T *)b, table, gamma, out, st); break;
  case DIAG_PHASE: diag_launch_op<T, DIAG_PHASE>(dp, (T *)a, (T *)b, table, gamma, out, st); break;
  case DIAG_MULTIPLY: diag_launch_op<T, DIAG_MULTIPLY>(dp, (T *)a, (T *)b, table, gamma, out, st); break;
  case DIAG_PAIR: diag_launch_op<T, DIAG_PAIR>(dp, (T *)a, (T *)b, table, gamma, out, st); break;
  default: diag_launch_op<T, DIAG_PAIR_T>(dp, (T *)a, (T *)b, table, gamma, out, st); break;
  }
}

// the pass, and for the sums (nv > 0) the finish: ws takes the partial rows, out the nv results
static int diag_run(int op, const ArtnMarginalDesc *d, const DiagPlan &dp, void *a, void *b, const void *table, double gamma, double *ws,
                    int nv, double *out, void *stream) {
  hipStream_t st = (hipStream_t)stream;
  double *first = nv ? ws : out;
  if (d->dtype == ARTN_C64) diag_launch<float2>(op, dp, a, b, table, gamma, first, st);
  else diag_launch<double2>(op, dp, a, b, table, gamma, first, st);
  if (nv) {
    const int n_partial = (int)std::min<int64_t>(dp.info.n_tiles, ARTN_BORN_MAX_GRID);
    hipLaunchKernelGGL(artn_k_diag_finish, dim3(1), dim3(ARTN_BORN_THREADS), 0, st, (const double *)ws, n_partial, nv, out);
  }
  HIP_TRY(hipGetLastError());
  return ARTN_OK;
}

static int diag_table_ok(const DiagPlan &dp, const void *table, int64_t table_bytes, const char *entry) {
  if (int rc = state_table_fits(table_bytes, dp.info.table_bytes, "artn_diag_query")) return rc;
  return state_table_aligned(table, entry);
}
static int diag_workspace_ok(const DiagPlan &dp, const void *ws, int64_t ws_bytes, const double *out, const char *entry) {
  if (ws_bytes < dp.info.workspace_bytes) return fail(ARTN_E_INVALID, "workspace smaller than artn_diag_query reports");
  if ((((uintptr_t)ws | (uintptr_t)out) & 7) != 0)
    return fail(ARTN_E_UNSUPPORTED, std::string(entry) + " needs 8-byte aligned output and workspace");
  return ARTN_OK;
}

extern "C" {

int artn_diag_query(const ArtnMarginalDesc *d, const uint8_t *ops, int64_t n_terms, ArtnDiagInfo *info, uint64_t *zmask,
                    uint64_t *lo, uint64_t *hi, int32_t *group, uint64_t *group_lo) {
  if (!info) return fail(ARTN_E_INVALID, "null info");
  DiagPlan dp;
  if (int rc = diag_plan(d, ops, n_terms, dp)) return rc;
  *info = dp.info;
  const uint64_t in = ((uint64_t)1 << dp.tb) - 1;
  if (zmask) std::copy(dp.zm.begin(), dp.zm.end(), zmask);
  if (lo)
    for (int64_t t = 0; t < n_terms; ++t) lo[t] = dp.zm[t] & in;
  if (hi)
    for (int64_t t = 0; t < n_terms; ++t) hi[t] = dp.zm[t] >> dp.tb;
  if (group) std::copy(dp.group.begin(), dp.group.end(), group);
  if (group_lo) std::copy(dp.group_lo.begin(), dp.group_lo.end(), group_lo);
  return ARTN_OK;
}

int artn_diag_pack(const ArtnMarginalDesc *d, const uint8_t *ops, const double *coeff, int64_t n_terms, void *table,
                   int64_t table_bytes) {
  DiagPlan dp;
  if (int rc = diag_plan(d, ops, n_terms, dp)) return rc;
  if (!coeff || !table) return fail(ARTN_E_INVALID, "null pointer");
  for (int64_t t = 0; t < n_terms; ++t)
    if (!std::isfinite(coeff[t])) return fail(ARTN_E_INVALID, "the coefficient of term " + std::to_string(t) + " is not finite");
  if (int rc = diag_table_ok(dp, table, table_bytes, "artn_diag_pack")) return rc;
  const ArtnDiagInfo &di = dp.info;
  ArtnDiagTable *h = (ArtnDiagTable *)table;
  double *S = (double *)(h + 1);
  ArtnDiagGroup *grp = (ArtnDiagGroup *)(S + ((size_t)1 << dp.tb));
  ArtnDiagTerm *trm = (ArtnDiagTerm *)(grp + di.n_groups);
  *h = ArtnDiagTable{(uint64_t)n_terms, (uint64_t)di.n_static, (uint64_t)di.n_dynamic, (uint64_t)di.n_groups, (uint64_t)dp.tb,
                     (uint64_t)di.n_tiles, {0, 0}};
  // S[l]: the static terms in the caller's order, one plain addition each (the contract of include/artn.h)
  std::vector<int64_t> stat;
  for (int64_t t = 0; t < n_terms; ++t)
    if (dp.group[t] < 0) stat.push_back(t);
  for (uint64_t l = 0; l < ((uint64_t)1 << dp.tb); ++l) {
    volatile double acc = 0.0; // (volatile: one rounded addition per term, whatever the host compiler would like to do)
    for (int64_t t : stat) {
      const double c = coeff[t];
      acc = acc + ((__builtin_popcountll(l & dp.zm[t]) & 1) ? -c : c);
    }
    S[l] = acc;
  }
  uint64_t at = 0;
  for (int32_t g = 0; g < di.n_groups; ++g) {
    const auto &m = dp.members[g];
    grp[g] = ArtnDiagGroup{dp.group_lo[g], at, (uint64_t)m.size(), 0};
    for (int64_t t : m) trm[at++] = ArtnDiagTerm{dp.zm[t] >> dp.tb, coeff[t]};
  }
  return ARTN_OK;
}

int artn_diag_values(const ArtnMarginalDesc *d, const uint8_t *ops, int64_t n_terms, const void *table, int64_t table_bytes,
                     double *out, void *stream) {
  if (artn_device_count() < 1) return fail(ARTN_E_NODEVICE, "no gfx950 device visible");
  DiagPlan dp;
  if (int rc = diag_plan(d, ops, n_terms, dp)) return rc;
  if (!table || !out) return fail(ARTN_E_INVALID, "null pointer");
  if (int rc = diag_table_ok(dp, table, table_bytes, "artn_diag_values")) return rc;
  if (((uintptr_t)out & 7) != 0) return fail(ARTN_E_UNSUPPORTED, "artn_diag_values needs an 8-byte aligned output");
  return diag_run(DIAG_VALUES, d, dp, nullptr, nullptr, table, 0.0, nullptr, 0, out, stream);
}

int artn_diag_expect(const ArtnMarginalDesc *d, const void *a, const uint8_t *ops, int64_t n_terms, const void *table,
                     int64_t table_bytes, void *ws, int64_t ws_bytes, double *out3, void *stream) {
  if (artn_device_count() < 1) return fail(ARTN_E_NODEVICE, "no gfx950 device visible");
  DiagPlan dp;
  if (int rc = diag_plan(d, ops, n_terms, dp)) return rc;
  if (!a || !table || !ws || !out3) return fail(ARTN_E_INVALID, "null pointer");
  if (int rc = diag_table_ok(dp, table, table_bytes, "artn_diag_expect")) return rc;
  if (int rc = diag_workspace_ok(dp, ws, ws_bytes, out3, "artn_diag_expect")) return rc;
  if (int rc = state_array_aligned(a, "artn_diag_expect")) return rc;
  return diag_run(DIAG_EXPECT, d, dp, (void *)a, nullptr, table, 0.0, (double *)ws, 3, out3, stream); // (the pass only reads a)
}

int artn_diag_apply(const ArtnMarginalDesc *d, void *a, const uint8_t *ops, int64_t n_terms, const void *table,
                    int64_t table_bytes, int32_t mode, double gamma, void *stream) {
  if (artn_device_count() < 1) return fail(ARTN_E_NODEVICE, "no gfx950 device visible");
  DiagPlan dp;
  if (int rc = diag_plan(d, ops, n_terms, dp)) return rc;
  if (mode != ARTN_DIAG_PHASE && mode != ARTN_DIAG_MULTIPLY) return fail(ARTN_E_INVALID, "unknown mode " + std::to_string(mode));
  if (mode == ARTN_DIAG_PHASE && !std::isfinite(gamma)) return fail(ARTN_E_INVALID, "gamma is not finite");
  if (!a || !table) return fail(ARTN_E_INVALID, "null pointer");
  if (int rc = diag_table_ok(dp, table, table_bytes, "artn_diag_apply")) return rc;
  if (int rc = state_array_aligned(a, "artn_diag_apply")) return rc;
  if (mode == ARTN_DIAG_PHASE && gamma == 0.0) return ARTN_OK;
  return diag_run(mode == ARTN_DIAG_PHASE ? DIAG_PHASE : DIAG_MULTIPLY, d, dp, a, nullptr, table, gamma, nullptr, 0, nullptr, stream);
}

int artn_diag_pair(const ArtnMarginalDesc *d, void *lam, void *phi, const uint8_t *ops, int64_t n_terms, const void *table,
                   int64_t table_bytes, int32_t mode, double gamma, void *ws, int64_t ws_bytes, double *out2, void *stream) {
  if (artn_device_count() < 1) return fail(ARTN_E_NODEVICE, "no gfx950 device visible");
  DiagPlan dp;
  if (int rc = diag_plan(d, ops, n_terms, dp)) return rc;
  if (mode != ARTN_DIAG_PAIR_EVOLVE && mode != ARTN_DIAG_PAIR_TRANSITION) return fail(ARTN_E_INVALID, "unknown mode " + std::to_string(mode));
  if (!std::isfinite(gamma)) return fail(ARTN_E_INVALID, "gamma is not finite");
  if (!lam || !phi || !table || !ws || !out2) return fail(ARTN_E_INVALID, "null pointer");
  if (int rc = diag_table_ok(dp, table, table_bytes, "artn_diag_pair")) return rc;
  if (int rc = diag_workspace_ok(dp, ws, ws_bytes, out2, "artn_diag_pair")) return rc;
  if ((((uintptr_t)lam | (uintptr_t)phi) & 15) != 0) return fail(ARTN_E_UNSUPPORTED, "artn_diag_pair needs 16-byte aligned arrays");
  if (int rc = state_disjoint(lam, phi, (uintptr_t)dp.info.bytes_read[ARTN_DIAG_OP_PHASE], "artn_diag_pair")) return rc;
  const bool evolve = mode == ARTN_DIAG_PAIR_EVOLVE && gamma != 0.0;
  return diag_run(evolve ? DIAG_PAIR : DIAG_PAIR_T, d, dp, lam, phi, table, gamma, (double *)ws, 2, out2, stream);
}

} // extern "C"
