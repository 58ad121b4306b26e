// artn_pauli.hip -- host half of the Pauli-string entry points of include/artn.h (kernels: artn_pauli_kernel.h for the
// expectation values, artn_pauli_apply_kernel.h for y = H a, artn_pauli_evolve_kernel.h for the in-place circuits,
// artn_pauli_adjoint_kernel.h for the same circuits on two states with transition elements).  What the circuits share with
// the gate circuits of artn_gates.hip -- run records, launchers, apply entries -- is artn_run_circuit_host.h.
//
// A translation unit of its own (build/obj/pauli.o).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <string>
#include <unordered_map>
#include <vector>

#include "artn_host.h"
#include "artn_state_host.h"
#include "artn_pauli_kernel.h"
#include "artn_pauli_apply_kernel.h"
#include "artn_pauli_evolve_kernel.h"
#include "artn_pauli_adjoint_kernel.h"
#include "artn_run_circuit_host.h"

struct PauliPlan {
  int64_t n = 1;
  std::vector<uint64_t> xm, zm;
  std::vector<int32_t> ny, group;
  std::vector<std::vector<int64_t>> members; // group -> its terms, in the caller's order
  ArtnPauliInfo info = {};
};

// The layout checks of artn_marginal (artn_state_host.h) and power-of-two extents, then every term's memory-bit masks and the
// groups of equal xmask in the order they first appear.
static int pauli_plan(const ArtnMarginalDesc *d, const uint8_t *ops, int64_t n_terms, PauliPlan &pl) {
  if (int rc = state_desc(d, "Pauli expectations take", ARTN_MARG_MAX_DIMS, false)) return rc;
  if (n_terms < 1) return fail(ARTN_E_INVALID, "at least one Pauli string is needed");
  if (!ops) return fail(ARTN_E_INVALID, "null pointer");
  const int nd = d->n_dims;
  StateLayout l;
  if (int rc = state_layout(d, l)) return rc;
  if (int rc = state_bits_only(l, "Pauli expectations take")) return rc;
  const int64_t n = pl.n = l.n;
  pl.xm.assign(n_terms, 0), pl.zm.assign(n_terms, 0), pl.ny.assign(n_terms, 0), pl.group.assign(n_terms, 0);
  int bit[ARTN_MARG_MAX_DIMS];
  state_dim_bits(d, bit);
  std::unordered_map<uint64_t, int32_t> group_of;
  for (int64_t t = 0; t < n_terms; ++t) {
    uint64_t x = 0, z = 0;
    int32_t y = 0;
    if (int rc = state_string_masks(d, bit, ops + t * nd, t, x, z, y)) return rc;
    pl.xm[t] = x, pl.zm[t] = z, pl.ny[t] = y;
    auto it = group_of.find(x);
    if (it == group_of.end()) {
      it = group_of.emplace(x, (int32_t)pl.members.size()).first;
      pl.members.emplace_back();
    }
    pl.group[t] = it->second;
    pl.members[it->second].push_back(t);
  }
  int64_t launches = 0;
  for (const auto &m : pl.members) launches += ((int64_t)m.size() + ARTN_PAULI_TERMS - 1) / ARTN_PAULI_TERMS;
  if (pl.members.size() > (size_t)INT32_MAX || launches > INT32_MAX) return fail(ARTN_E_UNSUPPORTED, "too many Pauli strings in one call");
  const int64_t tiles = std::max<int64_t>(n >> ARTN_PAULI_TILE_BITS, 1);
  pl.info.n_groups = (int32_t)pl.members.size();
  pl.info.n_launches = (int32_t)launches;
  pl.info.terms_per_launch = ARTN_PAULI_TERMS;
  pl.info.workspace_bytes = std::min<int64_t>(tiles, ARTN_BORN_MAX_GRID) * (ARTN_PAULI_TERMS + 1) * (int64_t)sizeof(double);
  pl.info.bytes_read = launches * n * (d->dtype == ARTN_C64 ? 8 : 16);
  return ARTN_OK;
}

template <typename T, int FORM>
static void pauli_launch_form(int nt, dim3 grid, hipStream_t st, const T *a, long tiles, const ArtnPauliArgs &p, double *part) {
  const dim3 block(ARTN_BORN_THREADS);
  if (nt <= 1) hipLaunchKernelGGL((artn_k_pauli<T, FORM, 1>), grid, block, 0, st, a, tiles, p, part);
  else if (nt <= 4) hipLaunchKernelGGL((artn_k_pauli<T, FORM, 4>), grid, block, 0, st, a, tiles, p, part);
  else hipLaunchKernelGGL((artn_k_pauli<T, FORM, ARTN_PAULI_TERMS>), grid, block, 0, st, a, tiles, p, part);
}

// one launch of the terms m[first .. first + p.nt) of a group, and its finish
template <typename T>
static void pauli_launch(const PauliPlan &pl, const T *a, ArtnPauliArgs &p, const ArtnPauliFinish &f, double *part, double *out, hipStream_t st) {
  const uint64_t in = ((uint64_t)1 << ARTN_PAULI_TILE_BITS) - 1;
  int n_partial = 1, nv = ARTN_PAULI_TERMS + 1;
  if (pl.n <= (int64_t)in) {
    hipLaunchKernelGGL(artn_k_pauli_small<T>, dim3(1), dim3(ARTN_BORN_THREADS), 0, st, a, (long)pl.n, p, part);
  } else {
    const int form = p.xm == 0 ? 0 : (p.xm & ~in) == 0 ? 1 : 2;
    const long tiles = (long)(pl.n >> ARTN_PAULI_TILE_BITS) >> (form == 2 ? 1 : 0);
    const dim3 grid((unsigned)std::min<long>(tiles, ARTN_BORN_MAX_GRID));
    if (form == 0) pauli_launch_form<T, 0>(p.nt, grid, st, a, tiles, p, part);
    else if (form == 1) pauli_launch_form<T, 1>(p.nt, grid, st, a, tiles, p, part);
    else pauli_launch_form<T, 2>(p.nt, grid, st, a, tiles, p, part);
    n_partial = (int)grid.x;
    nv = (p.nt <= 1 ? 1 : p.nt <= 4 ? 4 : ARTN_PAULI_TERMS) + 1;
  }
  hipLaunchKernelGGL(artn_k_pauli_finish, dim3(1), dim3(64), 0, st, (const double *)part, n_partial, nv, f, out);
}

// y = H a: the groups of a plan in summation order (stable by xm_hi), the folded coefficients, the table.
struct PauliApplyPlan {
  PauliPlan pl;
  std::vector<int32_t> order, pos; // order[p] = the group at position p; pos[g] = the position of group g
  std::vector<double> folded;      // [n_terms][2]: c_k (-i)^ny_k
  ArtnPauliApplyInfo info = {};
};

static int pauli_apply_plan(const ArtnMarginalDesc *d, const uint8_t *ops, const double *coeff, int64_t n_terms, PauliApplyPlan &ap) {
  if (int rc = pauli_plan(d, ops, n_terms, ap.pl)) return rc;
  const PauliPlan &pl = ap.pl;
  const int32_t ng = (int32_t)pl.members.size();
  auto hi = [&](int32_t g) { return pl.xm[pl.members[g][0]] >> ARTN_PAULI_TILE_BITS; };
  ap.order.resize(ng), ap.pos.resize(ng);
  for (int32_t g = 0; g < ng; ++g) ap.order[g] = g;
  std::stable_sort(ap.order.begin(), ap.order.end(), [&](int32_t x, int32_t y) { return hi(x) < hi(y); });
  int32_t n_hi = 0;
  for (int32_t p = 0; p < ng; ++p) {
    ap.pos[ap.order[p]] = p;
    if (p == 0 || hi(ap.order[p]) != hi(ap.order[p - 1])) ++n_hi;
  }
  ap.folded.resize(2 * n_terms);
  for (int64_t t = 0; t < n_terms; ++t) {
    const double re = coeff ? coeff[2 * t] : 1.0, im = coeff ? coeff[2 * t + 1] : 0.0;
    double *f = &ap.folded[2 * t];
    switch (pl.ny[t] & 3) { // c (-i)^ny
    case 0: f[0] = re, f[1] = im; break;
    case 1: f[0] = im, f[1] = -re; break;
    case 2: f[0] = -re, f[1] = -im; break;
    default: f[0] = -im, f[1] = re; break;
    }
  }
  const int64_t elem = d->dtype == ARTN_C64 ? 8 : 16;
  ap.info.n_groups = ng;
  ap.info.n_xmask_hi = n_hi;
  ap.info.n_launches = 1;
  ap.info.table_bytes = (int64_t)sizeof(ArtnPauliApplyHeader) * (1 + (int64_t)ng + n_terms);
  ap.info.bytes_read = ap.info.bytes_written = pl.n * elem;
  return ARTN_OK;
}

template <typename T>
static void pauli_apply_launch(const PauliPlan &pl, const T *a, T *y, const ArtnPauliApplyGroup *grp, const ArtnPauliApplyTerm *trm,
                               int n_groups, hipStream_t st) {
  const dim3 block(ARTN_BORN_THREADS);
  if (pl.n < ((int64_t)1 << ARTN_PAULI_TILE_BITS)) {
    hipLaunchKernelGGL(artn_k_pauli_apply_small<T>, dim3(1), block, 0, st, a, y, (long)pl.n, grp, trm, n_groups);
  } else {
    const long tiles = (long)(pl.n >> ARTN_PAULI_TILE_BITS);
    const dim3 grid((unsigned)std::min<long>(tiles, ARTN_PAULI_APPLY_MAX_GRID));
    hipLaunchKernelGGL(artn_k_pauli_apply<T>, grid, block, 0, st, a, y, tiles, grp, trm, n_groups);
  }
}

extern "C" {

int artn_pauli_apply_query(const ArtnMarginalDesc *d, const uint8_t *ops, const double *coeff, int64_t n_terms,
                           ArtnPauliApplyInfo *info, uint64_t *xmask, uint64_t *zmask, int32_t *n_y, int32_t *group, double *folded,
                           uint64_t *group_xmask, int32_t *group_pos) {
  if (!info) return fail(ARTN_E_INVALID, "null info");
  PauliApplyPlan ap;
  if (int rc = pauli_apply_plan(d, ops, coeff, n_terms, ap)) return rc;
  const PauliPlan &pl = ap.pl;
  *info = ap.info;
  if (xmask) std::copy(pl.xm.begin(), pl.xm.end(), xmask);
  if (zmask) std::copy(pl.zm.begin(), pl.zm.end(), zmask);
  if (n_y) std::copy(pl.ny.begin(), pl.ny.end(), n_y);
  if (group) std::copy(pl.group.begin(), pl.group.end(), group);
  if (folded) std::copy(ap.folded.begin(), ap.folded.end(), folded);
  if (group_xmask)
    for (size_t g = 0; g < pl.members.size(); ++g) group_xmask[g] = pl.xm[pl.members[g][0]];
  if (group_pos) std::copy(ap.pos.begin(), ap.pos.end(), group_pos);
  return ARTN_OK;
}

int artn_pauli_apply_pack(const ArtnMarginalDesc *d, const uint8_t *ops, const double *coeff, int64_t n_terms, void *table,
                          int64_t table_bytes) {
  PauliApplyPlan ap;
  if (int rc = pauli_apply_plan(d, ops, coeff, n_terms, ap)) return rc;
  if (!table) return fail(ARTN_E_INVALID, "null pointer");
  if (int rc = state_table_fits(table_bytes, ap.info.table_bytes, "artn_pauli_apply_query")) return rc;
  if (int rc = state_table_aligned(table, "artn_pauli_apply_pack")) return rc;
  const PauliPlan &pl = ap.pl;
  ArtnPauliApplyHeader *h = (ArtnPauliApplyHeader *)table;
  ArtnPauliApplyGroup *grp = (ArtnPauliApplyGroup *)(h + 1);
  ArtnPauliApplyTerm *trm = (ArtnPauliApplyTerm *)(grp + pl.members.size());
  *h = ArtnPauliApplyHeader{(uint64_t)pl.members.size(), (uint64_t)n_terms, (uint64_t)ap.info.n_xmask_hi, 0};
  uint64_t at = 0;
  for (size_t p = 0; p < ap.order.size(); ++p) {
    const auto &m = pl.members[ap.order[p]];
    grp[p] = ArtnPauliApplyGroup{pl.xm[m[0]], at, (uint64_t)m.size(), 0};
    for (int64_t t : m) trm[at++] = ArtnPauliApplyTerm{pl.zm[t], pl.zm[t] & 3, ap.folded[2 * t], ap.folded[2 * t + 1]};
  }
  return ARTN_OK;
}

int artn_pauli_apply(const ArtnMarginalDesc *d, const void *a, void *y, const uint8_t *ops, int64_t n_terms, const void *table,
                     int64_t table_bytes, void *stream) {
  if (artn_device_count() < 1) return fail(ARTN_E_NODEVICE, "no gfx950 device visible");
  PauliApplyPlan ap;
  if (int rc = pauli_apply_plan(d, ops, nullptr, n_terms, ap)) return rc; // (the coefficients are in the table)
  if (!a || !y || !table) return fail(ARTN_E_INVALID, "null pointer");
  if (int rc = state_table_fits(table_bytes, ap.info.table_bytes, "artn_pauli_apply_query")) return rc;
  if ((((uintptr_t)a | (uintptr_t)y) & 15) != 0) return fail(ARTN_E_UNSUPPORTED, "artn_pauli_apply needs 16-byte aligned arrays");
  if (int rc = state_table_aligned(table, "artn_pauli_apply")) return rc;
  const uintptr_t bytes = (uintptr_t)ap.info.bytes_read, pa = (uintptr_t)a, py = (uintptr_t)y;
  if (pa < py + bytes && py < pa + bytes) return fail(ARTN_E_INVALID, "artn_pauli_apply: y overlaps a (there is no in-place form)");
  const int ng = ap.info.n_groups;
  const ArtnPauliApplyGroup *grp = (const ArtnPauliApplyGroup *)((const ArtnPauliApplyHeader *)table + 1);
  const ArtnPauliApplyTerm *trm = (const ArtnPauliApplyTerm *)(grp + ng);
  hipStream_t st = (hipStream_t)stream;
  if (d->dtype == ARTN_C64) pauli_apply_launch(ap.pl, (const float2 *)a, (float2 *)y, grp, trm, ng, st);
  else pauli_apply_launch(ap.pl, (const double2 *)a, (double2 *)y, grp, trm, ng, st);
  HIP_TRY(hipGetLastError());
  return ARTN_OK;
}

int artn_pauli_query(const ArtnMarginalDesc *d, const uint8_t *ops, int64_t n_terms, ArtnPauliInfo *info, uint64_t *xmask,
                     uint64_t *zmask, int32_t *n_y, int32_t *group) {
  if (!info) return fail(ARTN_E_INVALID, "null info");
  PauliPlan pl;
  if (int rc = pauli_plan(d, ops, n_terms, pl)) return rc;
  *info = pl.info;
  if (xmask) std::copy(pl.xm.begin(), pl.xm.end(), xmask);
  if (zmask) std::copy(pl.zm.begin(), pl.zm.end(), zmask);
  if (n_y) std::copy(pl.ny.begin(), pl.ny.end(), n_y);
  if (group) std::copy(pl.group.begin(), pl.group.end(), group);
  return ARTN_OK;
}

int artn_pauli_expect(const ArtnMarginalDesc *d, const void *a, const uint8_t *ops, int64_t n_terms, double *out, void *ws,
                      int64_t ws_bytes, void *stream) {
  if (artn_device_count() < 1) return fail(ARTN_E_NODEVICE, "no gfx950 device visible");
  PauliPlan pl;
  if (int rc = pauli_plan(d, ops, n_terms, pl)) return rc;
  if (!a || !out || !ws) return fail(ARTN_E_INVALID, "null pointer");
  if (ws_bytes < pl.info.workspace_bytes) return fail(ARTN_E_INVALID, "workspace smaller than artn_pauli_query reports");
  if (int rc = state_array_aligned(a, "artn_pauli_expect")) return rc;
  if ((((uintptr_t)out | (uintptr_t)ws) & 7) != 0) return fail(ARTN_E_UNSUPPORTED, "artn_pauli_expect needs 8-byte aligned output and workspace");
  hipStream_t st = (hipStream_t)stream;
  const bool pair_form = pl.n >= ((int64_t)1 << ARTN_PAULI_TILE_BITS);
  bool first = true;
  for (const auto &m : pl.members) {
    const uint64_t xm = pl.xm[m[0]];
    const bool halved = pair_form && (xm >> ARTN_PAULI_TILE_BITS) != 0; // FORM 2: half the index space, weight 2
    for (size_t at = 0; at < m.size(); at += ARTN_PAULI_TERMS) {
      ArtnPauliArgs p = {};
      ArtnPauliFinish f = {};
      p.xm = xm;
      p.nt = f.nt = (int32_t)std::min<size_t>(ARTN_PAULI_TERMS, m.size() - at);
      p.hbit = xm ? 63 - __builtin_clzll(xm) : 0;
      p.norm = first;
      f.norm_index = first ? n_terms : -1;
      for (int t = 0; t < p.nt; ++t) {
        const int64_t term = m[at + t];
        const int32_t ny = pl.ny[term];
        p.zm[t] = pl.zm[term];
        p.sel[t] = (uint8_t)((pl.zm[term] & 3) | (uint64_t)((ny & 1) << 2));
        f.out_index[t] = term;
        f.scale[t] = (int8_t)(((ny & 3) == 1 || (ny & 3) == 2 ? -1 : 1) * (halved ? 2 : 1));
      }
      if (d->dtype == ARTN_C64) pauli_launch(pl, (const float2 *)a, p, f, (double *)ws, out, st);
      else pauli_launch(pl, (const double2 *)a, p, f, (double *)ws, out, st);
      first = false;
    }
  }
  HIP_TRY(hipGetLastError());
  return ARTN_OK;
}

} // extern "C"

// In-place circuits: the runs of a circuit (include/artn.h: PLAN), their bases and every step's slot mask.
struct PauliEvolveRunPlan {
  int64_t first = 0, count = 0;
  std::vector<uint64_t> basis; // reduced echelon, ascending pivots
  std::vector<int> pivot;
};
struct PauliEvolvePlan {
  PauliPlan pl;
  int64_t n = 1, n_recs = 0; // pl.n and the steps
  std::vector<PauliEvolveRunPlan> runs;
  std::vector<int32_t> run_of, slot_mask;
  ArtnPauliEvolveInfo info = {};
};

// v reduced by the basis; when something is left, it joins (its highest bit is the pivot, cleared from every other vector)
static void pauli_evolve_span_add(std::vector<uint64_t> &basis, std::vector<int> &pivot, uint64_t v) {
  for (size_t j = 0; j < basis.size(); ++j)
    if ((v >> pivot[j]) & 1) v ^= basis[j];
  if (!v) return;
  const int p = 63 - __builtin_clzll(v);
  for (uint64_t &b : basis)
    if ((b >> p) & 1) b ^= v;
  basis.push_back(v), pivot.push_back(p);
}

static int pauli_evolve_plan(const ArtnMarginalDesc *d, const uint8_t *ops, int64_t n_steps, int32_t max_rank, PauliEvolvePlan &ep) {
  if (int rc = pauli_plan(d, ops, n_steps, ep.pl)) return rc;
  const PauliPlan &pl = ep.pl;
  if (int rc = state_max_rank(d->dtype, max_rank, ARTN_PAULI_EVOLVE_MAX_RANK, false, max_rank)) return rc;
  if (n_steps > INT32_MAX) return fail(ARTN_E_UNSUPPORTED, "too many steps in one circuit");
  const int cap = state_rank_cap(pl.n, ARTN_PAULI_TILE_BITS, max_rank);
  const uint64_t in = ((uint64_t)1 << ARTN_PAULI_TILE_BITS) - 1;
  ep.n = pl.n, ep.n_recs = n_steps;
  ep.run_of.assign(n_steps, 0), ep.slot_mask.assign(n_steps, 0);
  PauliEvolveRunPlan cur;
  auto close = [&]() {
    // ascending pivots, then every step's slot mask: bit j = the step's xm_hi at pivot j (each pivot lies in one basis vector)
    std::vector<size_t> idx(cur.basis.size());
    for (size_t j = 0; j < idx.size(); ++j) idx[j] = j;
    std::sort(idx.begin(), idx.end(), [&](size_t x, size_t y) { return cur.pivot[x] < cur.pivot[y]; });
    PauliEvolveRunPlan r = cur;
    for (size_t j = 0; j < idx.size(); ++j) r.basis[j] = cur.basis[idx[j]], r.pivot[j] = cur.pivot[idx[j]];
    for (int64_t k = r.first; k < r.first + r.count; ++k) {
      int32_t m = 0;
      for (size_t j = 0; j < r.pivot.size(); ++j) m |= (int32_t)((pl.xm[k] >> r.pivot[j]) & 1) << j;
      ep.slot_mask[k] = m, ep.run_of[k] = (int32_t)ep.runs.size();
    }
    ep.runs.push_back(r);
  };
  for (int64_t k = 0; k < n_steps; ++k) {
    const uint64_t hi = pl.xm[k] & ~in;
    if (hi) {
      std::vector<uint64_t> b = cur.basis;
      std::vector<int> p = cur.pivot;
      pauli_evolve_span_add(b, p, hi);
      if ((int)b.size() > cap && !cur.basis.empty()) { // (a run always takes its first step with a high flip)
        close();
        cur = PauliEvolveRunPlan();
        cur.first = k;
        pauli_evolve_span_add(cur.basis, cur.pivot, hi);
      } else {
        cur.basis = b, cur.pivot = p;
      }
    }
    ++cur.count;
  }
  close();
  const int64_t elem = d->dtype == ARTN_C64 ? 8 : 16, nr = (int64_t)ep.runs.size();
  ep.info.n_runs = ep.info.n_launches = (int32_t)nr;
  ep.info.max_rank = cap;
  ep.info.table_bytes = (int64_t)sizeof(ArtnPauliEvolveHeader) + nr * (int64_t)sizeof(ArtnPauliEvolveRun) + n_steps * (int64_t)sizeof(ArtnPauliEvolveStep);
  ep.info.bytes_read = ep.info.bytes_written = nr * pl.n * elem;
  return ARTN_OK;
}


// what the shared host half (artn_run_circuit_host.h) reads of the family
struct PauliEvolveFamily {
  using Plan = PauliEvolvePlan;
  using Header = ArtnPauliEvolveHeader;
  using Run = ArtnPauliEvolveRun;
  using Rec = ArtnPauliEvolveStep;
  static constexpr int MAX_RANK = ARTN_PAULI_EVOLVE_MAX_RANK;
  static constexpr long MAX_GRID = ARTN_PAULI_EVOLVE_MAX_GRID;
  static constexpr const char *query = "artn_pauli_evolve_query", *apply = "artn_pauli_evolve";
  static void basis(const PauliEvolveRunPlan &rp, Run &rec) { std::copy(rp.basis.begin(), rp.basis.end(), rec.basis); }
  template <typename T, int R>
  static constexpr auto run = artn_k_pauli_evolve<T, R>;
  template <typename T>
  static constexpr auto small = artn_k_pauli_evolve_small<T>;
};

// the per-step and per-run arrays of a query (any may be NULL)
static void pauli_evolve_report(const PauliEvolvePlan &ep, uint64_t *xmask, uint64_t *zmask, int32_t *n_y, int32_t *run, int32_t *slot_mask,
                                int32_t *run_rank, uint64_t *run_basis, int32_t *run_pivot) {
  const PauliPlan &pl = ep.pl;
  if (xmask) std::copy(pl.xm.begin(), pl.xm.end(), xmask);
  if (zmask) std::copy(pl.zm.begin(), pl.zm.end(), zmask);
  if (n_y) std::copy(pl.ny.begin(), pl.ny.end(), n_y);
  run_circuit_report<PauliEvolveFamily>(ep, run, slot_mask, run_rank, run_pivot);
  for (size_t r = 0; run_basis && r < ep.runs.size(); ++r)
    for (size_t j = 0; j < ARTN_PAULI_EVOLVE_MAX_RANK; ++j)
      run_basis[r * ARTN_PAULI_EVOLVE_MAX_RANK + j] = j < ep.runs[r].basis.size() ? ep.runs[r].basis[j] : 0;
}

// the table of include/artn.h into host memory (at least ep.info.table_bytes)
static void pauli_evolve_fill(const PauliEvolvePlan &ep, const double *coeff, void *table) {
  const PauliPlan &pl = ep.pl;
  const uint64_t in = ((uint64_t)1 << ARTN_PAULI_TILE_BITS) - 1;
  ArtnPauliEvolveRun *runs;
  ArtnPauliEvolveStep *stp;
  state_table_parts<ArtnPauliEvolveHeader>(table, ep.runs.size(), runs, stp);
  run_circuit_fill_runs<PauliEvolveFamily>(ep, table, runs);
  for (int64_t k = 0; k < ep.n_recs; ++k) {
    // (below one tile the small kernel reads the whole xmask here: it has no bits above the tile)
    stp[k] = ArtnPauliEvolveStep{pl.xm[k] & in, (uint64_t)ep.slot_mask[k], pl.zm[k], (uint64_t)pl.ny[k],
                                 coeff[4 * k], coeff[4 * k + 1], coeff[4 * k + 2], coeff[4 * k + 3]};
  }
}

extern "C" {

int artn_pauli_evolve_query(const ArtnMarginalDesc *d, const uint8_t *ops, const double *coeff, int64_t n_steps, int32_t max_rank,
                            ArtnPauliEvolveInfo *info, uint64_t *xmask, uint64_t *zmask, int32_t *n_y, int32_t *run,
                            int32_t *slot_mask, int32_t *run_rank, uint64_t *run_basis, int32_t *run_pivot) {
  if (!info) return fail(ARTN_E_INVALID, "null info");
  if (!coeff) return fail(ARTN_E_INVALID, "null pointer");
  PauliEvolvePlan ep;
  if (int rc = pauli_evolve_plan(d, ops, n_steps, max_rank, ep)) return rc;
  *info = ep.info;
  pauli_evolve_report(ep, xmask, zmask, n_y, run, slot_mask, run_rank, run_basis, run_pivot);
  return ARTN_OK;
}

int artn_pauli_evolve_pack(const ArtnMarginalDesc *d, const uint8_t *ops, const double *coeff, int64_t n_steps, int32_t max_rank,
                           void *table, int64_t table_bytes) {
  PauliEvolvePlan ep;
  if (int rc = pauli_evolve_plan(d, ops, n_steps, max_rank, ep)) return rc;
  if (!table || !coeff) return fail(ARTN_E_INVALID, "null pointer");
  if (int rc = state_table_fits(table_bytes, ep.info.table_bytes, "artn_pauli_evolve_query")) return rc;
  if (int rc = state_table_aligned(table, "artn_pauli_evolve_pack")) return rc;
  pauli_evolve_fill(ep, coeff, table);
  return ARTN_OK;
}

int artn_pauli_evolve(const ArtnMarginalDesc *d, void *a, const uint8_t *ops, int64_t n_steps, int32_t max_rank, const void *table,
                      int64_t table_bytes, void *stream) {
  return run_circuit_apply<PauliEvolveFamily>(d, a, table, table_bytes, stream, [&](PauliEvolvePlan &ep) {
    return pauli_evolve_plan(d, ops, n_steps, max_rank, ep); // (the coefficients are in the table)
  });
}

} // extern "C"

// The same circuits on two states with transition elements (include/artn.h: ADJOINT; kernels: artn_pauli_adjoint_kernel.h).
// The plan is pauli_evolve_plan at the two-state rank; only the limits, the byte counts and the workspace are the adjoint's own.
struct PauliAdjointPlan {
  PauliEvolvePlan one;
  ArtnPauliAdjointInfo info = {};
};
struct PauliAdjointFamily {
  using One = PauliEvolveFamily;
  using Plan = PauliAdjointPlan;
  using Info = ArtnPauliAdjointInfo;
  using Rec = ArtnPauliEvolveStep;
  static constexpr int MAX_RANK = ARTN_PAULI_ADJOINT_MAX_RANK;
  static constexpr const char *query = "artn_pauli_adjoint_query", *apply = "artn_pauli_adjoint";
  template <typename T, int R>
  static constexpr auto run = artn_k_pauli_adjoint<T, R>;
  template <typename T>
  static constexpr auto small = artn_k_pauli_adjoint_small<T>;
  static constexpr auto finish = artn_k_pauli_adjoint_finish;
};

static int pauli_adjoint_plan(const ArtnMarginalDesc *d, const uint8_t *ops, const uint8_t *measure, int64_t n_steps, int32_t max_rank,
                              PauliAdjointPlan &ap) {
  if (int rc = run_pair_rank<PauliAdjointFamily>(d, max_rank)) return rc;
  if (int rc = pauli_evolve_plan(d, ops, n_steps, max_rank, ap.one)) return rc;
  run_pair_info<PauliAdjointFamily>(ap, measure ? std::count_if(measure, measure + n_steps, [](uint8_t f) { return f != 0; }) : n_steps);
  ap.info.table_bytes = ap.one.info.table_bytes;
  return ARTN_OK;
}

extern "C" {

int artn_pauli_adjoint_query(const ArtnMarginalDesc *d, const uint8_t *ops, const double *coeff, const uint8_t *measure, int64_t n_steps,
                             int32_t max_rank, ArtnPauliAdjointInfo *info, uint64_t *xmask, uint64_t *zmask, int32_t *n_y, int32_t *run,
                             int32_t *slot_mask, int32_t *run_rank, uint64_t *run_basis, int32_t *run_pivot) {
  if (!info) return fail(ARTN_E_INVALID, "null info");
  if (!coeff) return fail(ARTN_E_INVALID, "null pointer");
  PauliAdjointPlan ap;
  if (int rc = pauli_adjoint_plan(d, ops, measure, n_steps, max_rank, ap)) return rc;
  *info = ap.info;
  pauli_evolve_report(ap.one, xmask, zmask, n_y, run, slot_mask, run_rank, run_basis, run_pivot);
  return ARTN_OK;
}

int artn_pauli_adjoint_pack(const ArtnMarginalDesc *d, const uint8_t *ops, const double *coeff, const uint8_t *measure, int64_t n_steps,
                            int32_t max_rank, void *table, int64_t table_bytes) {
  PauliAdjointPlan ap;
  if (int rc = pauli_adjoint_plan(d, ops, measure, n_steps, max_rank, ap)) return rc;
  if (!table || !coeff) return fail(ARTN_E_INVALID, "null pointer");
  if (int rc = state_table_fits(table_bytes, ap.info.table_bytes, "artn_pauli_adjoint_query")) return rc;
  if (int rc = state_table_aligned(table, "artn_pauli_adjoint_pack")) return rc;
  const PauliEvolvePlan &ep = ap.one;
  pauli_evolve_fill(ep, coeff, table);
  ArtnPauliEvolveRun *runs;
  ArtnPauliEvolveStep *stp;
  state_table_parts<ArtnPauliEvolveHeader>(table, ep.runs.size(), runs, stp);
  for (int64_t k = 0; k < n_steps; ++k) { // n_y, the measure flag and the rank of the step's run share a word
    const uint64_t flag = !measure || measure[k] ? 1 : 0, rank = (uint64_t)ep.runs[ep.run_of[k]].basis.size();
    stp[k].n_y |= flag << 8 | rank << 16;
  }
  return ARTN_OK;
}

int artn_pauli_adjoint(const ArtnMarginalDesc *d, void *lam, void *phi, const uint8_t *ops, int64_t n_steps, int32_t max_rank,
                       const void *table, int64_t table_bytes, void *workspace, int64_t workspace_bytes, double *out, void *stream) {
  return run_pair_apply<PauliAdjointFamily>(d, lam, phi, table, table_bytes, workspace, workspace_bytes, out, stream, [&](PauliAdjointPlan &ap) {
    return pauli_adjoint_plan(d, ops, nullptr, n_steps, max_rank, ap); // (coefficients and flags are in the table)
  });
}

} // extern "C"
