// artn_gates.hip -- host half of the dense-gate entry points of include/artn.h (kernels: artn_gates_kernel.h; the same circuits on
// two states with transition elements: artn_gates_adjoint_kernel.h).  What the circuits share with the Pauli circuits of
// artn_pauli.hip -- run records, launchers, apply entries -- is artn_run_circuit_host.h.
//
// A translation unit of its own (build/obj/gates.o).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "artn_host.h"
#include "artn_state_host.h"
#include "artn_gates_kernel.h"
#include "artn_gates_adjoint_kernel.h"
#include "artn_run_circuit_host.h"

struct GatesRunPlan {
  int64_t first = 0, count = 0;
  std::vector<int> pivot; // the distinct high target bits, ascending once the run is closed
};
struct GatesPlan {
  int64_t n = 1, n_recs = 0;               // elements; gates
  std::vector<int32_t> k, bits;            // bits: [n_gates][2] in the order the dims are listed, -1 for the absent one
  std::vector<int32_t> run_of, slot_mask, flags;
  std::vector<GatesRunPlan> runs;
  ArtnGatesInfo info = {};
};

// The layout checks of artn_pauli_query (dense, power-of-two extents), then every gate's memory bits and the runs (include/artn.h:
// PLAN).  `mat` may be null (artn_gates_apply: the matrices are in the table); the flags are then not set.
static int gates_plan(const ArtnMarginalDesc *d, const int32_t *k, const int32_t *dims, const double *mat, int64_t n_gates,
                      int32_t max_rank, GatesPlan &gp) {
  if (int rc = state_desc(d, "gate circuits take", ARTN_MARG_MAX_DIMS, false)) return rc;
  if (n_gates < 1) return fail(ARTN_E_INVALID, "at least one gate is needed");
  if (!k || !dims) return fail(ARTN_E_INVALID, "null pointer");
  const int nd = d->n_dims;
  StateLayout l;
  if (int rc = state_layout(d, l)) return rc;
  if (int rc = state_bits_only(l, "gate circuits take")) return rc;
  const int64_t n = gp.n = l.n;
  gp.n_recs = n_gates;
  if (int rc = state_max_rank(d->dtype, max_rank, ARTN_GATES_MAX_RANK, false, max_rank)) return rc;
  if (n_gates > INT32_MAX) return fail(ARTN_E_UNSUPPORTED, "too many gates in one circuit");
  gp.k.assign(k, k + n_gates), gp.bits.assign(2 * n_gates, -1), gp.flags.assign(n_gates, 0);
  for (int64_t g = 0; g < n_gates; ++g) {
    const std::string who = "gate " + std::to_string(g) + ": ";
    if (k[g] != 1 && k[g] != 2) return fail(ARTN_E_UNSUPPORTED, who + "gates act on one or two dimensions, not " + std::to_string(k[g]));
    for (int j = 0; j < k[g]; ++j) {
      const int32_t dim = dims[2 * g + j];
      if (dim < 0 || dim >= nd) return fail(ARTN_E_INVALID, who + "dimension " + std::to_string(dim) + " out of range");
      if (d->extent[dim] != 2)
        return fail(ARTN_E_INVALID, who + "gates act on dimensions of extent 2; dimension " + std::to_string(dim) + " has extent " +
                                        std::to_string(d->extent[dim]));
      gp.bits[2 * g + j] = __builtin_ctzll((uint64_t)d->stride[dim]);
    }
    if (k[g] == 2 && dims[2 * g] == dims[2 * g + 1]) return fail(ARTN_E_INVALID, who + "the two dimensions must differ");
    if (!mat) continue;
    bool diagonal;
    if (!state_matrix_scan(mat + 32 * g, 1 << k[g], diagonal)) return fail(ARTN_E_INVALID, who + "a matrix entry is not finite");
    const bool low = gp.bits[2 * g] < 2 && gp.bits[2 * g + 1] < 2;
    gp.flags[g] = (diagonal ? ARTN_GATE_DIAGONAL : 0) | (diagonal || low ? ARTN_GATE_LOCAL : 0);
  }
  const int cap = state_rank_cap(n, ARTN_PAULI_TILE_BITS, max_rank);
  gp.run_of.assign(n_gates, 0), gp.slot_mask.assign(n_gates, 0);
  GatesRunPlan cur;
  auto close = [&]() {
    std::sort(cur.pivot.begin(), cur.pivot.end());
    for (int64_t g = cur.first; g < cur.first + cur.count; ++g) {
      int32_t m = 0;
      for (size_t j = 0; j < cur.pivot.size(); ++j)
        if (gp.bits[2 * g] == cur.pivot[j] || gp.bits[2 * g + 1] == cur.pivot[j]) m |= 1 << j;
      gp.slot_mask[g] = m, gp.run_of[g] = (int32_t)gp.runs.size();
    }
    gp.runs.push_back(cur);
  };
  for (int64_t g = 0; g < n_gates; ++g) {
    std::vector<int> p = cur.pivot;
    bool high = false;
    for (int j = 0; j < 2; ++j) {
      const int b = gp.bits[2 * g + j];
      if (b < ARTN_PAULI_TILE_BITS) continue;
      high = true;
      if (std::find(p.begin(), p.end(), b) == p.end()) p.push_back(b);
    }
    if (high) {
      // (a run always takes its first gate with a high bit; when that gate alone exceeds the cap, gates on ITS bits still join)
      if ((int)p.size() > std::max<int>(cap, (int)cur.pivot.size()) && !cur.pivot.empty()) {
        close();
        cur = GatesRunPlan();
        cur.first = g;
        for (int j = 0; j < 2; ++j)
          if (gp.bits[2 * g + j] >= ARTN_PAULI_TILE_BITS) cur.pivot.push_back(gp.bits[2 * g + j]);
      } else {
        cur.pivot = p;
      }
    }
    ++cur.count;
  }
  close();
  const int64_t elem = d->dtype == ARTN_C64 ? 8 : 16, nr = (int64_t)gp.runs.size();
  gp.info.n_runs = gp.info.n_launches = (int32_t)nr;
  gp.info.max_rank = cap;
  gp.info.table_bytes = (int64_t)sizeof(ArtnGatesHeader) + nr * (int64_t)sizeof(ArtnGatesRun) + n_gates * (int64_t)sizeof(ArtnGatesGate);
  gp.info.bytes_read = gp.info.bytes_written = nr * n * elem;
  return ARTN_OK;
}

// what the shared host half (artn_run_circuit_host.h) reads of the family
struct GatesFamily {
  using Plan = GatesPlan;
  using Header = ArtnGatesHeader;
  using Run = ArtnGatesRun;
  using Rec = ArtnGatesGate;
  static constexpr int MAX_RANK = ARTN_GATES_MAX_RANK;
  static constexpr long MAX_GRID = ARTN_GATES_MAX_GRID;
  static constexpr const char *query = "artn_gates_query", *apply = "artn_gates_apply";
  static void basis(const GatesRunPlan &, Run &) {}
  template <typename T, int R>
  static constexpr auto run = artn_k_gates<T, R>;
  template <typename T>
  static constexpr auto small = artn_k_gates_small<T>;
};

// the record of gate g
static ArtnGatesGate gates_fill_gate(const GatesPlan &gp, int64_t g, const double *mat) {
  ArtnGatesGate rec = {};
  const int kg = gp.k[g], rows = 1 << kg;
  const GatesRunPlan &rp = gp.runs[gp.run_of[g]];
  rec.k = (uint64_t)kg, rec.flags = (uint64_t)gp.flags[g];
  for (int j = 0; j < kg; ++j) { // T_j: the LAST listed target first
    const int b = gp.bits[2 * g + (kg - 1 - j)];
    rec.bit[j] = (uint64_t)b;
    rec.lo[j] = b < ARTN_PAULI_TILE_BITS ? (uint64_t)1 << b : 0;
    for (size_t p = 0; p < rp.pivot.size(); ++p)
      if (rp.pivot[p] == b) rec.slot[j] = (uint64_t)1 << p;
  }
  for (int r = 0; r < rows; ++r)
    for (int c = 0; c < rows; ++c) rec.m[r][c][0] = mat[32 * g + 2 * (r * rows + c)], rec.m[r][c][1] = mat[32 * g + 2 * (r * rows + c) + 1];
  return rec;
}

// the per-gate and per-run arrays of a query (any may be null)
static void gates_report(const GatesPlan &gp, int32_t *bits, int32_t *run, int32_t *slot_mask, int32_t *local, int32_t *run_rank,
                         int32_t *run_pivot) {
  if (bits) std::copy(gp.bits.begin(), gp.bits.end(), bits);
  for (int64_t g = 0; local && g < gp.n_recs; ++g) local[g] = (gp.flags[g] & ARTN_GATE_LOCAL) ? 1 : 0;
  run_circuit_report<GatesFamily>(gp, run, slot_mask, run_rank, run_pivot);
}

extern "C" {

int artn_gates_query(const ArtnMarginalDesc *d, const int32_t *k, const int32_t *dims, const double *mat, int64_t n_gates,
                     int32_t max_rank, ArtnGatesInfo *info, int32_t *bits, int32_t *run, int32_t *slot_mask, int32_t *local,
                     int32_t *run_rank, int32_t *run_pivot) {
  if (!info) return fail(ARTN_E_INVALID, "null info");
  if (!mat) return fail(ARTN_E_INVALID, "null pointer");
  GatesPlan gp;
  if (int rc = gates_plan(d, k, dims, mat, n_gates, max_rank, gp)) return rc;
  *info = gp.info;
  gates_report(gp, bits, run, slot_mask, local, run_rank, run_pivot);
  return ARTN_OK;
}

int artn_gates_pack(const ArtnMarginalDesc *d, const int32_t *k, const int32_t *dims, const double *mat, int64_t n_gates,
                    int32_t max_rank, void *table, int64_t table_bytes) {
  if (!mat) return fail(ARTN_E_INVALID, "null pointer");
  GatesPlan gp;
  if (int rc = gates_plan(d, k, dims, mat, n_gates, max_rank, gp)) return rc;
  if (!table) return fail(ARTN_E_INVALID, "null pointer");
  if (int rc = state_table_fits(table_bytes, gp.info.table_bytes, "artn_gates_query")) return rc;
  if (int rc = state_table_aligned(table, "artn_gates_pack")) return rc;
  ArtnGatesRun *runs;
  ArtnGatesGate *gates;
  state_table_parts<ArtnGatesHeader>(table, gp.runs.size(), runs, gates);
  run_circuit_fill_runs<GatesFamily>(gp, table, runs);
  for (int64_t g = 0; g < n_gates; ++g) gates[g] = gates_fill_gate(gp, g, mat);
  return ARTN_OK;
}

int artn_gates_apply(const ArtnMarginalDesc *d, void *a, const int32_t *k, const int32_t *dims, const double *mat, int64_t n_gates,
                     int32_t max_rank, const void *table, int64_t table_bytes, void *stream) {
  return run_circuit_apply<GatesFamily>(d, a, table, table_bytes, stream,
                                        [&](GatesPlan &gp) { return gates_plan(d, k, dims, mat, n_gates, max_rank, gp); });
}

} // extern "C"

// The same circuits on two states with transition elements (include/artn.h: GATE ADJOINT; kernels: artn_gates_adjoint_kernel.h).
// The plan is gates_plan at the two-state rank; only the limits, the measure, the byte counts and the workspace are the adjoint's own.
struct GatesAdjointPlan {
  GatesPlan one;
  std::vector<uint8_t> flag, diag; // per gate: measured; its M is diagonal
  ArtnGatesAdjointInfo info = {};
};
struct GatesAdjointFamily {
  using One = GatesFamily;
  using Plan = GatesAdjointPlan;
  using Info = ArtnGatesAdjointInfo;
  using Rec = ArtnGatesAdjointGate;
  static constexpr int MAX_RANK = ARTN_GATES_ADJOINT_MAX_RANK;
  static constexpr const char *query = "artn_gates_adjoint_query", *apply = "artn_gates_adjoint";
  template <typename T, int R>
  static constexpr auto run = artn_k_gates_adjoint<T, R>;
  template <typename T>
  static constexpr auto small = artn_k_gates_adjoint_small<T>;
  static constexpr auto finish = artn_k_gates_adjoint_finish;
};

// `mat` and the measure may be null (artn_gates_adjoint: they are in the table).
static int gates_adjoint_plan(const ArtnMarginalDesc *d, const int32_t *k, const int32_t *dims, const double *mat, const double *measure_mat,
                              const uint8_t *measure_flag, int64_t n_gates, int32_t max_rank, GatesAdjointPlan &ap) {
  if (int rc = run_pair_rank<GatesAdjointFamily>(d, max_rank)) return rc;
  if (int rc = gates_plan(d, k, dims, mat, n_gates, max_rank, ap.one)) return rc;
  const GatesPlan &gp = ap.one;
  ap.flag.assign(n_gates, 0), ap.diag.assign(n_gates, 0);
  int64_t flagged = 0;
  for (int64_t g = 0; measure_flag && g < n_gates; ++g) {
    if (!measure_flag[g]) continue;
    if (!measure_mat) return fail(ARTN_E_INVALID, "null measure_mat with a flagged gate");
    bool diagonal;
    if (!state_matrix_scan(measure_mat + 32 * g, 1 << gp.k[g], diagonal))
      return fail(ARTN_E_INVALID, "gate " + std::to_string(g) + ": an entry of the measure matrix is not finite");
    ap.flag[g] = 1, ap.diag[g] = diagonal, ++flagged;
  }
  run_pair_info<GatesAdjointFamily>(ap, flagged);
  ap.info.table_bytes = (int64_t)sizeof(ArtnGatesHeader) + (int64_t)gp.runs.size() * (int64_t)sizeof(ArtnGatesRun) +
                        n_gates * (int64_t)sizeof(ArtnGatesAdjointGate);
  return ARTN_OK;
}

extern "C" {

int artn_gates_adjoint_query(const ArtnMarginalDesc *d, const int32_t *k, const int32_t *dims, const double *mat,
                             const double *measure_mat, const uint8_t *measure_flag, int64_t n_gates, int32_t max_rank,
                             ArtnGatesAdjointInfo *info, int32_t *bits, int32_t *run, int32_t *slot_mask, int32_t *local,
                             int32_t *run_rank, int32_t *run_pivot) {
  if (!info) return fail(ARTN_E_INVALID, "null info");
  if (!mat) return fail(ARTN_E_INVALID, "null pointer");
  GatesAdjointPlan ap;
  if (int rc = gates_adjoint_plan(d, k, dims, mat, measure_mat, measure_flag, n_gates, max_rank, ap)) return rc;
  *info = ap.info;
  gates_report(ap.one, bits, run, slot_mask, local, run_rank, run_pivot);
  return ARTN_OK;
}

int artn_gates_adjoint_pack(const ArtnMarginalDesc *d, const int32_t *k, const int32_t *dims, const double *mat,
                            const double *measure_mat, const uint8_t *measure_flag, int64_t n_gates, int32_t max_rank, void *table,
                            int64_t table_bytes) {
  if (!mat) return fail(ARTN_E_INVALID, "null pointer");
  GatesAdjointPlan ap;
  if (int rc = gates_adjoint_plan(d, k, dims, mat, measure_mat, measure_flag, n_gates, max_rank, ap)) return rc;
  if (!table) return fail(ARTN_E_INVALID, "null pointer");
  if (int rc = state_table_fits(table_bytes, ap.info.table_bytes, "artn_gates_adjoint_query")) return rc;
  if (int rc = state_table_aligned(table, "artn_gates_adjoint_pack")) return rc;
  const GatesPlan &gp = ap.one;
  ArtnGatesRun *runs;
  ArtnGatesAdjointGate *gates;
  state_table_parts<ArtnGatesHeader>(table, gp.runs.size(), runs, gates);
  run_circuit_fill_runs<GatesFamily>(gp, table, runs);
  for (int64_t g = 0; g < n_gates; ++g) {
    ArtnGatesAdjointGate rec = {};
    rec.g = gates_fill_gate(gp, g, mat);
    const int rows = 1 << gp.k[g];
    if (ap.flag[g])
      for (int r = 0; r < rows; ++r)
        for (int c = 0; c < rows; ++c)
          rec.mm[r][c][0] = measure_mat[32 * g + 2 * (r * rows + c)], rec.mm[r][c][1] = measure_mat[32 * g + 2 * (r * rows + c) + 1];
    rec.measure = (uint64_t)ap.flag[g] | (uint64_t)ap.diag[g] << 1 | (uint64_t)gp.runs[gp.run_of[g]].pivot.size() << 8;
    gates[g] = rec;
  }
  return ARTN_OK;
}

int artn_gates_adjoint(const ArtnMarginalDesc *d, void *lam, void *phi, const int32_t *k, const int32_t *dims, int64_t n_gates,
                       int32_t max_rank, const void *table, int64_t table_bytes, void *workspace, int64_t workspace_bytes,
                       double *out, void *stream) {
  return run_pair_apply<GatesAdjointFamily>(d, lam, phi, table, table_bytes, workspace, workspace_bytes, out, stream, [&](GatesAdjointPlan &ap) {
    return gates_adjoint_plan(d, k, dims, nullptr, nullptr, nullptr, n_gates, max_rank, ap); // (matrices and flags are in the table)
  });
}

} // extern "C"
