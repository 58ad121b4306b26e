// artn_run_circuit_host.h -- the one host half of the four run-circuit families (artn_pauli.hip: artn_pauli_evolve*,
// artn_pauli_adjoint*; artn_gates.hip: artn_gates_*, artn_gates_adjoint*): the run records of a table and of a query, the
// launchers and the apply entries, over a traits struct F that the family's own unit defines beside its plan.  A single-state F:
//
//   F::Plan                        n, n_recs, runs[] (first, count, pivot[]: the rank of a run is pivot.size()), run_of, slot_mask, info
//   F::Header, F::Run, F::Rec      the parts of its table (include/artn.h)
//   F::MAX_RANK, F::MAX_GRID       the rank limit and the grid cap
//   F::query, F::apply             the names of its entries, as the refusals quote them
//   F::basis(run plan, record)     what a run record holds beyond first, count, rank and pivot[]
//   F::run<T, R>, F::small<T>      its kernels: (a, n_blocks, run, recs) and (a, n, recs, n_recs)
//
// A two-state F: F::One (its single-state family: plan, header, run records, grid cap), F::Plan (`one`, the single-state plan, and
// `info`), F::Info, F::Rec, F::MAX_RANK, F::query, F::apply, F::run<T, R> and F::small<T> with (lam, phi) for a and (ws, groups) /
// (ws) behind the records, and F::finish, one workgroup per record: (ws, groups, tiles, recs, out).
//
// The cutting walk, the record fillers and the query and pack entries are the family's own: what a pivot is differs, and so
// does the order of their refusals.  The checks of the apply entries, their order, the codes and the texts are one
// (tests/test_state_layout_cpu.py, tests/test_pauli_evolve_cpu.py, tests/test_gates_cpu.py and their adjoint twins).
#pragma once
#include "artn_state_host.h"
#include "artn_pauli_adjoint_kernel.h" // (the tile, the threads and the workspace slots of a workgroup; the gate kernels include it too)

// the header and the run records of a table (include/artn.h: TABLE)
template <typename F>
static void run_circuit_fill_runs(const typename F::Plan &p, void *table, typename F::Run *runs) {
  *(typename F::Header *)table = typename F::Header{(uint64_t)p.runs.size(), (uint64_t)p.n_recs, (uint64_t)p.info.max_rank, 0};
  for (size_t r = 0; r < p.runs.size(); ++r) {
    const auto &rp = p.runs[r];
    typename F::Run rec = {};
    rec.first = (uint64_t)rp.first, rec.count = (uint64_t)rp.count, rec.rank = (uint64_t)rp.pivot.size();
    for (size_t j = 0; j < rp.pivot.size(); ++j) rec.pivot[j] = (uint64_t)rp.pivot[j];
    F::basis(rp, rec);
    runs[r] = rec;
  }
}

// what every query reports of the runs: per record its run and slot mask, per run its rank and pivots (any may be null)
template <typename F>
static void run_circuit_report(const typename F::Plan &p, int32_t *run, int32_t *slot_mask, int32_t *run_rank, int32_t *run_pivot) {
  if (run) std::copy(p.run_of.begin(), p.run_of.end(), run);
  if (slot_mask) std::copy(p.slot_mask.begin(), p.slot_mask.end(), slot_mask);
  for (size_t r = 0; r < p.runs.size(); ++r) {
    const auto &pivot = p.runs[r].pivot;
    if (run_rank) run_rank[r] = (int32_t)pivot.size();
    if (run_pivot)
      for (size_t j = 0; j < F::MAX_RANK; ++j) run_pivot[r * F::MAX_RANK + j] = j < pivot.size() ? pivot[j] : -1;
  }
}

// One launch per run, a block of 2^R tiles in LDS; below one tile the small kernel.
template <typename F, typename T>
static hipError_t run_circuit_launch(const typename F::Plan &p, T *a, const void *table, hipStream_t st) {
  const typename F::Run *runs;
  const typename F::Rec *recs;
  state_table_parts<typename F::Header>(table, p.runs.size(), runs, recs);
  const dim3 block(ARTN_BORN_THREADS);
  if (p.n < ((int64_t)1 << ARTN_PAULI_TILE_BITS)) {
    hipLaunchKernelGGL(F::template small<T>, dim3(1), block, 0, st, a, (long)p.n, recs, (int)p.n_recs);
    return hipSuccess;
  }
  const long tiles = (long)(p.n >> ARTN_PAULI_TILE_BITS);
  for (size_t r = 0; r < p.runs.size(); ++r) {
    const hipError_t e = state_with_rank<T, F::MAX_RANK>((int)p.runs[r].pivot.size(), [&](auto rank) {
      constexpr int R = decltype(rank)::value;
      const size_t lds = ((size_t)sizeof(T) << ARTN_PAULI_TILE_BITS) << R;
      if (hipError_t e = ensure_lds<F::template run<T, R>>(lds); e != hipSuccess) return e;
      const long n_blocks = tiles >> R;
      const dim3 grid((unsigned)std::min<long>(n_blocks, F::MAX_GRID));
      hipLaunchKernelGGL((F::template run<T, R>), grid, block, lds, st, a, n_blocks, runs + r, recs);
      return hipSuccess;
    });
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// ... on two states: twice the LDS, the workspace slots of `groups` workgroups per record, and the finish launch at the end
template <typename F, typename T>
static hipError_t run_pair_launch(const typename F::One::Plan &p, T *lam, T *phi, const void *table, double *ws, double *out, hipStream_t st) {
  const typename F::One::Run *runs;
  const typename F::Rec *recs;
  state_table_parts<typename F::One::Header>(table, p.runs.size(), runs, recs);
  const dim3 block(ARTN_BORN_THREADS);
  const long tiles = (long)std::max<int64_t>(p.n >> ARTN_PAULI_TILE_BITS, 1);
  const long groups = std::min<long>(tiles, F::One::MAX_GRID);
  if (p.n < ((int64_t)1 << ARTN_PAULI_TILE_BITS))
    hipLaunchKernelGGL(F::template small<T>, dim3(1), block, 0, st, lam, phi, (long)p.n, recs, (int)p.n_recs, ws);
  else
    for (size_t r = 0; r < p.runs.size(); ++r) {
      const hipError_t e = state_with_rank<T, F::MAX_RANK>((int)p.runs[r].pivot.size(), [&](auto rank) {
        constexpr int R = decltype(rank)::value;
        const size_t lds = ((size_t)2 * sizeof(T) << ARTN_PAULI_TILE_BITS) << R;
        if (hipError_t e = ensure_lds<F::template run<T, R>>(lds); e != hipSuccess) return e;
        const long n_blocks = tiles >> R;
        const dim3 grid((unsigned)std::min<long>(n_blocks, F::One::MAX_GRID)); // (at most `groups`: the workspace slots of a record)
        hipLaunchKernelGGL((F::template run<T, R>), grid, block, lds, st, lam, phi, n_blocks, runs + r, recs, ws, groups);
        return hipSuccess;
      });
      if (e != hipSuccess) return e;
    }
  hipLaunchKernelGGL(F::finish, dim3((unsigned)p.n_recs), block, 0, st, (const double *)ws, groups, tiles, recs, out);
  return hipSuccess;
}

// The head of a two-state plan: the descriptor and max_rank at the two-state limits, before the single-state plan sees them.
template <typename F>
static int run_pair_rank(const ArtnMarginalDesc *d, int32_t &max_rank) {
  if (!d) return fail(ARTN_E_INVALID, "null descriptor");
  return state_max_rank(d->dtype, max_rank, F::MAX_RANK, true, max_rank);
}

// The two-state info from the single-state one (table_bytes stays the family's own).
template <typename F>
static void run_pair_info(typename F::Plan &p, int64_t n_measured) {
  const auto &one = p.one.info;
  const int64_t groups = std::min<int64_t>(std::max<int64_t>(p.one.n >> ARTN_PAULI_TILE_BITS, 1), F::One::MAX_GRID);
  p.info = typename F::Info{};
  p.info.n_runs = one.n_runs;
  p.info.n_launches = one.n_runs + 1;
  p.info.max_rank = one.max_rank;
  p.info.n_measured = (int32_t)n_measured;
  p.info.workspace_bytes = p.one.n_recs * groups * ARTN_PAULI_ADJOINT_WAVES * 2 * (int64_t)sizeof(double);
  p.info.bytes_read = 2 * one.bytes_read;
  p.info.bytes_written = 2 * one.bytes_written;
}

// The apply entries.  plan(p) is the family's plan with the entry's own arguments (what the table holds is null).
template <typename F, typename PlanFn>
static int run_circuit_apply(const ArtnMarginalDesc *d, void *a, const void *table, int64_t table_bytes, void *stream, PlanFn &&plan) {
  if (artn_device_count() < 1) return fail(ARTN_E_NODEVICE, "no gfx950 device visible");
  typename F::Plan p;
  if (int rc = plan(p)) return rc;
  if (!a || !table) return fail(ARTN_E_INVALID, "null pointer");
  if (int rc = state_table_fits(table_bytes, p.info.table_bytes, F::query)) return rc;
  if (int rc = state_array_aligned(a, F::apply)) return rc;
  if (int rc = state_table_aligned(table, F::apply)) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (d->dtype == ARTN_C64) HIP_TRY(run_circuit_launch<F>(p, (float2 *)a, table, st));
  else HIP_TRY(run_circuit_launch<F>(p, (double2 *)a, table, st));
  HIP_TRY(hipGetLastError());
  return ARTN_OK;
}

template <typename F, typename PlanFn>
static int run_pair_apply(const ArtnMarginalDesc *d, void *lam, void *phi, const void *table, int64_t table_bytes, void *workspace,
                          int64_t workspace_bytes, double *out, void *stream, PlanFn &&plan) {
  if (artn_device_count() < 1) return fail(ARTN_E_NODEVICE, "no gfx950 device visible");
  typename F::Plan p;
  if (int rc = plan(p)) return rc;
  const std::string entry = F::apply;
  if (!lam || !phi || !table || !workspace || !out) return fail(ARTN_E_INVALID, "null pointer");
  if (int rc = state_table_fits(table_bytes, p.info.table_bytes, F::query)) return rc;
  if (workspace_bytes < p.info.workspace_bytes) return fail(ARTN_E_INVALID, std::string("workspace smaller than ") + F::query + " reports");
  if ((((uintptr_t)lam | (uintptr_t)phi | (uintptr_t)workspace) & 15) != 0)
    return fail(ARTN_E_UNSUPPORTED, entry + " needs 16-byte aligned arrays and workspace");
  if ((((uintptr_t)table | (uintptr_t)out) & 7) != 0) return fail(ARTN_E_UNSUPPORTED, entry + " needs an 8-byte aligned table and output");
  if (int rc = state_disjoint(lam, phi, (uintptr_t)p.one.n * (d->dtype == ARTN_C64 ? 8 : 16), F::apply)) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (d->dtype == ARTN_C64) HIP_TRY(run_pair_launch<F>(p.one, (float2 *)lam, (float2 *)phi, table, (double *)workspace, out, st));
  else HIP_TRY(run_pair_launch<F>(p.one, (double2 *)lam, (double2 *)phi, table, (double *)workspace, out, st));
  HIP_TRY(hipGetLastError());
  return ARTN_OK;
}
