// artn_gates.hip -- host half of the dense-gate entry points of include/artn.h (kernels: artn_gates_kernel.h).
//
// A translation unit of its own (build/obj/gates.o).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "artn_host.h"
#include "artn_gates_kernel.h"

struct GatesRunPlan {
  int64_t first = 0, count = 0;
  std::vector<int> pivot; // the distinct high target bits, ascending once the run is closed
};
struct GatesPlan {
  int64_t n = 1;
  std::vector<int32_t> k, bits;            // bits: [n_gates][2] in the order the dims are listed, -1 for the absent one
  std::vector<int32_t> run_of, slot_mask, flags;
  std::vector<GatesRunPlan> runs;
  ArtnGatesInfo info = {};
};

// The layout checks of artn_pauli_query (dense, power-of-two extents), then every gate's memory bits and the runs (include/artn.h:
// PLAN).  `mat` may be null (artn_gates_apply: the matrices are in the table); the flags are then not set.
static int gates_plan(const ArtnMarginalDesc *d, const int32_t *k, const int32_t *dims, const double *mat, int64_t n_gates,
                      int32_t max_rank, GatesPlan &gp) {
  if (!d) return fail(ARTN_E_INVALID, "null descriptor");
  if (d->dtype != ARTN_C64 && d->dtype != ARTN_C128) return fail(ARTN_E_UNSUPPORTED, "gate circuits take complex64 or complex128");
  if (d->n_dims < 0) return fail(ARTN_E_INVALID, "bad number of dimensions");
  if (d->n_dims > ARTN_MARG_MAX_DIMS) return fail(ARTN_E_UNSUPPORTED, "gate circuits take at most 96 dimensions");
  if (n_gates < 1) return fail(ARTN_E_INVALID, "at least one gate is needed");
  if (!k || !dims) return fail(ARTN_E_INVALID, "null pointer");
  const int nd = d->n_dims;
  std::vector<int> order;
  bool pow2 = true;
  for (int i = 0; i < nd; ++i) {
    if (d->extent[i] < 1) return fail(ARTN_E_INVALID, "extent below 1");
    if (d->extent[i] == 1) continue; // (carries no index)
    if (d->stride[i] < 1) return fail(ARTN_E_INVALID, "the tensor is not dense: stride below 1");
    if (d->extent[i] & (d->extent[i] - 1)) pow2 = false;
    order.push_back(i);
  }
  std::sort(order.begin(), order.end(), [&](int x, int y) { return d->stride[x] < d->stride[y]; });
  int64_t n = 1;
  bool too_big = false;
  for (int i : order) {
    if (d->stride[i] != n) return fail(ARTN_E_INVALID, "the tensor is not dense: its strides overlap or leave gaps");
    if (d->extent[i] > ((int64_t)1 << 40) / n) {
      too_big = true;
      break;
    }
    n *= d->extent[i];
  }
  if (!pow2) return fail(ARTN_E_UNSUPPORTED, "gate circuits take power-of-two extents");
  if (too_big) return fail(ARTN_E_UNSUPPORTED, "gate circuits take at most 2^40 elements");
  gp.n = n;
  const int lib_max = d->dtype == ARTN_C64 ? ARTN_GATES_MAX_RANK : ARTN_GATES_MAX_RANK - 1;
  if (max_rank < -1) return fail(ARTN_E_INVALID, "max_rank below -1");
  if (max_rank > lib_max)
    return fail(ARTN_E_UNSUPPORTED, "max_rank " + std::to_string(max_rank) + " above the maximum " + std::to_string(lib_max) + " of this dtype");
  if (n_gates > INT32_MAX) return fail(ARTN_E_UNSUPPORTED, "too many gates in one circuit");
  if (max_rank < 0) max_rank = lib_max - 1; // 64 KiB of LDS per workgroup
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
    const int rows = 1 << k[g];
    const double *m = mat + 32 * g;
    bool diagonal = true;
    for (int e = 0; e < 2 * rows * rows; ++e) {
      if (!std::isfinite(m[e])) return fail(ARTN_E_INVALID, who + "a matrix entry is not finite");
      if (m[e] != 0.0 && (e / 2) / rows != (e / 2) % rows) diagonal = false;
    }
    const bool low = gp.bits[2 * g] < 2 && gp.bits[2 * g + 1] < 2;
    gp.flags[g] = (diagonal ? ARTN_GATE_DIAGONAL : 0) | (diagonal || low ? ARTN_GATE_LOCAL : 0);
  }
  int tile_bits = 0;
  while (((int64_t)1 << (ARTN_PAULI_TILE_BITS + tile_bits + 1)) <= n) ++tile_bits;
  const int cap = std::min<int>(max_rank, tile_bits);
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

template <typename T, int R>
static hipError_t gates_launch_rank(T *a, long tiles, const ArtnGatesRun *run, const ArtnGatesGate *gates, hipStream_t st) {
  const size_t lds = ((size_t)sizeof(T) << ARTN_PAULI_TILE_BITS) << R;
  if (hipError_t e = ensure_lds<artn_k_gates<T, R>>(lds); e != hipSuccess) return e;
  const long n_blocks = tiles >> R;
  const dim3 grid((unsigned)std::min<long>(n_blocks, ARTN_GATES_MAX_GRID));
  hipLaunchKernelGGL((artn_k_gates<T, R>), grid, dim3(ARTN_BORN_THREADS), lds, st, a, n_blocks, run, gates);
  return hipSuccess;
}

template <typename T>
static hipError_t gates_launch(const GatesPlan &gp, T *a, const void *table, hipStream_t st) {
  const ArtnGatesRun *runs = (const ArtnGatesRun *)((const ArtnGatesHeader *)table + 1);
  const ArtnGatesGate *gates = (const ArtnGatesGate *)(runs + gp.runs.size());
  if (gp.n < ((int64_t)1 << ARTN_PAULI_TILE_BITS)) {
    hipLaunchKernelGGL(artn_k_gates_small<T>, dim3(1), dim3(ARTN_BORN_THREADS), 0, st, a, (long)gp.n, gates, (int)gp.k.size());
    return hipSuccess;
  }
  const long tiles = (long)(gp.n >> ARTN_PAULI_TILE_BITS);
  for (size_t r = 0; r < gp.runs.size(); ++r) {
    hipError_t e = hipErrorInvalidValue;
    switch ((int)gp.runs[r].pivot.size()) {
    case 0: e = gates_launch_rank<T, 0>(a, tiles, runs + r, gates, st); break;
    case 1: e = gates_launch_rank<T, 1>(a, tiles, runs + r, gates, st); break;
    case 2: e = gates_launch_rank<T, 2>(a, tiles, runs + r, gates, st); break;
    case 3: e = gates_launch_rank<T, 3>(a, tiles, runs + r, gates, st); break;
    case 4:
      if constexpr (sizeof(T) == 8) e = gates_launch_rank<T, 4>(a, tiles, runs + r, gates, st);
      break;
    }
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
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
  if (bits) std::copy(gp.bits.begin(), gp.bits.end(), bits);
  if (run) std::copy(gp.run_of.begin(), gp.run_of.end(), run);
  if (slot_mask) std::copy(gp.slot_mask.begin(), gp.slot_mask.end(), slot_mask);
  if (local)
    for (int64_t g = 0; g < n_gates; ++g) local[g] = (gp.flags[g] & ARTN_GATE_LOCAL) ? 1 : 0;
  for (size_t r = 0; r < gp.runs.size(); ++r) {
    const GatesRunPlan &rp = gp.runs[r];
    if (run_rank) run_rank[r] = (int32_t)rp.pivot.size();
    if (run_pivot)
      for (size_t j = 0; j < ARTN_GATES_MAX_RANK; ++j) run_pivot[r * ARTN_GATES_MAX_RANK + j] = j < rp.pivot.size() ? rp.pivot[j] : -1;
  }
  return ARTN_OK;
}

int artn_gates_pack(const ArtnMarginalDesc *d, const int32_t *k, const int32_t *dims, const double *mat, int64_t n_gates,
                    int32_t max_rank, void *table, int64_t table_bytes) {
  if (!mat) return fail(ARTN_E_INVALID, "null pointer");
  GatesPlan gp;
  if (int rc = gates_plan(d, k, dims, mat, n_gates, max_rank, gp)) return rc;
  if (!table) return fail(ARTN_E_INVALID, "null pointer");
  if (table_bytes < gp.info.table_bytes) return fail(ARTN_E_INVALID, "table smaller than artn_gates_query reports");
  if (((uintptr_t)table & 7) != 0) return fail(ARTN_E_UNSUPPORTED, "artn_gates_pack needs an 8-byte aligned table");
  ArtnGatesHeader *h = (ArtnGatesHeader *)table;
  ArtnGatesRun *runs = (ArtnGatesRun *)(h + 1);
  ArtnGatesGate *gates = (ArtnGatesGate *)(runs + gp.runs.size());
  *h = ArtnGatesHeader{(uint64_t)gp.runs.size(), (uint64_t)n_gates, (uint64_t)gp.info.max_rank, 0};
  for (size_t r = 0; r < gp.runs.size(); ++r) {
    const GatesRunPlan &rp = gp.runs[r];
    ArtnGatesRun rec = {};
    rec.first = (uint64_t)rp.first, rec.count = (uint64_t)rp.count, rec.rank = (uint64_t)rp.pivot.size();
    for (size_t j = 0; j < rp.pivot.size(); ++j) rec.pivot[j] = (uint64_t)rp.pivot[j];
    runs[r] = rec;
  }
  for (int64_t g = 0; g < n_gates; ++g) {
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
    gates[g] = rec;
  }
  return ARTN_OK;
}

int artn_gates_apply(const ArtnMarginalDesc *d, void *a, const int32_t *k, const int32_t *dims, const double *mat, int64_t n_gates,
                     int32_t max_rank, const void *table, int64_t table_bytes, void *stream) {
  if (artn_device_count() < 1) return fail(ARTN_E_NODEVICE, "no gfx950 device visible");
  GatesPlan gp;
  if (int rc = gates_plan(d, k, dims, mat, n_gates, max_rank, gp)) return rc;
  if (!a || !table) return fail(ARTN_E_INVALID, "null pointer");
  if (table_bytes < gp.info.table_bytes) return fail(ARTN_E_INVALID, "table smaller than artn_gates_query reports");
  if (((uintptr_t)a & 15) != 0) return fail(ARTN_E_UNSUPPORTED, "artn_gates_apply needs a 16-byte aligned array");
  if (((uintptr_t)table & 7) != 0) return fail(ARTN_E_UNSUPPORTED, "artn_gates_apply needs an 8-byte aligned table");
  hipStream_t st = (hipStream_t)stream;
  if (d->dtype == ARTN_C64) HIP_TRY(gates_launch(gp, (float2 *)a, table, st));
  else HIP_TRY(gates_launch(gp, (double2 *)a, table, st));
  HIP_TRY(hipGetLastError());
  return ARTN_OK;
}

} // extern "C"
