// artn_cgate_batch.hip -- host half of the conditional-gate entry points artn_cgate_batch_* of include/artn.h (kernel:
// artn_cgate_batch_kernel.h).  The plan is that of artn_cgate.hip (artn_cgate_host.h) on an index space without the batch bits
// (state_batch_dims of artn_state_host.h, shared with artn_batch.hip).
//
// A translation unit of its own (build/obj/cgate_batch.o).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "artn_host.h"
#include "artn_state_host.h"
#include "artn_cgate_batch_kernel.h"
#include "artn_cgate_host.h"

struct CgateBatchPlan : CgatePlan {
  BatchDims batch;
  ArtnBatchFields fields = {};
  ArtnCgateBatchInfo binfo = {};
};

static int64_t cgate_batch_table_bytes(int t, int m) {
  return (int64_t)sizeof(ArtnCgateTable) + (int64_t)sizeof(ArtnCgateBatchCases) + (int64_t)m * ((int64_t)16 << (2 * t));
}

// cgate_plan's checks, then the cases, then batch_plan's batch checks, then the selector; the tile without batch bits and high
// controls.  keys, mats and selector may be null (artn_cgate_batch_apply: keys and matrices are in the table).
static int cgate_batch_plan(const ArtnMarginalDesc *d, int32_t t, const int32_t *targets, int32_t c, const int32_t *controls,
                            const int32_t *values, int32_t nb, const int32_t *batch_dims, int32_t m, const int64_t *keys, int64_t mask,
                            const double *mats, const void *selector, int64_t selector_stride, CgateBatchPlan &cp) {
  int64_t n = 0;
  if (int rc = cgate_head(d, t, targets, c, controls, "conditional gates take", "conditional gates", cp, n)) return rc;
  if (nb > 0 && !batch_dims) return fail(ARTN_E_INVALID, "null pointer");
  if (nb < 0) return fail(ARTN_E_INVALID, "a negative number of batch dimensions: " + std::to_string(nb));
  // the index bits of a trajectory, before anything else is said about the dimensions (as artn_cgate_query does for the state)
  int sub = cp.n_bits;
  for (int i = 0; i < nb; ++i)
    if (batch_dims[i] >= 0 && batch_dims[i] < d->n_dims && d->extent[batch_dims[i]] > 1) sub -= __builtin_ctzll((uint64_t)d->extent[batch_dims[i]]);
  if (sub < 0 || (int64_t)t + c > sub)
    return fail(ARTN_E_INVALID, "a gate on " + std::to_string(t) + " dimensions under " + std::to_string(c) +
                                    " controls needs a trajectory of at least 2^" + std::to_string(t) +
                                    " elements once the controls are taken out; these have 2^" + std::to_string(std::max(sub, 0)) + " in all");
  if (m < 1 || m > ARTN_CGATE_BATCH_MAX_CASES)
    return fail(ARTN_E_INVALID, "a conditional gate has 1 to " + std::to_string(ARTN_CGATE_BATCH_MAX_CASES) + " cases, not " + std::to_string(m));
  if (mask < -1) return fail(ARTN_E_INVALID, "the mask is -1 (all bits) or lies in 0 .. 2^63 - 1");
  std::vector<int32_t> seen;
  if (int rc = cgate_dims(d, targets, controls, values, cp, seen)) return rc;
  if (int rc = state_batch_dims(d, nb, batch_dims, seen, (size_t)t, "target", cp.batch)) return rc;
  if (keys)
    for (int j = 0; j < m; ++j) {
      if (keys[j] < 0) return fail(ARTN_E_INVALID, "a key lies in 0 .. 2^63 - 1; case " + std::to_string(j) + " has " + std::to_string((long long)keys[j]));
      if (keys[j] & ~mask)
        return fail(ARTN_E_INVALID, "the key of case " + std::to_string(j) + " (" + std::to_string((long long)keys[j]) +
                                        ") has bits outside the mask: the case could never be chosen");
      for (int i = 0; i < j; ++i)
        if (keys[i] == keys[j]) return fail(ARTN_E_INVALID, "the keys must differ; key " + std::to_string((long long)keys[j]) + " is repeated");
    }
  bool all_diagonal = true;
  if (mats)
    for (int j = 0; j < m; ++j) {
      bool diagonal = false;
      if (!state_matrix_scan(mats + ((size_t)j << (2 * t + 1)), 1 << t, diagonal))
        return fail(ARTN_E_INVALID, "an entry of the matrix of case " + std::to_string(j) + " is not finite");
      all_diagonal = all_diagonal && diagonal;
    }
  if (selector_stride < 1)
    return fail(ARTN_E_INVALID, "a selector stride of at least one 8-byte word is needed, not " + std::to_string((long long)selector_stride));
  if (((uintptr_t)selector & 7) != 0) return fail(ARTN_E_UNSUPPORTED, "conditional gates need an 8-byte aligned selector");
  const int c_high = cp.c_high, batch_bits = cp.batch.bits;
  state_tile_plan(d->dtype, cp.n_bits - c_high - batch_bits, cp.high_mask | cp.batch.mask, cp);
  cp.n_tiles = (int64_t)1 << (cp.n_bits - c_high - cp.tb); // (the walk covers every trajectory)
  if (int rc = cgate_holes(cp, "conditional gates take")) return rc;
  cp.fields.n = (int32_t)cp.batch.shift.size();
  ArtnCgateBatchInfo &bi = cp.binfo;
  for (size_t f = 0; f < cp.batch.shift.size(); ++f) {
    cp.fields.shift[f] = bi.field_shift[f] = cp.batch.shift[f];
    cp.fields.width[f] = bi.field_width[f] = cp.batch.width[f];
    cp.fields.pos[f] = bi.field_pos[f] = cp.batch.pos[f];
  }
  bi.t = t, bi.c = c, bi.c_high = c_high, bi.c_low = c - c_high, bi.tile_bits = cp.tb, bi.diagonal = mats && all_diagonal ? 1 : 0;
  bi.n_selected = n >> c, bi.n_tiles = cp.n_tiles, bi.segment = cp.segment, bi.lds_bytes = cp.lds_bytes;
  bi.table_bytes = cgate_batch_table_bytes(t, m);
  bi.bytes_read = bi.bytes_written = (n >> c_high) * cp.elem;
  bi.m = m, bi.batch_bits = batch_bits, bi.n_fields = cp.fields.n, bi.B = (int64_t)1 << batch_bits;
  bi.grid = (int32_t)std::min<int64_t>(cp.n_tiles, ARTN_WGATE_MAX_GRID);
  return ARTN_OK;
}

template <typename T>
static void cgate_batch_launch(const CgateBatchPlan &cp, T *a, const void *table, const void *selector, int64_t stride, int64_t mask,
                               hipStream_t st) {
  const ArtnCgateTable *tab = (const ArtnCgateTable *)table;
  const long long *sel = (const long long *)selector;
  const long long s = (long long)stride, k = (long long)mask;
  const dim3 grid((unsigned)cp.binfo.grid), block(ARTN_BORN_THREADS);
  const size_t lds = (size_t)cp.binfo.lds_bytes;
  state_with_k<1, ARTN_WGATE_MAX_K>(cp.t, [&](auto kk) {
    hipLaunchKernelGGL((artn_k_cgate_batch<T, decltype(kk)::value>), grid, block, lds, st, a, tab, sel, s, k, cp.fields);
  });
}

extern "C" {

int artn_cgate_batch_query(const ArtnMarginalDesc *d, int32_t t, const int32_t *targets, int32_t c, const int32_t *controls,
                           const int32_t *control_values, int32_t nb, const int32_t *batch_dims, int32_t m, const int64_t *keys,
                           int64_t mask, const double *mats, const void *selector, int64_t selector_stride, ArtnCgateBatchInfo *info,
                           int32_t *target_bits, int32_t *control_bits, int32_t *tile_bits) {
  if (!info) return fail(ARTN_E_INVALID, "null info");
  CgateBatchPlan cp;
  if (int rc = cgate_batch_plan(d, t, targets, c, controls, control_values, nb, batch_dims, m, keys, mask, mats, selector,
                                selector_stride, cp))
    return rc;
  *info = cp.binfo;
  if (target_bits) std::copy(cp.target.begin(), cp.target.end(), target_bits);
  if (control_bits) std::copy(cp.control.begin(), cp.control.end(), control_bits);
  if (tile_bits) std::copy(cp.tile.begin(), cp.tile.end(), tile_bits);
  return ARTN_OK;
}

int artn_cgate_batch_pack(const ArtnMarginalDesc *d, int32_t t, const int32_t *targets, int32_t c, const int32_t *controls,
                          const int32_t *control_values, int32_t nb, const int32_t *batch_dims, int32_t m, const int64_t *keys,
                          int64_t mask, const double *mats, void *table, int64_t table_bytes) {
  if (!keys || !mats) return fail(ARTN_E_INVALID, "null pointer");
  CgateBatchPlan cp;
  if (int rc = cgate_batch_plan(d, t, targets, c, controls, control_values, nb, batch_dims, m, keys, mask, mats, nullptr, 1, cp)) return rc;
  if (!table) return fail(ARTN_E_INVALID, "null pointer");
  if (int rc = state_table_fits(table_bytes, cp.binfo.table_bytes, "artn_cgate_batch_query")) return rc;
  if (int rc = state_table_aligned(table, "artn_cgate_batch_pack")) return rc;
  ArtnCgateTable tab = {};
  ArtnCgateBatchCases cs = {};
  const int rows = 1 << t;
  cgate_tile_fields(cp, tab);
  tab.flags = cp.binfo.diagonal ? ARTN_GATE_DIAGONAL : 0;
  cs.m = (uint64_t)m;
  for (int j = 0; j < ARTN_CGATE_BATCH_MAX_CASES; ++j) cs.key[j] = -1;
  for (int j = 0; j < m; ++j) {
    const double *mat = mats + ((size_t)j << (2 * t + 1));
    bool diagonal = true;
    state_matrix_scan(mat, rows, diagonal);
    bool identity = diagonal;
    for (int row = 0; row < rows; ++row)
      if (mat[2 * (row * rows + row)] != 1.0 || mat[2 * (row * rows + row) + 1] != 0.0) identity = false;
    cs.key[j] = keys[j];
    cs.flags[j] = (diagonal ? ARTN_CGATE_CASE_DIAGONAL : 0) | (identity ? ARTN_CGATE_CASE_IDENTITY : 0);
    cs.block_mask[j] = state_block_mask(mat, rows);
    tab.block_mask |= cs.block_mask[j];
  }
  *(ArtnCgateTable *)table = tab;
  ArtnCgateBatchCases *cases = (ArtnCgateBatchCases *)((ArtnCgateTable *)table + 1);
  *cases = cs;
  std::copy(mats, mats + ((size_t)m << (2 * t + 1)), (double *)(cases + 1));
  return ARTN_OK;
}

int artn_cgate_batch_apply(const ArtnMarginalDesc *d, void *a, int32_t t, const int32_t *targets, int32_t c, const int32_t *controls,
                           const int32_t *control_values, int32_t nb, const int32_t *batch_dims, int32_t m, const void *table,
                           int64_t table_bytes, const void *selector, int64_t selector_stride, int64_t mask, void *stream) {
  if (artn_device_count() < 1) return fail(ARTN_E_NODEVICE, "no gfx950 device visible");
  CgateBatchPlan cp;
  if (int rc = cgate_batch_plan(d, t, targets, c, controls, control_values, nb, batch_dims, m, nullptr, mask, nullptr, selector,
                                selector_stride, cp))
    return rc;
  if (!a || !table || !selector) return fail(ARTN_E_INVALID, "null pointer");
  if (int rc = state_table_fits(table_bytes, cp.binfo.table_bytes, "artn_cgate_batch_query")) return rc;
  if (int rc = state_array_aligned(a, "artn_cgate_batch_apply")) return rc;
  if (int rc = state_table_aligned(table, "artn_cgate_batch_apply")) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (d->dtype == ARTN_C64) cgate_batch_launch(cp, (float2 *)a, table, selector, selector_stride, mask, st);
  else cgate_batch_launch(cp, (double2 *)a, table, selector, selector_stride, mask, st);
  HIP_TRY(hipGetLastError());
  return ARTN_OK;
}

} // extern "C"
