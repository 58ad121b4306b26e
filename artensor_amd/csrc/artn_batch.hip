// artn_batch.hip -- host half of the batched-trajectory entry points artn_measure_batch_* and artn_channel_batch_* of
// include/artn.h (kernels: artn_batch_kernel.h).
//
// A translation unit of its own (build/obj/batch.o).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "artn_host.h"
#include "artn_state_host.h"
#include "artn_batch_kernel.h"

struct BatchPlan : TilePlan {
  int n_bits = 0, batch_bits = 0;
  uint64_t batch_mask = 0; // over memory bits
  std::vector<int> dim_bit; // memory bits of the measured / target dimensions, in the order listed
  ArtnBatchFields fields = {};
  ArtnBatchInfo info = {};
};

// The descriptor and layout checks of the unbatched families in the wording of `who` ("batched measurement takes", "batched
// channels take"), the k listed dimensions (`what`, `role`: "measurements", "measured" / "channels", "target"), then the batch
// dimensions: what is wrong with them (ARTN_E_INVALID) before what the layout does not support.  D = 2^k.
static int batch_plan(const ArtnMarginalDesc *d, int32_t k, const int32_t *dims, int32_t nb, const int32_t *batch_dims, const char *who,
                      const char *what, const char *role, BatchPlan &bp) {
  if (int rc = state_desc(d, who, ARTN_MARG_MAX_DIMS, false)) return rc;
  if (!dims || (nb > 0 && !batch_dims)) return fail(ARTN_E_INVALID, "null pointer");
  if (nb < 0) return fail(ARTN_E_INVALID, "a negative number of batch dimensions: " + std::to_string(nb));
  StateLayout l;
  if (int rc = state_layout(d, l)) return rc;
  if (int rc = state_bits_only(l, who)) return rc;
  bp.n_bits = __builtin_ctzll((uint64_t)l.n);
  std::vector<int32_t> seen;
  for (int j = 0; j < k; ++j) {
    if (int rc = state_tile_dim(d, dims[j], seen, (size_t)k, false, what)) return rc;
    seen.push_back(dims[j]);
    bp.dim_bit.push_back(__builtin_ctzll((uint64_t)d->stride[dims[j]]));
  }
  BatchDims bd;
  if (int rc = state_batch_dims(d, nb, batch_dims, seen, (size_t)k, role, bd)) return rc;
  bp.batch_bits = bd.bits, bp.batch_mask = bd.mask;
  if (bp.batch_bits + k > 24)
    return fail(ARTN_E_UNSUPPORTED, "B * D = 2^" + std::to_string(bp.batch_bits + k) + " is above 2^24, what the streaming marginal keeps");
  bp.fields.n = (int32_t)bd.shift.size();
  ArtnBatchInfo &bi = bp.info;
  for (size_t f = 0; f < bd.shift.size(); ++f) { // (listed order: the most significant field first)
    bp.fields.shift[f] = bd.shift[f], bp.fields.width[f] = bd.width[f], bp.fields.pos[f] = bd.pos[f];
    bi.field_shift[f] = bd.shift[f], bi.field_width[f] = bd.width[f], bi.field_pos[f] = bd.pos[f];
  }
  bp.elem = d->dtype == ARTN_C64 ? 8 : 16;
  bi.n_fields = bp.fields.n, bi.batch_bits = bp.batch_bits;
  bi.B = (int64_t)1 << bp.batch_bits, bi.D = (int64_t)1 << k, bi.n = l.n;
  bi.record_bytes = ARTN_MEASURE_RECORD_BYTES * bi.B;
  bi.bytes_written = l.n * bp.elem;
  return ARTN_OK;
}

// ---- measurement ---------------------------------------------------------------------------------------------------------
static int batch_measure_plan(const ArtnMarginalDesc *d, int32_t k, const int32_t *dims, int32_t nb, const int32_t *batch_dims,
                              BatchPlan &bp, ArtnMeasureArgs &a) {
  if (k < 1) return fail(ARTN_E_INVALID, "at least one dimension is measured");
  if (k > ARTN_MEASURE_MAX_DIMS)
    return fail(ARTN_E_INVALID, "at most " + std::to_string(ARTN_MEASURE_MAX_DIMS) + " dimensions are measured in one call");
  if (int rc = batch_plan(d, k, dims, nb, batch_dims, "batched measurement takes", "measurements", "measured", bp)) return rc;
  a = {};
  a.k = k, a.vec_shift = d->dtype == ARTN_C64 ? 1 : 0;
  for (int j = 0; j < k; ++j) a.bit[j] = (uint8_t)bp.dim_bit[j], a.mask |= (uint64_t)1 << bp.dim_bit[j];
  for (int b = a.vec_shift; b < 40; ++b)
    if (a.mask >> b & 1) a.hi_bit[a.n_hi++] = (uint8_t)(b - a.vec_shift);
  ArtnBatchInfo &bi = bp.info;
  const int64_t nvec = bi.n * bp.elem / 16; // (k >= 1: n >= 2, a whole number of vectors)
  bi.grid = (int32_t)std::min<int64_t>((nvec + ARTN_MEASURE_THREADS - 1) / ARTN_MEASURE_THREADS, ARTN_MEASURE_MAX_GRID);
  bi.launches = 2, bi.reset_launches = 3;
  bi.bytes_read = (bi.n >> k) * bp.elem;
  return ARTN_OK;
}

template <typename T>
static void batch_measure_launch(T *a, const BatchPlan &bp, const ArtnMeasureArgs &p, const ArtnMeasureRecord *rec, bool reset, hipStream_t st) {
  const long nvec = (long)(bp.info.n >> p.vec_shift);
  const dim3 grid((unsigned)bp.info.grid), block(ARTN_MEASURE_THREADS);
  if (!reset) {
    hipLaunchKernelGGL(artn_k_measure_batch_collapse<T>, grid, block, 0, st, a, nvec, p, bp.fields, rec);
    return;
  }
  const long nvec_dst = nvec >> p.n_hi;
  const unsigned move_grid = (unsigned)std::min<long>((nvec_dst + ARTN_MEASURE_THREADS - 1) / ARTN_MEASURE_THREADS, ARTN_MEASURE_MAX_GRID);
  hipLaunchKernelGGL(artn_k_measure_batch_move<T>, dim3(move_grid), block, 0, st, a, nvec_dst, p, bp.fields, rec);
  hipLaunchKernelGGL(artn_k_measure_batch_clear<T>, grid, block, 0, st, a, nvec, p, bp.fields, rec);
}

// ---- channels --------------------------------------------------------------------------------------------------------------
static int batch_form(int32_t form) {
  if (form == ARTN_CHANNEL_DENSE)
    return fail(ARTN_E_UNSUPPORTED, "batched channels take the FIXED and DIAGONAL forms: the DENSE form needs a reduced density matrix "
                                    "per trajectory, which does not exist");
  if (form != ARTN_CHANNEL_FIXED && form != ARTN_CHANNEL_DIAGONAL) return fail(ARTN_E_INVALID, "unknown weight form " + std::to_string(form));
  return ARTN_OK;
}
static int batch_counts(int32_t t, int32_t m, int32_t form) {
  if (t < 1 || t > ARTN_WGATE_MAX_K)
    return fail(ARTN_E_UNSUPPORTED, "channels act on one to five dimensions, not " + std::to_string(t));
  if (m < 1 || m > ARTN_CHANNEL_MAX_OPS)
    return fail(ARTN_E_INVALID, "a channel has 1 to " + std::to_string(ARTN_CHANNEL_MAX_OPS) + " operators, not " + std::to_string(m));
  return batch_form(form);
}
static int64_t batch_table_bytes(int t, int m, int form) {
  const int64_t wd = form == ARTN_CHANNEL_FIXED ? 1 : (int64_t)1 << t;
  return (int64_t)sizeof(ArtnChannelTable) + (int64_t)m * ((int64_t)sizeof(ArtnChannelOp) + 8 * wd + ((int64_t)16 << (2 * t)));
}

// The tile of artn_wgate_query with the batch bits kept out of it (include/artn.h: CHANNELS), and the walk of its tiles.
static int batch_channel_plan(const ArtnMarginalDesc *d, int32_t t, const int32_t *dims, int32_t nb, const int32_t *batch_dims, int32_t m,
                              int32_t form, const double *mats, BatchPlan &bp, ArtnBatchWalk &wk) {
  if (t < 1 || t > ARTN_WGATE_MAX_K)
    return fail(ARTN_E_UNSUPPORTED, "channels act on one to five dimensions, not " + std::to_string(t));
  if (int rc = batch_plan(d, t, dims, nb, batch_dims, "batched channels take", "channels", "target", bp)) return rc;
  if (int rc = batch_counts(t, m, form)) return rc;
  const int sub_bits = bp.n_bits - bp.batch_bits;
  if (t > sub_bits)
    return fail(ARTN_E_INVALID, "a channel on " + std::to_string(t) + " dimensions needs a trajectory of at least 2^" + std::to_string(t) +
                                    " elements; these have 2^" + std::to_string(sub_bits));
  if (mats)
    for (int j = 0; j < m; ++j) {
      bool diagonal = false;
      if (!state_matrix_scan(mats + ((size_t)j << (2 * t + 1)), 1 << t, diagonal))
        return fail(ARTN_E_INVALID, "an entry of operator " + std::to_string(j) + " is not finite");
    }
  bp.target = bp.dim_bit;
  state_tile_plan(d->dtype, sub_bits, bp.batch_mask, bp);
  bp.n_tiles = (int64_t)1 << (bp.n_bits - bp.tb); // (the walk covers every trajectory)
  wk = {};
  wk.seg_bits = bp.seg_bits, wk.f = bp.fields;
  for (int j = bp.seg_bits; j < bp.tb; ++j) {
    if (wk.n_holes == ARTN_BATCH_MAX_HOLES) return fail(ARTN_E_UNSUPPORTED, "batched channels: too many separate tile bits");
    wk.hole[wk.n_holes++] = bp.tile[j];
  }
  ArtnBatchInfo &bi = bp.info;
  bi.tile_bits = bp.tb, bi.launches = 2, bi.reset_launches = 0;
  bi.grid = (int32_t)std::min<int64_t>(bp.n_tiles, ARTN_WGATE_MAX_GRID);
  bi.n_tiles = bp.n_tiles, bi.segment = bp.segment, bi.lds_bytes = bp.lds_bytes;
  bi.table_bytes = batch_table_bytes(t, m, form);
  bi.bytes_read = bi.bytes_written;
  return ARTN_OK;
}

template <typename T>
static void batch_channel_launch(const BatchPlan &bp, const ArtnBatchWalk &wk, int t, int m, T *a, const void *table, const void *records,
                                 hipStream_t st) {
  const ArtnChannelTable *tab = (const ArtnChannelTable *)table;
  const ArtnChannelRecord *rec = (const ArtnChannelRecord *)records;
  const dim3 grid((unsigned)bp.info.grid), block(ARTN_BORN_THREADS);
  const size_t lds = (size_t)bp.info.lds_bytes;
  state_with_k<1, ARTN_WGATE_MAX_K>(t, [&](auto k) {
    hipLaunchKernelGGL((artn_k_channel_batch<T, decltype(k)::value>), grid, block, lds, st, a, tab, rec, m, wk);
  });
}

extern "C" {

int artn_measure_batch_query(const ArtnMarginalDesc *d, int32_t k, const int32_t *dims, int32_t nb, const int32_t *batch_dims,
                             ArtnBatchInfo *info) {
  if (!info) return fail(ARTN_E_INVALID, "null info");
  BatchPlan bp;
  ArtnMeasureArgs p;
  if (int rc = batch_measure_plan(d, k, dims, nb, batch_dims, bp, p)) return rc;
  *info = bp.info;
  return ARTN_OK;
}

int artn_measure_batch_choose(const double *q, int64_t B, int64_t D, const double *uniform, const int64_t *forced, int32_t renormalize,
                              void *records, void *stream) {
  if (artn_device_count() < 1) return fail(ARTN_E_NODEVICE, "no gfx950 device visible");
  if (D < 1 || D > ((int64_t)1 << ARTN_MEASURE_MAX_DIMS)) return fail(ARTN_E_INVALID, "the number of outcomes is out of range");
  if (B < 1 || B > ((int64_t)1 << ARTN_BATCH_MAX_BITS)) return fail(ARTN_E_INVALID, "the number of trajectories is out of range");
  if (!q || !records || (!forced && !uniform)) return fail(ARTN_E_INVALID, "null pointer");
  if ((((uintptr_t)q | (uintptr_t)uniform | (uintptr_t)forced | (uintptr_t)records) & 7) != 0)
    return fail(ARTN_E_UNSUPPORTED, "artn_measure_batch_choose needs 8-byte aligned arrays");
  const unsigned grid = (unsigned)((B + ARTN_BATCH_CHOOSE_THREADS - 1) / ARTN_BATCH_CHOOSE_THREADS);
  hipLaunchKernelGGL(artn_k_measure_batch_choose, dim3(grid), dim3(ARTN_BATCH_CHOOSE_THREADS), 0, (hipStream_t)stream, q, (long)B, (long)D,
                     uniform, (const long long *)forced, (int)renormalize, (ArtnMeasureRecord *)records);
  HIP_TRY(hipGetLastError());
  return ARTN_OK;
}

int artn_measure_batch_collapse(const ArtnMarginalDesc *d, void *a, int32_t k, const int32_t *dims, int32_t nb, const int32_t *batch_dims,
                                const void *records, int32_t reset, void *stream) {
  if (artn_device_count() < 1) return fail(ARTN_E_NODEVICE, "no gfx950 device visible");
  BatchPlan bp;
  ArtnMeasureArgs p;
  if (int rc = batch_measure_plan(d, k, dims, nb, batch_dims, bp, p)) return rc;
  if (!a || !records) return fail(ARTN_E_INVALID, "null pointer");
  if (int rc = state_array_aligned(a, "artn_measure_batch_collapse")) return rc;
  if (((uintptr_t)records & 7) != 0) return fail(ARTN_E_UNSUPPORTED, "artn_measure_batch_collapse needs 8-byte aligned records");
  hipStream_t st = (hipStream_t)stream;
  if (d->dtype == ARTN_C64)
    batch_measure_launch<float2>((float2 *)a, bp, p, (const ArtnMeasureRecord *)records, reset != 0, st);
  else
    batch_measure_launch<double2>((double2 *)a, bp, p, (const ArtnMeasureRecord *)records, reset != 0, st);
  HIP_TRY(hipGetLastError());
  return ARTN_OK;
}

int artn_channel_batch_query(const ArtnMarginalDesc *d, int32_t t, const int32_t *dims, int32_t nb, const int32_t *batch_dims, int32_t m,
                             int32_t form, const double *mats, ArtnBatchInfo *info, int32_t *target_bits, int32_t *tile_bits) {
  if (!info) return fail(ARTN_E_INVALID, "null info");
  BatchPlan bp;
  ArtnBatchWalk wk;
  if (int rc = batch_channel_plan(d, t, dims, nb, batch_dims, m, form, mats, bp, wk)) return rc;
  *info = bp.info;
  if (target_bits) std::copy(bp.target.begin(), bp.target.end(), target_bits);
  if (tile_bits) std::copy(bp.tile.begin(), bp.tile.end(), tile_bits);
  return ARTN_OK;
}

int artn_channel_batch_pack(const ArtnMarginalDesc *d, int32_t t, const int32_t *dims, int32_t nb, const int32_t *batch_dims, int32_t m,
                            int32_t form, const double *mats, const double *weights, void *table, int64_t table_bytes) {
  if (!mats || !weights) return fail(ARTN_E_INVALID, "null pointer");
  BatchPlan bp;
  ArtnBatchWalk wk;
  if (int rc = batch_channel_plan(d, t, dims, nb, batch_dims, m, form, mats, bp, wk)) return rc;
  // operators, weights, matrices, block masks and flags: those of the unbatched table ...
  if (int rc = artn_channel_pack(d, t, dims, m, form, mats, weights, table, table_bytes)) return rc;
  // ... and the tile fields from the batch plan (state_tile_header, with room for no more high bits than the table lists)
  ArtnWgateTable &g = ((ArtnChannelTable *)table)->gate;
  g.tile_bits = (uint64_t)bp.tb, g.n_tiles = (uint64_t)bp.n_tiles, g.segment = (uint64_t)bp.segment;
  g.group_bits = (uint64_t)(bp.tb - t), g.n_high = (uint64_t)(bp.tb - bp.seg_bits);
  for (int j = 0; j < ARTN_WGATE_MAX_K; ++j) g.target_bit[j] = g.target_pos[j] = g.high_bit[j] = g.swizzle[j] = 0;
  for (int j = 0; j < 16; ++j) g.mem_col[j] = g.lds_col[j] = 0;
  for (int j = bp.seg_bits; j < bp.tb && j - bp.seg_bits < ARTN_WGATE_MAX_K; ++j) g.high_bit[j - bp.seg_bits] = (uint64_t)bp.tile[j];
  state_tile_cols(bp, g.mem_col, g.lds_col, g.target_bit, g.target_pos, g.swizzle);
  return ARTN_OK;
}

int artn_channel_batch_choose(const void *table, int64_t table_bytes, int32_t t, int32_t m, int32_t form, const double *input,
                              const double *uniform, int64_t B, int32_t renormalize, void *records, void *stream) {
  if (artn_device_count() < 1) return fail(ARTN_E_NODEVICE, "no gfx950 device visible");
  if (int rc = batch_counts(t, m, form)) return rc;
  if (B < 1 || B > ((int64_t)1 << ARTN_BATCH_MAX_BITS)) return fail(ARTN_E_INVALID, "the number of trajectories is out of range");
  if (!table || !uniform || !records || (form != ARTN_CHANNEL_FIXED && !input)) return fail(ARTN_E_INVALID, "null pointer");
  if (int rc = state_table_fits(table_bytes, batch_table_bytes(t, m, form), "artn_channel_batch_query")) return rc;
  if (int rc = state_table_aligned(table, "artn_channel_batch_choose")) return rc;
  if ((((uintptr_t)input | (uintptr_t)uniform | (uintptr_t)records) & 7) != 0)
    return fail(ARTN_E_UNSUPPORTED, "artn_channel_batch_choose needs 8-byte aligned arrays");
  const unsigned grid = (unsigned)((B + ARTN_BATCH_CHOOSE_THREADS - 1) / ARTN_BATCH_CHOOSE_THREADS);
  hipLaunchKernelGGL(artn_k_channel_batch_choose, dim3(grid), dim3(ARTN_BATCH_CHOOSE_THREADS), 0, (hipStream_t)stream,
                     (const ArtnChannelTable *)table, (int)t, (int)m, (int)form, input, uniform, (long)B, (int)renormalize,
                     (ArtnChannelRecord *)records);
  HIP_TRY(hipGetLastError());
  return ARTN_OK;
}

int artn_channel_batch_apply(const ArtnMarginalDesc *d, void *a, int32_t t, const int32_t *dims, int32_t nb, const int32_t *batch_dims,
                             int32_t m, const void *table, int64_t table_bytes, const void *records, void *stream) {
  if (artn_device_count() < 1) return fail(ARTN_E_NODEVICE, "no gfx950 device visible");
  BatchPlan bp;
  ArtnBatchWalk wk;
  if (int rc = batch_channel_plan(d, t, dims, nb, batch_dims, m, ARTN_CHANNEL_FIXED, nullptr, bp, wk)) return rc;
  if (!a || !table || !records) return fail(ARTN_E_INVALID, "null pointer");
  // (the smallest table of any form: the kernel's own reads are bounded by the m and weight_doubles the table states, which
  // artn_channel_batch_pack wrote for a table of the size its query reported)
  if (int rc = state_table_fits(table_bytes, bp.info.table_bytes, "artn_channel_batch_query")) return rc;
  if (int rc = state_array_aligned(a, "artn_channel_batch_apply")) return rc;
  if (int rc = state_table_aligned(table, "artn_channel_batch_apply")) return rc;
  if (((uintptr_t)records & 7) != 0) return fail(ARTN_E_UNSUPPORTED, "artn_channel_batch_apply needs 8-byte aligned records");
  hipStream_t st = (hipStream_t)stream;
  if (d->dtype == ARTN_C64) batch_channel_launch(bp, wk, t, m, (float2 *)a, table, records, st);
  else batch_channel_launch(bp, wk, t, m, (double2 *)a, table, records, st);
  HIP_TRY(hipGetLastError());
  return ARTN_OK;
}

} // extern "C"
