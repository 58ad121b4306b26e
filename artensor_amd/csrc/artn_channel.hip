// artn_channel.hip -- host half of the noise-channel entry points artn_channel_* of include/artn.h (kernels: artn_channel_kernel.h).
//
// A translation unit of its own (build/obj/channel.o).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "artn_host.h"
#include "artn_state_host.h"
#include "artn_channel_kernel.h"

static_assert(sizeof(ArtnChannelTable) == 512 && sizeof(ArtnChannelOp) == 16, "the table's header and operator records");
static_assert(sizeof(ArtnChannelRecord) == ARTN_MEASURE_RECORD_BYTES, "int64 outcome, then probability, total and scale");

struct ChannelPlan : TilePlan {
  int t = 0, m = 0, form = 0, n_bits = 0;
  ArtnChannelInfo info = {};
};

static int64_t channel_weight_doubles(int form, int t) {
  return form == ARTN_CHANNEL_FIXED ? 1 : form == ARTN_CHANNEL_DIAGONAL ? (int64_t)1 << t : (int64_t)2 << (2 * t);
}

// t, m and form alone: what artn_channel_choose can check (it sees no descriptor)
static int channel_counts(int32_t t, int32_t m, int32_t form) {
  if (t < 1 || t > ARTN_WGATE_MAX_K)
    return fail(ARTN_E_UNSUPPORTED, "channels act on one to five dimensions, not " + std::to_string(t));
  if (m < 1 || m > ARTN_CHANNEL_MAX_OPS)
    return fail(ARTN_E_INVALID, "a channel has 1 to " + std::to_string(ARTN_CHANNEL_MAX_OPS) + " operators, not " + std::to_string(m));
  if (form != ARTN_CHANNEL_FIXED && form != ARTN_CHANNEL_DIAGONAL && form != ARTN_CHANNEL_DENSE)
    return fail(ARTN_E_INVALID, "unknown weight form " + std::to_string(form));
  return ARTN_OK;
}

static int64_t channel_table_bytes(int t, int m, int form) {
  return (int64_t)sizeof(ArtnChannelTable) + (int64_t)m * ((int64_t)sizeof(ArtnChannelOp) + 8 * channel_weight_doubles(form, t) +
                                                           ((int64_t)16 << (2 * t)));
}
static int64_t channel_record_bytes(int t) { return ARTN_MEASURE_RECORD_BYTES + ((int64_t)16 << (2 * t)); }

// The layout checks and the tile of artn_wgate_query (include/artn.h: PLAN), then m and the form.  `mats` may be null: nothing
// is scanned then.
static int channel_plan(const ArtnMarginalDesc *d, int32_t t, const int32_t *dims, int32_t m, int32_t form, const double *mats,
                        ChannelPlan &cp) {
  if (int rc = state_desc(d, "channels take", ARTN_MARG_MAX_DIMS, false)) return rc;
  if (!dims) return fail(ARTN_E_INVALID, "null pointer");
  StateLayout l;
  if (int rc = state_layout(d, l)) return rc;
  if (int rc = state_bits_only(l, "channels take")) return rc;
  const int64_t n = l.n;
  if (t < 1 || t > ARTN_WGATE_MAX_K)
    return fail(ARTN_E_UNSUPPORTED, "channels act on one to five dimensions, not " + std::to_string(t));
  const int n_bits = __builtin_ctzll((uint64_t)n);
  if (t > n_bits)
    return fail(ARTN_E_INVALID, "a channel on " + std::to_string(t) + " dimensions needs a state of at least 2^" + std::to_string(t) +
                                    " elements; this one has " + std::to_string((long long)n));
  cp.t = t, cp.m = m, cp.form = form, cp.n_bits = n_bits;
  if (int rc = state_tile_targets(d, t, dims, "channels", cp.target)) return rc;
  if (int rc = channel_counts(t, m, form)) return rc;
  if (mats)
    for (int j = 0; j < m; ++j) {
      bool diagonal = false;
      if (!state_matrix_scan(mats + ((size_t)j << (2 * t + 1)), 1 << t, diagonal))
        return fail(ARTN_E_INVALID, "an entry of operator " + std::to_string(j) + " is not finite");
    }
  state_tile_plan(d->dtype, n_bits, 0, cp);
  ArtnChannelInfo &ci = cp.info;
  ci.t = t, ci.m = m, ci.form = form, ci.tile_bits = cp.tb;
  for (int f = 0; f < 3; ++f) ci.launches[f] = 2, ci.reduction[f] = f;
  ci.n_tiles = cp.n_tiles, ci.segment = cp.segment, ci.lds_bytes = cp.lds_bytes;
  ci.weight_doubles = channel_weight_doubles(form, t);
  ci.table_bytes = channel_table_bytes(t, m, form), ci.record_bytes = channel_record_bytes(t);
  ci.bytes_read = ci.bytes_written = n * cp.elem;
  return ARTN_OK;
}

template <typename T>
static void channel_launch(const ChannelPlan &cp, T *a, const void *table, const void *record, hipStream_t st) {
  const ArtnChannelTable *tab = (const ArtnChannelTable *)table;
  const ArtnChannelRecord *rec = (const ArtnChannelRecord *)record;
  const dim3 grid((unsigned)std::min<int64_t>(cp.info.n_tiles, ARTN_WGATE_MAX_GRID)), block(ARTN_BORN_THREADS);
  const size_t lds = (size_t)cp.info.lds_bytes;
  const int m = cp.m;
  state_with_k<1, ARTN_WGATE_MAX_K>(cp.t, [&](auto k) {
    hipLaunchKernelGGL((artn_k_channel<T, decltype(k)::value>), grid, block, lds, st, a, tab, rec, m);
  });
}

static int channel_record_fits(int64_t record_bytes, int t) {
  if (record_bytes < channel_record_bytes(t)) return fail(ARTN_E_INVALID, "record smaller than artn_channel_query reports");
  return ARTN_OK;
}

extern "C" {

int artn_channel_query(const ArtnMarginalDesc *d, int32_t t, const int32_t *dims, int32_t m, int32_t form, const double *mats,
                       ArtnChannelInfo *info, int32_t *target_bits, int32_t *tile_bits) {
  if (!info) return fail(ARTN_E_INVALID, "null info");
  ChannelPlan cp;
  if (int rc = channel_plan(d, t, dims, m, form, mats, cp)) return rc;
  *info = cp.info;
  if (target_bits) std::copy(cp.target.begin(), cp.target.end(), target_bits);
  if (tile_bits) std::copy(cp.tile.begin(), cp.tile.end(), tile_bits);
  return ARTN_OK;
}

int artn_channel_pack(const ArtnMarginalDesc *d, int32_t t, const int32_t *dims, int32_t m, int32_t form, const double *mats,
                      const double *weights, void *table, int64_t table_bytes) {
  if (!mats || !weights) return fail(ARTN_E_INVALID, "null pointer");
  ChannelPlan cp;
  if (int rc = channel_plan(d, t, dims, m, form, mats, cp)) return rc;
  const int64_t wd = cp.info.weight_doubles;
  for (int64_t e = 0; e < wd * m; ++e)
    if (!std::isfinite(weights[e])) return fail(ARTN_E_INVALID, "a weight of operator " + std::to_string(e / wd) + " is not finite");
  if (!table) return fail(ARTN_E_INVALID, "null pointer");
  if (int rc = state_table_fits(table_bytes, cp.info.table_bytes, "artn_channel_query")) return rc;
  if (int rc = state_table_aligned(table, "artn_channel_pack")) return rc;
  ArtnChannelTable ct = {};
  ArtnWgateTable &g = ct.gate;
  const int rows = 1 << t;
  state_tile_header(cp, t, false, g); // (the flag "diagonal": below, once every operator has been scanned)
  ct.m = (uint64_t)m, ct.form = (uint64_t)form, ct.weight_doubles = (uint64_t)wd;
  // per operator: the block mask, "diagonal" and "exactly the identity"
  ArtnChannelOp *ops = (ArtnChannelOp *)((ArtnChannelTable *)table + 1);
  bool all_diagonal = true;
  for (int j = 0; j < m; ++j) {
    const double *mat = mats + ((size_t)j << (2 * t + 1));
    ArtnChannelOp op = {};
    op.block_mask = state_block_mask(mat, rows);
    bool diagonal = true;
    state_matrix_scan(mat, rows, diagonal);
    bool identity = diagonal;
    for (int row = 0; row < rows; ++row)
      if (mat[2 * (row * rows + row)] != 1.0 || mat[2 * (row * rows + row) + 1] != 0.0) identity = false;
    op.flags = (diagonal ? ARTN_CHANNEL_OP_DIAGONAL : 0) | (identity ? ARTN_CHANNEL_OP_IDENTITY : 0);
    ops[j] = op;
    g.block_mask |= op.block_mask;
    all_diagonal = all_diagonal && diagonal;
  }
  g.flags = all_diagonal ? ARTN_GATE_DIAGONAL : 0;
  *(ArtnChannelTable *)table = ct;
  double *w = (double *)(ops + m);
  std::copy(weights, weights + wd * m, w);
  std::copy(mats, mats + ((size_t)m << (2 * t + 1)), w + wd * m);
  return ARTN_OK;
}

int artn_channel_choose(const void *table, int64_t table_bytes, int32_t t, int32_t m, int32_t form, const double *input,
                        const double *uniform, int32_t renormalize, void *record, int64_t record_bytes, void *stream) {
  if (artn_device_count() < 1) return fail(ARTN_E_NODEVICE, "no gfx950 device visible");
  if (int rc = channel_counts(t, m, form)) return rc;
  if (!table || !uniform || !record || (form != ARTN_CHANNEL_FIXED && !input)) return fail(ARTN_E_INVALID, "null pointer");
  if (int rc = state_table_fits(table_bytes, channel_table_bytes(t, m, form), "artn_channel_query")) return rc;
  if (int rc = channel_record_fits(record_bytes, t)) return rc;
  if (int rc = state_table_aligned(table, "artn_channel_choose")) return rc;
  if ((((uintptr_t)input | (uintptr_t)uniform | (uintptr_t)record) & 7) != 0)
    return fail(ARTN_E_UNSUPPORTED, "artn_channel_choose needs 8-byte aligned arrays");
  hipLaunchKernelGGL(artn_k_channel_choose, dim3(1), dim3(ARTN_CHANNEL_THREADS), 0, (hipStream_t)stream,
                     (const ArtnChannelTable *)table, (int)t, (int)m, (int)form, input, uniform, (int)renormalize,
                     (ArtnChannelRecord *)record);
  HIP_TRY(hipGetLastError());
  return ARTN_OK;
}

int artn_channel_apply(const ArtnMarginalDesc *d, void *a, int32_t t, const int32_t *dims, int32_t m, const void *table,
                       int64_t table_bytes, const void *record, int64_t record_bytes, void *stream) {
  if (artn_device_count() < 1) return fail(ARTN_E_NODEVICE, "no gfx950 device visible");
  ChannelPlan cp;
  if (int rc = channel_plan(d, t, dims, m, ARTN_CHANNEL_FIXED, nullptr, cp)) return rc;
  if (!a || !table || !record) return fail(ARTN_E_INVALID, "null pointer");
  // (the smallest table of any form: the kernel reads the header and the operator records only)
  if (int rc = state_table_fits(table_bytes, cp.info.table_bytes, "artn_channel_query")) return rc;
  if (int rc = channel_record_fits(record_bytes, t)) return rc;
  if (int rc = state_array_aligned(a, "artn_channel_apply")) return rc;
  if (int rc = state_table_aligned(table, "artn_channel_apply")) return rc;
  if (((uintptr_t)record & 7) != 0) return fail(ARTN_E_UNSUPPORTED, "artn_channel_apply needs an 8-byte aligned record");
  hipStream_t st = (hipStream_t)stream;
  if (d->dtype == ARTN_C64) channel_launch(cp, (float2 *)a, table, record, st);
  else channel_launch(cp, (double2 *)a, table, record, st);
  HIP_TRY(hipGetLastError());
  return ARTN_OK;
}

} // extern "C"
