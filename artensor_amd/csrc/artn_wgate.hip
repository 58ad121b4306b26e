// artn_wgate.hip -- host half of the one-gate entry points artn_wgate_* of include/artn.h (kernel: artn_wgate_kernel.h).
//
// A translation unit of its own (build/obj/wgate.o).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "artn_host.h"
#include "artn_state_host.h"
#include "artn_wgate_kernel.h"

struct WgatePlan : TilePlan {
  int k = 0, n_bits = 0;
  ArtnWgateInfo info = {};
};

// The layout checks of artn_gates_query, then the target bits and the tile (include/artn.h: PLAN).  `mat` may be null
// (artn_wgate_apply: the matrix is in the table); the flag "diagonal" is then not set.
static int wgate_plan(const ArtnMarginalDesc *d, int32_t k, const int32_t *dims, const double *mat, WgatePlan &wp) {
  if (int rc = state_desc(d, "wide gates take", ARTN_MARG_MAX_DIMS, false)) return rc;
  if (!dims) return fail(ARTN_E_INVALID, "null pointer");
  StateLayout l;
  if (int rc = state_layout(d, l)) return rc;
  if (int rc = state_bits_only(l, "wide gates take")) return rc;
  const int64_t n = l.n;
  if (k < 1 || k > ARTN_WGATE_MAX_K)
    return fail(ARTN_E_UNSUPPORTED, "wide gates act on one to five dimensions, not " + std::to_string(k));
  const int n_bits = __builtin_ctzll((uint64_t)n);
  if (k > n_bits)
    return fail(ARTN_E_INVALID, "a gate on " + std::to_string(k) + " dimensions needs a state of at least 2^" + std::to_string(k) +
                                    " elements; this one has " + std::to_string((long long)n));
  wp.k = k, wp.n_bits = n_bits;
  if (int rc = state_tile_targets(d, k, dims, "gates", wp.target)) return rc;
  bool diagonal = false;
  if (mat && !state_matrix_scan(mat, 1 << k, diagonal)) return fail(ARTN_E_INVALID, "a matrix entry is not finite");
  state_tile_plan(d->dtype, n_bits, 0, wp);
  wp.info.k = k, wp.info.tile_bits = wp.tb, wp.info.diagonal = diagonal ? 1 : 0;
  wp.info.n_tiles = wp.n_tiles, wp.info.segment = wp.segment, wp.info.lds_bytes = wp.lds_bytes;
  wp.info.table_bytes = (int64_t)sizeof(ArtnWgateTable) + ((int64_t)16 << (2 * k));
  wp.info.bytes_read = wp.info.bytes_written = n * wp.elem;
  return ARTN_OK;
}

template <typename T>
static void wgate_launch(const WgatePlan &wp, T *a, const void *table, hipStream_t st) {
  const ArtnWgateTable *tab = (const ArtnWgateTable *)table;
  const dim3 grid((unsigned)std::min<int64_t>(wp.info.n_tiles, ARTN_WGATE_MAX_GRID)), block(ARTN_BORN_THREADS);
  const size_t lds = (size_t)wp.info.lds_bytes;
  state_with_k(wp.k, [&](auto k) { hipLaunchKernelGGL((artn_k_wgate<T, decltype(k)::value>), grid, block, lds, st, a, tab); });
}

extern "C" {

int artn_wgate_query(const ArtnMarginalDesc *d, int32_t k, const int32_t *dims, const double *mat, ArtnWgateInfo *info,
                     int32_t *target_bits, int32_t *tile_bits) {
  if (!info) return fail(ARTN_E_INVALID, "null info");
  if (!mat) return fail(ARTN_E_INVALID, "null pointer");
  WgatePlan wp;
  if (int rc = wgate_plan(d, k, dims, mat, wp)) return rc;
  *info = wp.info;
  if (target_bits) std::copy(wp.target.begin(), wp.target.end(), target_bits);
  if (tile_bits) std::copy(wp.tile.begin(), wp.tile.end(), tile_bits);
  return ARTN_OK;
}

int artn_wgate_pack(const ArtnMarginalDesc *d, int32_t k, const int32_t *dims, const double *mat, void *table, int64_t table_bytes) {
  if (!mat) return fail(ARTN_E_INVALID, "null pointer");
  WgatePlan wp;
  if (int rc = wgate_plan(d, k, dims, mat, wp)) return rc;
  if (!table) return fail(ARTN_E_INVALID, "null pointer");
  if (int rc = state_table_fits(table_bytes, wp.info.table_bytes, "artn_wgate_query")) return rc;
  if (int rc = state_table_aligned(table, "artn_wgate_pack")) return rc;
  ArtnWgateTable t = {};
  const int rows = 1 << k, gb = wp.tb - k;
  t.k = (uint64_t)k, t.tile_bits = (uint64_t)wp.tb, t.n_tiles = (uint64_t)wp.info.n_tiles, t.segment = (uint64_t)wp.info.segment;
  t.flags = wp.info.diagonal ? ARTN_GATE_DIAGONAL : 0, t.group_bits = (uint64_t)gb, t.n_high = (uint64_t)(wp.tb - wp.seg_bits);
  for (int j = wp.seg_bits; j < wp.tb; ++j) t.high_bit[j - wp.seg_bits] = (uint64_t)wp.tile[j]; // (all targets: include/artn.h)
  state_tile_cols(wp, t.mem_col, t.lds_col, t.target_bit, t.target_pos, t.swizzle);
  t.block_mask = state_block_mask(mat, rows);
  *(ArtnWgateTable *)table = t;
  std::copy(mat, mat + 2 * rows * rows, (double *)((ArtnWgateTable *)table + 1));
  return ARTN_OK;
}

int artn_wgate_apply(const ArtnMarginalDesc *d, void *a, int32_t k, const int32_t *dims, const void *table, int64_t table_bytes,
                     void *stream) {
  if (artn_device_count() < 1) return fail(ARTN_E_NODEVICE, "no gfx950 device visible");
  WgatePlan wp;
  if (int rc = wgate_plan(d, k, dims, nullptr, wp)) return rc;
  if (!a || !table) return fail(ARTN_E_INVALID, "null pointer");
  if (int rc = state_table_fits(table_bytes, wp.info.table_bytes, "artn_wgate_query")) return rc;
  if (int rc = state_array_aligned(a, "artn_wgate_apply")) return rc;
  if (int rc = state_table_aligned(table, "artn_wgate_apply")) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (d->dtype == ARTN_C64) wgate_launch(wp, (float2 *)a, table, st);
  else wgate_launch(wp, (double2 *)a, table, st);
  HIP_TRY(hipGetLastError());
  return ARTN_OK;
}

} // extern "C"
