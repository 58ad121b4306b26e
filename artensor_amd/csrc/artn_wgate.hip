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

struct WgatePlan {
  int k = 0, n_bits = 0, tb = 0, seg_bits = 0;
  std::vector<int> target;  // memory bits in the order listed
  std::vector<int> tile;    // tile bits, ascending
  ArtnWgateInfo info = {};
};

// The layout checks of artn_gates_query, then the target bits and the tile (include/artn.h: PLAN).  `mat` may be null
// (artn_wgate_apply: the matrix is in the table); the flag "diagonal" is then not set.
static int wgate_plan(const ArtnMarginalDesc *d, int32_t k, const int32_t *dims, const double *mat, WgatePlan &wp) {
  if (int rc = state_desc(d, "wide gates take", ARTN_MARG_MAX_DIMS, false)) return rc;
  if (!dims) return fail(ARTN_E_INVALID, "null pointer");
  const int nd = d->n_dims;
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
  for (int j = 0; j < k; ++j) {
    const int32_t dim = dims[j];
    if (dim < 0 || dim >= nd) return fail(ARTN_E_INVALID, "dimension " + std::to_string(dim) + " out of range");
    if (d->extent[dim] != 2)
      return fail(ARTN_E_INVALID, "gates act on dimensions of extent 2; dimension " + std::to_string(dim) + " has extent " +
                                      std::to_string(d->extent[dim]));
    for (int i = 0; i < j; ++i)
      if (dims[i] == dim) return fail(ARTN_E_INVALID, "the dimensions must differ; dimension " + std::to_string(dim) + " is repeated");
    wp.target.push_back(__builtin_ctzll((uint64_t)d->stride[dim]));
  }
  bool diagonal = false;
  if (mat && !state_matrix_scan(mat, 1 << k, diagonal)) return fail(ARTN_E_INVALID, "a matrix entry is not finite");
  const int tb_max = d->dtype == ARTN_C64 ? ARTN_WGATE_TILE_BITS_C64 : ARTN_WGATE_TILE_BITS_C128;
  wp.tb = std::min(tb_max, n_bits);
  wp.tile = wp.target;
  for (int b = 0; (int)wp.tile.size() < wp.tb; ++b)
    if (std::find(wp.target.begin(), wp.target.end(), b) == wp.target.end()) wp.tile.push_back(b);
  std::sort(wp.tile.begin(), wp.tile.end());
  wp.seg_bits = 0;
  while (wp.seg_bits < wp.tb && wp.tile[wp.seg_bits] == wp.seg_bits) ++wp.seg_bits;
  const int64_t elem = d->dtype == ARTN_C64 ? 8 : 16;
  wp.info.k = k, wp.info.tile_bits = wp.tb, wp.info.diagonal = diagonal ? 1 : 0;
  wp.info.n_tiles = n >> wp.tb, wp.info.segment = (int64_t)1 << wp.seg_bits;
  wp.info.lds_bytes = elem << wp.tb;
  wp.info.table_bytes = (int64_t)sizeof(ArtnWgateTable) + ((int64_t)16 << (2 * k));
  wp.info.bytes_read = wp.info.bytes_written = n * elem;
  return ARTN_OK;
}

template <typename T>
static void wgate_launch(const WgatePlan &wp, T *a, const void *table, hipStream_t st) {
  const ArtnWgateTable *tab = (const ArtnWgateTable *)table;
  const dim3 grid((unsigned)std::min<int64_t>(wp.info.n_tiles, ARTN_WGATE_MAX_GRID)), block(ARTN_BORN_THREADS);
  const size_t lds = (size_t)wp.info.lds_bytes;
  switch (wp.k) {
  case 1: hipLaunchKernelGGL((artn_k_wgate<T, 1>), grid, block, lds, st, a, tab); break;
  case 2: hipLaunchKernelGGL((artn_k_wgate<T, 2>), grid, block, lds, st, a, tab); break;
  case 3: hipLaunchKernelGGL((artn_k_wgate<T, 3>), grid, block, lds, st, a, tab); break;
  case 4: hipLaunchKernelGGL((artn_k_wgate<T, 4>), grid, block, lds, st, a, tab); break;
  case 5: hipLaunchKernelGGL((artn_k_wgate<T, 5>), grid, block, lds, st, a, tab); break;
  }
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
  // the swizzle: the window is the lowest P = min(6, gb) tile-local bits; its non-targets are group bits 0 .. P-j-1 and LDS
  // index bits of the same number, its j targets get the LDS index bits P-j .. P-1
  const int window = std::min(6, gb);
  int low_targets = 0;
  for (int p = 0; p < window; ++p)
    if (std::find(wp.target.begin(), wp.target.end(), wp.tile[p]) != wp.target.end()) ++low_targets;
  int rank = 0, seen = 0; // non-targets / window targets below the position
  for (int p = 0; p < wp.tb; ++p) {
    t.mem_col[p] = (uint64_t)1 << wp.tile[p];
    const auto at = std::find(wp.target.begin(), wp.target.end(), wp.tile[p]);
    if (at == wp.target.end()) {
      t.lds_col[p] = (uint64_t)1 << rank++;
      continue;
    }
    const int listed = (int)(at - wp.target.begin()), row_bit = k - 1 - listed; // the LAST listed target is row bit 0
    t.target_bit[listed] = (uint64_t)wp.tile[p], t.target_pos[listed] = (uint64_t)p;
    if (p < window) t.swizzle[row_bit] = (uint64_t)1 << (window - low_targets + seen++);
    t.lds_col[p] = ((uint64_t)1 << (gb + row_bit)) ^ t.swizzle[row_bit];
  }
  const int r = std::min(rows, ARTN_WGATE_ROWS), nb = rows / r;
  for (int row = 0; row < rows; ++row)
    for (int col = 0; col < rows; ++col)
      if (mat[2 * (row * rows + col)] != 0.0 || mat[2 * (row * rows + col) + 1] != 0.0)
        t.block_mask |= (uint64_t)1 << ((row / r) * nb + col / r);
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
