// artn_cgate.hip -- host half of the controlled-gate entry points artn_cgate_* of include/artn.h (kernel: artn_cgate_kernel.h).
//
// A translation unit of its own (build/obj/cgate.o).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "artn_host.h"
#include "artn_state_host.h"
#include "artn_cgate_kernel.h"
#include "artn_cgate_host.h"

// The layout checks of artn_wgate_query, then targets, controls, their classes, the tile and the holes (include/artn.h: PLAN).
// `mat` may be null (artn_cgate_apply: the matrix is in the table); the flag "diagonal" is then not set.
static int cgate_plan(const ArtnMarginalDesc *d, int32_t t, const int32_t *targets, int32_t c, const int32_t *controls,
                      const int32_t *values, const double *mat, CgatePlan &cp) {
  int64_t n = 0;
  if (int rc = cgate_head(d, t, targets, c, controls, "controlled gates take", "controlled gates", cp, n)) return rc;
  const int n_bits = cp.n_bits;
  if (t > n_bits)
    return fail(ARTN_E_INVALID, "a gate on " + std::to_string(t) + " dimensions needs a state of at least 2^" + std::to_string(t) +
                                    " elements; this one has " + std::to_string((long long)n));
  std::vector<int32_t> seen;
  if (int rc = cgate_dims(d, targets, controls, values, cp, seen)) return rc;
  const int c_high = cp.c_high;
  bool diagonal = false;
  if (mat && !state_matrix_scan(mat, 1 << t, diagonal)) return fail(ARTN_E_INVALID, "a matrix entry is not finite");
  state_tile_plan(d->dtype, n_bits - c_high, cp.high_mask, cp);
  if (int rc = cgate_holes(cp, "controlled gates take")) return rc;
  cp.info.t = t, cp.info.c = c, cp.info.c_high = c_high, cp.info.c_low = c - c_high;
  cp.info.tile_bits = cp.tb, cp.info.diagonal = diagonal ? 1 : 0;
  cp.info.n_selected = n >> c, cp.info.n_tiles = cp.n_tiles, cp.info.segment = cp.segment, cp.info.lds_bytes = cp.lds_bytes;
  cp.info.table_bytes = (int64_t)sizeof(ArtnCgateTable) + ((int64_t)16 << (2 * t));
  cp.info.bytes_read = cp.info.bytes_written = (n >> c_high) * cp.elem;
  return ARTN_OK;
}

template <typename T>
static void cgate_launch(const CgatePlan &cp, T *a, const void *table, const void *cond, int64_t mask, int64_t value, hipStream_t st) {
  const ArtnCgateTable *tab = (const ArtnCgateTable *)table;
  const long long *cnd = (const long long *)cond;
  const long long m = (long long)mask, v = (long long)value;
  const dim3 grid((unsigned)std::min<int64_t>(cp.info.n_tiles, ARTN_WGATE_MAX_GRID)), block(ARTN_BORN_THREADS);
  const size_t lds = (size_t)cp.info.lds_bytes;
  state_with_k<1, ARTN_WGATE_MAX_K>(cp.t, [&](auto k) {
    hipLaunchKernelGGL((artn_k_cgate<T, decltype(k)::value>), grid, block, lds, st, a, tab, cnd, m, v);
  });
}

extern "C" {

int artn_cgate_query(const ArtnMarginalDesc *d, int32_t t, const int32_t *targets, int32_t c, const int32_t *controls,
                     const int32_t *control_values, const double *mat, ArtnCgateInfo *info, int32_t *target_bits,
                     int32_t *control_bits, int32_t *tile_bits) {
  if (!info) return fail(ARTN_E_INVALID, "null info");
  if (!mat) return fail(ARTN_E_INVALID, "null pointer");
  CgatePlan cp;
  if (int rc = cgate_plan(d, t, targets, c, controls, control_values, mat, cp)) return rc;
  *info = cp.info;
  if (target_bits) std::copy(cp.target.begin(), cp.target.end(), target_bits);
  if (control_bits) std::copy(cp.control.begin(), cp.control.end(), control_bits);
  if (tile_bits) std::copy(cp.tile.begin(), cp.tile.end(), tile_bits);
  return ARTN_OK;
}

int artn_cgate_pack(const ArtnMarginalDesc *d, int32_t t, const int32_t *targets, int32_t c, const int32_t *controls,
                    const int32_t *control_values, const double *mat, void *table, int64_t table_bytes) {
  if (!mat) return fail(ARTN_E_INVALID, "null pointer");
  CgatePlan cp;
  if (int rc = cgate_plan(d, t, targets, c, controls, control_values, mat, cp)) return rc;
  if (!table) return fail(ARTN_E_INVALID, "null pointer");
  if (int rc = state_table_fits(table_bytes, cp.info.table_bytes, "artn_cgate_query")) return rc;
  if (int rc = state_table_aligned(table, "artn_cgate_pack")) return rc;
  ArtnCgateTable tab = {};
  const int rows = 1 << t;
  cgate_tile_fields(cp, tab);
  tab.flags = cp.info.diagonal ? ARTN_GATE_DIAGONAL : 0;
  tab.block_mask = state_block_mask(mat, rows);
  *(ArtnCgateTable *)table = tab;
  std::copy(mat, mat + 2 * rows * rows, (double *)((ArtnCgateTable *)table + 1));
  return ARTN_OK;
}

int artn_cgate_apply(const ArtnMarginalDesc *d, void *a, int32_t t, const int32_t *targets, int32_t c, const int32_t *controls,
                     const int32_t *control_values, const void *table, int64_t table_bytes, const void *cond, int64_t cond_mask,
                     int64_t cond_value, void *stream) {
  if (artn_device_count() < 1) return fail(ARTN_E_NODEVICE, "no gfx950 device visible");
  CgatePlan cp;
  if (int rc = cgate_plan(d, t, targets, c, controls, control_values, nullptr, cp)) return rc;
  if (!a || !table) return fail(ARTN_E_INVALID, "null pointer");
  if (int rc = state_table_fits(table_bytes, cp.info.table_bytes, "artn_cgate_query")) return rc;
  if (int rc = state_array_aligned(a, "artn_cgate_apply")) return rc;
  if (int rc = state_table_aligned(table, "artn_cgate_apply")) return rc;
  if (((uintptr_t)cond & 7) != 0) return fail(ARTN_E_UNSUPPORTED, "artn_cgate_apply needs an 8-byte aligned condition");
  hipStream_t st = (hipStream_t)stream;
  if (d->dtype == ARTN_C64) cgate_launch(cp, (float2 *)a, table, cond, cond_mask, cond_value, st);
  else cgate_launch(cp, (double2 *)a, table, cond, cond_mask, cond_value, st);
  HIP_TRY(hipGetLastError());
  return ARTN_OK;
}

} // extern "C"
