// artn_mgate.hip -- host half of the matrix-core gate entry points artn_mgate_* of include/artn.h (kernel: artn_mgate_kernel.h).
//
// A translation unit of its own (build/obj/mgate.o).  The plan is the wide gates' (artn_state_host.h: state_tile_plan,
// state_tile_cols), which is generic in k; only the table type, the range of k and the order of the packed matrix differ.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "artn_host.h"
#include "artn_state_host.h"
#include "artn_mgate_kernel.h"

// a full tile at the widest gate keeps 2^(TB - 7) groups: at least the 16 columns of one instruction, segments of >= 128 bytes
static_assert(ARTN_WGATE_TILE_BITS_C64 - ARTN_MGATE_MAX_K >= 4 && ARTN_WGATE_TILE_BITS_C128 - ARTN_MGATE_MAX_K >= 4, "16 groups per tile");
static_assert((8 << (ARTN_WGATE_TILE_BITS_C64 - ARTN_MGATE_MAX_K)) >= 128 && (16 << (ARTN_WGATE_TILE_BITS_C128 - ARTN_MGATE_MAX_K)) >= 128,
              "segments of at least 128 bytes");

struct MgatePlan : TilePlan {
  int k = 0, n_bits = 0;
  ArtnMgateInfo info = {};
};

// The checks of artn_wgate_query in its order, with k in 3..7.  `mat` may be null (artn_mgate_apply: the matrix is in the table).
static int mgate_plan(const ArtnMarginalDesc *d, int32_t k, const int32_t *dims, const double *mat, MgatePlan &mp) {
  if (int rc = state_desc(d, "matrix gates take", ARTN_MARG_MAX_DIMS, false)) return rc;
  if (!dims) return fail(ARTN_E_INVALID, "null pointer");
  StateLayout l;
  if (int rc = state_layout(d, l)) return rc;
  if (int rc = state_bits_only(l, "matrix gates take")) return rc;
  const int64_t n = l.n;
  if (k < ARTN_MGATE_MIN_K || k > ARTN_MGATE_MAX_K)
    return fail(ARTN_E_UNSUPPORTED, "matrix gates act on three to seven dimensions, not " + std::to_string(k));
  const int n_bits = __builtin_ctzll((uint64_t)n);
  if (k > n_bits)
    return fail(ARTN_E_INVALID, "a gate on " + std::to_string(k) + " dimensions needs a state of at least 2^" + std::to_string(k) +
                                    " elements; this one has " + std::to_string((long long)n));
  mp.k = k, mp.n_bits = n_bits;
  if (int rc = state_tile_targets(d, k, dims, "gates", mp.target)) return rc;
  bool diagonal = false;
  if (mat && !state_matrix_scan(mat, 1 << k, diagonal)) return fail(ARTN_E_INVALID, "a matrix entry is not finite");
  state_tile_plan(d->dtype, n_bits, 0, mp);
  // (a tile of a larger state is made of segments of at least 128 bytes; a state below one tile is one segment or more)
  if (mp.n_tiles > 1 && mp.segment * mp.elem < 128) return fail(ARTN_E_LAUNCH, "internal: a tile segment below 128 bytes");
  mp.info.k = k, mp.info.tile_bits = mp.tb, mp.info.diagonal = diagonal ? 1 : 0;
  mp.info.n_tiles = mp.n_tiles, mp.info.segment = mp.segment, mp.info.lds_bytes = mp.lds_bytes;
  mp.info.table_bytes = (int64_t)sizeof(ArtnMgateTable) + ((int64_t)16 << (2 * k));
  mp.info.bytes_read = mp.info.bytes_written = n * mp.elem;
  return ARTN_OK;
}

// f(std::integral_constant<int, K>) for the run-time k = 3 .. 7; the plan admits no other k
template <int K = ARTN_MGATE_MIN_K, typename F>
static void mgate_with_k(int k, F &&f) {
  if constexpr (K <= ARTN_MGATE_MAX_K) {
    if (k == K) f(std::integral_constant<int, K>());
    else mgate_with_k<K + 1>(k, f);
  }
}

template <typename T>
static void mgate_launch(const MgatePlan &mp, T *a, const void *table, hipStream_t st) {
  const ArtnMgateTable *tab = (const ArtnMgateTable *)table;
  const dim3 grid((unsigned)std::min<int64_t>(mp.info.n_tiles, ARTN_WGATE_MAX_GRID)), block(ARTN_BORN_THREADS);
  const size_t lds = (size_t)mp.info.lds_bytes;
  mgate_with_k(mp.k, [&](auto k) { hipLaunchKernelGGL((artn_k_mgate<T, decltype(k)::value>), grid, block, lds, st, a, tab); });
}

extern "C" {

int artn_mgate_query(const ArtnMarginalDesc *d, int32_t k, const int32_t *dims, const double *mat, ArtnMgateInfo *info,
                     int32_t *target_bits, int32_t *tile_bits) {
  if (!info) return fail(ARTN_E_INVALID, "null info");
  if (!mat) return fail(ARTN_E_INVALID, "null pointer");
  MgatePlan mp;
  if (int rc = mgate_plan(d, k, dims, mat, mp)) return rc;
  *info = mp.info;
  if (target_bits) std::copy(mp.target.begin(), mp.target.end(), target_bits);
  if (tile_bits) std::copy(mp.tile.begin(), mp.tile.end(), tile_bits);
  return ARTN_OK;
}

int artn_mgate_pack(const ArtnMarginalDesc *d, int32_t k, const int32_t *dims, const double *mat, void *table, int64_t table_bytes) {
  if (!mat) return fail(ARTN_E_INVALID, "null pointer");
  MgatePlan mp;
  if (int rc = mgate_plan(d, k, dims, mat, mp)) return rc;
  if (!table) return fail(ARTN_E_INVALID, "null pointer");
  if (int rc = state_table_fits(table_bytes, mp.info.table_bytes, "artn_mgate_query")) return rc;
  if (int rc = state_table_aligned(table, "artn_mgate_pack")) return rc;
  ArtnMgateTable t = {};
  const int rows = 1 << k, steps = rows / 2, gb = mp.tb - k;
  t.k = (uint64_t)k, t.tile_bits = (uint64_t)mp.tb, t.n_tiles = (uint64_t)mp.info.n_tiles, t.segment = (uint64_t)mp.info.segment;
  t.flags = mp.info.diagonal ? ARTN_GATE_DIAGONAL : 0, t.group_bits = (uint64_t)gb, t.n_high = (uint64_t)(mp.tb - mp.seg_bits);
  for (int j = mp.seg_bits; j < mp.tb; ++j) t.high_bit[j - mp.seg_bits] = (uint64_t)mp.tile[j]; // (all targets: include/artn.h)
  state_tile_cols(mp, t.mem_col, t.lds_col, t.target_bit, t.target_pos, t.swizzle);
  *(ArtnMgateTable *)table = t;
  // the matrix in fragment order (include/artn.h: TABLE): [rb][s][n][h][c] <- U[8 rb + n][2 s + h], c = Re, Im
  double *out = (double *)((ArtnMgateTable *)table + 1);
  for (int rb = 0; rb < rows / 8; ++rb)
    for (int s = 0; s < steps; ++s)
      for (int n = 0; n < 8; ++n)
        for (int h = 0; h < 2; ++h)
          for (int c = 0; c < 2; ++c)
            out[((((int64_t)rb * steps + s) * 8 + n) * 2 + h) * 2 + c] = mat[2 * ((int64_t)(8 * rb + n) * rows + 2 * s + h) + c];
  return ARTN_OK;
}

int artn_mgate_apply(const ArtnMarginalDesc *d, void *a, int32_t k, const int32_t *dims, const void *table, int64_t table_bytes,
                     void *stream) {
  if (artn_device_count() < 1) return fail(ARTN_E_NODEVICE, "no gfx950 device visible");
  MgatePlan mp;
  if (int rc = mgate_plan(d, k, dims, nullptr, mp)) return rc;
  if (!a || !table) return fail(ARTN_E_INVALID, "null pointer");
  if (int rc = state_table_fits(table_bytes, mp.info.table_bytes, "artn_mgate_query")) return rc;
  if (int rc = state_array_aligned(a, "artn_mgate_apply")) return rc;
  if (int rc = state_table_aligned(table, "artn_mgate_apply")) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (d->dtype == ARTN_C64) mgate_launch(mp, (float2 *)a, table, st);
  else mgate_launch(mp, (double2 *)a, table, st);
  HIP_TRY(hipGetLastError());
  return ARTN_OK;
}

} // extern "C"
