// artn_dense_gate_host.h -- the one host half of the dense-gate families (artn_wgate.hip, artn_mgate.hip): the plan and the
// query, pack and apply entries over a traits struct F that the family's own unit defines beside its kernel:
//
//   F::Table                       the table's header type (include/artn.h); the matrix follows it
//   F::MIN_K, F::MAX_K             the widths the family takes
//   F::who, F::range               its wording: "wide gates take", "wide gates act on one to five dimensions, not "
//   F::query, F::pack, F::apply    the names of its three entries, as the refusals quote them
//   F::refuse(plan)                one more refusal once the tile is planned, or ARTN_OK
//   F::write(mat, rows, table)     what follows the header, and block_mask where the table has one
//   F::launch<T, K>(grid, block, lds, stream, a, table)   the family's kernel
//
// The checks, their order, the codes and the texts are one for both families (tests/test_state_layout_cpu.py,
// tests/test_wide_gates_cpu.py, tests/test_matrix_gates_cpu.py).
#pragma once
#include "artn_state_host.h"
#include "artn_wgate_kernel.h" // (the tile and grid constants of the plan; the matrix gates' kernel includes it too)

struct DenseGatePlan : TilePlan {
  int k = 0;
  ArtnWgateInfo info = {}; // (ArtnMgateInfo is the same type)
};

// The layout checks of artn_gates_query, then the target bits and the tile (include/artn.h: PLAN).  `mat` may be null
// (apply: the matrix is in the table); the flag "diagonal" is then not set.
template <typename F>
static int dense_gate_plan(const ArtnMarginalDesc *d, int32_t k, const int32_t *dims, const double *mat, DenseGatePlan &gp) {
  if (int rc = state_desc(d, F::who, ARTN_MARG_MAX_DIMS, false)) return rc;
  if (!dims) return fail(ARTN_E_INVALID, "null pointer");
  StateLayout l;
  if (int rc = state_layout(d, l)) return rc;
  if (int rc = state_bits_only(l, F::who)) return rc;
  const int64_t n = l.n;
  if (k < F::MIN_K || k > F::MAX_K) return fail(ARTN_E_UNSUPPORTED, F::range + std::to_string(k));
  const int n_bits = __builtin_ctzll((uint64_t)n);
  if (k > n_bits)
    return fail(ARTN_E_INVALID, "a gate on " + std::to_string(k) + " dimensions needs a state of at least 2^" + std::to_string(k) +
                                    " elements; this one has " + std::to_string((long long)n));
  gp.k = k;
  if (int rc = state_tile_targets(d, k, dims, "gates", gp.target)) return rc;
  bool diagonal = false;
  if (mat && !state_matrix_scan(mat, 1 << k, diagonal)) return fail(ARTN_E_INVALID, "a matrix entry is not finite");
  state_tile_plan(d->dtype, n_bits, 0, gp);
  if (int rc = F::refuse(gp)) return rc;
  gp.info.k = k, gp.info.tile_bits = gp.tb, gp.info.diagonal = diagonal ? 1 : 0;
  gp.info.n_tiles = gp.n_tiles, gp.info.segment = gp.segment, gp.info.lds_bytes = gp.lds_bytes;
  gp.info.table_bytes = (int64_t)sizeof(typename F::Table) + ((int64_t)16 << (2 * k));
  gp.info.bytes_read = gp.info.bytes_written = n * gp.elem;
  return ARTN_OK;
}

template <typename F>
static int dense_gate_query(const ArtnMarginalDesc *d, int32_t k, const int32_t *dims, const double *mat, ArtnWgateInfo *info,
                            int32_t *target_bits, int32_t *tile_bits) {
  if (!info) return fail(ARTN_E_INVALID, "null info");
  if (!mat) return fail(ARTN_E_INVALID, "null pointer");
  DenseGatePlan gp;
  if (int rc = dense_gate_plan<F>(d, k, dims, mat, gp)) return rc;
  *info = gp.info;
  if (target_bits) std::copy(gp.target.begin(), gp.target.end(), target_bits);
  if (tile_bits) std::copy(gp.tile.begin(), gp.tile.end(), tile_bits);
  return ARTN_OK;
}

template <typename F>
static int dense_gate_pack(const ArtnMarginalDesc *d, int32_t k, const int32_t *dims, const double *mat, void *table, int64_t table_bytes) {
  if (!mat) return fail(ARTN_E_INVALID, "null pointer");
  DenseGatePlan gp;
  if (int rc = dense_gate_plan<F>(d, k, dims, mat, gp)) return rc;
  if (!table) return fail(ARTN_E_INVALID, "null pointer");
  if (int rc = state_table_fits(table_bytes, gp.info.table_bytes, F::query)) return rc;
  if (int rc = state_table_aligned(table, F::pack)) return rc;
  typename F::Table t = {};
  state_tile_header(gp, k, gp.info.diagonal != 0, t);
  *(typename F::Table *)table = t;
  F::write(mat, 1 << k, (typename F::Table *)table);
  return ARTN_OK;
}

template <typename F, typename T>
static void dense_gate_launch(const DenseGatePlan &gp, T *a, const void *table, hipStream_t st) {
  const typename F::Table *tab = (const typename F::Table *)table;
  const dim3 grid((unsigned)std::min<int64_t>(gp.info.n_tiles, ARTN_WGATE_MAX_GRID)), block(ARTN_BORN_THREADS);
  const size_t lds = (size_t)gp.info.lds_bytes;
  state_with_k<F::MIN_K, F::MAX_K>(gp.k, [&](auto k) { F::template launch<T, decltype(k)::value>(grid, block, lds, st, a, tab); });
}

template <typename F>
static int dense_gate_apply(const ArtnMarginalDesc *d, void *a, int32_t k, const int32_t *dims, const void *table, int64_t table_bytes,
                            void *stream) {
  if (artn_device_count() < 1) return fail(ARTN_E_NODEVICE, "no gfx950 device visible");
  DenseGatePlan gp;
  if (int rc = dense_gate_plan<F>(d, k, dims, nullptr, gp)) return rc;
  if (!a || !table) return fail(ARTN_E_INVALID, "null pointer");
  if (int rc = state_table_fits(table_bytes, gp.info.table_bytes, F::query)) return rc;
  if (int rc = state_array_aligned(a, F::apply)) return rc;
  if (int rc = state_table_aligned(table, F::apply)) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (d->dtype == ARTN_C64) dense_gate_launch<F>(gp, (float2 *)a, table, st);
  else dense_gate_launch<F>(gp, (double2 *)a, table, st);
  HIP_TRY(hipGetLastError());
  return ARTN_OK;
}
