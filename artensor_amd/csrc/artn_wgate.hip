// artn_wgate.hip -- the one-gate entry points artn_wgate_* of include/artn.h (kernel: artn_wgate_kernel.h).
//
// A translation unit of its own (build/obj/wgate.o).  The host half is the dense gates' shared one (artn_dense_gate_host.h:
// dense_gate_plan, _query, _pack, _apply); this unit says what is the wide gates' own.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "artn_host.h"
#include "artn_dense_gate_host.h"
#include "artn_wgate_kernel.h"

struct WgateFamily {
  using Table = ArtnWgateTable;
  static constexpr int MIN_K = 1, MAX_K = ARTN_WGATE_MAX_K;
  static constexpr const char *who = "wide gates take", *range = "wide gates act on one to five dimensions, not ";
  static constexpr const char *query = "artn_wgate_query", *pack = "artn_wgate_pack", *apply = "artn_wgate_apply";
  static int refuse(const TilePlan &) { return ARTN_OK; }
  // the matrix as it is given, and the mask of its non-zero blocks
  static void write(const double *mat, int rows, Table *table) {
    table->block_mask = state_block_mask(mat, rows);
    std::copy(mat, mat + 2 * rows * rows, (double *)(table + 1));
  }
  template <typename T, int K>
  static void launch(dim3 grid, dim3 block, size_t lds, hipStream_t st, T *a, const Table *tab) {
    hipLaunchKernelGGL((artn_k_wgate<T, K>), grid, block, lds, st, a, tab);
  }
};

extern "C" {

int artn_wgate_query(const ArtnMarginalDesc *d, int32_t k, const int32_t *dims, const double *mat, ArtnWgateInfo *info,
                     int32_t *target_bits, int32_t *tile_bits) {
  return dense_gate_query<WgateFamily>(d, k, dims, mat, info, target_bits, tile_bits);
}

int artn_wgate_pack(const ArtnMarginalDesc *d, int32_t k, const int32_t *dims, const double *mat, void *table, int64_t table_bytes) {
  return dense_gate_pack<WgateFamily>(d, k, dims, mat, table, table_bytes);
}

int artn_wgate_apply(const ArtnMarginalDesc *d, void *a, int32_t k, const int32_t *dims, const void *table, int64_t table_bytes,
                     void *stream) {
  return dense_gate_apply<WgateFamily>(d, a, k, dims, table, table_bytes, stream);
}

} // extern "C"
