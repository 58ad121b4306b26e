// artn_mgate.hip -- the matrix-core gate entry points artn_mgate_* of include/artn.h (kernel: artn_mgate_kernel.h).
//
// A translation unit of its own (build/obj/mgate.o).  The host half is the dense gates' shared one (artn_dense_gate_host.h:
// dense_gate_plan, _query, _pack, _apply); this unit says what is the matrix gates' own.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "artn_host.h"
#include "artn_dense_gate_host.h"
#include "artn_mgate_kernel.h"

struct MgateFamily {
  // a full tile at the widest gate keeps 2^(TB - 7) groups: at least the 16 columns of one instruction, segments of >= 128 bytes
  static_assert(ARTN_WGATE_TILE_BITS_C64 - ARTN_MGATE_MAX_K >= 4 && ARTN_WGATE_TILE_BITS_C128 - ARTN_MGATE_MAX_K >= 4, "16 groups per tile");
  static_assert((8 << (ARTN_WGATE_TILE_BITS_C64 - ARTN_MGATE_MAX_K)) >= 128 && (16 << (ARTN_WGATE_TILE_BITS_C128 - ARTN_MGATE_MAX_K)) >= 128,
                "segments of at least 128 bytes");

  using Table = ArtnMgateTable;
  static constexpr int MIN_K = ARTN_MGATE_MIN_K, MAX_K = ARTN_MGATE_MAX_K;
  static constexpr const char *who = "matrix gates take", *range = "matrix gates act on three to seven dimensions, not ";
  static constexpr const char *query = "artn_mgate_query", *pack = "artn_mgate_pack", *apply = "artn_mgate_apply";
  // (a tile of a larger state is made of segments of at least 128 bytes; a state below one tile is one segment or more)
  static int refuse(const TilePlan &tp) {
    if (tp.n_tiles > 1 && tp.segment * tp.elem < 128) return fail(ARTN_E_LAUNCH, "internal: a tile segment below 128 bytes");
    return ARTN_OK;
  }
  // the matrix in fragment order (include/artn.h: TABLE): [rb][s][n][h][c] <- U[8 rb + n][2 s + h], c = Re, Im
  static void write(const double *mat, int rows, Table *table) {
    const int steps = rows / 2;
    double *out = (double *)(table + 1);
    for (int rb = 0; rb < rows / 8; ++rb)
      for (int s = 0; s < steps; ++s)
        for (int n = 0; n < 8; ++n)
          for (int h = 0; h < 2; ++h)
            for (int c = 0; c < 2; ++c)
              out[((((int64_t)rb * steps + s) * 8 + n) * 2 + h) * 2 + c] = mat[2 * ((int64_t)(8 * rb + n) * rows + 2 * s + h) + c];
  }
  template <typename T, int K>
  static void launch(dim3 grid, dim3 block, size_t lds, hipStream_t st, T *a, const Table *tab) {
    hipLaunchKernelGGL((artn_k_mgate<T, K>), grid, block, lds, st, a, tab);
  }
};

extern "C" {

int artn_mgate_query(const ArtnMarginalDesc *d, int32_t k, const int32_t *dims, const double *mat, ArtnMgateInfo *info,
                     int32_t *target_bits, int32_t *tile_bits) {
  return dense_gate_query<MgateFamily>(d, k, dims, mat, info, target_bits, tile_bits);
}

int artn_mgate_pack(const ArtnMarginalDesc *d, int32_t k, const int32_t *dims, const double *mat, void *table, int64_t table_bytes) {
  return dense_gate_pack<MgateFamily>(d, k, dims, mat, table, table_bytes);
}

int artn_mgate_apply(const ArtnMarginalDesc *d, void *a, int32_t k, const int32_t *dims, const void *table, int64_t table_bytes,
                     void *stream) {
  return dense_gate_apply<MgateFamily>(d, a, k, dims, table, table_bytes, stream);
}

} // extern "C"
