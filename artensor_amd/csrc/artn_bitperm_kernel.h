// artn_bitperm_kernel.h -- ONE pass of an in-place permutation of the index bits of an amplitude array on gfx950.
//
//   artn_k_bitperm<T>   one launch: a workgroup grid-strides over TILES of 2^TB elements (include/artn.h: PLAN), loads a tile
//                       into LDS, and stores it back to the SAME addresses with its tile-local index bits permuted -- one read
//                       and one write of the state, no second buffer, no arithmetic: an element is only ever moved as the 8 or
//                       16 bytes it is.  A state below 2^TB elements is one tile in one workgroup.
//
// A tile's index bits are the bits the pass moves, every bit below a 128-byte line and the lowest other ones, so a tile is made
// of contiguous segments of at least 128 bytes and every global access is a 16-byte one of consecutive lanes.  The bits outside
// the tile are not moved by the pass, so a tile is closed under it: every element is written by the workgroup that loaded it.
//
// Per tile, phases 1 and 4 of artn_k_wgate (artn_wgate_kernel.h: the same chunk type, LDS helpers and column split) with nothing
// in between and a SECOND LDS column table on the store side:
//   1 load    tile-local index u -> LDS index L(u) = XOR of load_col[j] over the set bits j of u
//   2 barrier
//   3 store   the element that belongs at tile-local index w is the one loaded from tau^-1(w), so it is read from
//             L(tau^-1 w) = XOR of store_col[j] over the set bits of w: store_col[j] = load_col[tau^-1 j], computed on the host.
//   4 barrier (the next tile overwrites the image)
// The kernel is generic: the permutation lives in the table.  The host chooses L so that both phases spread over the LDS banks
// (DESIGN section 24).
//
// Hazards.  The tiles of a launch are disjoint and cover the state (tests/test_bit_permutation_cpu.py follows the walk of the
// packed table); no workgroup reads what another writes; no atomics.  The passes of one call are launches on one stream.
#ifndef ARTN_BITPERM_KERNEL_H
#define ARTN_BITPERM_KERNEL_H

#include "artn.h"
#include "artn_gates_kernel.h"
#include "artn_wgate_kernel.h"

template <typename T>
__global__ __launch_bounds__(ARTN_BORN_THREADS) void artn_k_bitperm(T *a, const ArtnBitpermPass *__restrict__ tab) {
  using W = WgateChunk<T>;
  using C = typename W::type;
  constexpr int NT = ARTN_BORN_THREADS, LOG_NT = 8;
  constexpr int CHUNKS = (1 << W::TB) / W::E / NT; // 16-byte chunks of a full tile per thread
  static_assert(NT == 1 << LOG_NT && CHUNKS >= 1, "tile shape");
  T *lds = (T *)artn_wgate_lds;
  const int tid = threadIdx.x;
  const int tb = (int)tab->tile_bits, n_loc = 1 << tb;
  if (tb > W::TB) return; // (uniform; a table packed for another dtype: the launch does nothing)
  const long n_tiles = (long)tab->n_tiles;
  const int seg_bits = (int)tab->segment_bits, n_holes = (int)tab->n_holes;
  const int load0 = (int)tab->load_col[0], store0 = (int)tab->store_col[0];
  // the thread's part of the memory offset and of the two LDS indices of its chunks
  const uint64_t mt = wgate_thread_cols<W, LOG_NT>(tab->mem_col, tid);
  const int lt = (int)wgate_thread_cols<W, LOG_NT>(tab->load_col, tid);
  const int st = (int)wgate_thread_cols<W, LOG_NT>(tab->store_col, tid);

  for (long q = blockIdx.x; q < n_tiles; q += gridDim.x) {
    // ---- the tile's first element: q << log2(segment) with a 0 inserted at every hole bit, ascending (uniform, 64-bit)
    uint64_t base = (uint64_t)q << seg_bits;
#pragma unroll 1
    for (int j = 0; j < n_holes; ++j) {
      const int p = (int)tab->hole_bit[j];
      base = ((base >> p) << (p + 1)) | (base & (((uint64_t)1 << p) - 1));
    }
    // ---- 1: memory -> LDS through the load columns
    C chunk[CHUNKS];
#pragma unroll
    for (int i = 0; i < CHUNKS; ++i) {
      const uint64_t mi = wgate_chunk_cols<W, LOG_NT>(tab->mem_col, i);
      if (((i * NT + tid) << W::LOG_E) < n_loc) chunk[i] = *(const C *)(a + (base | (mt ^ mi)));
    }
#pragma unroll
    for (int i = 0; i < CHUNKS; ++i) {
      const int li = (int)wgate_chunk_cols<W, LOG_NT>(tab->load_col, i);
      if (((i * NT + tid) << W::LOG_E) < n_loc) wgate_to_lds(lds, lt ^ li, load0, chunk[i]);
    }
    __syncthreads();
    // ---- 3: LDS through the store columns -> the same addresses
#pragma unroll
    for (int i = 0; i < CHUNKS; ++i) {
      const uint64_t mi = wgate_chunk_cols<W, LOG_NT>(tab->mem_col, i);
      const int si = (int)wgate_chunk_cols<W, LOG_NT>(tab->store_col, i);
      if (((i * NT + tid) << W::LOG_E) < n_loc) *(C *)(a + (base | (mt ^ mi))) = wgate_from_lds(lds, st ^ si, store0);
    }
    __syncthreads(); // the next tile overwrites the image
  }
}

#endif // ARTN_BITPERM_KERNEL_H
