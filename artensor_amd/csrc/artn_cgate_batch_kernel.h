// artn_cgate_batch_kernel.h -- a dense gate on K = 1..5 target qubits under any number of control qubits, CHOSEN PER TRAJECTORY
// from a table of at most 16 cases by an int64 selector in device memory, in place, on B trajectories in one amplitude array on
// gfx950.
//
//   artn_k_cgate_batch<T, K>   artn_k_cgate (its four phases, its LDS layout, its chunk helpers, gates_term and its group mask:
//                              the arithmetic is the same function) with its difference (a), one condition for the launch,
//                              replaced by a choice per tile:
//     tile walk     the host plans the tile with the batch bits and the high controls kept out of it, so a tile lies in ONE
//                   trajectory.  The holes are the tile bits above the contiguous part and the high controls; the batch bits are
//                   walked by the tile number like any other free bit.  base |= high_want as there.
//     choice        b = batch_index(fields, base) and o = sel[b * stride] are uniform per tile (a scalar load).  o < 0, no case j
//                   with key_j == (o & mask), or a case flagged as the exact identity: `continue` before the first access to the
//                   state.  Otherwise mat and block_mask are those of case j.
//     group mask    unchanged: low controls lie below a 128-byte line, batch bits at or above it, so they never meet.
//
// Table: ArtnCgateTable (the tile fields; flags and block_mask are the OR over the cases), ArtnCgateBatchCases, then the m
// matrices as float64 (Re, Im), row-major.
//
// Hazards.  Those of artn_cgate_kernel.h: the tiles of a launch are disjoint sets of elements (the table walk visits every
// element with the wanted high control bits exactly once: tests/test_conditional_gates_cpu.py follows it), every element is
// written by the workgroup that loaded it, after the barrier that follows the last read of the tile's LDS image; a skipped tile
// is left before its first access to the state, and the skip is uniform over the workgroup, so no barrier is left half taken.
// Selector and table are only read.  Plain vector loads and stores, no atomics; launches -- the one that wrote the selector
// included -- are ordered by the stream.
#ifndef ARTN_CGATE_BATCH_KERNEL_H
#define ARTN_CGATE_BATCH_KERNEL_H

#include "artn.h"
#include "artn_batch_kernel.h"
#include "artn_gates_kernel.h"
#include "artn_wgate_kernel.h"

template <typename T, int K>
__global__ __launch_bounds__(ARTN_BORN_THREADS) void artn_k_cgate_batch(T *a, const ArtnCgateTable *__restrict__ tab,
                                                                        const long long *__restrict__ sel, long long sel_stride,
                                                                        long long sel_mask, ArtnBatchFields f) {
  using S = decltype(T::x);
  using W = WgateChunk<T>;
  using C = typename W::type;
  constexpr int NT = ARTN_BORN_THREADS, LOG_NT = 8;
  constexpr int ROWS = 1 << K, R = ROWS < ARTN_WGATE_ROWS ? ROWS : ARTN_WGATE_ROWS, NB = ROWS / R;
  constexpr int LOG_R = K < 3 ? K : 3;
  constexpr int CHUNKS = (1 << W::TB) / W::E / NT; // 16-byte chunks of a full tile per thread
  constexpr int ITEMS = (1 << W::TB) / R / NT;     // items of a full tile per thread
  static_assert(NT == 1 << LOG_NT && R == 1 << LOG_R && CHUNKS >= 1 && ITEMS >= 1, "tile shape");
  T *lds = (T *)artn_wgate_lds;
  const ArtnCgateBatchCases *__restrict__ cases = (const ArtnCgateBatchCases *)(tab + 1);
  const double *__restrict__ mats = (const double *)(cases + 1);
  const int tid = threadIdx.x;
  const int m = (int)cases->m;
  if ((int)tab->t != K || m < 1 || m > ARTN_CGATE_BATCH_MAX_CASES) return; // (uniform; a table packed for another gate: nothing)
  const int tb = (int)tab->tile_bits, gb = tb - K, n_loc = 1 << tb;
  const long n_tiles = (long)tab->n_tiles;
  const int seg_bits = (int)tab->segment_bits, n_holes = (int)tab->n_holes;
  const uint64_t high_want = tab->high_want;
  const int group_mask = (int)tab->group_mask, group_want = (int)tab->group_want;
  const int col0 = (int)tab->lds_col[0];

  // phases 1 and 4: the thread's part of the memory offset and of the LDS index of its chunks
  uint64_t mt = 0;
  int vt = 0;
#pragma unroll
  for (int b = 0; b < LOG_NT; ++b)
    if ((tid >> b) & 1) mt ^= tab->mem_col[b + W::LOG_E], vt ^= (int)tab->lds_col[b + W::LOG_E];
  // phases 2 and 3: the swizzle of the rows inside a block (uniform)
  int swj[R];
#pragma unroll
  for (int j = 0; j < R; ++j) {
    swj[j] = 0;
#pragma unroll
    for (int i = 0; i < LOG_R; ++i)
      if ((j >> i) & 1) swj[j] ^= (int)tab->swizzle[i];
  }
  const int gp = gb > 6 ? gb : 6; // lanes of an item index: a wavefront never spans two row blocks

  for (long q = blockIdx.x; q < n_tiles; q += gridDim.x) {
    // ---- the tile's first element (uniform)
    uint64_t base = (uint64_t)q << seg_bits;
#pragma unroll 1
    for (int j = 0; j < n_holes; ++j) {
      const int p = (int)tab->hole_bit[j];
      base = ((base >> p) << (p + 1)) | (base & (((uint64_t)1 << p) - 1));
    }
    base |= high_want;
    // ---- the tile's trajectory, its selector and its case (uniform)
    const long long o = sel[batch_index(f, base) * sel_stride];
    if (o < 0) continue; // (a dead trajectory: neither read nor written)
    const long long key = o & sel_mask;
    int j_case = -1;
#pragma unroll 1
    for (int j = 0; j < m; ++j)
      if (cases->key[j] == key) j_case = j; // (the keys differ: at most one)
    if (j_case < 0 || (cases->flags[j_case] & ARTN_CGATE_CASE_IDENTITY)) continue;
    const uint64_t block_mask = cases->block_mask[j_case];
    const double *__restrict__ mat = mats + (long)(2 * ROWS * ROWS) * j_case;
    // ---- 1: memory -> LDS
    C chunk[CHUNKS];
#pragma unroll
    for (int i = 0; i < CHUNKS; ++i) {
      uint64_t mi = 0; // (uniform)
#pragma unroll
      for (int b = 0; (i >> b) != 0; ++b)
        if ((i >> b) & 1) mi ^= tab->mem_col[b + LOG_NT + W::LOG_E];
      if (((i * NT + tid) << W::LOG_E) < n_loc) chunk[i] = *(const C *)(a + (base | (mt ^ mi)));
    }
#pragma unroll
    for (int i = 0; i < CHUNKS; ++i) {
      int vi = 0; // (uniform)
#pragma unroll
      for (int b = 0; (i >> b) != 0; ++b)
        if ((i >> b) & 1) vi ^= (int)tab->lds_col[b + LOG_NT + W::LOG_E];
      if (((i * NT + tid) << W::LOG_E) < n_loc) wgate_to_lds(lds, vt ^ vi, col0, chunk[i]);
    }
    __syncthreads();
    // ---- 2: the outputs of the thread's items
    S outr[ITEMS][R], outi[ITEMS][R];
#pragma unroll
    for (int w = 0; w < ITEMS; ++w) {
      const int it = w * NT + tid;
      const int rb = __builtin_amdgcn_readfirstlane(it >> gp); // (the same in every lane of a wavefront: gp >= 6)
      if (rb >= NB) continue;                                  // (uniform)
      const int g = it & ((1 << gp) - 1);
      // lanes beyond the groups of a small tile, and groups whose low control bits are not the wanted ones
      const bool live = g < (1 << gb) && (g & group_mask) == group_want;
      const int gs = live ? g : 0;
      double re[R], im[R];
#pragma unroll
      for (int j = 0; j < R; ++j) re[j] = -0.0, im[j] = -0.0;
      if (live) {
#pragma unroll 1
        for (int dh = NB - 1; dh >= 0; --dh) {
          const int cb = rb ^ dh;
          if (!((block_mask >> (rb * NB + cb)) & 1)) continue; // (uniform)
          int swb = 0;
#pragma unroll
          for (int i = LOG_R; i < K; ++i)
            if ((cb >> (i - LOG_R)) & 1) swb ^= (int)tab->swizzle[i];
          S xr[R], xi[R];
#pragma unroll
          for (int j = 0; j < R; ++j) {
            const T x = lds[(((cb * R + j) << gb) | gs) ^ swb ^ swj[j]];
            xr[j] = x.x, xi[j] = x.y;
          }
          const double *__restrict__ mb = mat + 2 * ((long)(rb * R) * ROWS + cb * R);
#pragma unroll
          for (int dl = R - 1; dl >= 0; --dl)
#pragma unroll
            for (int j = 0; j < R; ++j) {
              const int c = j ^ dl;
              gates_term(mb[2 * (j * ROWS + c)], mb[2 * (j * ROWS + c) + 1], xr[c], xi[c], re[j], im[j]);
            }
        }
      }
#pragma unroll
      for (int j = 0; j < R; ++j) outr[w][j] = (S)re[j], outi[w][j] = (S)im[j];
    }
    __syncthreads(); // every thread has read its inputs
    // ---- 3: the outputs to their places
#pragma unroll
    for (int w = 0; w < ITEMS; ++w) {
      const int it = w * NT + tid;
      const int rb = __builtin_amdgcn_readfirstlane(it >> gp);
      if (rb >= NB) continue;
      const int g = it & ((1 << gp) - 1);
      if (g >= (1 << gb) || (g & group_mask) != group_want) continue;
      int swb = 0;
#pragma unroll
      for (int i = LOG_R; i < K; ++i)
        if ((rb >> (i - LOG_R)) & 1) swb ^= (int)tab->swizzle[i];
#pragma unroll
      for (int j = 0; j < R; ++j) {
        T y;
        y.x = outr[w][j], y.y = outi[w][j];
        lds[(((rb * R + j) << gb) | g) ^ swb ^ swj[j]] = y;
      }
    }
    __syncthreads();
    // ---- 4: LDS -> memory
#pragma unroll
    for (int i = 0; i < CHUNKS; ++i) {
      uint64_t mi = 0;
      int vi = 0;
#pragma unroll
      for (int b = 0; (i >> b) != 0; ++b)
        if ((i >> b) & 1) mi ^= tab->mem_col[b + LOG_NT + W::LOG_E], vi ^= (int)tab->lds_col[b + LOG_NT + W::LOG_E];
      if (((i * NT + tid) << W::LOG_E) < n_loc) *(C *)(a + (base | (mt ^ mi))) = wgate_from_lds(lds, vt ^ vi, col0);
    }
    __syncthreads(); // the next tile overwrites the image
  }
}

#endif // ARTN_CGATE_BATCH_KERNEL_H
