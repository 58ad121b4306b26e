// artn_wgate_kernel.h -- ONE dense gate on K = 1..5 qubits, in place, on an amplitude array on gfx950.
//
//   artn_k_wgate<T, K>   one launch: a workgroup grid-strides over TILES of 2^TB elements (include/artn.h: PLAN), holds a tile
//                        in LDS, forms every output from the 2^K members of its group and writes the tile back -- one read and
//                        one write of the state.  A state below 2^TB elements is one tile in one workgroup.
//
// A tile's index bits are the K target memory bits and the lowest TB - K other ones, so a tile is made of contiguous segments
// of at least 2^(TB-K) elements and every global access is a 16-byte one of consecutive lanes, wherever the targets lie.
//
// Per tile, four phases with a barrier between them:
//   1 load     thread t takes the 16-byte chunks t, t + 256 ... of the tile in tile-local order.  Both the memory offset and the
//              LDS index of a tile-local index u are XORs of one column per set bit of u (mem_col, lds_col of the table), so
//              they split into a per-thread part (computed once per launch) and a uniform part per chunk.
//   2 compute  an ITEM is (row block rb, group g): R = min(2^K, 8) consecutive output rows of one group.  Lanes are consecutive
//              groups; rb is uniform over a wavefront, so every coefficient is a scalar load and every zero test a scalar branch.
//              Terms come in the contract's order d = 2^K - 1 .. 0, d = dh * R + dl: for each dh (a loop) the R inputs of column
//              block cb = rb ^ dh are read from LDS, then dl = R - 1 .. 0 and the rows are unrolled, column (j ^ dl) of the
//              block a constant register index -- no indexed register array, no scratch.  A block of the matrix that is all
//              zero (block_mask) is skipped whole: its products are all left out anyway.  Outputs are rounded once and kept.
//   3 scatter  once every thread has read: the outputs go to their places in LDS.
//   4 store    as phase 1, LDS to memory.
//
// LDS layout: element (row c, group g) at index ((c << GB) | g) ^ sw(c), GB = TB - K.  In phases 2 and 3 the lanes of a
// wavefront are consecutive g at one c: consecutive addresses (XOR with a constant permutes an aligned block), no bank conflict.
// In phases 1 and 4 the lanes are consecutive tile-local indices; the host's swizzle gives each target among the lowest six
// tile-local bits an LDS index bit of its own below bit 6, so those accesses spread over the banks as well.
//
// Arithmetic: gates_term of artn_gates_kernel.h adds every term; accumulators start at -0.0; one rounding per component to T.
//
// artn_k_cgate (artn_cgate_kernel.h) and artn_k_channel (artn_channel_kernel.h) repeat this tile loop, and all three still write
// it out: the rule of artn_block_kernel.h (a function is what compiles to the instructions of the text it replaces) admitted no
// cut.  Tried on all 30 instantiations, compared with tools/compare_device_code.py (profiles/tile_kernel_device_code.md):
//   - the whole loop as one __forceinline__ function template over the table type, with a walk policy (tile base, live item, a
//     compile-time MASKED for cgate's branch): no instantiation keeps its text; VGPRs move by -8 .. +2 (K = 3: 132 -> 134,
//     156 -> 150).  The same with the function's table parameter __restrict__: +34 .. +42 VGPRs everywhere (98 -> 132).
//     Even the unchanged kernel body moved into a function differs, so the boundary itself is the cause: the kernel argument's
//     noalias is not known inside the callee when it is simplified before inlining.
//   - phases 1 and 4 alone as functions (table, base, mt, vt passed in): 241 .. 280 VGPRs and 32 AGPRs, from 98 .. 156.
//   - wgate_thread_cols for mt and vt: two loops of branches in place of one, other text.
// The host half has no such constraint and is shared: artn_state_host.h.
#ifndef ARTN_WGATE_KERNEL_H
#define ARTN_WGATE_KERNEL_H

#include "artn.h"
#include "artn_gates_kernel.h"

#define ARTN_WGATE_MAX_GRID ARTN_GATES_MAX_GRID /* workgroups; each takes tiles g, g + G ... */

typedef float wgate_f4 __attribute__((ext_vector_type(4)));
typedef double wgate_d2 __attribute__((ext_vector_type(2)));

template <typename T>
struct WgateChunk; // one 16-byte global access: E elements
template <>
struct WgateChunk<float2> {
  using type = wgate_f4;
  static constexpr int E = 2, LOG_E = 1, TB = ARTN_WGATE_TILE_BITS_C64;
};
template <>
struct WgateChunk<double2> {
  using type = wgate_d2;
  static constexpr int E = 1, LOG_E = 0, TB = ARTN_WGATE_TILE_BITS_C128;
};

__device__ __forceinline__ void wgate_to_lds(float2 *lds, int v, int col0, wgate_f4 c) {
  lds[v] = make_float2(c.x, c.y), lds[v ^ col0] = make_float2(c.z, c.w);
}
__device__ __forceinline__ void wgate_to_lds(double2 *lds, int v, int, wgate_d2 c) { *(wgate_d2 *)&lds[v] = c; }
__device__ __forceinline__ wgate_f4 wgate_from_lds(const float2 *lds, int v, int col0) {
  const float2 lo = lds[v], hi = lds[v ^ col0];
  return wgate_f4{lo.x, lo.y, hi.x, hi.y};
}
__device__ __forceinline__ wgate_d2 wgate_from_lds(const double2 *lds, int v, int) { return *(const wgate_d2 *)&lds[v]; }

// The split of phases 1 and 4 as functions, for kernels that carry more than one column table (artn_bitperm_kernel.h): chunk
// i * NT + tid of a tile is the XOR of one column per set bit; the thread's bits give a part computed once per launch, the bits
// of i a uniform part per chunk.  `col` is indexed by tile-local bit.
template <typename W, int LOG_NT>
__device__ __forceinline__ uint64_t wgate_thread_cols(const uint64_t *__restrict__ col, int tid) {
  uint64_t x = 0;
#pragma unroll
  for (int b = 0; b < LOG_NT; ++b)
    if ((tid >> b) & 1) x ^= col[b + W::LOG_E];
  return x;
}
template <typename W, int LOG_NT>
__device__ __forceinline__ uint64_t wgate_chunk_cols(const uint64_t *__restrict__ col, int i) {
  uint64_t x = 0; // (uniform)
#pragma unroll
  for (int b = 0; (i >> b) != 0; ++b)
    if ((i >> b) & 1) x ^= col[b + LOG_NT + W::LOG_E];
  return x;
}

extern __shared__ __attribute__((aligned(16))) unsigned char artn_wgate_lds[];

template <typename T, int K>
__global__ __launch_bounds__(ARTN_BORN_THREADS) void artn_k_wgate(T *a, const ArtnWgateTable *__restrict__ tab) {
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
  const double *__restrict__ mat = (const double *)(tab + 1);
  const int tid = threadIdx.x;
  if ((int)tab->k != K) return; // (uniform; a table packed for another gate: the launch does nothing)
  const int tb = (int)tab->tile_bits, gb = tb - K, n_loc = 1 << tb;
  const long n_tiles = (long)tab->n_tiles;
  const int seg_bits = tb - (int)tab->n_high;
  const uint64_t block_mask = tab->block_mask;
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
    uint64_t base = (uint64_t)q << seg_bits;
#pragma unroll
    for (int j = 0; j < ARTN_WGATE_MAX_K; ++j)
      if (j < (int)tab->n_high) { // (uniform)
        const int p = (int)tab->high_bit[j];
        base = ((base >> p) << (p + 1)) | (base & (((uint64_t)1 << p) - 1));
      }
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
      const int gs = g < (1 << gb) ? g : 0; // (a state below one tile: lanes beyond its groups read group 0 and write nothing)
      double re[R], im[R];
#pragma unroll
      for (int j = 0; j < R; ++j) re[j] = -0.0, im[j] = -0.0;
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
      if (g >= (1 << gb)) continue;
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

#endif // ARTN_WGATE_KERNEL_H
