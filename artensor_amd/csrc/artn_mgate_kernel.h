// artn_mgate_kernel.h -- ONE dense gate on K = 3..7 qubits, in place, on the float64 matrix cores of gfx950.
//
//   artn_k_mgate<T, K>   one launch: a workgroup grid-strides over the TILES of the wide gates' plan (include/artn.h: PLAN of
//                        artn_wgate_query, for k up to 7), holds a tile in LDS, forms Y[2^K x G] = U X[2^K x G] over its G groups
//                        with v_mfma_f64_16x16x4_f64 and writes the tile back -- one read and one write of the state.
//
// The four phases of artn_k_wgate (artn_wgate_kernel.h) with phase 2 replaced; phases 1 and 4, the LDS layout
// ((c << GB) | g) ^ sw(c) and the column tables are the wide gate's, read from an ArtnMgateTable (arrays for 7 targets).
//
//   2 compute  One instruction multiplies a ROW BLOCK rb (output rows 8 rb .. 8 rb + 7, re and im interleaved: 16 rows of the A
//              operand), a STEP s (input rows 2 s and 2 s + 1, re and im: the 4 contracted values) and a COLUMN BLOCK cb (groups
//              16 cb .. 16 cb + 15).  Lane roles: artn_gemm128_kernel.h:16.  Lane l = (j = l & 15, q = l >> 4):
//                A  row (n = j >> 1, ro = j & 1), contracted (h = q >> 1, p = q & 1): (ro, p) = (0,0) Re u, (0,1) -Im u,
//                   (1,0) Im u, (1,1) Re u of u = U[8 rb + n][2 s + h] -- entry ro ^ p of the packed pair, sign flipped for (0,1);
//                B  group 16 cb + j of input row 2 s + h, component p: for one q the 16 lanes read 16 consecutive elements of the
//                   image (XOR with a constant permutes an aligned block), complex64 converted to float64 at the read (exact);
//                D  register r of lane (j, q): output row 8 rb + (q >> 1) + 2 r, component q & 1, group 16 cb + j.
//              The 4 wavefronts share the 2^K / 8 row blocks and the G / 16 column blocks of a full tile as WR x WC slices: each
//              owns RBW x CBW = 8 (complex64) or 4 (complex128) blocks, 32 or 16 doubles of accumulators, in registers.  For
//              K >= 5 a wavefront owns a slice of the output rows and every column; for K = 3, 4 there are fewer than four row
//              blocks and the columns are shared as well.  Steps come in the order s = 0 .. 2^(K-1) - 1 (the contract's order).
//              Coefficients: for K <= 6 the wavefront's fragments (RBW * 2^(K-1) doubles per lane, 64 at K = 6) are loaded once
//              per launch and stay in registers across the tiles; at K = 7 (256 KiB) they stream from the table, which every
//              workgroup shares in L2 -- plain global loads inside the unrolled step loop.
//   3 scatter  once every wavefront has read: each accumulator rounded once to T's component type and written to its place.
//
// A state below one tile may have fewer than 16 groups (down to one): the missing B columns read group (16 cb + j) mod G, a
// valid address, and phase 3 does not write them.  No atomics, no inline assembly; every index on the state is 64-bit.
#ifndef ARTN_MGATE_KERNEL_H
#define ARTN_MGATE_KERNEL_H

#include "artn.h"
#include "artn_wgate_kernel.h"

typedef double mgate_d4 __attribute__((ext_vector_type(4)));

template <typename T, int K>
struct MgateShape {
  using W = WgateChunk<T>;
  static constexpr int ROWS = 1 << K, RB = ROWS / 8, STEPS = ROWS / 2;
  static constexpr int CB = (1 << (W::TB - K)) / 16;      // column blocks of a full tile
  static constexpr int WR = RB < 4 ? RB : 4, WC = 4 / WR; // the four wavefronts: WR slices of the row blocks x WC of the columns
  static constexpr int RBW = RB / WR, CBW = CB / WC;
  static constexpr bool HOLD = K <= 6; // the coefficient fragments stay in registers
  static_assert(K >= ARTN_MGATE_MIN_K && K <= ARTN_MGATE_MAX_K && CB >= 1 && RBW >= 1 && CBW >= 1 && WR * WC == 4, "shape");
};

__device__ __forceinline__ double mgate_lds_read(const unsigned char *lds, int byte, float) { return (double)*(const float *)(lds + byte); }
__device__ __forceinline__ double mgate_lds_read(const unsigned char *lds, int byte, double) { return *(const double *)(lds + byte); }

template <typename T, int K>
__global__ __launch_bounds__(ARTN_BORN_THREADS) void artn_k_mgate(T *a, const ArtnMgateTable *__restrict__ tab) {
  using S = decltype(T::x);
  using W = WgateChunk<T>;
  using C = typename W::type;
  using M = MgateShape<T, K>;
  constexpr int NT = ARTN_BORN_THREADS, LOG_NT = 8;
  constexpr int CHUNKS = (1 << W::TB) / W::E / NT; // 16-byte chunks of a full tile per thread
  constexpr int LOG_T = sizeof(T) == 8 ? 3 : 4;
  static_assert(NT == 1 << LOG_NT && CHUNKS >= 1 && sizeof(T) == 1 << LOG_T, "tile shape");
  T *lds = (T *)artn_wgate_lds;
  unsigned char *ldsb = artn_wgate_lds;
  const double *__restrict__ mat = (const double *)(tab + 1);
  const int tid = threadIdx.x;
  if ((int)tab->k != K) return; // (uniform; a table packed for another gate: the launch does nothing)
  const int tb = (int)tab->tile_bits, gb = tb - K, n_loc = 1 << tb;
  const long n_tiles = (long)tab->n_tiles;
  const int seg_bits = tb - (int)tab->n_high;
  const int col0 = (int)tab->lds_col[0];

  // phases 1 and 4: the thread's part of the memory offset and of the LDS index of its chunks
  uint64_t mt = 0;
  int vt = 0;
#pragma unroll
  for (int b = 0; b < LOG_NT; ++b)
    if ((tid >> b) & 1) mt ^= tab->mem_col[b + W::LOG_E], vt ^= (int)tab->lds_col[b + W::LOG_E];

  // phases 2 and 3: the lane's roles
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = lane & 15, q = lane >> 4, h = q >> 1, p = q & 1;
  const int rb0 = (wave / M::WC) * M::RBW, cb0 = (wave % M::WC) * M::CBW; // (uniform)
  int swz[K]; // (uniform)
#pragma unroll
  for (int i = 0; i < K; ++i) swz[i] = (int)tab->swizzle[i];
  const int gmask = (1 << gb) - 1;
  // B: byte address of (input row h, group 16 cb + j, component p); step s adds (XOR) the uniform part of row 2 s
  int xb[M::CBW];
#pragma unroll
  for (int cbi = 0; cbi < M::CBW; ++cbi)
    xb[cbi] = ((((h << gb) ^ (h ? swz[0] : 0) ^ ((16 * (cb0 + cbi) + j) & gmask)) << LOG_T)) | (p * (int)sizeof(S));
  // A: the lane's entry of the packed pair block of (rb, s), 32 doubles apart
  const double *__restrict__ frag = mat + (j >> 1) * 4 + h * 2 + ((j ^ q) & 1);
  const bool flip = !(j & 1) && p;
  double af[M::HOLD ? M::RBW * M::STEPS : 1];
  if constexpr (M::HOLD) {
#pragma unroll
    for (int rbi = 0; rbi < M::RBW; ++rbi)
#pragma unroll
      for (int s = 0; s < M::STEPS; ++s) {
        const double v = frag[((long)(rb0 + rbi) * M::STEPS + s) * 32];
        af[rbi * M::STEPS + s] = flip ? -v : v;
      }
  }

  for (long t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    uint64_t base = (uint64_t)t << seg_bits;
#pragma unroll
    for (int i = 0; i < ARTN_MGATE_MAX_K; ++i)
      if (i < (int)tab->n_high) { // (uniform)
        const int hb = (int)tab->high_bit[i];
        base = ((base >> hb) << (hb + 1)) | (base & (((uint64_t)1 << hb) - 1));
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
    // ---- 2: the wavefront's blocks of Y = U X
    mgate_d4 acc[M::RBW][M::CBW];
#pragma unroll
    for (int rbi = 0; rbi < M::RBW; ++rbi)
#pragma unroll
      for (int cbi = 0; cbi < M::CBW; ++cbi) acc[rbi][cbi] = mgate_d4{0.0, 0.0, 0.0, 0.0};
    if constexpr (M::HOLD) {
#pragma unroll
      for (int s = 0; s < M::STEPS; ++s) {
        int sws = 0; // (uniform: the swizzle of input row 2 s)
#pragma unroll
        for (int i = 1; i < K; ++i)
          if ((s >> (i - 1)) & 1) sws ^= swz[i];
        const int rowb = (((2 * s) << gb) ^ sws) << LOG_T;
        double x[M::CBW];
#pragma unroll
        for (int cbi = 0; cbi < M::CBW; ++cbi) x[cbi] = mgate_lds_read(ldsb, xb[cbi] ^ rowb, S());
#pragma unroll
        for (int rbi = 0; rbi < M::RBW; ++rbi)
#pragma unroll
          for (int cbi = 0; cbi < M::CBW; ++cbi)
            acc[rbi][cbi] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[rbi * M::STEPS + s], x[cbi], acc[rbi][cbi], 0, 0, 0);
      }
    } else {
      const double *__restrict__ fw = frag + (long)rb0 * M::STEPS * 32;
#pragma unroll 4
      for (int s = 0; s < M::STEPS; ++s) {
        int sws = 0; // (uniform)
#pragma unroll
        for (int i = 1; i < K; ++i)
          if ((s >> (i - 1)) & 1) sws ^= swz[i];
        const int rowb = (((2 * s) << gb) ^ sws) << LOG_T;
        double x[M::CBW], w[M::RBW];
#pragma unroll
        for (int rbi = 0; rbi < M::RBW; ++rbi) {
          const double v = fw[((long)rbi * M::STEPS + s) * 32];
          w[rbi] = flip ? -v : v;
        }
#pragma unroll
        for (int cbi = 0; cbi < M::CBW; ++cbi) x[cbi] = mgate_lds_read(ldsb, xb[cbi] ^ rowb, S());
#pragma unroll
        for (int rbi = 0; rbi < M::RBW; ++rbi)
#pragma unroll
          for (int cbi = 0; cbi < M::CBW; ++cbi)
            acc[rbi][cbi] = __builtin_amdgcn_mfma_f64_16x16x4f64(w[rbi], x[cbi], acc[rbi][cbi], 0, 0, 0);
      }
    }
    __syncthreads(); // every wavefront has read its inputs
    // ---- 3: the outputs, rounded once, to their places
#pragma unroll
    for (int rbi = 0; rbi < M::RBW; ++rbi) {
      int swb = 0; // (uniform: the swizzle of output row 8 rb)
#pragma unroll
      for (int i = 3; i < K; ++i)
        if (((rb0 + rbi) >> (i - 3)) & 1) swb ^= swz[i];
#pragma unroll
      for (int cbi = 0; cbi < M::CBW; ++cbi) {
        const int g = 16 * (cb0 + cbi) + j;
        if (g > gmask) continue; // (a state below one tile: columns beyond its groups)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = 8 * (rb0 + rbi) + 2 * r + h;
          const int idx = ((row << gb) | g) ^ swb ^ ((r & 1) ? swz[1] : 0) ^ ((r & 2) ? swz[2] : 0) ^ (h ? swz[0] : 0);
          *(S *)(ldsb + ((idx << LOG_T) | (p * (int)sizeof(S)))) = (S)acc[rbi][cbi][r];
        }
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

#endif // ARTN_MGATE_KERNEL_H
