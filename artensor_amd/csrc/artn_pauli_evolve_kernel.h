// artn_pauli_evolve_kernel.h -- circuits of Pauli steps a <- alpha a + beta P a, in place, on an amplitude array on gfx950.
//
// With the masks of artn_pauli_kernel.h, (P a)[i] = (-i)^ny (-1)^popcount(i & zm) a[i ^ xm]: a step only mixes the two members of
// each pair (i, i ^ xm).  The host (artn_pauli.hip) cuts the circuit into RUNS whose high flips xm_hi (xm with the ten tile bits
// cleared) span a GF(2) space of rank R; the orbits of that space split the tiles into BLOCKS of 2^R tiles, and
//
//   artn_k_pauli_evolve<T, R>     one launch per run: a workgroup grid-strides over blocks, holds the 2^R tiles of a block, applies
//                                 every step of the run to it and writes it back -- one read and one write of the state per run
//   artn_k_pauli_evolve_small<T>  states below 2^10 elements: one workgroup, the whole circuit in one launch
//
// A block, its slots and pieces, the stage and its plane layout: artn_block_kernel.h, with the run's reduced-echelon basis as the
// vectors.  The partner of element (slot s, piece t, e) under a step is (s ^ m, t ^ (xm_lo >> 2), e ^ (xm_lo & 3)), m the step's
// slot mask.
//
// Who updates what.  Every thread computes its OWN elements from its own registers and the partner's value and writes nothing else:
//   register steps   m = 0 and xm_lo < 4 (diagonal steps, flips in bits 0-1 only): the partner is one of the thread's own four
//                    elements of the same slot -- no LDS, no barrier;
//   staged steps     everything else: the partner piece of each slot (slot s ^ m) comes from the stage.
// Stream order separates runs.  No atomics.
//
// Sign of (P a)[i] at element (slot s, thread t, e): parity(tile_s << 10 & zm) (uniform per slot) ^ parity(4t & zm) (per thread)
// ^ parity(e & zm) (per element), XORed into the sign bits of the partner's components; (-i)^ny is a swap and sign changes of beta.
//
// Arithmetic.  pauli_evolve_pair is the ONE function that computes a step on an element, for every kernel form and every R:
// operands to float64, four products accumulated by fma in a fixed order, products with an exactly zero coefficient component left
// out (the accumulator starts at -0.0, the identity of + that keeps the sign of a zero), one rounding per component to T.  Between
// steps the block is held as T.  So the result does not depend on where the runs are cut, bit for bit.
#ifndef ARTN_PAULI_EVOLVE_KERNEL_H
#define ARTN_PAULI_EVOLVE_KERNEL_H

#include "artn.h"
#include "artn_pauli_apply_kernel.h"
#include "artn_block_kernel.h"

#define ARTN_PAULI_EVOLVE_MAX_GRID ARTN_BORN_MAX_GRID /* workgroups; each takes blocks g, g + G ... */

struct PauliEvolveCoef {
  double ar, ai, br, bi; // alpha, and beta (-i)^ny
};

// the step's coefficients from its table record (uniform: scalar loads and selects)
__device__ __forceinline__ PauliEvolveCoef pauli_evolve_coef(const ArtnPauliEvolveStep &st) {
  PauliEvolveCoef c;
  c.ar = st.alpha_re, c.ai = st.alpha_im;
  const double re = st.beta_re, im = st.beta_im;
  switch ((int)(st.n_y & 3)) { // beta (-i)^ny
  case 0: c.br = re, c.bi = im; break;
  case 1: c.br = im, c.bi = -re; break;
  case 2: c.br = -re, c.bi = -im; break;
  default: c.br = -im, c.bi = re; break;
  }
  return c;
}

__device__ __forceinline__ float pauli_evolve_flip(float v, uint32_t sign_hi) { // sign_hi: 0 or 0x80000000
  return __uint_as_float(__float_as_uint(v) ^ sign_hi);
}
__device__ __forceinline__ double pauli_evolve_flip(double v, uint32_t sign_hi) { return pauli_flip(v, sign_hi); }

// new (xr, xi) = alpha (xr, xi) + beta (yr, yi); (yr, yi) is the partner with its sign already applied
template <typename S>
__device__ __forceinline__ void pauli_evolve_pair(const PauliEvolveCoef &c, S &xr, S &xi, S yr, S yi) {
  const double ar = (double)xr, ai = (double)xi, br = (double)yr, bi = (double)yi;
  double re = -0.0, im = -0.0;
  if (c.bi != 0.0) re = fma(-c.bi, bi, re), im = fma(c.bi, br, im);
  if (c.br != 0.0) re = fma(c.br, br, re), im = fma(c.br, bi, im);
  if (c.ai != 0.0) re = fma(-c.ai, ai, re), im = fma(c.ai, ar, im);
  if (c.ar != 0.0) re = fma(c.ar, ar, re), im = fma(c.ar, ai, im);
  xr = (S)re, xi = (S)im;
}

__device__ __forceinline__ PauliPiece64 pauli_pack4(const float re[4], const float im[4]) {
  return PauliPiece64{make_float4(re[0], im[0], re[1], im[1]), make_float4(re[2], im[2], re[3], im[3])};
}
__device__ __forceinline__ PauliPiece128 pauli_pack4(const double re[4], const double im[4]) {
  return PauliPiece128{make_double2(re[0], im[0]), make_double2(re[1], im[1]), make_double2(re[2], im[2]), make_double2(re[3], im[3])};
}

// the four elements of one slot: own (xr, xi) updated from the partner piece (yr, yi) in PIECE order (bits 0-1 of xm still to apply)
template <typename S>
__device__ __forceinline__ void pauli_evolve_piece(const PauliEvolveCoef &c, int r, uint32_t sg, const uint32_t pe[4], S xr[4],
                                                   S xi[4], S yr[4], S yi[4]) {
  block_swap4(r, yr, yi);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const uint32_t s = sg ^ pe[e];
    pauli_evolve_pair(c, xr[e], xi[e], pauli_evolve_flip(yr[e], s), pauli_evolve_flip(yi[e], s));
  }
}

extern __shared__ __attribute__((aligned(16))) unsigned char artn_pauli_evolve_lds[];

template <typename T, int R>
__global__ __launch_bounds__(ARTN_BORN_THREADS) void artn_k_pauli_evolve(T *a, long n_blocks, const ArtnPauliEvolveRun *__restrict__ run,
                                                                         const ArtnPauliEvolveStep *__restrict__ steps) {
  using S = decltype(T::x);
  using C = typename PauliChunk<T>::type;
  constexpr int Q = (int)sizeof(T) / 4; // 16-byte chunks of a piece
  constexpr int NS = 1 << R;            // slots of a block
  C *stage = (C *)artn_pauli_evolve_lds; // [NS][Q][256]
  const int tid = threadIdx.x;
  if ((int)run->rank != R) return; // (uniform; a table packed for another max_rank: the launch does nothing)
  const ArtnPauliEvolveStep *stp = steps + run->first;
  const int n_steps = (int)run->count;
  uint64_t span[NS]; // XOR of the basis over the bits of s, as TILE-index masks
  span[0] = 0;
#pragma unroll
  for (int j = 0; j < R; ++j) {
    const uint64_t b = run->basis[j] >> ARTN_PAULI_TILE_BITS;
#pragma unroll
    for (int s = 0; s < (1 << j); ++s) span[s | (1 << j)] = span[s] ^ b;
  }
  for (long q = blockIdx.x; q < n_blocks; q += gridDim.x) {
    const uint64_t rep = block_rep<R>(run, q);
    S xr[NS][4], xi[NS][4];
#pragma unroll
    for (int s = 0; s < NS; ++s)
      pauli_unpack4(pauli_piece_ld((const C *)(a + (long)((rep ^ span[s]) << ARTN_PAULI_TILE_BITS) + 4 * tid), 1), xr[s], xi[s]);
    for (int k = 0; k < n_steps; ++k) {
      const PauliEvolveCoef c = pauli_evolve_coef(stp[k]);
      const uint64_t zm = stp[k].zmask;
      const int xm_lo = (int)stp[k].xm_lo, m = (int)stp[k].slot_mask, r = xm_lo & 3, pmask = xm_lo >> 2;
      const uint32_t pt = (uint32_t)(__popcll((uint64_t)(4 * tid) & zm) & 1) << 31;
      const uint32_t z0 = (uint32_t)(zm & 1) << 31, z1 = (uint32_t)((zm >> 1) & 1) << 31;
      const uint32_t pe[4] = {0u, z0, z1, z0 ^ z1};
      const bool staged = m != 0 || pmask != 0; // (uniform)
      if (staged) {
        __syncthreads(); // every thread has read the previous image
#pragma unroll
        for (int s = 0; s < NS; ++s) pauli_piece_st(&stage[s * Q * ARTN_BORN_THREADS + tid], ARTN_BORN_THREADS, pauli_pack4(xr[s], xi[s]));
        __syncthreads();
      }
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        const uint32_t sg = pt ^ ((uint32_t)(__popcll(((rep ^ span[s]) << ARTN_PAULI_TILE_BITS) & zm) & 1) << 31);
        S yr[4], yi[4];
        if (staged) {
          pauli_unpack4(pauli_piece_ld(&stage[(s ^ m) * Q * ARTN_BORN_THREADS + (tid ^ pmask)], ARTN_BORN_THREADS), yr, yi);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) yr[e] = xr[s][e], yi[e] = xi[s][e];
        }
        pauli_evolve_piece(c, r, sg, pe, xr[s], xi[s], yr, yi);
      }
    }
#pragma unroll
    for (int s = 0; s < NS; ++s)
      pauli_piece_st((C *)(a + (long)((rep ^ span[s]) << ARTN_PAULI_TILE_BITS) + 4 * tid), 1, pauli_pack4(xr[s], xi[s]));
  }
}

// States below one tile: the state lives in LDS as T; thread t owns elements t, t + 256 ... < n (at most two).
template <typename T>
__global__ __launch_bounds__(ARTN_BORN_THREADS) void artn_k_pauli_evolve_small(T *a, long n, const ArtnPauliEvolveStep *__restrict__ stp,
                                                                               int n_steps) {
  using S = decltype(T::x);
  constexpr int PER = (1 << ARTN_PAULI_TILE_BITS) / 2 / ARTN_BORN_THREADS; // n <= 2^9
  __shared__ T img[(1 << ARTN_PAULI_TILE_BITS) / 2];
  const int tid = threadIdx.x;
  S xr[PER], xi[PER];
#pragma unroll
  for (int u = 0; u < PER; ++u) {
    const long i = tid + u * ARTN_BORN_THREADS;
    xr[u] = xi[u] = (S)0;
    if (i < n) xr[u] = a[i].x, xi[u] = a[i].y;
  }
  for (int k = 0; k < n_steps; ++k) {
    const PauliEvolveCoef c = pauli_evolve_coef(stp[k]);
    const uint64_t zm = stp[k].zmask;
    const long xm = (long)stp[k].xm_lo; // (the whole mask: n <= 2^9)
    __syncthreads();
    block_small_st(img, n, tid, xr, xi);
    __syncthreads();
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const long i = tid + u * ARTN_BORN_THREADS, j = i ^ xm;
      if (i >= n || j >= n) continue; // (j >= n never: xm < n)
      const uint32_t sg = (uint32_t)(__popcll((uint64_t)i & zm) & 1) << 31;
      const T b = img[j];
      pauli_evolve_pair(c, xr[u], xi[u], pauli_evolve_flip(b.x, sg), pauli_evolve_flip(b.y, sg));
    }
  }
  block_small_st(a, n, tid, xr, xi);
}

#endif // ARTN_PAULI_EVOLVE_KERNEL_H
