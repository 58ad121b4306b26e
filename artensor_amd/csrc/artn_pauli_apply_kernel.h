// artn_pauli_apply_kernel.h -- y = H a for H a sum of Pauli strings, on an amplitude array on gfx950, in one launch.
//
// With the masks of artn_pauli_kernel.h, (P a)[i] = (-i)^ny (-1)^popcount(i & zm) a[i ^ xm].  The terms of a call are grouped by xm:
//
//   y[i] = sum_g W_g(i) a[i ^ xm_g],     W_g(i) = sum_{k in g} f_k (-1)^popcount(i & zm_k),     f_k = c_k (-i)^ny_k (folded on the host)
//
//   artn_k_pauli_apply<T>         a workgroup owns output tiles; every y[i] is written once and never read   (n >= 2^10)
//   artn_k_pauli_apply_small<T>   one workgroup, one element per thread-iteration, the full popcount per term  (n < 2^10)
//
// The tile of artn_k_pauli: 2^10 consecutive elements, thread t owns elements 4t .. 4t+3 and keeps their eight float64
// accumulators.  The groups come in table order (the host sorts them by xm_hi = xm with the tile bits cleared).  Whenever xm_hi
// changes, the workgroup copies the partner tile base ^ xm_hi into LDS with 16-byte loads (the thread's own piece, so the copy is
// a plain contiguous read); every group that shares xm_hi is then served from that copy: piece t ^ (xm_lo >> 2), and bits 0-1 of
// xm swap registers.  The copy is kept as Q = sizeof(T) / 4 planes of 256 x 16 bytes, plane q holding chunk q of every piece: a
// ds_read_b128 of plane q at piece t ^ m touches 16 distinct 16-byte slots in each of its lane groups for every m -- no bank
// conflict (an XOR permutes the slots of an aligned group of 16).  Identity group: xm_hi = 0 and the piece is the thread's own.
//
// W_g: the group's terms are read from the table (uniform addresses: scalar loads).  The sign of term k at element base + 4t + e is
// parity(base & zm) ^ parity(4t & zm) ^ parity(e & zm).  The first two go into the sign bits of f_k, which is then added to one of
// four CLASS sums picked by zm & 3 (uniform: a scalar branch, no indexed registers -- the number of terms is unbounded and
// nothing is kept per term); after the term loop pauli_sums4 turns the four class sums into the four per-element weights.
// Then y += W * partner with four fma per element.  Everything is float64 for both dtypes; one rounding to T at the store.
// Summation order of an element = table order of the groups, and inside a group the table order of its terms.  No atomics.
#ifndef ARTN_PAULI_APPLY_KERNEL_H
#define ARTN_PAULI_APPLY_KERNEL_H

#include "artn.h"
#include "artn_pauli_kernel.h"

#define ARTN_PAULI_APPLY_MAX_GRID ARTN_BORN_MAX_GRID /* workgroups; each takes tiles g, g + G ... */

// a thread's piece as PauliPiece<T>: named 16-byte chunks, no array (hipcc moves a private array that lives across a barrier to LDS)
struct PauliPiece64 {
  float4 c0, c1;
};
struct PauliPiece128 {
  double2 c0, c1, c2, c3;
};
__device__ __forceinline__ void pauli_unpack4(const PauliPiece64 &p, float re[4], float im[4]) {
  re[0] = p.c0.x, im[0] = p.c0.y, re[1] = p.c0.z, im[1] = p.c0.w, re[2] = p.c1.x, im[2] = p.c1.y, re[3] = p.c1.z, im[3] = p.c1.w;
}
__device__ __forceinline__ void pauli_unpack4(const PauliPiece128 &p, double re[4], double im[4]) {
  re[0] = p.c0.x, im[0] = p.c0.y, re[1] = p.c1.x, im[1] = p.c1.y, re[2] = p.c2.x, im[2] = p.c2.y, re[3] = p.c3.x, im[3] = p.c3.y;
}
__device__ __forceinline__ PauliPiece64 pauli_piece_ld(const float4 *src, int stride) {
  return PauliPiece64{src[0], src[stride]};
}
__device__ __forceinline__ PauliPiece128 pauli_piece_ld(const double2 *src, int stride) {
  return PauliPiece128{src[0], src[stride], src[2 * stride], src[3 * stride]};
}
__device__ __forceinline__ void pauli_piece_st(float4 *dst, int stride, const PauliPiece64 &p) { dst[0] = p.c0, dst[stride] = p.c1; }
__device__ __forceinline__ void pauli_piece_st(double2 *dst, int stride, const PauliPiece128 &p) {
  dst[0] = p.c0, dst[stride] = p.c1, dst[2 * stride] = p.c2, dst[3 * stride] = p.c3;
}
// the 16-byte chunk of a piece: two complex64 or one complex128
template <typename T> struct PauliChunk;
template <> struct PauliChunk<float2> { using type = float4; };
template <> struct PauliChunk<double2> { using type = double2; };
__device__ __forceinline__ void pauli_st4(float2 *y, long i, const double re[4], const double im[4]) {
  *(float4 *)(y + i) = make_float4((float)re[0], (float)im[0], (float)re[1], (float)im[1]);
  *(float4 *)(y + i + 2) = make_float4((float)re[2], (float)im[2], (float)re[3], (float)im[3]);
}
__device__ __forceinline__ void pauli_st4(double2 *y, long i, const double re[4], const double im[4]) {
#pragma unroll
  for (int e = 0; e < 4; ++e) y[i + e] = make_double2(re[e], im[e]);
}

template <typename T>
__global__ __launch_bounds__(ARTN_BORN_THREADS) void artn_k_pauli_apply(const T *__restrict__ a, T *__restrict__ y, long tiles,
                                                                        const ArtnPauliApplyGroup *__restrict__ grp,
                                                                        const ArtnPauliApplyTerm *__restrict__ trm, int n_groups) {
  using S = decltype(T::x);
  using C = typename PauliChunk<T>::type;
  constexpr int Q = (int)sizeof(T) / 4; // 16-byte chunks of a thread's piece: 2 (complex64), 4 (complex128)
  constexpr uint64_t in = ((uint64_t)1 << ARTN_PAULI_TILE_BITS) - 1;
  __shared__ C stage[Q][ARTN_BORN_THREADS];
  const int tid = threadIdx.x;
  for (long k = blockIdx.x; k < tiles; k += gridDim.x) {
    const uint64_t base = (uint64_t)k << ARTN_PAULI_TILE_BITS;
    double yr[4] = {0.0, 0.0, 0.0, 0.0}, yi[4] = {0.0, 0.0, 0.0, 0.0};
    uint64_t staged = ~(uint64_t)0; // xm_hi of the copy in LDS (none yet for this tile)
    for (int g = 0; g < n_groups; ++g) {
      const uint64_t xm = grp[g].xmask, xm_hi = xm & ~in;
      if (xm_hi != staged) { // (uniform)
        const auto own = pauli_piece_ld((const C *)(a + (long)(base ^ xm_hi) + 4 * tid), 1);
        __syncthreads(); // every thread has read the previous copy
        pauli_piece_st(&stage[0][tid], ARTN_BORN_THREADS, own);
        __syncthreads();
        staged = xm_hi;
      }
      const int xm_lo = (int)(xm & in), r = xm_lo & 3, ptid = tid ^ (xm_lo >> 2);
      S br[4], bi[4];
      pauli_unpack4(pauli_piece_ld(&stage[0][ptid], ARTN_BORN_THREADS), br, bi);
      if (r & 1) pauli_swap(br[0], br[1]), pauli_swap(bi[0], bi[1]), pauli_swap(br[2], br[3]), pauli_swap(bi[2], bi[3]);
      if (r & 2) pauli_swap(br[0], br[2]), pauli_swap(bi[0], bi[2]), pauli_swap(br[1], br[3]), pauli_swap(bi[1], bi[3]);
      double cr[4] = {0.0, 0.0, 0.0, 0.0}, ci[4] = {0.0, 0.0, 0.0, 0.0}; // class sums
      const uint64_t first = grp[g].first, end = first + grp[g].count;
      for (uint64_t t = first; t < end; ++t) {
        const uint64_t zm = trm[t].zmask, cls = trm[t].sign_class;
        const uint32_t sg = (uint32_t)((__popcll(base & zm) ^ __popcll((uint64_t)(4 * tid) & zm)) & 1) << 31;
        const double fr = pauli_flip(trm[t].re, sg), fi = pauli_flip(trm[t].im, sg);
        if (cls == 0) cr[0] += fr, ci[0] += fi; // (cls is uniform: scalar branches)
        else if (cls == 1) cr[1] += fr, ci[1] += fi;
        else if (cls == 2) cr[2] += fr, ci[2] += fi;
        else cr[3] += fr, ci[3] += fi;
      }
      double wr[4], wi[4];
      pauli_sums4(cr, wr);
      pauli_sums4(ci, wi);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const double pr = (double)br[e], pi = (double)bi[e];
        yr[e] = fma(-wi[e], pi, fma(wr[e], pr, yr[e]));
        yi[e] = fma(wi[e], pr, fma(wr[e], pi, yi[e]));
      }
    }
    pauli_st4(y, (long)base + 4 * tid, yr, yi);
  }
}

// States below one tile: one workgroup, thread t takes i = t, t + 256 ... < n.
template <typename T>
__global__ __launch_bounds__(ARTN_BORN_THREADS) void artn_k_pauli_apply_small(const T *__restrict__ a, T *__restrict__ y, long n,
                                                                              const ArtnPauliApplyGroup *__restrict__ grp,
                                                                              const ArtnPauliApplyTerm *__restrict__ trm, int n_groups) {
  using S = decltype(T::x);
  for (long i = threadIdx.x; i < n; i += ARTN_BORN_THREADS) {
    double yr = 0.0, yi = 0.0;
    for (int g = 0; g < n_groups; ++g) {
      const long j = i ^ (long)grp[g].xmask;
      if (j >= n) continue; // (never: xm < n)
      const T b = a[j];
      double wr = 0.0, wi = 0.0;
      const uint64_t first = grp[g].first, end = first + grp[g].count;
      for (uint64_t t = first; t < end; ++t) {
        const uint32_t sg = (uint32_t)(__popcll((uint64_t)i & trm[t].zmask) & 1) << 31;
        wr += pauli_flip(trm[t].re, sg), wi += pauli_flip(trm[t].im, sg);
      }
      const double pr = (double)b.x, pi = (double)b.y;
      yr = fma(-wi, pi, fma(wr, pr, yr));
      yi = fma(wi, pr, fma(wr, pi, yi));
    }
    T v;
    v.x = (S)yr, v.y = (S)yi;
    y[i] = v;
  }
}

#endif // ARTN_PAULI_APPLY_KERNEL_H
