// artn_pauli_kernel.h -- expectation values of Pauli strings on an amplitude array on gfx950.
//
// A Pauli string is a signed permutation of the basis: with xm the memory bits under X or Y, zm those under Z or Y and ny the
// number of Y,
//
//   <psi|P|psi> = sg * sum_i (-1)^popcount(i & zm) c(q_i),   q_i = conj(a[i ^ xm]) a[i],
//
// c = Re for even ny and Im for odd ny, sg = +1, -1, -1, +1 for ny mod 4 = 0, 1, 2, 3.  One launch serves up to ARTN_PAULI_TERMS
// terms that share xm: every q_i is formed once, each term keeps a float64 accumulator of its own in every thread.
//
//   artn_k_pauli<T, FORM, NT>   per-workgroup partials of NT terms and of sum |a|^2            (states of at least 2^10 elements)
//        FORM 0   xm == 0             q_i = |a_i|^2, one load stream over all i
//        FORM 1   xm < 2^10           all i, weight 1; the partner lies in the same tile
//        FORM 2   xm >= 2^10          the i whose highest xm bit is 0, weight 2; the partner tile is base ^ xm_hi
//   artn_k_pauli_small<T>       the same for states below one tile: one workgroup, every i, guarded
//   artn_k_pauli_finish         one workgroup: partials -> results, ascending, times weight * sg
//
// A tile is 2^10 consecutive elements, thread t owns elements 4t .. 4t+3 of it (16-byte loads, as artn_k_born_overlap).  The
// partner a[i ^ xm] comes from a second global load: tile base ^ xm_hi, piece t ^ (xm_lo >> 2), and bits 0-1 of xm swap
// registers inside the thread -- an XOR inside a tile only permutes which lane reads which piece of the same bytes.  The sign of
// term t at element base + 4t + e is parity(base & zm) ^ parity(4t & zm) ^ parity(e & zm): the last one picks one of four signed
// sums of the thread's four terms (formed once for all terms), the middle one is a per-thread constant, the first one is uniform
// per workgroup and tile.  Summation order (a function of n and the masks alone): workgroup g of G takes tiles g, g + G ... in
// ascending order, the threads' accumulators feed born_wg_tree, the finish kernel adds the G partials in ascending order.  No
// floating-point atomics: bit-identical from run to run.  Terms as in artn_born_kernel.h: convert to float64 first, one rounding
// per Re q and Im q.
#ifndef ARTN_PAULI_KERNEL_H
#define ARTN_PAULI_KERNEL_H

#include "artn_born_kernel.h"

#define ARTN_PAULI_TERMS 16      /* terms of one launch */
#define ARTN_PAULI_TILE_BITS 10  /* 256 threads x 4 elements */

struct ArtnPauliArgs {
  uint64_t xm;                    // shared by the terms of the launch
  uint64_t zm[ARTN_PAULI_TERMS];  // 0 for the unused slots
  uint8_t sel[ARTN_PAULI_TERMS];  // (zm & 3) | (ny & 1) << 2: which signed sum of the thread's four q the term takes
  int32_t nt;                     // terms in use
  int32_t hbit;                   // FORM 2: the highest bit of xm
  int32_t norm;                   // non-zero: accumulate sum |a|^2 as well
  int32_t reserved;
};
struct ArtnPauliFinish {
  int64_t out_index[ARTN_PAULI_TERMS]; // where term t of the launch goes (the caller's term order)
  int64_t norm_index;                  // where sum |a|^2 goes, or -1
  int32_t nt;
  int8_t scale[ARTN_PAULI_TERMS];      // weight * sg: +-1 or +-2
};

__device__ __forceinline__ void pauli_ld4(const float2 *a, long i, float re[4], float im[4]) {
  const float4 v0 = *(const float4 *)(a + i), v1 = *(const float4 *)(a + i + 2);
  re[0] = v0.x, im[0] = v0.y, re[1] = v0.z, im[1] = v0.w, re[2] = v1.x, im[2] = v1.y, re[3] = v1.z, im[3] = v1.w;
}
__device__ __forceinline__ void pauli_ld4(const double2 *a, long i, double re[4], double im[4]) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const double2 v = a[i + e];
    re[e] = v.x, im[e] = v.y;
  }
}
template <typename S> __device__ __forceinline__ void pauli_swap(S &x, S &y) {
  const S t = x;
  x = y, y = t;
}
__device__ __forceinline__ double pauli_flip(double v, uint32_t sign_hi) { // sign_hi: 0 or 0x80000000
  return __hiloint2double((int)((uint32_t)__double2hiint(v) ^ sign_hi), __double2loint(v));
}
// the four signed sums of a thread's terms: s[k] = sum_e (-1)^popcount(e & k) q[e]
__device__ __forceinline__ void pauli_sums4(const double q[4], double s[4]) {
  const double a = q[0] + q[1], b = q[0] - q[1], c = q[2] + q[3], d = q[2] - q[3];
  s[0] = a + c, s[1] = b + d, s[2] = a - c, s[3] = b - d;
}

template <typename T, int FORM, int NT>
__global__ __launch_bounds__(ARTN_BORN_THREADS) void artn_k_pauli(const T *__restrict__ a, long tiles, ArtnPauliArgs p,
                                                                  double *__restrict__ partial) {
  using S = decltype(T::x);
  constexpr int NS = FORM == 0 ? 4 : 8; // signed sums: of Re q, and of Im q where there is a partner
  __shared__ double red[ARTN_BORN_THREADS][NT + 1];
  const int tid = threadIdx.x;
  double acc[NT + 1];
  uint32_t thr[NT]; // sign bit of parity(4 tid & zm)
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    acc[t] = 0.0;
    thr[t] = (uint32_t)(__popcll((uint64_t)(4 * tid) & p.zm[t]) & 1) << 31;
  }
  acc[NT] = 0.0;
  const uint64_t in = ((uint64_t)1 << ARTN_PAULI_TILE_BITS) - 1, xm_hi = p.xm & ~in;
  const int xm_lo = (int)(p.xm & in), r = xm_lo & 3, ptid = tid ^ (xm_lo >> 2);
  const int hb = p.hbit - ARTN_PAULI_TILE_BITS; // FORM 2: bit of the TILE index that stays 0
#pragma unroll 2
  for (long k = blockIdx.x; k < tiles; k += gridDim.x) {
    const uint64_t kt = FORM == 2 ? ((((uint64_t)k >> hb) << (hb + 1)) | ((uint64_t)k & (((uint64_t)1 << hb) - 1))) : (uint64_t)k;
    const uint64_t base = kt << ARTN_PAULI_TILE_BITS;
    S ar[4], ai[4];
    pauli_ld4(a, (long)base + 4 * tid, ar, ai);
    double s[NS];
    if constexpr (FORM == 0) {
      double q[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) q[e] = born_sq(ar[e], ai[e]);
      pauli_sums4(q, s);
      if (p.norm) acc[NT] += s[0];
    } else {
      S br[4], bi[4];
      if (FORM == 1 && (xm_lo >> 2) == 0) { // (xm below 4: the partner piece is the thread's own)
#pragma unroll
        for (int e = 0; e < 4; ++e) br[e] = ar[e], bi[e] = ai[e];
      } else {
        pauli_ld4(a, (long)(base ^ xm_hi) + 4 * ptid, br, bi);
      }
      if (r & 1) pauli_swap(br[0], br[1]), pauli_swap(bi[0], bi[1]), pauli_swap(br[2], br[3]), pauli_swap(bi[2], bi[3]);
      if (r & 2) pauli_swap(br[0], br[2]), pauli_swap(bi[0], bi[2]), pauli_swap(br[1], br[3]), pauli_swap(bi[1], bi[3]);
      double qr[4], qi[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const double xr = (double)ar[e], xi = (double)ai[e], yr = (double)br[e], yi = (double)bi[e];
        qr[e] = fma(yr, xr, yi * xi);    // Re conj(b) a
        qi[e] = fma(yr, xi, -(yi * xr)); // Im conj(b) a
      }
      pauli_sums4(qr, s);
      pauli_sums4(qi, s + 4);
      if (p.norm) {
        double m = 0.0;
#pragma unroll
        for (int e = 0; e < 4; ++e) m += born_sq(ar[e], ai[e]);
        if constexpr (FORM == 2) {
#pragma unroll
          for (int e = 0; e < 4; ++e) m += born_sq(br[e], bi[e]);
        }
        acc[NT] += m;
      }
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int w = p.sel[t] & (NS - 1);
      double v = s[0];
#pragma unroll
      for (int j = 1; j < NS; ++j) v = (w == j) ? s[j] : v; // (w is uniform: selects, never private memory)
      acc[t] += pauli_flip(v, thr[t] ^ ((uint32_t)(__popcll(base & p.zm[t]) & 1) << 31));
    }
  }
  born_wg_tree<NT + 1>(red, acc);
  if (tid <= NT) partial[(long)blockIdx.x * (NT + 1) + tid] = red[0][tid];
}

// States below one tile: one workgroup, thread t takes i = t, t + 256 ... < n, every i with weight 1.
template <typename T>
__global__ __launch_bounds__(ARTN_BORN_THREADS) void artn_k_pauli_small(const T *__restrict__ a, long n, ArtnPauliArgs p,
                                                                        double *__restrict__ partial) {
  constexpr int NT = ARTN_PAULI_TERMS;
  __shared__ double red[ARTN_BORN_THREADS][NT + 1];
  double acc[NT + 1];
#pragma unroll
  for (int t = 0; t <= NT; ++t) acc[t] = 0.0;
  for (long i = threadIdx.x; i < n; i += ARTN_BORN_THREADS) {
    const long j = i ^ (long)p.xm;
    if (j >= n) continue; // (never: xm < n)
    const T x = a[i], y = a[j];
    const double xr = (double)x.x, xi = (double)x.y, yr = (double)y.x, yi = (double)y.y;
    const double qr = fma(yr, xr, yi * xi), qi = fma(yr, xi, -(yi * xr));
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const double v = (p.sel[t] & 4) ? qi : qr;
      acc[t] += pauli_flip(v, (uint32_t)(__popcll((uint64_t)i & p.zm[t]) & 1) << 31);
    }
    acc[NT] += born_sq(x.x, x.y);
  }
  born_wg_tree<NT + 1>(red, acc);
  if (threadIdx.x <= NT) partial[threadIdx.x] = red[0][threadIdx.x];
}

// partial: n_partial rows of nv doubles (nv - 1 term slots, then sum |a|^2)  (static, as the non-template kernels of
// artn_born_kernel.h: this header is included by more than one translation unit)
static __global__ __launch_bounds__(64) void artn_k_pauli_finish(const double *__restrict__ partial, int n_partial, int nv, ArtnPauliFinish f,
                                                          double *__restrict__ out) {
  const int q = threadIdx.x;
  const bool term = q < f.nt, norm = q == nv - 1 && f.norm_index >= 0;
  if (!term && !norm) return;
  double v = 0.0;
#pragma unroll 8
  for (int g = 0; g < n_partial; ++g) v += partial[(long)g * nv + q];
  if (term) out[f.out_index[q]] = (double)f.scale[q] * v;
  else out[f.norm_index] = v;
}

#endif // ARTN_PAULI_KERNEL_H
