// artn_krylov_kernel.h -- the vector algebra of Krylov drivers on gfx950: many inner products against one vector in one pass, and a
// linear combination of up to 64 vectors with its norm in one pass.  Both are elementwise over the flat memory range of n elements
// (every vector of a call has the same dense layout, so the layout itself never matters), float64 arithmetic in an order fixed by
// n alone, no atomics, every partial sum with one owner.
//
//   artn_k_krylov_dots<T, NB>     per-workgroup partials of <V_j|w>, j < NB <= ARTN_KRYLOV_BATCH, and of |w|^2
//   artn_k_krylov_dots_finish     one workgroup per group of four partials -> out[2j], out[2j + 1] = <V_j|w>, out[2m] = |w|^2
//   artn_k_krylov_combine<T>      y <- sum_j c_j X_j, per-workgroup partials of |y|^2 of the stored values (artn_k_born_finish ends it)
//
// The dots are artn_k_born_overlap<T, true> with a = V_j, b = w for NB vectors at once: the same terms, the same tile ownership
// (workgroup g of G takes the 1024-element tiles g, g + G, ..; thread t elements 4t .. 4t + 3; the ragged tail goes to thread 0 of
// workgroup 0 after its tiles), born_wg_tree over the accumulators four at a time (one 8 KiB LDS array), born_finish_sum per group:
// each result is bit for bit what artn_born_overlap gives for that pair.  |y|^2 of the combination follows artn_k_born_overlap<T, false>
// in the same way, on the values as stored.
//
// Pointers and coefficients travel BY VALUE in the kernel arguments (wave-uniform: the loops over j read them as scalars).
#ifndef ARTN_KRYLOV_KERNEL_H
#define ARTN_KRYLOV_KERNEL_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "artn.h"
#include "artn_born_kernel.h"

struct ArtnKrylovDotsArgs {
  const void *v[ARTN_KRYLOV_BATCH];
};
struct ArtnKrylovCombineArgs {
  const void *x[ARTN_KRYLOV_MAX_VECS];
  double c[ARTN_KRYLOV_MAX_VECS][2];
};

// E consecutive elements from element i (E = 4: i a multiple of 4, 16-byte loads; E = 1: the ragged tail) as float64
template <int E> __device__ __forceinline__ void krylov_load(const float2 *p, long i, double r[E], double m[E]) {
  if constexpr (E == 4) {
    const float4 v0 = *(const float4 *)(p + i), v1 = *(const float4 *)(p + i + 2);
    r[0] = (double)v0.x, m[0] = (double)v0.y, r[1] = (double)v0.z, m[1] = (double)v0.w;
    r[2] = (double)v1.x, m[2] = (double)v1.y, r[3] = (double)v1.z, m[3] = (double)v1.w;
  } else {
    const float2 v = p[i];
    r[0] = (double)v.x, m[0] = (double)v.y;
  }
}
template <int E> __device__ __forceinline__ void krylov_load(const double2 *p, long i, double r[E], double m[E]) {
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const double2 v = p[i + e];
    r[e] = v.x, m[e] = v.y;
  }
}

// ---- dots ----------------------------------------------------------------------------------------------------------
template <typename T, int NB, int E>
__device__ __forceinline__ void krylov_dots_step(const ArtnKrylovDotsArgs &args, const T *__restrict__ w, long i, double re[NB],
                                                 double im[NB], double &nw) {
  double yr[E], yi[E];
  krylov_load<E>(w, i, yr, yi);
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    double xr[E], xi[E];
    krylov_load<E>((const T *)args.v[j], i, xr, xi);
#pragma unroll
    for (int e = 0; e < E; ++e) {
      re[j] += fma(xr[e], yr[e], xi[e] * yi[e]);    // Re conj(x) y
      im[j] += fma(xr[e], yi[e], -(xi[e] * yr[e])); // Im conj(x) y
    }
  }
#pragma unroll
  for (int e = 0; e < E; ++e) nw += fma(yr[e], yr[e], yi[e] * yi[e]);
}

// partial: this launch's first group of four; group q of the launch (vectors 2q and 2q + 1) lies at partial + q * G * 4, [g][4].
// partial_w: the group of |w|^2 (written when write_nw is set: the first launch of a call), {|w|^2, 0, 0, 0} per workgroup.
template <typename T, int NB>
__global__ __launch_bounds__(ARTN_BORN_THREADS) void artn_k_krylov_dots(ArtnKrylovDotsArgs args, const T *__restrict__ w, long n,
                                                                        int write_nw, double *__restrict__ partial,
                                                                        double *__restrict__ partial_w) {
  __shared__ double red[ARTN_BORN_THREADS][4];
  double re[NB], im[NB], nw = 0.0;
#pragma unroll
  for (int j = 0; j < NB; ++j) re[j] = 0.0, im[j] = 0.0;
  const long n4 = n >> 2; // whole segments
  const long step = (long)gridDim.x * ARTN_BORN_THREADS;
  for (long s = (long)blockIdx.x * ARTN_BORN_THREADS + threadIdx.x; s < n4; s += step)
    krylov_dots_step<T, NB, 4>(args, w, s * 4, re, im, nw);
  if (blockIdx.x == 0 && threadIdx.x == 0)
    for (long i = n4 * 4; i < n; ++i) krylov_dots_step<T, NB, 1>(args, w, i, re, im, nw);
  const long G = gridDim.x;
#pragma unroll
  for (int q = 0; q < (NB + 1) / 2; ++q) {
    const double v[4] = {re[2 * q], im[2 * q], 2 * q + 1 < NB ? re[2 * q + 1 < NB ? 2 * q + 1 : 0] : 0.0,
                         2 * q + 1 < NB ? im[2 * q + 1 < NB ? 2 * q + 1 : 0] : 0.0};
    born_wg_tree<4>(red, v);
    if (threadIdx.x < 4) partial[((long)q * G + blockIdx.x) * 4 + threadIdx.x] = red[0][threadIdx.x];
    __syncthreads(); // (red[0] has been read before the next slice overwrites it)
  }
  if (write_nw) {
    const double v[4] = {nw, 0.0, 0.0, 0.0};
    born_wg_tree<4>(red, v);
    if (threadIdx.x < 4) partial_w[(long)blockIdx.x * 4 + threadIdx.x] = red[0][threadIdx.x];
  }
}

// workgroup k < ceil(m / 2): vectors 2k and 2k + 1; workgroup ceil(m / 2): |w|^2.  out holds 2m + 1 doubles.
static __global__ __launch_bounds__(ARTN_BORN_THREADS) void artn_k_krylov_dots_finish(const double *__restrict__ partial, int n_partial,
                                                                               int m, double *__restrict__ out) {
  __shared__ double red[ARTN_BORN_THREADS][4];
  const int k = blockIdx.x;
  born_finish_sum(partial + (long)k * n_partial * 4, n_partial, 4, red);
  if (threadIdx.x == 0) {
    if (k < (m + 1) / 2) {
      out[4 * k] = red[0][0], out[4 * k + 1] = red[0][1];
      if (2 * k + 1 < m) out[4 * k + 2] = red[0][2], out[4 * k + 3] = red[0][3];
    } else {
      out[2 * m] = red[0][0];
    }
  }
}

// ---- combine -------------------------------------------------------------------------------------------------------
// One float64 fma chain per component over j = 0 .. m - 1: re takes c_r x_r then -c_i x_i, im takes c_r x_i then c_i x_r; the chain
// starts from the first product.  (The launcher has dropped the terms whose coefficient is exactly 0: m = 0 stores zeros.)
template <typename T, int E>
__device__ __forceinline__ void krylov_chain(const ArtnKrylovCombineArgs &args, int m, long i, double re[E], double im[E]) {
#pragma unroll
  for (int e = 0; e < E; ++e) re[e] = 0.0, im[e] = 0.0;
  if (m < 1) return;
  {
    const double cr = args.c[0][0], ci = args.c[0][1];
    double xr[E], xi[E];
    krylov_load<E>((const T *)args.x[0], i, xr, xi);
#pragma unroll
    for (int e = 0; e < E; ++e) {
      re[e] = fma(-ci, xi[e], cr * xr[e]);
      im[e] = fma(ci, xr[e], cr * xi[e]);
    }
  }
#pragma unroll 4
  for (int j = 1; j < m; ++j) {
    const double cr = args.c[j][0], ci = args.c[j][1];
    double xr[E], xi[E];
    krylov_load<E>((const T *)args.x[j], i, xr, xi);
#pragma unroll
    for (int e = 0; e < E; ++e) {
      re[e] = fma(-ci, xi[e], fma(cr, xr[e], re[e]));
      im[e] = fma(ci, xr[e], fma(cr, xi[e], im[e]));
    }
  }
}

// rounds to the dtype, stores, and returns |stored|^2 per element (the terms of artn_k_born_overlap<T, false>)
__device__ __forceinline__ void krylov_store4(float2 *y, long i, const double re[4], const double im[4], double t[4]) {
  const float4 v0 = make_float4((float)re[0], (float)im[0], (float)re[1], (float)im[1]);
  const float4 v1 = make_float4((float)re[2], (float)im[2], (float)re[3], (float)im[3]);
  *(float4 *)(y + i) = v0, *(float4 *)(y + i + 2) = v1;
  t[0] = born_sq(v0.x, v0.y), t[1] = born_sq(v0.z, v0.w), t[2] = born_sq(v1.x, v1.y), t[3] = born_sq(v1.z, v1.w);
}
__device__ __forceinline__ void krylov_store4(double2 *y, long i, const double re[4], const double im[4], double t[4]) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    y[i + e] = make_double2(re[e], im[e]);
    t[e] = born_sq(re[e], im[e]);
  }
}
__device__ __forceinline__ double krylov_store1(float2 *y, long i, double re, double im) {
  const float2 v = make_float2((float)re, (float)im);
  y[i] = v;
  return born_sq(v.x, v.y);
}
__device__ __forceinline__ double krylov_store1(double2 *y, long i, double re, double im) {
  y[i] = make_double2(re, im);
  return born_sq(re, im);
}

// y may be one of the inputs (the same pointer): a thread has read every input of its elements before it stores them, and no
// other thread touches them.  (No __restrict__ on y or the inputs for that reason.)
template <typename T>
__global__ __launch_bounds__(ARTN_BORN_THREADS) void artn_k_krylov_combine(ArtnKrylovCombineArgs args, int m, T *y, long n,
                                                                           double *__restrict__ partial) {
  __shared__ double red[ARTN_BORN_THREADS][1];
  double acc[1] = {0.0};
  const long n4 = n >> 2;
  const long step = (long)gridDim.x * ARTN_BORN_THREADS;
  for (long s = (long)blockIdx.x * ARTN_BORN_THREADS + threadIdx.x; s < n4; s += step) {
    double re[4], im[4], t[4];
    krylov_chain<T, 4>(args, m, s * 4, re, im);
    krylov_store4(y, s * 4, re, im, t);
    acc[0] += ((t[0] + t[1]) + (t[2] + t[3]));
  }
  if (blockIdx.x == 0 && threadIdx.x == 0)
    for (long i = n4 * 4; i < n; ++i) {
      double re[1], im[1];
      krylov_chain<T, 1>(args, m, i, re, im);
      acc[0] += krylov_store1(y, i, re[0], im[0]);
    }
  born_wg_tree<1>(red, acc);
  if (threadIdx.x == 0) partial[blockIdx.x] = red[0][0];
}

#endif // ARTN_KRYLOV_KERNEL_H
