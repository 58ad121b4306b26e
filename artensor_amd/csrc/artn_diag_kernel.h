// artn_diag_kernel.h -- diagonal operators on gfx950: f(i) = sum_k c_k (-1)^popcount(i & zmask_k) evaluated once per element
// and used by one streaming pass (include/artn.h: DIAGONAL OPERATORS).
//
//   artn_k_diag<T, OP>   T = float2 / double2; OP = DIAG_VALUES, DIAG_EXPECT, DIAG_PHASE, DIAG_MULTIPLY, DIAG_PAIR (both states
//                        take the phase, and the transition element), DIAG_PAIR_T (the transition element alone)
//   artn_k_diag_finish   one workgroup: the per-workgroup partials -> the sums, in the fixed order of artn_k_born_finish
//
// A workgroup of 256 threads owns the tiles blockIdx.x, blockIdx.x + gridDim.x, ... of 2^10 elements.  Once per workgroup S (the
// static terms, 2^TB float64), the masks of the groups and the first DIAG_LDS_TERMS dynamic term records go to LDS.  Per tile h:
// every thread issues its 16-byte loads (consecutive lanes, consecutive addresses); thread 4g then forms w_g(h), the sequential
// chain over the terms of group g in the caller's order, into one of two LDS buffers (so one barrier per tile is enough); after
// the barrier each thread forms f for its four elements: S[l], then the groups in order, + or - w_g by popcount(l & lo_g).
// Every addition is a plain float64 addition of the contract (nothing here can contract to an fma: no product feeds a sum).
// States below 2^10 elements have only static terms and are handled by one workgroup, element by element.
//
// Sums (EXPECT, PAIR): private float64 accumulators per thread over its elements in ascending tile order, the fixed tree of
// born_wg_tree (in the LDS of S, which is no longer read then), one partial row of four per workgroup, artn_k_diag_finish.
#ifndef ARTN_DIAG_KERNEL_H
#define ARTN_DIAG_KERNEL_H

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "artn.h"
#include "artn_born_kernel.h"

#define DIAG_VALUES 0
#define DIAG_EXPECT 1
#define DIAG_PHASE 2
#define DIAG_MULTIPLY 3
#define DIAG_PAIR 4
#define DIAG_PAIR_T 5
#define DIAG_LDS_TERMS 512 /* dynamic term records kept in LDS (8 KiB); the records beyond are read from the table */
#define DIAG_CHUNK 8       /* term records fetched together in front of their additions */

template <typename T> struct DiagRaw { using type = double2; };
template <> struct DiagRaw<float2> { using type = float4; };

__device__ __forceinline__ void diag_unpack(const float4 v, double re[2], double im[2]) {
  re[0] = (double)v.x, im[0] = (double)v.y, re[1] = (double)v.z, im[1] = (double)v.w;
}
__device__ __forceinline__ void diag_unpack(const double2 v, double re[1], double im[1]) { re[0] = v.x, im[0] = v.y; }
__device__ __forceinline__ void diag_pack(float4 &v, const double re[2], const double im[2]) {
  v = make_float4((float)re[0], (float)im[0], (float)re[1], (float)im[1]);
}
__device__ __forceinline__ void diag_pack(double2 &v, const double re[1], const double im[1]) { v = make_double2(re[0], im[0]); }

// One element: (ar, ai) of `a` and, in the pair forms, (br, bi) of `b` (a = lam, b = phi); acc[] the thread's sums.
template <int OP>
__device__ __forceinline__ void diag_elem(double &ar, double &ai, double &br, double &bi, double f, double gamma, double acc[4]) {
  if constexpr (OP == DIAG_EXPECT) {
    const double p = fma(ar, ar, ai * ai);
    acc[0] += p;
    acc[1] = fma(p, f, acc[1]);
    acc[2] = fma(p * f, f, acc[2]);
  }
  if constexpr (OP == DIAG_PAIR || OP == DIAG_PAIR_T) {
    const double ur = fma(ar, br, ai * bi), ui = fma(ar, bi, -(ai * br)); // conj(lam) phi
    acc[0] = fma(ur, f, acc[0]);
    acc[1] = fma(ui, f, acc[1]);
  }
  if constexpr (OP == DIAG_PHASE || OP == DIAG_PAIR) {
    const double ph = gamma * f;
    double s, c;
    sincos(ph, &s, &c);
    const double re = fma(ar, c, ai * s), im = fma(ai, c, -(ar * s));
    ar = re, ai = im;
    if constexpr (OP == DIAG_PAIR) {
      const double re2 = fma(br, c, bi * s), im2 = fma(bi, c, -(br * s));
      br = re2, bi = im2;
    }
  }
  if constexpr (OP == DIAG_MULTIPLY) {
    ar = ar * f, ai = ai * f;
  }
}

template <typename T, int OP>
__global__ __launch_bounds__(ARTN_BORN_THREADS) void artn_k_diag(T *__restrict__ a, T *__restrict__ b,
                                                                 const ArtnDiagTable *__restrict__ tab, int tb, long n_tiles,
                                                                 int n_groups, double gamma, double *__restrict__ out) {
  using V = typename DiagRaw<T>::type;
  constexpr int EPA = 16 / sizeof(T);                                    // elements of one 16-byte access
  constexpr int NA = (1 << ARTN_DIAG_TILE_BITS) / (ARTN_BORN_THREADS * EPA); // accesses per thread and tile
  constexpr bool SUMS = OP == DIAG_EXPECT || OP == DIAG_PAIR || OP == DIAG_PAIR_T;
  constexpr bool LOADS = OP != DIAG_VALUES, TWO = OP == DIAG_PAIR || OP == DIAG_PAIR_T;
  constexpr bool STORES = OP == DIAG_PHASE || OP == DIAG_MULTIPLY || OP == DIAG_PAIR;
  __shared__ double S[1 << ARTN_DIAG_TILE_BITS];
  __shared__ ArtnDiagTerm lterm[DIAG_LDS_TERMS];
  __shared__ double w[2][ARTN_DIAG_MAX_GROUPS];
  __shared__ uint32_t glo[ARTN_DIAG_MAX_GROUPS];
  static_assert(sizeof(S) == sizeof(double) * ARTN_BORN_THREADS * 4, "S is reused as the reduction buffer");
  const int tid = threadIdx.x;
  const double *Sg = (const double *)(tab + 1);
  const ArtnDiagGroup *grp = (const ArtnDiagGroup *)(Sg + ((long)1 << tb));
  const ArtnDiagTerm *trm = (const ArtnDiagTerm *)(grp + n_groups);
  double acc[4] = {0.0, 0.0, 0.0, 0.0};

  for (int l = tid; l < (1 << tb); l += ARTN_BORN_THREADS) S[l] = Sg[l];

  if (tb < ARTN_DIAG_TILE_BITS) {
    // the small form: one workgroup, every term static
    __syncthreads();
    if (blockIdx.x == 0)
      for (int l = tid; l < (1 << tb); l += ARTN_BORN_THREADS) {
        const double f = S[l];
        if constexpr (OP == DIAG_VALUES) {
          out[l] = f;
        } else {
          double ar = (double)a[l].x, ai = (double)a[l].y, br = 0.0, bi = 0.0;
          if constexpr (TWO) br = (double)b[l].x, bi = (double)b[l].y;
          diag_elem<OP>(ar, ai, br, bi, f, gamma, acc);
          if constexpr (STORES) {
            a[l].x = (decltype(a[l].x))ar, a[l].y = (decltype(a[l].y))ai;
            if constexpr (OP == DIAG_PAIR) b[l].x = (decltype(b[l].x))br, b[l].y = (decltype(b[l].y))bi;
          }
        }
      }
  } else {
    uint64_t my_first = 0, my_end = 0; // thread 4g forms w_g
    const bool chain = (tid & 3) == 0 && (tid >> 2) < n_groups;
    if (chain) {
      const ArtnDiagGroup g = grp[tid >> 2];
      my_first = g.first, my_end = g.first + g.count;
      glo[tid >> 2] = (uint32_t)g.lo;
    }
    {
      const long n_dyn = (long)tab->n_dynamic;
      for (int t = tid; t < DIAG_LDS_TERMS && t < n_dyn; t += ARTN_BORN_THREADS) lterm[t] = trm[t];
    }
    __syncthreads();
    int buf = 0;
    for (long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x, buf ^= 1) {
      const long base = tile << ARTN_DIAG_TILE_BITS;
      V va[NA], vb[NA];
      if constexpr (LOADS) {
#pragma unroll
        for (int j = 0; j < NA; ++j) {
          const long at = base + (long)(j * ARTN_BORN_THREADS + tid) * EPA;
          va[j] = *(const V *)(a + at);
          if constexpr (TWO) vb[j] = *(const V *)(b + at);
        }
      }
      if (chain) {
        double wg = 0.0;
        for (uint64_t t = my_first; t < my_end; t += DIAG_CHUNK) {
          ArtnDiagTerm r[DIAG_CHUNK];
#pragma unroll
          for (int q = 0; q < DIAG_CHUNK; ++q) {
            const uint64_t at = t + q < my_end ? t + q : my_end - 1;
            r[q] = at < DIAG_LDS_TERMS ? lterm[at] : trm[at];
          }
#pragma unroll
          for (int q = 0; q < DIAG_CHUNK; ++q)
            if (t + q < my_end) wg += (__popcll((uint64_t)tile & r[q].hi) & 1) ? -r[q].c : r[q].c;
        }
        w[buf][tid >> 2] = wg;
      }
      __syncthreads();
      double f[NA][EPA];
#pragma unroll
      for (int j = 0; j < NA; ++j)
#pragma unroll
        for (int e = 0; e < EPA; ++e) f[j][e] = S[(j * ARTN_BORN_THREADS + tid) * EPA + e];
      for (int g = 0; g < n_groups; ++g) {
        const double wg = w[buf][g];
        const uint32_t m = glo[g];
#pragma unroll
        for (int j = 0; j < NA; ++j)
#pragma unroll
          for (int e = 0; e < EPA; ++e) {
            const uint32_t l = (uint32_t)((j * ARTN_BORN_THREADS + tid) * EPA + e);
            f[j][e] += (__popc(l & m) & 1) ? -wg : wg;
          }
      }
#pragma unroll
      for (int j = 0; j < NA; ++j) {
        const long at = base + (long)(j * ARTN_BORN_THREADS + tid) * EPA;
        if constexpr (OP == DIAG_VALUES) {
#pragma unroll
          for (int e = 0; e < EPA; ++e) out[at + e] = f[j][e];
        } else {
          double ar[EPA], ai[EPA], br[EPA], bi[EPA];
          diag_unpack(va[j], ar, ai);
          if constexpr (TWO) diag_unpack(vb[j], br, bi);
          else {
#pragma unroll
            for (int e = 0; e < EPA; ++e) br[e] = bi[e] = 0.0;
          }
#pragma unroll
          for (int e = 0; e < EPA; ++e) diag_elem<OP>(ar[e], ai[e], br[e], bi[e], f[j][e], gamma, acc);
          if constexpr (STORES) {
            V o;
            diag_pack(o, ar, ai);
            *(V *)(a + at) = o;
            if constexpr (OP == DIAG_PAIR) {
              diag_pack(o, br, bi);
              *(V *)(b + at) = o;
            }
          }
        }
      }
    }
  }
  if constexpr (SUMS) {
    __syncthreads(); // (S is read no more)
    born_wg_tree<4>((double(*)[4])S, acc);
    if (tid < 4) out[(long)blockIdx.x * 4 + tid] = S[tid];
  }
}

// out[0 .. nv) = the sums of the partial rows (four float64 each), in the order of artn_k_born_finish
static __global__ __launch_bounds__(ARTN_BORN_THREADS) void artn_k_diag_finish(const double *__restrict__ partial, int n_partial, int nv,
                                                                        double *__restrict__ out) {
  __shared__ double red[ARTN_BORN_THREADS][4];
  born_finish_sum(partial, n_partial, 4, red);
  if ((int)threadIdx.x < nv) out[threadIdx.x] = red[0][threadIdx.x];
}

#endif // ARTN_DIAG_KERNEL_H
