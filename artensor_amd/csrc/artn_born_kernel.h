// artn_born_kernel.h -- Born statistics of an amplitude array on gfx950: <a|b> and norms, block sums and their prefix,
// sample resolution, marginals.  Every kernel is one streaming pass over the amplitudes with float64 accumulation in an
// order that depends on the problem size alone (never on scheduling): no floating-point atomics anywhere, every partial
// has one owner, every reduction is a fixed tree or a fixed sequence.  Each complex64 term is converted to float64 FIRST
// and squared there, so |a|^2 = fl(re*re + im*im) carries one rounding (the products are exact in float64).
//
//   artn_k_born_overlap<T, PAIR>   per-workgroup partials {Re<a|b>, Im<a|b>, |a|^2, |b|^2}  (PAIR = false: |a|^2 alone)
//   artn_k_born_finish             one workgroup: partials -> the four results, fixed order
//   artn_k_born_block_sums<T>      one workgroup per block of 2^B elements: block_sum[j]
//   artn_k_born_prefix             one workgroup: inclusive prefix of the block sums (properties below)
//   artn_k_born_pick<T>            one workgroup per block: resolves every (sorted) target that falls into it
//   artn_k_marginal_stream<T>      power-of-two extents: chunks of 2^12 contiguous elements, float64 bins in LDS
//   artn_k_marginal_finish         sums the partial rows of artn_k_marginal_stream in a fixed order
//   artn_k_marginal_generic<T>     any extents: one thread per output element
//
// The hierarchical prefix (used for the block sums and, inside a block, for its 4-element segments): thread k scans its
// K consecutive entries sequentially (local[]), one thread scans the per-thread totals sequentially (base[]), then
// P[i] = fl(base[k] + local[i]).  Because total[k] IS local[last of k], P is non-decreasing across thread boundaries too, and
// P[i] > P[i-1] only where entry i is non-zero: a bisection for "smallest i with P[i] > r" always lands on a non-zero entry.
//
// (artn_pauli_kernel.h includes this header for born_wg_tree and the term helpers: the kernels that are no templates are `static`,
// so that a second translation unit neither emits nor redefines them.)
#ifndef ARTN_BORN_KERNEL_H
#define ARTN_BORN_KERNEL_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#define ARTN_BORN_THREADS 256
#define ARTN_BORN_MIN_BLOCK_BITS 10
#define ARTN_BORN_MAX_BLOCK_BITS 14
#define ARTN_BORN_MAX_GRID 2048        /* workgroups of the overlap pass (8 per CU) */
#define ARTN_BORN_MAX_SEGS (1 << (ARTN_BORN_MAX_BLOCK_BITS - 2))
#define ARTN_BORN_PREFIX_THREADS 1024
#define ARTN_MARG_CHUNK_BITS 12        /* streaming marginal: elements per chunk = 2^12 (32 KiB of float64 terms in LDS) */
#define ARTN_MARG_MAX_KEPT_BITS 24     /* streaming marginal: at most 2^24 kept (output) elements */
#define ARTN_MARG_MAX_DIMS 96

// ---- terms ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double born_sq(float re, float im) {
  const double r = (double)re, m = (double)im;
  return fma(r, r, m * m); // r*r and m*m are exact (24-bit significands): one rounding in all
}
__device__ __forceinline__ double born_sq(double re, double im) { return fma(re, re, im * im); }
__device__ __forceinline__ double born_term(const float2 *a, long i) { const float2 v = a[i]; return born_sq(v.x, v.y); }
__device__ __forceinline__ double born_term(const double2 *a, long i) { const double2 v = a[i]; return born_sq(v.x, v.y); }

// |a[i..i+3]|^2 of one whole 4-element segment (i a multiple of 4, a 16-byte aligned): 16-byte loads
__device__ __forceinline__ void born_seg4(const float2 *a, long i, double t[4]) {
  const float4 v0 = *(const float4 *)(a + i), v1 = *(const float4 *)(a + i + 2);
  t[0] = born_sq(v0.x, v0.y), t[1] = born_sq(v0.z, v0.w), t[2] = born_sq(v1.x, v1.y), t[3] = born_sq(v1.z, v1.w);
}
__device__ __forceinline__ void born_seg4(const double2 *a, long i, double t[4]) {
#pragma unroll
  for (int e = 0; e < 4; ++e) t[e] = born_term(a, i + e);
}
// the same with elements at or beyond n counted as zero
template <typename T> __device__ __forceinline__ void born_seg4_tail(const T *a, long i, long n, double t[4]) {
#pragma unroll
  for (int e = 0; e < 4; ++e) t[e] = (i + e < n) ? born_term(a, i + e) : 0.0;
}

// fixed-order tree over the 256 threads of a workgroup, NV values per thread; result in red[0..NV)
template <int NV> __device__ __forceinline__ void born_wg_tree(double (*red)[NV], const double v[NV]) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int q = 0; q < NV; ++q) red[tid][q] = v[q];
  __syncthreads();
  for (int s = ARTN_BORN_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) {
#pragma unroll
      for (int q = 0; q < NV; ++q) red[tid][q] += red[tid + s][q];
    }
    __syncthreads();
  }
}

// ---- overlap -------------------------------------------------------------------------------------------------------
// Workgroup g of G owns the 1024-element tiles g, g + G, g + 2G ...; inside a tile thread t owns elements 4t..4t+3.  Each thread
// adds its terms in that order into private float64 accumulators; the workgroup tree and the finish kernel are fixed too.
template <typename T, bool PAIR>
__global__ __launch_bounds__(ARTN_BORN_THREADS) void artn_k_born_overlap(const T *__restrict__ a, const T *__restrict__ b, long n,
                                                                         double *__restrict__ partial) {
  constexpr int NV = PAIR ? 4 : 1;
  __shared__ double red[ARTN_BORN_THREADS][NV];
  double acc[NV];
#pragma unroll
  for (int q = 0; q < NV; ++q) acc[q] = 0.0;
  const long n4 = n >> 2; // whole segments
  const long step = (long)gridDim.x * ARTN_BORN_THREADS;
  long s = (long)blockIdx.x * ARTN_BORN_THREADS + threadIdx.x;
  if constexpr (!PAIR) {
#pragma unroll 4
    for (; s < n4; s += step) {
      double t[4];
      born_seg4(a, s * 4, t);
      acc[0] += ((t[0] + t[1]) + (t[2] + t[3]));
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
      for (long i = n4 * 4; i < n; ++i) acc[0] += born_term(a, i);
  } else {
    auto one = [&](long i) {
      const auto x = a[i];
      const auto y = b[i];
      const double xr = (double)x.x, xi = (double)x.y, yr = (double)y.x, yi = (double)y.y;
      acc[0] += fma(xr, yr, xi * yi);  // Re conj(x) y
      acc[1] += fma(xr, yi, -(xi * yr)); // Im conj(x) y
      acc[2] += fma(xr, xr, xi * xi);
      acc[3] += fma(yr, yr, yi * yi);
    };
#pragma unroll 2
    for (; s < n4; s += step) {
      if constexpr (sizeof(T) == 8) {
        const float4 x0 = *(const float4 *)(a + s * 4), x1 = *(const float4 *)(a + s * 4 + 2);
        const float4 y0 = *(const float4 *)(b + s * 4), y1 = *(const float4 *)(b + s * 4 + 2);
        const float xs[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
        const float ys[8] = {y0.x, y0.y, y0.z, y0.w, y1.x, y1.y, y1.z, y1.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const double xr = (double)xs[2 * e], xi = (double)xs[2 * e + 1], yr = (double)ys[2 * e], yi = (double)ys[2 * e + 1];
          acc[0] += fma(xr, yr, xi * yi);
          acc[1] += fma(xr, yi, -(xi * yr));
          acc[2] += fma(xr, xr, xi * xi);
          acc[3] += fma(yr, yr, yi * yi);
        }
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) one(s * 4 + e);
      }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
      for (long i = n4 * 4; i < n; ++i) one(i);
  }
  born_wg_tree<NV>(red, acc);
  if (threadIdx.x < NV) partial[(long)blockIdx.x * NV + threadIdx.x] = red[0][threadIdx.x];
}

// out4 = {Re, Im, |a|^2, |b|^2}; nv = 1: the partials hold |a|^2 alone and out4 = {|a|^2, 0, |a|^2, |a|^2}
// (the sums of the finish, left in red[0][0..4): artn_krylov_kernel.h finishes its groups of four partials with the same code)
__device__ __forceinline__ void born_finish_sum(const double *__restrict__ partial, int n_partial, int nv, double (*red)[4]) {
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int g = threadIdx.x; g < n_partial; g += ARTN_BORN_THREADS)
    for (int q = 0; q < nv; ++q) acc[q] += partial[(long)g * nv + q];
  born_wg_tree<4>(red, acc);
}
static __global__ __launch_bounds__(ARTN_BORN_THREADS) void artn_k_born_finish(const double *__restrict__ partial, int n_partial, int nv,
                                                                        double *__restrict__ out4) {
  __shared__ double red[ARTN_BORN_THREADS][4];
  born_finish_sum(partial, n_partial, nv, red);
  if (threadIdx.x == 0) {
    if (nv == 1) {
      out4[0] = red[0][0], out4[1] = 0.0, out4[2] = red[0][0], out4[3] = red[0][0];
    } else {
      out4[0] = red[0][0], out4[1] = red[0][1], out4[2] = red[0][2], out4[3] = red[0][3];
    }
  }
}

// ---- blocks --------------------------------------------------------------------------------------------------------
// (LDS index of segment s: one pad per 16 entries keeps the per-thread runs of the scan off one bank)
#define BORN_PIDX(s) ((s) + ((s) >> 4))
#define BORN_PSEG_DOUBLES (ARTN_BORN_MAX_SEGS + (ARTN_BORN_MAX_SEGS >> 4))

// Where the segments of a block lie.  tile(q, tid): the first element of segment q * ARTN_BORN_THREADS + tid, as the scan walks
// them; seg(s): of segment s, wherever a pick lands.  BornSegLinear is a block of consecutive memory elements;
// artn_sample_batch_kernel.h has the one of a trajectory whose local bits are spread over memory.
struct BornSegLinear {
  long base;
  __device__ __forceinline__ long tile(int q, int tid) const { return base + ((long)(q * ARTN_BORN_THREADS + tid)) * 4; }
  __device__ __forceinline__ long seg(int s) const { return base + (long)s * 4; }
};

// Inclusive prefix sums of the 4-element segment sums of a block of 2^bbits elements into pseg[BORN_PIDX(s)]; `whole` (uniform):
// every element of the block exists, otherwise those whose address is at or beyond n count as zero.  Segment sum =
// ((t0 + t1) + t2) + t3; prefix as described at the top of this file.
template <typename T, typename AT>
__device__ __forceinline__ void born_block_scan_at(const T *__restrict__ a, long n, bool whole, const AT &at, int bbits, double *pseg,
                                                   double *tot) {
  const int tid = threadIdx.x;
  const int S = 1 << (bbits - 2), K = S / ARTN_BORN_THREADS; // bbits >= 10: K >= 1
  if (whole) {
#pragma unroll 4
    for (int q = 0; q < K; ++q) {
      double t[4];
      born_seg4(a, at.tile(q, tid), t);
      pseg[BORN_PIDX(q * ARTN_BORN_THREADS + tid)] = ((t[0] + t[1]) + t[2]) + t[3];
    }
  } else {
    for (int q = 0; q < K; ++q) {
      double t[4];
      born_seg4_tail(a, at.tile(q, tid), n, t);
      pseg[BORN_PIDX(q * ARTN_BORN_THREADS + tid)] = ((t[0] + t[1]) + t[2]) + t[3];
    }
  }
  __syncthreads();
  double run = 0.0;
  for (int q = 0; q < K; ++q) {
    const int i = BORN_PIDX(tid * K + q);
    run += pseg[i];
    pseg[i] = run;
  }
  tot[tid] = run;
  __syncthreads();
  if (tid == 0) {
    double e = 0.0;
#pragma unroll 8
    for (int k = 0; k < ARTN_BORN_THREADS; ++k) {
      const double x = tot[k];
      tot[k] = e;
      e += x;
    }
  }
  __syncthreads();
  const double b = tot[tid];
  if (tid > 0)
    for (int q = 0; q < K; ++q) {
      const int i = BORN_PIDX(tid * K + q);
      pseg[i] = b + pseg[i];
    }
  __syncthreads();
}
// the block [base, base + 2^bbits) of consecutive elements
template <typename T>
__device__ __forceinline__ void born_block_scan(const T *__restrict__ a, long n, long base, int bbits, double *pseg, double *tot) {
  born_block_scan_at(a, n, base + ((long)1 << bbits) <= n, BornSegLinear{base}, bbits, pseg, tot);
}

template <typename T>
__global__ __launch_bounds__(ARTN_BORN_THREADS) void artn_k_born_block_sums(const T *__restrict__ a, long n, int bbits,
                                                                            double *__restrict__ block_sum) {
  __shared__ double pseg[BORN_PSEG_DOUBLES];
  __shared__ double tot[ARTN_BORN_THREADS];
  born_block_scan(a, n, (long)blockIdx.x << bbits, bbits, pseg, tot);
  if (threadIdx.x == 0) block_sum[blockIdx.x] = pseg[BORN_PIDX((1 << (bbits - 2)) - 1)];
}

// the body of artn_k_born_prefix: one workgroup of ARTN_BORN_PREFIX_THREADS threads, one row of nb sums (tot: LDS, one per thread)
__device__ __forceinline__ void born_prefix_row(const double *__restrict__ block_sum, double *__restrict__ prefix, long nb, double *tot) {
  const int tid = threadIdx.x;
  const long K = (nb + ARTN_BORN_PREFIX_THREADS - 1) / ARTN_BORN_PREFIX_THREADS;
  const long lo = tid * K < nb ? tid * K : nb, hi = lo + K < nb ? lo + K : nb;
  double run = 0.0;
#pragma unroll 8
  for (long i = lo; i < hi; ++i) {
    run += block_sum[i];
    prefix[i] = run;
  }
  tot[tid] = run;
  __syncthreads();
  if (tid == 0) {
    double e = 0.0;
#pragma unroll 8
    for (int k = 0; k < ARTN_BORN_PREFIX_THREADS; ++k) {
      const double x = tot[k];
      tot[k] = e;
      e += x;
    }
  }
  __syncthreads();
  const double b = tot[tid];
  if (tid > 0)
    for (long i = lo; i < hi; ++i) prefix[i] = b + prefix[i]; // (each thread re-reads its own stores only)
}
static __global__ __launch_bounds__(ARTN_BORN_PREFIX_THREADS) void artn_k_born_prefix(const double *__restrict__ block_sum,
                                                                               double *__restrict__ prefix, long nb) {
  __shared__ double tot[ARTN_BORN_PREFIX_THREADS];
  born_prefix_row(block_sum, prefix, nb, tot);
}

template <typename X> __device__ __forceinline__ long born_lower_bound_of(const X &x, long m, double v) { // first s with x(s) >= v
  long lo = 0, hi = m;
  while (lo < hi) {
    const long mid = (lo + hi) >> 1;
    if (x(mid) >= v) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}
__device__ __forceinline__ long born_lower_bound(const double *__restrict__ x, long m, double v) { // first s with x[s] >= v
  return born_lower_bound_of([&](long s) { return x[s]; }, m, v);
}

// One target of a scanned block: r = target - (what lies before the block), ptot the block's own total.  The block's S segments
// are pseg[BORN_PIDX(s0 .. s0 + S - 1)] (entries after the last non-zero segment equal ptot).  The smallest element whose running
// sum exceeds r, never one with |a|^2 == 0; r at or past ptot: the last non-zero element.  *index is the element's address.
template <typename T, typename AT>
__device__ __forceinline__ void born_pick_one(const T *__restrict__ a, long n, const AT &at, int s0, int S, const double *pseg, double ptot,
                                              double r, long long *__restrict__ index, double *__restrict__ prob) {
  const bool beyond = !(ptot > r); // at or past the block's own total: the last non-zero element
  int lo = 0, hi = S - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    const double p = pseg[BORN_PIDX(s0 + mid)];
    if (beyond ? (p >= ptot) : (p > r)) hi = mid;
    else lo = mid + 1;
  }
  double t[4];
  const long i0 = at.seg(lo);
  born_seg4_tail(a, i0, n, t);
  double run = lo ? pseg[BORN_PIDX(s0 + lo - 1)] : 0.0;
  int pick = -1, lastnz = -1;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    run += t[e];
    if (t[e] > 0.0) {
      lastnz = e;
      if (pick < 0 && !beyond && run > r) pick = e;
    }
  }
  if (pick < 0) pick = lastnz;
  *index = pick < 0 ? -1 : (long long)(i0 + pick);
  *prob = pick == 0 ? t[0] : pick == 1 ? t[1] : pick == 2 ? t[2] : pick == 3 ? t[3] : 0.0;
}

// Workgroup j resolves the targets t with prefix[j-1] <= t < prefix[j] (the last block whose prefix grew also takes every t at or
// beyond the total).  `targets` must be ascending: the workgroup finds its range by bisection and reads its block ONCE for all of
// them; blocks without a target return before touching the amplitudes.
template <typename T>
__global__ __launch_bounds__(ARTN_BORN_THREADS) void artn_k_born_pick(const T *__restrict__ a, long n, int bbits, long nb,
                                                                      const double *__restrict__ prefix,
                                                                      const double *__restrict__ targets, long m,
                                                                      long long *__restrict__ out_index, double *__restrict__ out_prob) {
  __shared__ double pseg[BORN_PSEG_DOUBLES];
  __shared__ double tot[ARTN_BORN_THREADS];
  const long j = blockIdx.x;
  const double total = prefix[nb - 1];
  const double hi_t = prefix[j], lo_t = j ? prefix[j - 1] : 0.0;
  if (!(hi_t > lo_t)) return; // nothing in this block
  const long s_lo = born_lower_bound(targets, m, lo_t);
  const long s_hi = (hi_t == total) ? m : born_lower_bound(targets, m, hi_t);
  if (s_lo >= s_hi) return;
  const long base = j << bbits;
  born_block_scan(a, n, base, bbits, pseg, tot);
  const int S = 1 << (bbits - 2);
  const double ptot = pseg[BORN_PIDX(S - 1)];
  for (long s = s_lo + threadIdx.x; s < s_hi; s += ARTN_BORN_THREADS)
    born_pick_one(a, n, BornSegLinear{base}, 0, S, pseg, ptot, targets[s] - lo_t, out_index + s, out_prob + s);
}

// ---- marginals -----------------------------------------------------------------------------------------------------
__host__ __device__ inline uint64_t born_pdep(uint64_t v, uint64_t mask) { // bit x of v -> the x-th set bit of mask
  uint64_t r = 0;
  for (uint64_t bb = 1; mask; bb <<= 1) {
    const uint64_t low = mask & (~mask + 1);
    if (v & bb) r |= low;
    mask ^= low;
  }
  return r;
}
__host__ __device__ inline uint64_t born_pext(uint64_t v, uint64_t mask) {
  uint64_t r = 0;
  for (uint64_t bb = 1; mask; bb <<= 1) {
    const uint64_t low = mask & (~mask + 1);
    if (v & low) r |= bb;
    mask ^= low;
  }
  return r;
}

// Streaming plan (power-of-two extents; memory bit = bit of the flat memory index).  Packed kept index pk: bit x of pk is the x-th
// kept memory bit in ascending order; its low bin_bits bits lie inside a chunk (the LDS bins), the rest select the partial row.
struct ArtnMargStream {
  uint64_t kmask_in, dmask_in;       // kept / dropped memory bits below the chunk size
  uint64_t kmask_above, dmask_above; // kept / dropped memory bits at or above it, as bits of the CHUNK index
  uint64_t item_mask, rest_mask;     // in-chunk bits spread over work items (kept bits + the lowest dropped ones) / summed per item
  int32_t bin_bits, above_bits, drop_above_bits, group_bits; // group_bits: log2 partial rows per kept-above value
  int32_t kept_bits;
  uint8_t out_bit[ARTN_MARG_MAX_KEPT_BITS]; // packed kept bit x -> bit of the output index
};

// Workgroup (ka, g): the chunks whose kept-above bits spell ka and whose dropped-above bits spell g * per .. (g + 1) * per - 1, in
// that order.  A chunk's terms go to LDS once; work item w (one owner thread) adds the terms of its bin and slice in ascending
// memory order to acc[w].  Afterwards the slices of a bin are added in ascending order: ws[row * bins + bin].
template <typename T>
__global__ __launch_bounds__(ARTN_BORN_THREADS) void artn_k_marginal_stream(const T *__restrict__ a, ArtnMargStream p,
                                                                            double *__restrict__ ws) {
  constexpr int CH = 1 << ARTN_MARG_CHUNK_BITS;
  __shared__ double terms[CH];
  __shared__ double acc[CH];
  const int tid = threadIdx.x;
  const int item_bits = p.bin_bits > 8 ? p.bin_bits : 8, W = 1 << item_bits, bins = 1 << p.bin_bits;
  for (int w = tid; w < W; w += ARTN_BORN_THREADS) acc[w] = 0.0;
  const uint64_t ka = (uint64_t)blockIdx.x >> p.group_bits, g = (uint64_t)blockIdx.x & (((uint64_t)1 << p.group_bits) - 1);
  const uint64_t per = (uint64_t)1 << (p.drop_above_bits - p.group_bits);
  const uint64_t chunk_kept = born_pdep(ka, p.kmask_above);
  for (uint64_t k = 0; k < per; ++k) {
    const long base = (long)((chunk_kept | born_pdep(g * per + k, p.dmask_above)) << ARTN_MARG_CHUNK_BITS);
    __syncthreads(); // (the previous chunk's terms have been consumed)
#pragma unroll 4
    for (int s = tid; s < CH / 4; s += ARTN_BORN_THREADS) {
      double t[4];
      born_seg4(a, base + (long)s * 4, t);
      *(double2 *)&terms[s * 4] = make_double2(t[0], t[1]);
      *(double2 *)&terms[s * 4 + 2] = make_double2(t[2], t[3]);
    }
    __syncthreads();
    for (int w = tid; w < W; w += ARTN_BORN_THREADS) {
      const uint32_t at = (uint32_t)born_pdep((uint64_t)w, p.item_mask);
      const uint32_t rm = (uint32_t)p.rest_mask;
      double sum = acc[w];
      uint32_t sub = 0;
      do {
        sum += terms[at | sub];
        sub = (sub - rm) & rm; // next subset of rest_mask, ascending
      } while (sub);
      acc[w] = sum;
    }
  }
  __syncthreads();
  const uint64_t slice_mask = p.item_mask & ~p.kmask_in;
  const int slices = W >> p.bin_bits;
  for (int b = tid; b < bins; b += ARTN_BORN_THREADS) {
    const uint64_t at = born_pdep((uint64_t)b, p.kmask_in);
    double v = 0.0;
    for (int sl = 0; sl < slices; ++sl) v += acc[born_pext(at | born_pdep((uint64_t)sl, slice_mask), p.item_mask)];
    ws[(long)blockIdx.x * bins + b] = v;
  }
}

static __global__ __launch_bounds__(ARTN_BORN_THREADS) void artn_k_marginal_finish(const double *__restrict__ ws, ArtnMargStream p,
                                                                            double *__restrict__ out) {
  const long o = (long)blockIdx.x * ARTN_BORN_THREADS + threadIdx.x;
  if (o >= ((long)1 << p.kept_bits)) return;
  uint64_t pk = 0;
  for (int x = 0; x < p.kept_bits; ++x) pk |= (((uint64_t)o >> p.out_bit[x]) & 1) << x;
  const long bins = (long)1 << p.bin_bits, bin = (long)(pk & (uint64_t)(bins - 1)), ka = (long)(pk >> p.bin_bits);
  const long rows = (long)1 << p.group_bits;
  double v = 0.0;
#pragma unroll 8
  for (long g = 0; g < rows; ++g) v += ws[((ka << p.group_bits) + g) * bins + bin];
  out[o] = v;
}

// Any extents.  dims [0, n_keep) are the kept ones in output order (last fastest), the others are summed, last fastest.
struct ArtnMargGeneric {
  int32_t n_keep, n_drop;
  int64_t extent[ARTN_MARG_MAX_DIMS], stride[ARTN_MARG_MAX_DIMS];
};
template <typename T>
__global__ __launch_bounds__(ARTN_BORN_THREADS) void artn_k_marginal_generic(const T *__restrict__ a, ArtnMargGeneric p, long n_out,
                                                                             long n_sum, double *__restrict__ out) {
  const long o = (long)blockIdx.x * ARTN_BORN_THREADS + threadIdx.x;
  if (o >= n_out) return;
  long rem = o, at = 0;
  for (int d = p.n_keep - 1; d >= 0; --d) {
    at += (rem % p.extent[d]) * p.stride[d];
    rem /= p.extent[d];
  }
  double v = 0.0;
  for (long q = 0; q < n_sum; ++q) {
    long r = q, off = at;
    for (int d = p.n_keep + p.n_drop - 1; d >= p.n_keep; --d) {
      off += (r % p.extent[d]) * p.stride[d];
      r /= p.extent[d];
    }
    v += born_term(a, off);
  }
  out[o] = v;
}

#endif // ARTN_BORN_KERNEL_H
