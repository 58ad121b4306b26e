// artn_sample_batch_kernel.h -- bitstring sampling PER TRAJECTORY of a batched amplitude array on gfx950: B states in one tensor
// (artn_batch_kernel.h), B cumulative distributions, S sorted uniforms per trajectory resolved to element addresses.
//
// Index space: that of artn_pauli_batch_kernel.h.  A trajectory has M local bits, local bit j being the j-th lowest memory bit
// that is no batch bit; the address of (b, local) is pauli_batch_traj(b) | pauli_batch_local(local), both deposits bitwise.
// Memory bits 0-1 are local bits 0-1 (the line rule), so a 4-element segment is contiguous: the 16-byte loads of born_seg4.
//
// Arithmetic: that of artn_k_born_block_sums / artn_k_born_prefix / artn_k_born_pick (artn_born_kernel.h) on the 2^M elements of
// a trajectory in local-index order -- the kernels here run born_block_scan_at, born_prefix_row and born_pick_one, the bodies of
// those three, with the address of a segment swapped (SampleBatchSeg for BornSegLinear).  The target of (b, s) is the one
// multiply sample_batch_target(uniform[b][s], norm_b), rounded on its own (contraction is switched off inside it: fused into the
// subtraction of lo_t that follows, a target exactly on a block boundary would come out below it); every comparison of the range
// bisection is made on that product.  Row b therefore is what the unbatched kernels give on a dense copy of trajectory b with
// targets = uniforms[b] * norm_b, and does not depend on where the batch bits lie nor on the other rows.
//
//   artn_k_sample_batch_block_sums<T>   TILED.  A unit is (b, block j), j < nb_t = 2^row_bits; workgroups loop over units.
//                                       block_sum[b nb_t + j]
//   artn_k_sample_batch_prefix_rows     TILED, nb_t > 1024: one workgroup per trajectory, artn_k_born_prefix's body on row b
//   artn_k_sample_batch_prefix_packed   TILED, nb_t <= 1024: 1024 consecutive sums = 1024 / nb_t rows per workgroup, each row the
//                                       plain ascending running sum (what artn_k_born_prefix gives for nb <= 1024)
//                                       both write out_norm[b] = prefix[b][nb_t - 1]
//   artn_k_sample_batch_pick<T>         TILED.  A unit is (b, j): bisects row b of the uniforms for the block's targets, leaves
//                                       before touching the amplitudes when there is none, else scans the block once
//   artn_k_sample_batch_small<T>        SMALL, M < 10, B > 1: ONE launch.  A virtual tile of 2^10 consecutive r = (b << M) | local
//                                       holds 2^(10-M) whole trajectories of 2^(M-2) segment-owning threads; the first thread
//                                       of a trajectory forms the ascending running sum of its segments (born_block_scan_at for
//                                       K = 1 with tail zeros) and writes out_norm[b]; its threads resolve its uniforms.  Lanes
//                                       with r >= n are guarded; no sum and no bisection crosses a trajectory.
//
// out_index / out_prob are preset to -1 / 0 by the host (a target no block claims: a trajectory of norm 0 or NaN, a negative
// uniform).  No floating-point atomics; LDS is pseg + tot of the unbatched kernels; the state is only read.
#ifndef ARTN_SAMPLE_BATCH_KERNEL_H
#define ARTN_SAMPLE_BATCH_KERNEL_H

#include "artn_born_kernel.h"
#include "artn_pauli_batch_kernel.h"

#define ARTN_SAMPLE_BATCH_MAX_GRID (1 << 20) /* workgroups of a pass: one unit each up to 2^30 elements of complex64 */
#define ARTN_SAMPLE_BATCH_SMALL_BITS 10      /* M below this (and B > 1): the one-launch form */

struct ArtnSampleBatchArgs { // a kernel argument: every read of it is uniform
  long long B, S, n;         // trajectories, samples per trajectory, elements of the whole tensor
  int32_t local_bits;        // M
  int32_t block_bits;        // artn_born_plan(2^M).block_bits
  int32_t row_bits;          // log2 nb_t
  int32_t reserved;
  ArtnBatchFields f;         // the batch fields, ASCENDING by shift
};

// the target of one sample: ONE rounded multiply, as torch forms `uniforms * total` for the unbatched pick
__device__ __forceinline__ double sample_batch_target(double u, double total) {
#pragma clang fp contract(off)
  return u * total;
}

// the segments of the block of trajectory-and-block address `base` (uniform); piece: pauli_batch_local(4 tid), once per thread
struct SampleBatchSeg {
  uint64_t base, piece;
  const ArtnBatchFields &f;
  __device__ __forceinline__ long tile(int q, int) const { // (q is uniform: its deposit is scalar work)
    return (long)(base | piece | pauli_batch_local(f, (uint64_t)q << (2 + 8)));
  }
  __device__ __forceinline__ long seg(int s) const { return (long)(base | pauli_batch_local(f, (uint64_t)s << 2)); }
};
static_assert(ARTN_BORN_THREADS == 1 << 8, "SampleBatchSeg::tile: segment q * 256 + tid");

template <typename T>
__global__ __launch_bounds__(ARTN_BORN_THREADS) void artn_k_sample_batch_block_sums(const T *__restrict__ a, ArtnSampleBatchArgs g,
                                                                                    double *__restrict__ block_sum) {
  __shared__ double pseg[BORN_PSEG_DOUBLES];
  __shared__ double tot[ARTN_BORN_THREADS];
  const int bbits = g.block_bits, S4 = 1 << (bbits - 2);
  const bool whole = g.local_bits >= bbits; // (a single state below one block: its tail counts as zero, as unbatched)
  const uint64_t piece = pauli_batch_local(g.f, (uint64_t)(4 * threadIdx.x));
  const long units = (long)g.B << g.row_bits, rows = ((long)1 << g.row_bits) - 1;
  for (long u = blockIdx.x; u < units; u += gridDim.x) {
    const uint64_t b = (uint64_t)u >> g.row_bits, j = (uint64_t)(u & rows);
    const SampleBatchSeg at = {pauli_batch_traj(g.f, b) | pauli_batch_local(g.f, j << bbits), piece, g.f};
    born_block_scan_at(a, (long)g.n, whole, at, bbits, pseg, tot);
    if (threadIdx.x == 0) block_sum[u] = pseg[BORN_PIDX(S4 - 1)];
    __syncthreads(); // the next unit's scan overwrites pseg
  }
}

static __global__ __launch_bounds__(ARTN_BORN_PREFIX_THREADS) void artn_k_sample_batch_prefix_rows(const double *__restrict__ block_sum,
                                                                                            double *__restrict__ prefix, long nbt,
                                                                                            double *__restrict__ out_norm) {
  __shared__ double tot[ARTN_BORN_PREFIX_THREADS];
  const long row = (long)blockIdx.x * nbt;
  born_prefix_row(block_sum + row, prefix + row, nbt, tot);
  // (nbt is a multiple of the workgroup: the last thread owns the last entry and re-reads its own store)
  if (threadIdx.x == ARTN_BORN_PREFIX_THREADS - 1) out_norm[blockIdx.x] = prefix[row + nbt - 1];
}

static __global__ __launch_bounds__(ARTN_BORN_PREFIX_THREADS) void artn_k_sample_batch_prefix_packed(const double *__restrict__ block_sum,
                                                                                              double *__restrict__ prefix, long count,
                                                                                              int row_bits, double *__restrict__ out_norm) {
  __shared__ double row[ARTN_BORN_PREFIX_THREADS];
  const int tid = threadIdx.x, nbt = 1 << row_bits; // nbt divides the workgroup
  const long i = (long)blockIdx.x * ARTN_BORN_PREFIX_THREADS + tid;
  row[tid] = i < count ? block_sum[i] : 0.0;
  __syncthreads();
  if (i < count && (tid & (nbt - 1)) == 0) { // the first thread of a row: 0 + x0, + x1, ...
    double run = 0.0;
    for (int k = 0; k < nbt; ++k) {
      run += row[tid + k];
      row[tid + k] = run;
    }
    out_norm[i >> row_bits] = run;
  }
  __syncthreads();
  if (i < count) prefix[i] = row[tid];
}

template <typename T>
__global__ __launch_bounds__(ARTN_BORN_THREADS) void artn_k_sample_batch_pick(const T *__restrict__ a, ArtnSampleBatchArgs g,
                                                                              const double *__restrict__ prefix,
                                                                              const double *__restrict__ uniforms,
                                                                              long long *__restrict__ out_index, double *__restrict__ out_prob) {
  __shared__ double pseg[BORN_PSEG_DOUBLES];
  __shared__ double tot[ARTN_BORN_THREADS];
  const int bbits = g.block_bits, S4 = 1 << (bbits - 2);
  const bool whole = g.local_bits >= bbits;
  const uint64_t piece = pauli_batch_local(g.f, (uint64_t)(4 * threadIdx.x));
  const long units = (long)g.B << g.row_bits, nbt = (long)1 << g.row_bits, m = (long)g.S;
  for (long u = blockIdx.x; u < units; u += gridDim.x) { // (every branch below is uniform)
    const uint64_t b = (uint64_t)u >> g.row_bits, j = (uint64_t)(u & (nbt - 1));
    const double *__restrict__ pb = prefix + (long)b * nbt;
    const double total = pb[nbt - 1];
    const double hi_t = pb[j], lo_t = j ? pb[j - 1] : 0.0;
    if (!(hi_t > lo_t)) continue; // nothing in this block
    const double *__restrict__ ub = uniforms + (long)b * m;
    const auto target = [&](long s) { return sample_batch_target(ub[s], total); };
    const long s_lo = born_lower_bound_of(target, m, lo_t);
    const long s_hi = (hi_t == total) ? m : born_lower_bound_of(target, m, hi_t);
    if (s_lo >= s_hi) continue;
    const SampleBatchSeg at = {pauli_batch_traj(g.f, b) | pauli_batch_local(g.f, j << bbits), piece, g.f};
    born_block_scan_at(a, (long)g.n, whole, at, bbits, pseg, tot);
    const double ptot = pseg[BORN_PIDX(S4 - 1)];
    for (long s = s_lo + threadIdx.x; s < s_hi; s += ARTN_BORN_THREADS)
      born_pick_one(a, (long)g.n, at, 0, S4, pseg, ptot, target(s) - lo_t, out_index + (long)b * m + s, out_prob + (long)b * m + s);
    __syncthreads(); // the next unit's scan overwrites pseg
  }
}

template <typename T>
__global__ __launch_bounds__(ARTN_BORN_THREADS) void artn_k_sample_batch_small(const T *__restrict__ a, ArtnSampleBatchArgs g,
                                                                               const double *__restrict__ uniforms,
                                                                               long long *__restrict__ out_index, double *__restrict__ out_prob,
                                                                               double *__restrict__ out_norm) {
  __shared__ double pseg[BORN_PSEG_DOUBLES];
  __shared__ double tot[ARTN_BORN_THREADS];
  const int tid = threadIdx.x;
  const int M = g.local_bits;                       // 2 .. 9: a thread's four elements lie in one trajectory
  const int segs = 1 << (M - 2);                    // threads (= segments) of a trajectory
  const int lane = tid & (segs - 1), sg = tid >> (M - 2);
  const int per = ARTN_SAMPLE_BATCH_SMALL_BITS - M; // log2 trajectories of a virtual tile
  const uint64_t mine = pauli_batch_traj(g.f, (uint64_t)sg); // (loop-invariant)
  const uint64_t piece = pauli_batch_local(g.f, (uint64_t)(4 * lane)) | mine;
  const long vtiles = (long)((g.B + ((long long)1 << per) - 1) >> per), m = (long)g.S;
  for (long w = blockIdx.x; w < vtiles; w += gridDim.x) {
    const long long b = ((long long)w << per) | sg;
    const bool live = b < g.B; // (r = (b << M) | local < n)
    const uint64_t first = pauli_batch_traj(g.f, (uint64_t)w << per); // (the tile's first trajectory: uniform)
    double t[4] = {0.0, 0.0, 0.0, 0.0};
    if (live) born_seg4(a, (long)(first | piece), t);
    pseg[BORN_PIDX(tid)] = ((t[0] + t[1]) + t[2]) + t[3];
    __syncthreads();
    if (live && lane == 0) {
      double run = 0.0;
      for (int k = 0; k < segs; ++k) {
        const int i = BORN_PIDX(tid + k);
        run += pseg[i];
        pseg[i] = run;
      }
      tot[sg] = run;
      out_norm[b] = run;
    }
    __syncthreads();
    const double total = live ? tot[sg] : 0.0;
    if (total > 0.0) { // (the block has weight: lo_t = 0, hi_t = total, so every target from the first non-negative one on is its)
      const double *__restrict__ ub = uniforms + (long)b * m;
      const auto target = [&](long s) { return sample_batch_target(ub[s], total); };
      const SampleBatchSeg at = {first | mine, 0, g.f};
      for (long s = born_lower_bound_of(target, m, 0.0) + lane; s < m; s += segs)
        born_pick_one(a, (long)g.n, at, tid - lane, segs, pseg, total, target(s), out_index + (long)b * m + s, out_prob + (long)b * m + s);
    }
    __syncthreads(); // the next virtual tile overwrites pseg and tot
  }
}

#endif // ARTN_SAMPLE_BATCH_KERNEL_H
