// artn_gates_adjoint_kernel.h -- the run kernel of artn_gates_kernel.h on TWO arrays, lam and phi, with the transition element
// t_k = <lam| M_k |phi> of every flagged gate taken on the way (adjoint gradients of gate circuits: dE/dtheta_k = 2 Re t_k with
// M_k = dU_k U_k^+ on the reversed circuit of the U_k^+).
//
//   artn_k_gates_adjoint<T, R>     one launch per run: a workgroup grid-strides over blocks and holds the 2^R tiles of a block of
//                                  BOTH states; per gate: the measure (when flagged), then the gate on phi and on lam
//   artn_k_gates_adjoint_small<T>  states below 2^10 elements: one workgroup, the whole circuit in one launch
//   artn_k_gates_adjoint_finish    one workgroup per gate: partials -> out[k], ascending; 0 for the gates that are not flagged
//
// Blocks, slots, pieces, pivots and the thread-local / staged split are those of artn_k_gates; the update of each state is
// gates_slot, so each state ends bit for bit as artn_k_gates leaves it alone.  A thread holds 2 * 2^R pieces: the ranks lie one
// below the single-state ones for the same register image.
//
// The stage holds BOTH images at once, [2][2^R][Q][256] chunks, phi first: a staged gate costs the two barriers of the
// single-state kernel, and the LDS per workgroup at rank R equals the single-state kernel's at R + 1.  A gate is staged when the
// gate OR its measure needs a partner from another thread (a diagonal gate with a dense M is staged for the measure alone).
//
// The measure is a pass over the slots BEFORE the update pass and shares nothing live with it (its own coefficients, its own
// partner reads): interleaved, the compiler keeps the old lam and the float64 image of M phi alive behind the updates (the
// lesson of artn_k_pauli_adjoint).  (M phi)_i is the sum of artn_k_gates -- gates_term, d = 2^k - 1 .. 0, accumulators from
// -0.0 -- with the coefficients of M, kept in float64 and NOT rounded to T; conj(lam_i) * (M phi)_i is formed in float64 (one
// rounding per Re and Im), the four elements of a slot are added as (0 + 1) + (2 + 3), slots ascending, a butterfly over the 64
// lanes adds the wave's threads, and lane 0 of each wave keeps the sum of (gate, workgroup, wave) in the workspace: a plain load,
// add and store of a slot no other wave touches, written (not added) on the workgroup's first block.  No atomics.  The finish
// kernel adds a gate's G * 4 slots in a fixed order: t_k is bit-identical from run to run for one plan and may differ in the last
// bits between max_rank values.
#ifndef ARTN_GATES_ADJOINT_KERNEL_H
#define ARTN_GATES_ADJOINT_KERNEL_H

#include "artn_gates_kernel.h"
#include "artn_pauli_adjoint_kernel.h" /* pauli_adjoint_keep, ARTN_PAULI_ADJOINT_WAVES */

// the `measure` word of ArtnGatesAdjointGate (include/artn.h)
__device__ __forceinline__ bool gates_adjoint_flagged(const ArtnGatesAdjointGate &g) { return (g.measure & 1) != 0; }
__device__ __forceinline__ int gates_adjoint_nd(const ArtnGatesAdjointGate &g) { return (g.measure & 2) ? 1 : 1 << (int)g.g.k; }

// (tr, ti) += sum over the four elements of slot s of conj(lam) * (M phi): M phi in float64 as gates_slot forms it, not rounded
template <typename T, bool LANE, typename C, typename S>
__device__ __forceinline__ void gates_adjoint_measure(const double (&mm)[4][4][2], const GatesForm &f, const C *stage_phi, int s, int tid,
                                                      const double (&cf)[2][4][2], const S (&pr)[4], const S (&pi)[4], const S (&lr)[4],
                                                      const S (&li)[4], double &tr, double &ti) {
  const int ru_slot = ((s & f.m0) ? 1 : 0) | ((s & f.m1) ? 2 : 0); // (uniform)
  double re[4] = {-0.0, -0.0, -0.0, -0.0}, im[4] = {-0.0, -0.0, -0.0, -0.0};
  gates_partner<T, LANE, 3>(mm, f, stage_phi, s, tid, ru_slot, cf, pr, pi, re, im);
  gates_partner<T, LANE, 2>(mm, f, stage_phi, s, tid, ru_slot, cf, pr, pi, re, im);
  gates_partner<T, LANE, 1>(mm, f, stage_phi, s, tid, ru_slot, cf, pr, pi, re, im);
  gates_add<S, LANE, 0>(mm, f, ru_slot, cf, pr, pi, re, im);
  double qr[4], qi[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const double ar = (double)lr[e], ai = (double)li[e];
    qr[e] = fma(ar, re[e], ai * im[e]);    // Re conj(a) b
    qi[e] = fma(ar, im[e], -(ai * re[e])); // Im conj(a) b
  }
  tr += (qr[0] + qr[1]) + (qr[2] + qr[3]);
  ti += (qi[0] + qi[1]) + (qi[2] + qi[3]);
}

// ws: [n_gates][ws_groups][ARTN_PAULI_ADJOINT_WAVES][2] float64
template <typename T, int R>
__global__ __launch_bounds__(ARTN_BORN_THREADS) void artn_k_gates_adjoint(T *lam, T *phi, long n_blocks, const ArtnGatesRun *__restrict__ run,
                                                                          const ArtnGatesAdjointGate *__restrict__ gates, double *ws,
                                                                          long ws_groups) {
  using S = decltype(T::x);
  using C = typename PauliChunk<T>::type;
  constexpr int Q = (int)sizeof(T) / 4; // 16-byte chunks of a piece
  constexpr int NS = 1 << R;            // slots of a block
  C *stage_phi = (C *)artn_gates_lds;                    // [NS][Q][256]
  C *stage_lam = stage_phi + NS * Q * ARTN_BORN_THREADS; // [NS][Q][256]
  const int tid = threadIdx.x;
  if ((int)run->rank != R) return; // (uniform; a table packed for another max_rank: the launch does nothing)
  const ArtnGatesAdjointGate *gp = gates + run->first;
  const int n_gates = (int)run->count;
  double *slot0 = ws + ((long)run->first * ws_groups + blockIdx.x) * (2 * ARTN_PAULI_ADJOINT_WAVES) + 2 * (tid >> 6);
  const long slot_stride = ws_groups * (2 * ARTN_PAULI_ADJOINT_WAVES);
  uint64_t span[NS]; // the pivots of the bits of s, as TILE-index masks
  span[0] = 0;
#pragma unroll
  for (int j = 0; j < R; ++j) {
    const uint64_t b = (uint64_t)1 << ((int)run->pivot[j] - ARTN_PAULI_TILE_BITS);
#pragma unroll
    for (int s = 0; s < (1 << j); ++s) span[s | (1 << j)] = span[s] ^ b;
  }
  for (long q = blockIdx.x; q < n_blocks; q += gridDim.x) {
    const bool first = q == (long)blockIdx.x;
    const uint64_t rep = block_rep<R>(run, q);
    S pr[NS][4], pi[NS][4], lr[NS][4], li[NS][4];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const long at = (long)((rep ^ span[s]) << ARTN_PAULI_TILE_BITS) + 4 * tid;
      pauli_unpack4(pauli_piece_ld((const C *)(phi + at), 1), pr[s], pi[s]);
      pauli_unpack4(pauli_piece_ld((const C *)(lam + at), 1), lr[s], li[s]);
    }
    for (int k = 0; k < n_gates; ++k) {
      const ArtnGatesAdjointGate &rec = gp[k];
      const ArtnGatesGate &g = rec.g;
      const GatesForm f = gates_form(g);
      const bool flagged = gates_adjoint_flagged(rec); // (uniform)
      const int nd_m = gates_adjoint_nd(rec);
      const bool moves = (f.m0 | f.m1 | f.p0 | f.p1) != 0;                // (uniform)
      const bool staged = moves && (f.nd > 1 || (flagged && nd_m > 1)); // (uniform)
      const bool lane = (f.p0 | f.p1) != 0;                              // (uniform)
      if (staged) {
        __syncthreads(); // every thread has read the previous images
#pragma unroll
        for (int s = 0; s < NS; ++s) {
          pauli_piece_st(&stage_phi[s * Q * ARTN_BORN_THREADS + tid], ARTN_BORN_THREADS, pauli_pack4(pr[s], pi[s]));
          pauli_piece_st(&stage_lam[s * Q * ARTN_BORN_THREADS + tid], ARTN_BORN_THREADS, pauli_pack4(lr[s], li[s]));
        }
        __syncthreads();
      }
      // The measure: a pass of its own BEFORE the updates, on the images as they stand (see the head of this file).
      if (flagged) {
        GatesForm fm = f;
        fm.nd = nd_m;
        double tr = 0.0, ti = 0.0;
        double cm[2][4][2];
        if (lane) {
          gates_rows(rec.mm, fm, tid, cm);
#pragma unroll
          for (int s = 0; s < NS; ++s) gates_adjoint_measure<T, true>(rec.mm, fm, stage_phi, s, tid, cm, pr[s], pi[s], lr[s], li[s], tr, ti);
        } else {
#pragma unroll
          for (int s = 0; s < NS; ++s) gates_adjoint_measure<T, false>(rec.mm, fm, stage_phi, s, tid, cm, pr[s], pi[s], lr[s], li[s], tr, ti);
        }
        pauli_adjoint_keep(slot0 + k * slot_stride, first, tr, ti);
      }
      double cf[2][4][2];
      if (lane) {
        gates_rows(g.m, f, tid, cf);
#pragma unroll
        for (int s = 0; s < NS; ++s) {
          gates_slot<T, true>(g, f, stage_phi, s, tid, cf, pr[s], pi[s]);
          gates_slot<T, true>(g, f, stage_lam, s, tid, cf, lr[s], li[s]);
        }
      } else {
#pragma unroll
        for (int s = 0; s < NS; ++s) {
          gates_slot<T, false>(g, f, stage_phi, s, tid, cf, pr[s], pi[s]);
          gates_slot<T, false>(g, f, stage_lam, s, tid, cf, lr[s], li[s]);
        }
      }
    }
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const long at = (long)((rep ^ span[s]) << ARTN_PAULI_TILE_BITS) + 4 * tid;
      pauli_piece_st((C *)(phi + at), 1, pauli_pack4(pr[s], pi[s]));
      pauli_piece_st((C *)(lam + at), 1, pauli_pack4(lr[s], li[s]));
    }
  }
}

// States below one tile: both states live in LDS as T; thread t owns elements t, t + 256 ... < n (at most two) of each.  lo[] holds
// the whole flip mask of a target here (every bit lies below the tile).  Every gate is staged: correct, not fast.
template <typename T>
__global__ __launch_bounds__(ARTN_BORN_THREADS) void artn_k_gates_adjoint_small(T *lam, T *phi, long n,
                                                                                const ArtnGatesAdjointGate *__restrict__ gp, int n_gates,
                                                                                double *ws) {
  using S = decltype(T::x);
  constexpr int PER = (1 << ARTN_PAULI_TILE_BITS) / 2 / ARTN_BORN_THREADS; // n <= 2^9
  __shared__ T img_phi[(1 << ARTN_PAULI_TILE_BITS) / 2], img_lam[(1 << ARTN_PAULI_TILE_BITS) / 2];
  const int tid = threadIdx.x;
  S pr[PER], pi[PER], lr[PER], li[PER];
#pragma unroll
  for (int u = 0; u < PER; ++u) {
    const long i = tid + u * ARTN_BORN_THREADS;
    pr[u] = pi[u] = lr[u] = li[u] = (S)0;
    if (i < n) pr[u] = phi[i].x, pi[u] = phi[i].y, lr[u] = lam[i].x, li[u] = lam[i].y;
  }
  for (int k = 0; k < n_gates; ++k) {
    const ArtnGatesAdjointGate &rec = gp[k];
    const ArtnGatesGate &g = rec.g;
    const int nd = (g.flags & ARTN_GATE_DIAGONAL) ? 1 : 1 << (int)g.k;
    const int nd_m = gates_adjoint_nd(rec);
    const bool flagged = gates_adjoint_flagged(rec);
    const long f0 = (long)g.lo[0], f1 = (long)g.lo[1];
    __syncthreads();
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const long i = tid + u * ARTN_BORN_THREADS;
      T v, w;
      v.x = pr[u], v.y = pi[u], w.x = lr[u], w.y = li[u];
      if (i < n) img_phi[i] = v, img_lam[i] = w;
    }
    __syncthreads();
    if (flagged) { // (uniform)
      double tr = 0.0, ti = 0.0;
#pragma unroll
      for (int u = 0; u < PER; ++u) {
        const long i = tid + u * ARTN_BORN_THREADS;
        if (i >= n) continue;
        const int r = ((i & f0) ? 1 : 0) | ((i & f1) ? 2 : 0);
        double re = -0.0, im = -0.0;
#pragma unroll
        for (int d = 3; d >= 0; --d) {
          if (d >= nd_m) continue;
          const T b = img_phi[i ^ ((d & 1) ? f0 : 0) ^ ((d & 2) ? f1 : 0)]; // (below n: the flips are bits of the index)
          gates_term(rec.mm[r][r ^ d][0], rec.mm[r][r ^ d][1], b.x, b.y, re, im);
        }
        const double ar = (double)lr[u], ai = (double)li[u];
        tr += fma(ar, re, ai * im);
        ti += fma(ar, im, -(ai * re));
      }
      pauli_adjoint_keep(ws + (long)k * (2 * ARTN_PAULI_ADJOINT_WAVES) + 2 * (tid >> 6), true, tr, ti);
    }
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const long i = tid + u * ARTN_BORN_THREADS;
      if (i >= n) continue;
      const int r = ((i & f0) ? 1 : 0) | ((i & f1) ? 2 : 0);
      double re = -0.0, im = -0.0, se = -0.0, sm = -0.0;
#pragma unroll
      for (int d = 3; d >= 0; --d) {
        if (d >= nd) continue;
        const double cr = g.m[r][r ^ d][0], ci = g.m[r][r ^ d][1];
        if (d == 0) {
          gates_term(cr, ci, pr[u], pi[u], re, im);
          gates_term(cr, ci, lr[u], li[u], se, sm);
        } else {
          const long j = i ^ ((d & 1) ? f0 : 0) ^ ((d & 2) ? f1 : 0);
          const T b = img_phi[j], c = img_lam[j];
          gates_term(cr, ci, b.x, b.y, re, im);
          gates_term(cr, ci, c.x, c.y, se, sm);
        }
      }
      pr[u] = (S)re, pi[u] = (S)im, lr[u] = (S)se, li[u] = (S)sm;
    }
  }
#pragma unroll
  for (int u = 0; u < PER; ++u) {
    const long i = tid + u * ARTN_BORN_THREADS;
    T v, w;
    v.x = pr[u], v.y = pi[u], w.x = lr[u], w.y = li[u];
    if (i < n) phi[i] = v, lam[i] = w;
  }
}

// Workgroup k: out[k] = the gate's slots added: thread t takes slots t, t + 256 ... ascending, then the workgroup tree.  The slots
// of a gate: min(tiles >> rank of its run, grid limit) workgroups x ARTN_PAULI_ADJOINT_WAVES; the rank is in the gate record.
static __global__ __launch_bounds__(ARTN_BORN_THREADS) void artn_k_gates_adjoint_finish(const double *__restrict__ ws, long ws_groups,
                                                                                        long tiles,
                                                                                        const ArtnGatesAdjointGate *__restrict__ gates,
                                                                                        double *__restrict__ out) {
  __shared__ double red[ARTN_BORN_THREADS][2];
  const long k = blockIdx.x;
  const uint64_t word = gates[k].measure;
  if (!(word & 1)) { // (uniform)
    if (threadIdx.x < 2) out[2 * k + threadIdx.x] = 0.0;
    return;
  }
  long groups = tiles >> (int)((word >> 8) & 0xff);
  if (groups > ARTN_GATES_MAX_GRID) groups = ARTN_GATES_MAX_GRID;
  if (groups < 1) groups = 1;
  const double2 *src = (const double2 *)(ws + k * ws_groups * (2 * ARTN_PAULI_ADJOINT_WAVES));
  double acc[2] = {0.0, 0.0};
  for (long g = threadIdx.x; g < groups * ARTN_PAULI_ADJOINT_WAVES; g += ARTN_BORN_THREADS) {
    const double2 v = src[g];
    acc[0] += v.x, acc[1] += v.y;
  }
  born_wg_tree<2>(red, acc);
  if (threadIdx.x == 0) out[2 * k] = red[0][0], out[2 * k + 1] = red[0][1];
}

#endif // ARTN_GATES_ADJOINT_KERNEL_H
