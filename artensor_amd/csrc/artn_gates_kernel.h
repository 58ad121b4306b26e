// artn_gates_kernel.h -- circuits of dense one- and two-qubit gates, in place, on an amplitude array on gfx950.
//
// A gate on the memory bits T_0 (row bit 0: the LAST listed target) and T_1 (row bit 1; absent for one qubit) mixes element i with
// the up to three elements that differ from it in those bits:
//     new a[i] = sum_{d = 2^k - 1 .. 0} U[r][r ^ d] a[i ^ flip(d)],   r = the target bits of i,  flip(d) = T_0 if d & 1, T_1 if d & 2.
// The host (artn_gates.hip) cuts the circuit into RUNS whose distinct HIGH target bits (>= 10) number R; they are the pivots of
// the block structure of artn_pauli_evolve_kernel.h with unit basis vectors, and
//
//   artn_k_gates<T, R>     one launch per run: a workgroup grid-strides over blocks of 2^R tiles, holds a block, applies every
//                          gate of the run to it and writes it back -- one read and one write of the state per run
//   artn_k_gates_small<T>  states below 2^10 elements: one workgroup, the whole circuit in one launch
//
// A block is that of artn_block_kernel.h: thread t owns elements 4t .. 4t+3 (its PIECE) of every slot and keeps them in registers
// as T for the whole run.  A target is a SLOT bit (high: one bit m of the slot index), a PIECE bit (memory bits 2-9: one bit p of
// t) or a REGISTER bit (memory bits 0-1: one bit e of the element number); the partner of (slot s, piece t, element e) under d is
// (s ^ M(d), t ^ P(d), e ^ E(d)), each the XOR of the masks of the targets d flips.
//
// Who updates what.  Every thread computes its OWN elements and writes nothing else:
//   thread-local gates  diagonal matrices (only d = 0 has a coefficient) and gates whose targets are register bits: no LDS, no barrier;
//   staged gates        everything else: barrier, every thread stores its pieces of all slots to LDS, barrier, every thread reads
//                       the up to three partner pieces of each slot (slot s ^ M(d): an address, never an indexed register;
//                       a d that only flips register bits takes the thread's own piece) and updates its registers.
// The stage keeps the plane layout of artn_k_pauli_apply per slot, Q = sizeof(T) / 4 planes of 256 x 16 bytes.  A partner read is
// a ds_read_b128 of a plane at piece t ^ P(d): P(d) is one mask for the whole workgroup, so the 16 lanes of a lane group still
// touch the 16 distinct 16-byte slots of an aligned group -- the no-bank-conflict argument of artn_k_pauli_apply holds for all
// three partner reads unchanged.  Blocks are disjoint, so no two workgroups touch the same element; stream order separates runs.
//
// Coefficients.  The row r of an element has a part that is uniform over the workgroup (slot and register targets: s and e are
// unrolled constants) and a part that varies with the thread (piece targets).  Without a piece target r is uniform, the
// coefficient U[r][r ^ d] is a scalar load and the test for an exactly zero component a scalar branch.  With one, every thread
// loads the rows of its own piece bits once per gate -- U[r][r ^ d] for both values h of the remaining uniform row bit -- and a
// select on h picks the row inside the unrolled loops; the zero test is then per lane.
//
// Arithmetic.  gates_term is the ONE function that adds a term, for every kernel form and every R: operands to float64, the two
// products with Im U, then the two with Re U, by fma, products of an exactly zero coefficient component left out; the accumulators
// start at -0.0; terms come in the order d = 2^k - 1 .. 0; one rounding per component to T.  Between gates the block is held as T.
// So the result does not depend on where the runs are cut, bit for bit.
#ifndef ARTN_GATES_KERNEL_H
#define ARTN_GATES_KERNEL_H

#include "artn.h"
#include "artn_pauli_evolve_kernel.h"

#define ARTN_GATES_MAX_GRID ARTN_PAULI_EVOLVE_MAX_GRID /* workgroups; each takes blocks g, g + G ... */

// (re, im) += (cr + i ci) * (yr + i yi)
template <typename S>
__device__ __forceinline__ void gates_term(double cr, double ci, S yr, S yi, double &re, double &im) {
  const double br = (double)yr, bi = (double)yi;
  if (ci != 0.0) re = fma(-ci, bi, re), im = fma(ci, br, im);
  if (cr != 0.0) re = fma(cr, br, re), im = fma(cr, bi, im);
}

// a gate's masks (uniform): nd terms; per target the slot bit m, the piece bit p and the register bit e; hbit: the row bits
// that are not piece bits
struct GatesForm {
  int nd, m0, m1, p0, p1, e0, e1, hbit;
};

// The masks of a gate record, and below the thread's rows of a matrix: what artn_k_gates_adjoint calls.  artn_k_gates has both
// written out in its body: as calls they change the instructions of every one of its instantiations.
__device__ __forceinline__ GatesForm gates_form(const ArtnGatesGate &g) {
  GatesForm f;
  f.nd = (g.flags & ARTN_GATE_DIAGONAL) ? 1 : 1 << (int)g.k;
  f.m0 = (int)g.slot[0], f.m1 = (int)g.slot[1];
  f.p0 = (int)g.lo[0] >> 2, f.p1 = (int)g.lo[1] >> 2, f.e0 = (int)g.lo[0] & 3, f.e1 = (int)g.lo[1] & 3;
  f.hbit = ((int)g.k == 2 ? 3 : 1) & ~((f.p0 ? 1 : 0) | (f.p1 ? 2 : 0));
  return f;
}

// piece targets: the thread's part of the row, and its rows of the matrix `m` for both values of the row bit that may be left
__device__ __forceinline__ void gates_rows(const double (&m)[4][4][2], const GatesForm &f, int tid, double (&cf)[2][4][2]) {
  const int rl = ((tid & f.p0) ? 1 : 0) | ((tid & f.p1) ? 2 : 0);
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int r = rl | (h ? f.hbit : 0);
#pragma unroll
    for (int d = 0; d < 4; ++d) cf[h][d][0] = m[r][r ^ d][0], cf[h][d][1] = m[r][r ^ d][1];
  }
}

// Term D of the four elements of one slot: (re, im)[e] += U[r][r ^ D] * (yr, yi)[e], r = ru_slot + the register bits of e + the
// thread's piece bits; U is `m`, the gate's matrix or, in the adjoint kernel, the measure's.  LANE: cf[h][D] holds the thread's
// U[r][r ^ D] for the uniform row part 0 (h = 0) and hbit (h = 1).
template <typename S, bool LANE, int D>
__device__ __forceinline__ void gates_add(const double (&m)[4][4][2], const GatesForm &f, int ru_slot, const double (&cf)[2][4][2],
                                          const S (&yr)[4], const S (&yi)[4], double (&re)[4], double (&im)[4]) {
  if (D >= f.nd) return; // (uniform)
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int ru = ru_slot | ((e & f.e0) ? 1 : 0) | ((e & f.e1) ? 2 : 0); // (uniform)
    double cr, ci;
    if constexpr (LANE) {
      const bool h = (ru & f.hbit) != 0;
      cr = h ? cf[1][D][0] : cf[0][D][0], ci = h ? cf[1][D][1] : cf[0][D][1];
    } else {
      cr = m[ru][ru ^ D][0], ci = m[ru][ru ^ D][1];
    }
    gates_term(cr, ci, yr[e], yi[e], re[e], im[e]);
  }
}

// Term D >= 1 of one slot: the partner piece from the stage (or the own piece when D only flips register bits), its elements
// brought into the order of the own piece, then gates_add.
template <typename T, bool LANE, int D, typename C, typename S>
__device__ __forceinline__ void gates_partner(const double (&m)[4][4][2], const GatesForm &f, const C *stage, int s, int tid, int ru_slot,
                                              const double (&cf)[2][4][2], const S (&xr)[4], const S (&xi)[4], double (&re)[4],
                                              double (&im)[4]) {
  constexpr int Q = (int)sizeof(T) / 4;
  if (D >= f.nd) return; // (uniform)
  const int M = ((D & 1) ? f.m0 : 0) ^ ((D & 2) ? f.m1 : 0), P = ((D & 1) ? f.p0 : 0) ^ ((D & 2) ? f.p1 : 0);
  const int E = ((D & 1) ? f.e0 : 0) ^ ((D & 2) ? f.e1 : 0);
  S yr[4], yi[4];
  if (M | P) {
    pauli_unpack4(pauli_piece_ld(&stage[(s ^ M) * Q * ARTN_BORN_THREADS + (tid ^ P)], ARTN_BORN_THREADS), yr, yi);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) yr[e] = xr[e], yi[e] = xi[e];
  }
  block_swap4(E, yr, yi);
  gates_add<S, LANE, D>(m, f, ru_slot, cf, yr, yi, re, im);
}

// One slot of a block under one gate: the terms d = 3 .. 1 from the partners, d = 0 from the own elements, one rounding.
template <typename T, bool LANE, typename C, typename S>
__device__ __forceinline__ void gates_slot(const ArtnGatesGate &g, const GatesForm &f, const C *stage, int s, int tid,
                                           const double (&cf)[2][4][2], S (&xr)[4], S (&xi)[4]) {
  const int ru_slot = ((s & f.m0) ? 1 : 0) | ((s & f.m1) ? 2 : 0); // (uniform)
  double re[4] = {-0.0, -0.0, -0.0, -0.0}, im[4] = {-0.0, -0.0, -0.0, -0.0};
  gates_partner<T, LANE, 3>(g.m, f, stage, s, tid, ru_slot, cf, xr, xi, re, im);
  gates_partner<T, LANE, 2>(g.m, f, stage, s, tid, ru_slot, cf, xr, xi, re, im);
  gates_partner<T, LANE, 1>(g.m, f, stage, s, tid, ru_slot, cf, xr, xi, re, im);
  gates_add<S, LANE, 0>(g.m, f, ru_slot, cf, xr, xi, re, im);
#pragma unroll
  for (int e = 0; e < 4; ++e) xr[e] = (S)re[e], xi[e] = (S)im[e];
}

extern __shared__ __attribute__((aligned(16))) unsigned char artn_gates_lds[];

template <typename T, int R>
__global__ __launch_bounds__(ARTN_BORN_THREADS) void artn_k_gates(T *a, long n_blocks, const ArtnGatesRun *__restrict__ run,
                                                                  const ArtnGatesGate *__restrict__ gates) {
  using S = decltype(T::x);
  using C = typename PauliChunk<T>::type;
  constexpr int Q = (int)sizeof(T) / 4; // 16-byte chunks of a piece
  constexpr int NS = 1 << R;            // slots of a block
  C *stage = (C *)artn_gates_lds;       // [NS][Q][256]
  const int tid = threadIdx.x;
  if ((int)run->rank != R) return; // (uniform; a table packed for another max_rank: the launch does nothing)
  const ArtnGatesGate *gp = gates + run->first;
  const int n_gates = (int)run->count;
  uint64_t span[NS]; // the pivots of the bits of s, as TILE-index masks
  span[0] = 0;
#pragma unroll
  for (int j = 0; j < R; ++j) {
    const uint64_t b = (uint64_t)1 << ((int)run->pivot[j] - ARTN_PAULI_TILE_BITS);
#pragma unroll
    for (int s = 0; s < (1 << j); ++s) span[s | (1 << j)] = span[s] ^ b;
  }
  for (long q = blockIdx.x; q < n_blocks; q += gridDim.x) {
    const uint64_t rep = block_rep<R>(run, q);
    S xr[NS][4], xi[NS][4];
#pragma unroll
    for (int s = 0; s < NS; ++s)
      pauli_unpack4(pauli_piece_ld((const C *)(a + (long)((rep ^ span[s]) << ARTN_PAULI_TILE_BITS) + 4 * tid), 1), xr[s], xi[s]);
    for (int k = 0; k < n_gates; ++k) {
      const ArtnGatesGate &g = gp[k];
      GatesForm f;
      f.nd = (g.flags & ARTN_GATE_DIAGONAL) ? 1 : 1 << (int)g.k;
      f.m0 = (int)g.slot[0], f.m1 = (int)g.slot[1];
      f.p0 = (int)g.lo[0] >> 2, f.p1 = (int)g.lo[1] >> 2, f.e0 = (int)g.lo[0] & 3, f.e1 = (int)g.lo[1] & 3;
      f.hbit = ((int)g.k == 2 ? 3 : 1) & ~((f.p0 ? 1 : 0) | (f.p1 ? 2 : 0));
      const bool staged = f.nd > 1 && (f.m0 | f.m1 | f.p0 | f.p1) != 0; // (uniform)
      const bool lane = (f.p0 | f.p1) != 0;                             // (uniform)
      if (staged) {
        __syncthreads(); // every thread has read the previous image
#pragma unroll
        for (int s = 0; s < NS; ++s) pauli_piece_st(&stage[s * Q * ARTN_BORN_THREADS + tid], ARTN_BORN_THREADS, pauli_pack4(xr[s], xi[s]));
        __syncthreads();
      }
      double cf[2][4][2];
      if (lane) {
        // piece targets: the thread's part of the row, and its coefficients for both values of the row bit that may be left
        const int rl = ((tid & f.p0) ? 1 : 0) | ((tid & f.p1) ? 2 : 0);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int r = rl | (h ? f.hbit : 0);
#pragma unroll
          for (int d = 0; d < 4; ++d) cf[h][d][0] = g.m[r][r ^ d][0], cf[h][d][1] = g.m[r][r ^ d][1];
        }
#pragma unroll
        for (int s = 0; s < NS; ++s) gates_slot<T, true>(g, f, stage, s, tid, cf, xr[s], xi[s]);
      } else {
#pragma unroll
        for (int s = 0; s < NS; ++s) gates_slot<T, false>(g, f, stage, s, tid, cf, xr[s], xi[s]);
      }
    }
#pragma unroll
    for (int s = 0; s < NS; ++s)
      pauli_piece_st((C *)(a + (long)((rep ^ span[s]) << ARTN_PAULI_TILE_BITS) + 4 * tid), 1, pauli_pack4(xr[s], xi[s]));
  }
}

// States below one tile: the state lives in LDS as T; thread t owns elements t, t + 256 ... < n (at most two).  lo[] holds the
// whole flip mask of a target here (every bit lies below the tile).
template <typename T>
__global__ __launch_bounds__(ARTN_BORN_THREADS) void artn_k_gates_small(T *a, long n, const ArtnGatesGate *__restrict__ gp, int n_gates) {
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
  for (int k = 0; k < n_gates; ++k) {
    const ArtnGatesGate &g = gp[k];
    const int nd = (g.flags & ARTN_GATE_DIAGONAL) ? 1 : 1 << (int)g.k;
    const long f0 = (long)g.lo[0], f1 = (long)g.lo[1];
    if (nd > 1) { // (uniform)
      __syncthreads();
      block_small_st(img, n, tid, xr, xi);
      __syncthreads();
    }
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const long i = tid + u * ARTN_BORN_THREADS;
      if (i >= n) continue;
      const int r = ((i & f0) ? 1 : 0) | ((i & f1) ? 2 : 0);
      double re = -0.0, im = -0.0;
#pragma unroll
      for (int d = 3; d >= 0; --d) {
        if (d >= nd) continue;
        const double cr = g.m[r][r ^ d][0], ci = g.m[r][r ^ d][1];
        if (d == 0) {
          gates_term(cr, ci, xr[u], xi[u], re, im);
        } else {
          const T b = img[i ^ ((d & 1) ? f0 : 0) ^ ((d & 2) ? f1 : 0)]; // (below n: the flips are bits of the index)
          gates_term(cr, ci, b.x, b.y, re, im);
        }
      }
      xr[u] = (S)re, xi[u] = (S)im;
    }
  }
  block_small_st(a, n, tid, xr, xi);
}

#endif // ARTN_GATES_KERNEL_H
