// artn_pauli_adjoint_kernel.h -- the run kernel of artn_pauli_evolve_kernel.h on TWO arrays, lam and phi, with the transition
// element t_k = <lam| P_k |phi> of every flagged step taken on the way (adjoint gradients: dE/dtheta_k = 2 Im t_k).
//
//   artn_k_pauli_adjoint<T, R>     one launch per run: a workgroup grid-strides over blocks and holds the 2^R tiles of a block of
//                                  BOTH states; per step: the measure (when flagged), then the step on phi and on lam
//   artn_k_pauli_adjoint_small<T>  states below 2^10 elements: one workgroup, the whole circuit in one launch
//   artn_k_pauli_adjoint_finish    one workgroup per step: partials -> out[k], ascending; 0 for the steps that are not flagged
//
// Blocks, slots, pieces, the register/staged split and the sign of (P a)[i] are those of artn_k_pauli_evolve; the step arithmetic is
// pauli_evolve_pair, so each state ends bit for bit as artn_k_pauli_evolve leaves it alone.  A thread holds 2 * 2^R pieces: the
// ranks lie one below the single-state ones for the same register image.
//
// The stage holds BOTH images at once, [2][2^R][Q][256] chunks, phi first: a staged step costs the two barriers of the single-state
// kernel, not four, and the LDS per workgroup at rank R equals the single-state kernel's at R + 1 (64 KiB at the default rank,
// 128 KiB at the maximum).  Plane layout and the conflict-free ds_read_b128 at piece t ^ mask are unchanged.
//
// The measure is a pass over the slots before the update pass of the step (the update reads the partner piece of phi from
// LDS a second time; see the kernel for why).  The partner piece of phi with its sign is b_i / (-i)^ny; every thread adds
// conj(lam[i]) * that over its elements (operands to float64, one rounding per Re and Im of a term, slots ascending), a
// butterfly over the 64 lanes adds the wave's threads, and lane 0 of each wave keeps the wave's sum of (step, workgroup, wave) in
// the workspace: a plain load, add and store of a slot no other wave touches, written (not added) on the workgroup's first block.
// No LDS, no workgroup barrier, no atomics: a register step stays barrier-free when it is measured.  The finish kernel adds a
// step's G * 4 slots in a fixed order and multiplies by (-i)^ny (exact).  The order follows the blocks, so t_k is bit-identical
// from run to run for one plan and may differ in the last bits between max_rank values.
#ifndef ARTN_PAULI_ADJOINT_KERNEL_H
#define ARTN_PAULI_ADJOINT_KERNEL_H

#include "artn_pauli_evolve_kernel.h"

#define ARTN_PAULI_ADJOINT_WAVES (ARTN_BORN_THREADS / 64) /* workspace slots of a workgroup and step */

// bits of ArtnPauliEvolveStep::n_y in a table of artn_pauli_adjoint_pack (include/artn.h)
__device__ __forceinline__ bool pauli_adjoint_flagged(const ArtnPauliEvolveStep &st) { return ((st.n_y >> 8) & 1) != 0; }

// sum over the wave, the same value in every lane (a fixed butterfly)
__device__ __forceinline__ double pauli_adjoint_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// (tr, ti) += conj(own) * partner over the four elements of a slot; the partner piece in ELEMENT order, sign still to apply.
// The four terms are formed independently (one rounding per Re and Im, as artn_k_pauli) and added as (0 + 1) + (2 + 3): a chain
// of fma through every element of every slot would be the longest dependence of the step.
template <typename S>
__device__ __forceinline__ void pauli_adjoint_measure(uint32_t sg, const uint32_t pe[4], const S xr[4], const S xi[4], const S yr[4],
                                                      const S yi[4], double &tr, double &ti) {
  double qr[4], qi[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const uint32_t s = sg ^ pe[e];
    const double ar = (double)xr[e], ai = (double)xi[e];
    const double br = (double)pauli_evolve_flip(yr[e], s), bi = (double)pauli_evolve_flip(yi[e], s);
    qr[e] = fma(ar, br, ai * bi);    // Re conj(a) b
    qi[e] = fma(ar, bi, -(ai * br)); // Im conj(a) b
  }
  tr += (qr[0] + qr[1]) + (qr[2] + qr[3]);
  ti += (qi[0] + qi[1]) + (qi[2] + qi[3]);
}

// the wave's sum of a step into its workspace slot (lane 0; `first`: the workgroup's first block of the launch)
__device__ __forceinline__ void pauli_adjoint_keep(double *slot, bool first, double tr, double ti) {
  tr = pauli_adjoint_wave_sum(tr), ti = pauli_adjoint_wave_sum(ti);
  if ((threadIdx.x & 63) == 0) {
    double2 v = make_double2(tr, ti);
    if (!first) {
      const double2 old = *(const double2 *)slot;
      v.x += old.x, v.y += old.y;
    }
    *(double2 *)slot = v;
  }
}

// ws: [n_steps][ws_groups][ARTN_PAULI_ADJOINT_WAVES][2] float64
template <typename T, int R>
__global__ __launch_bounds__(ARTN_BORN_THREADS) void artn_k_pauli_adjoint(T *lam, T *phi, long n_blocks,
                                                                          const ArtnPauliEvolveRun *__restrict__ run,
                                                                          const ArtnPauliEvolveStep *__restrict__ steps, double *ws,
                                                                          long ws_groups) {
  using S = decltype(T::x);
  using C = typename PauliChunk<T>::type;
  constexpr int Q = (int)sizeof(T) / 4; // 16-byte chunks of a piece
  constexpr int NS = 1 << R;            // slots of a block
  C *stage_phi = (C *)artn_pauli_evolve_lds;                // [NS][Q][256]
  C *stage_lam = stage_phi + NS * Q * ARTN_BORN_THREADS;    // [NS][Q][256]
  const int tid = threadIdx.x;
  if ((int)run->rank != R) return; // (uniform; a table packed for another max_rank: the launch does nothing)
  const ArtnPauliEvolveStep *stp = steps + run->first;
  const int n_steps = (int)run->count;
  double *slot0 = ws + ((long)run->first * ws_groups + blockIdx.x) * (2 * ARTN_PAULI_ADJOINT_WAVES) + 2 * (tid >> 6);
  const long slot_stride = ws_groups * (2 * ARTN_PAULI_ADJOINT_WAVES);
  uint64_t span[NS]; // XOR of the basis over the bits of s, as TILE-index masks
  span[0] = 0;
#pragma unroll
  for (int j = 0; j < R; ++j) {
    const uint64_t b = run->basis[j] >> ARTN_PAULI_TILE_BITS;
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
    for (int k = 0; k < n_steps; ++k) {
      const PauliEvolveCoef c = pauli_evolve_coef(stp[k]);
      const uint64_t zm = stp[k].zmask;
      const int xm_lo = (int)stp[k].xm_lo, m = (int)stp[k].slot_mask, r = xm_lo & 3, pmask = xm_lo >> 2;
      const uint32_t pt = (uint32_t)(__popcll((uint64_t)(4 * tid) & zm) & 1) << 31;
      const uint32_t z0 = (uint32_t)(zm & 1) << 31, z1 = (uint32_t)((zm >> 1) & 1) << 31;
      const uint32_t pe[4] = {0u, z0, z1, z0 ^ z1};
      const bool staged = m != 0 || pmask != 0;        // (uniform)
      const bool flagged = pauli_adjoint_flagged(stp[k]); // (uniform)
      if (staged) {
        __syncthreads(); // every thread has read the previous images
#pragma unroll
        for (int s = 0; s < NS; ++s) {
          pauli_piece_st(&stage_phi[s * Q * ARTN_BORN_THREADS + tid], ARTN_BORN_THREADS, pauli_pack4(pr[s], pi[s]));
          pauli_piece_st(&stage_lam[s * Q * ARTN_BORN_THREADS + tid], ARTN_BORN_THREADS, pauli_pack4(lr[s], li[s]));
        }
        __syncthreads();
      }
      // The measure is a pass of its own BEFORE the updates, on the images as they stand: the partner piece of phi is read a
      // second time by the update pass below.  Measuring inside the update loop costs some 120 registers at R = 2: the compiler
      // merges the flagged blocks of all slots behind the updates and keeps the old lam and the signed partners alive for them.
      if (flagged) {
        double tr = 0.0, ti = 0.0;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
          const uint32_t sg = pt ^ ((uint32_t)(__popcll(((rep ^ span[s]) << ARTN_PAULI_TILE_BITS) & zm) & 1) << 31);
          S yr[4], yi[4];
          if (staged) {
            pauli_unpack4(pauli_piece_ld(&stage_phi[(s ^ m) * Q * ARTN_BORN_THREADS + (tid ^ pmask)], ARTN_BORN_THREADS), yr, yi);
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) yr[e] = pr[s][e], yi[e] = pi[s][e];
          }
          if (r & 1) pauli_swap(yr[0], yr[1]), pauli_swap(yi[0], yi[1]), pauli_swap(yr[2], yr[3]), pauli_swap(yi[2], yi[3]);
          if (r & 2) pauli_swap(yr[0], yr[2]), pauli_swap(yi[0], yi[2]), pauli_swap(yr[1], yr[3]), pauli_swap(yi[1], yi[3]);
          pauli_adjoint_measure(sg, pe, lr[s], li[s], yr, yi, tr, ti);
        }
        pauli_adjoint_keep(slot0 + k * slot_stride, first, tr, ti);
      }
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        const uint32_t sg = pt ^ ((uint32_t)(__popcll(((rep ^ span[s]) << ARTN_PAULI_TILE_BITS) & zm) & 1) << 31);
        const int from = (s ^ m) * Q * ARTN_BORN_THREADS + (tid ^ pmask);
        S yr[4], yi[4];
        if (staged) {
          pauli_unpack4(pauli_piece_ld(&stage_phi[from], ARTN_BORN_THREADS), yr, yi);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) yr[e] = pr[s][e], yi[e] = pi[s][e];
        }
        pauli_evolve_piece(c, r, sg, pe, pr[s], pi[s], yr, yi);
        if (staged) {
          pauli_unpack4(pauli_piece_ld(&stage_lam[from], ARTN_BORN_THREADS), yr, yi);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) yr[e] = lr[s][e], yi[e] = li[s][e];
        }
        pauli_evolve_piece(c, r, sg, pe, lr[s], li[s], yr, yi);
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

// States below one tile: both states live in LDS as T; thread t owns elements t, t + 256 ... < n (at most two) of each.
template <typename T>
__global__ __launch_bounds__(ARTN_BORN_THREADS) void artn_k_pauli_adjoint_small(T *lam, T *phi, long n,
                                                                                const ArtnPauliEvolveStep *__restrict__ stp, int n_steps,
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
  for (int k = 0; k < n_steps; ++k) {
    const PauliEvolveCoef c = pauli_evolve_coef(stp[k]);
    const uint64_t zm = stp[k].zmask;
    const long xm = (long)stp[k].xm_lo; // (the whole mask: n <= 2^9)
    const bool flagged = pauli_adjoint_flagged(stp[k]);
    __syncthreads();
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const long i = tid + u * ARTN_BORN_THREADS;
      T v, w;
      v.x = pr[u], v.y = pi[u], w.x = lr[u], w.y = li[u];
      if (i < n) img_phi[i] = v, img_lam[i] = w;
    }
    __syncthreads();
    double tr = 0.0, ti = 0.0;
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const long i = tid + u * ARTN_BORN_THREADS, j = i ^ xm;
      if (i >= n || j >= n) continue; // (j >= n never: xm < n)
      const uint32_t sg = (uint32_t)(__popcll((uint64_t)i & zm) & 1) << 31;
      const T b = img_phi[j], d = img_lam[j];
      const S br = pauli_evolve_flip(b.x, sg), bi = pauli_evolve_flip(b.y, sg);
      if (flagged) {
        const double ar = (double)lr[u], ai = (double)li[u];
        tr += fma(ar, (double)br, ai * (double)bi);
        ti += fma(ar, (double)bi, -(ai * (double)br));
      }
      pauli_evolve_pair(c, pr[u], pi[u], br, bi);
      pauli_evolve_pair(c, lr[u], li[u], pauli_evolve_flip(d.x, sg), pauli_evolve_flip(d.y, sg));
    }
    if (flagged) pauli_adjoint_keep(ws + (long)k * (2 * ARTN_PAULI_ADJOINT_WAVES) + 2 * (tid >> 6), true, tr, ti);
  }
#pragma unroll
  for (int u = 0; u < PER; ++u) {
    const long i = tid + u * ARTN_BORN_THREADS;
    T v, w;
    v.x = pr[u], v.y = pi[u], w.x = lr[u], w.y = li[u];
    if (i < n) phi[i] = v, lam[i] = w;
  }
}

// Workgroup k: out[k] = (-i)^ny * (the step's slots added: thread t takes slots t, t + 256 ... ascending, then the workgroup tree).
// The slots of a step: min(tiles >> rank of its run, grid limit) workgroups x ARTN_PAULI_ADJOINT_WAVES; the rank is in the step record.
static __global__ __launch_bounds__(ARTN_BORN_THREADS) void artn_k_pauli_adjoint_finish(const double *__restrict__ ws, long ws_groups,
                                                                                        long tiles,
                                                                                        const ArtnPauliEvolveStep *__restrict__ steps,
                                                                                        double *__restrict__ out) {
  __shared__ double red[ARTN_BORN_THREADS][2];
  const long k = blockIdx.x;
  const uint64_t word = steps[k].n_y;
  if (!((word >> 8) & 1)) { // (uniform)
    if (threadIdx.x < 2) out[2 * k + threadIdx.x] = 0.0;
    return;
  }
  long groups = tiles >> (int)((word >> 16) & 0xff);
  if (groups > ARTN_PAULI_EVOLVE_MAX_GRID) groups = ARTN_PAULI_EVOLVE_MAX_GRID;
  if (groups < 1) groups = 1;
  const double2 *src = (const double2 *)(ws + k * ws_groups * (2 * ARTN_PAULI_ADJOINT_WAVES));
  double acc[2] = {0.0, 0.0};
  for (long g = threadIdx.x; g < groups * ARTN_PAULI_ADJOINT_WAVES; g += ARTN_BORN_THREADS) {
    const double2 v = src[g];
    acc[0] += v.x, acc[1] += v.y;
  }
  born_wg_tree<2>(red, acc);
  if (threadIdx.x == 0) {
    const double re = red[0][0], im = red[0][1];
    switch ((int)(word & 3)) { // (-i)^ny
    case 0: out[2 * k] = re, out[2 * k + 1] = im; break;
    case 1: out[2 * k] = im, out[2 * k + 1] = -re; break;
    case 2: out[2 * k] = -re, out[2 * k + 1] = -im; break;
    default: out[2 * k] = -im, out[2 * k + 1] = re; break;
    }
  }
}

#endif // ARTN_PAULI_ADJOINT_KERNEL_H
