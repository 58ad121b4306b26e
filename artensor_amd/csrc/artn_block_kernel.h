// artn_block_kernel.h -- the block skeleton of the four run kernels artn_k_pauli_evolve, artn_k_pauli_adjoint, artn_k_gates and
// artn_k_gates_adjoint, and what their bodies share as functions.  Device code only; every helper is inlined into its kernel.
//
// A run has R pivots (tile-index bits, ascending) and R vectors over them: a reduced-echelon basis for Pauli steps, the unit
// vectors of the pivots for gates.  The orbits of their span split the tiles of 2^10 elements into BLOCKS of 2^R tiles:
// block q -> the representative tile `rep`, q with a 0 inserted at every pivot; SLOT s is the tile rep ^ span[s], span[s] the XOR
// of the vectors over the bits of s.  Thread t owns elements 4t .. 4t+3 (its PIECE) of every slot and keeps them in registers as
// T for the whole run: 16-byte global loads and stores, as artn_k_pauli_apply.  A step that needs another thread's values is
// STAGED: barrier, every thread stores its pieces of all slots to LDS, barrier, every thread reads the partner piece of each slot
// -- (slot, piece) is an address, never an indexed register -- and updates its own registers; it writes nothing else.  The stage
// keeps artn_k_pauli_apply's plane layout per slot, Q = sizeof(T) / 4 planes of 256 x 16 bytes: the ds_read_b128 of a plane at
// piece t ^ mask touches 16 distinct 16-byte slots in each lane group for every mask -- no bank conflict.  The adjoint kernels
// hold two such images, phi first.  Blocks are disjoint orbits, so no two workgroups touch the same element.
//
// What is a function here is what the compiler turns into the same instructions as the text it replaced.  The rest of the
// skeleton -- span[] from the run record, the loads and stores of a block, the stage and the partner read -- is still written
// out in each kernel: as functions (per block or per slot, with or without a callable for the basis) they changed register
// allocation and block layout of the instantiations with R >= 1, by up to a hundred VGPRs in artn_k_pauli_adjoint<float2, 3>.
// The same holds for a shared load loop of the _small kernels and for their two-array store loops.
#ifndef ARTN_BLOCK_KERNEL_H
#define ARTN_BLOCK_KERNEL_H

#include "artn.h"
#include "artn_pauli_kernel.h"

// the representative tile of block q
template <int R, typename Run>
__device__ __forceinline__ uint64_t block_rep(const Run *run, long q) {
  uint64_t rep = (uint64_t)q;
#pragma unroll
  for (int j = 0; j < R; ++j) {
    const int p = (int)run->pivot[j] - ARTN_PAULI_TILE_BITS;
    rep = ((rep >> p) << (p + 1)) | (rep & (((uint64_t)1 << p) - 1));
  }
  return rep;
}

// the four elements of a partner piece into the order of the own piece: element e takes e ^ r
template <typename S>
__device__ __forceinline__ void block_swap4(int r, S *yr, S *yi) {
  if (r & 1) pauli_swap(yr[0], yr[1]), pauli_swap(yi[0], yi[1]), pauli_swap(yr[2], yr[3]), pauli_swap(yi[2], yi[3]);
  if (r & 2) pauli_swap(yr[0], yr[2]), pauli_swap(yi[0], yi[2]), pauli_swap(yr[1], yr[3]), pauli_swap(yi[1], yi[3]);
}

// States below one tile (the _small kernels): thread t owns elements t, t + 256 ... < n, at most BLOCK_SMALL_PER of them.
#define BLOCK_SMALL_PER ((1 << ARTN_PAULI_TILE_BITS) / 2 / ARTN_BORN_THREADS) /* n <= 2^9 */

// registers -> dst[i], i < n: the LDS image of a step, and the state at the end
template <typename T, typename S>
__device__ __forceinline__ void block_small_st(T *dst, long n, int tid, const S (&xr)[BLOCK_SMALL_PER], const S (&xi)[BLOCK_SMALL_PER]) {
#pragma unroll
  for (int u = 0; u < BLOCK_SMALL_PER; ++u) {
    const long i = tid + u * ARTN_BORN_THREADS;
    T v;
    v.x = xr[u], v.y = xi[u];
    if (i < n) dst[i] = v;
  }
}

#endif // ARTN_BLOCK_KERNEL_H
