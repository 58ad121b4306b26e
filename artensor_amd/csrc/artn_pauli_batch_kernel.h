// artn_pauli_batch_kernel.h -- expectation values of Pauli strings PER TRAJECTORY of a batched amplitude array on gfx950: B states
// in one tensor (artn_batch_kernel.h), one pass over the tensor for up to ARTN_PAULI_TERMS strings of equal xmask, B rows out.
//
// Index space.  The tensor has n = 2^L elements, the batch dimensions hold batch_bits memory bits, all at or above a 128-byte
// line; a trajectory has M = L - batch_bits LOCAL bits, local bit j being the j-th lowest memory bit that is no batch bit.  The
// kernels walk the virtual index r = (b << M) | local; the address of r is
//     pauli_batch_local(local) | pauli_batch_traj(b)
// -- the local bits deposited into the positions that are no batch bits (a zero opened at every field, lowest first) and the
// bits of b deposited into the fields.  Both deposits are bitwise, so the address of (tile | piece) is the OR of the two
// deposits: the tile's and the trajectory's part are uniform per workgroup (kernel arguments and blockIdx alone: scalar work),
// the piece's part is computed once per thread.  Memory bits 0-1 are local bits 0-1 (the line rule), so a thread's four
// elements are contiguous and the loads are the 16-byte ones of artn_k_pauli.
//
// Masks.  Strings carry I on every batch dimension.  xl and zl are xmask and zmask compressed onto the local bits; forms, the
// halving bit, the thread's sign and the tile's sign are all taken from xl, zl and LOCAL indices, so a trajectory's result does
// not depend on where the batch bits lie.  Only the partner's address uses the global xmask: address ^ xmask is the address of
// local ^ xl in the same trajectory.
//
//   artn_k_pauli_batch<T, FORM, NT>        M >= 10.  FORM 0: xl == 0; 1: xl < 2^10; 2: xl >= 2^10, the local tiles whose highest
//                                          xl bit is 0, weight 2.  A local tile is 2^10 consecutive local indices, thread t owns
//                                          local elements 4t .. 4t+3.  A UNIT is (trajectory b, chunk c), 0 <= c < C: chunk c
//                                          takes local tiles c, c + C ... ascending; workgroups loop over units; a unit ends
//                                          with born_wg_tree and writes partial[(b C + c)(NT + 1) + q].
//   artn_k_pauli_batch_small<T, FORM, NT>  M < 10 (FORM 0, 1).  A virtual tile of 2^10 consecutive r holds 2^(10-M) whole
//                                          trajectories of 2^(M-2) threads each; the tree is SEGMENTED: born_wg_tree's strides
//                                          below 2^(M-2) only, so no sum crosses a trajectory.  Lanes with r >= n are guarded.
//                                          C = 1: partial[b (NT + 1) + q].
//   artn_k_pauli_batch_finish              one thread per (b, q): the C partials in ascending c, times scale.
//
// Arithmetic: that of artn_k_pauli term for term (pauli_batch_terms is its loop body) -- float64 first, one rounding per Re q
// and Im q, pauli_sums4, per-thread accumulators in ascending tile order, the workgroup tree, ascending partials.  With
// C = min(T, max(1, ARTN_BORN_MAX_GRID >> batch_bits)), T the local tile count (halved in FORM 2), B = 1 is artn_k_pauli's own
// order, and so is every trajectory whenever B T <= ARTN_BORN_MAX_GRID: each unit is one tile, as each workgroup there.  No
// floating-point atomics, no LDS beyond the 256 x 17 doubles of the unbatched kernel; the state is only read.
#ifndef ARTN_PAULI_BATCH_KERNEL_H
#define ARTN_PAULI_BATCH_KERNEL_H

#include "artn_batch_kernel.h"
#include "artn_pauli_kernel.h"

#define ARTN_PAULI_BATCH_MAX_GRID ARTN_BORN_MAX_GRID /* workgroups of a pass (8 per CU), as the unbatched pass */

struct ArtnPauliBatchArgs { // a kernel argument: every read of it is uniform
  ArtnPauliArgs p;          // xm: the GLOBAL xmask (partner addresses); zm, sel, hbit: LOCAL
  uint64_t xl;              // the local xmask
  int32_t local_bits;       // M
  int32_t chunk_bits;       // log2 C
  int32_t tile_bits;        // log2 T (T already halved in FORM 2)
  int32_t reserved;
  long long B;              // trajectories
  ArtnBatchFields f;        // the batch fields, ASCENDING by shift
};

// local index -> its part of the address: a zero opened at every batch field, lowest first
__device__ __forceinline__ uint64_t pauli_batch_local(const ArtnBatchFields &f, uint64_t v) {
  for (int j = 0; j < f.n; ++j) {
    const int s = f.shift[j], w = f.width[j];
    v = ((v >> s) << (s + w)) | (v & (((uint64_t)1 << s) - 1));
  }
  return v;
}
// trajectory -> its part of the address (the inverse of batch_index)
__device__ __forceinline__ uint64_t pauli_batch_traj(const ArtnBatchFields &f, uint64_t b) {
  uint64_t v = 0;
  for (int j = 0; j < f.n; ++j) v |= ((b >> f.pos[j]) & (((uint64_t)1 << f.width[j]) - 1)) << f.shift[j];
  return v;
}

// The loop body of artn_k_pauli on the thread's four elements at address `at`: partner at `pat` (own: the thread's own piece),
// r = xl & 3, sign_base = the local index of the tile's first element (its parity under zl is the tile's sign).
template <typename T, int FORM, int NT>
__device__ __forceinline__ void pauli_batch_terms(const T *__restrict__ a, long at, long pat, bool own, int r, const ArtnPauliArgs &p,
                                                  const uint32_t thr[NT], uint64_t sign_base, double acc[NT + 1]) {
  using S = decltype(T::x);
  constexpr int NS = FORM == 0 ? 4 : 8;
  S ar[4], ai[4];
  pauli_ld4(a, at, ar, ai);
  double s[NS];
  if constexpr (FORM == 0) {
    double q[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) q[e] = born_sq(ar[e], ai[e]);
    pauli_sums4(q, s);
    if (p.norm) acc[NT] += s[0];
  } else {
    S br[4], bi[4];
    if (FORM == 1 && own) {
#pragma unroll
      for (int e = 0; e < 4; ++e) br[e] = ar[e], bi[e] = ai[e];
    } else {
      pauli_ld4(a, pat, br, bi);
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
    acc[t] += pauli_flip(v, thr[t] ^ ((uint32_t)(__popcll(sign_base & p.zm[t]) & 1) << 31));
  }
}

template <typename T, int FORM, int NT>
__global__ __launch_bounds__(ARTN_BORN_THREADS) void artn_k_pauli_batch(const T *__restrict__ a, ArtnPauliBatchArgs g,
                                                                        double *__restrict__ partial) {
  __shared__ double red[ARTN_BORN_THREADS][NT + 1];
  const ArtnPauliArgs &p = g.p;
  const int tid = threadIdx.x;
  uint32_t thr[NT]; // sign bit of parity(4 tid & zl)
#pragma unroll
  for (int t = 0; t < NT; ++t) thr[t] = (uint32_t)(__popcll((uint64_t)(4 * tid) & p.zm[t]) & 1) << 31;
  const int r = (int)(g.xl & 3);
  const bool own = (g.xl >> 2) == 0;
  const uint64_t piece = pauli_batch_local(g.f, (uint64_t)(4 * tid)); // (loop-invariant, per thread)
  const uint64_t flip = p.xm & ~(uint64_t)3;                          // partner = address ^ flip, registers swapped by r
  const int hb = p.hbit - ARTN_PAULI_TILE_BITS;                       // FORM 2: bit of the LOCAL TILE index that stays 0
  const long tiles = (long)1 << g.tile_bits, C = (long)1 << g.chunk_bits;
  const long units = (long)g.B << g.chunk_bits;
  for (long u = blockIdx.x; u < units; u += gridDim.x) {
    const uint64_t b = (uint64_t)u >> g.chunk_bits;
    const long c = u & (C - 1);
    const uint64_t traj = pauli_batch_traj(g.f, b); // (uniform)
    double acc[NT + 1];
#pragma unroll
    for (int t = 0; t <= NT; ++t) acc[t] = 0.0;
#pragma unroll 2
    for (long k = c; k < tiles; k += C) {
      const uint64_t kt = FORM == 2 ? ((((uint64_t)k >> hb) << (hb + 1)) | ((uint64_t)k & (((uint64_t)1 << hb) - 1))) : (uint64_t)k;
      const uint64_t lbase = kt << ARTN_PAULI_TILE_BITS;               // local index of the tile's first element
      const uint64_t base = pauli_batch_local(g.f, lbase) | traj;      // (uniform)
      const uint64_t at = base | piece;
      pauli_batch_terms<T, FORM, NT>(a, (long)at, (long)(at ^ flip), own, r, p, thr, lbase, acc);
    }
    born_wg_tree<NT + 1>(red, acc);
    if (tid <= NT) partial[u * (NT + 1) + tid] = red[0][tid];
    __syncthreads(); // the next unit's tree overwrites red
  }
}

template <typename T, int FORM, int NT>
__global__ __launch_bounds__(ARTN_BORN_THREADS) void artn_k_pauli_batch_small(const T *__restrict__ a, ArtnPauliBatchArgs g,
                                                                              double *__restrict__ partial) {
  static_assert(FORM < 2, "a trajectory below one tile has no partner tile");
  __shared__ double red[ARTN_BORN_THREADS][NT + 1];
  const ArtnPauliArgs &p = g.p;
  const int tid = threadIdx.x;
  const int M = g.local_bits;                          // 3 .. 9: a thread's four elements lie in one trajectory
  const int seg = 1 << (M - 2);                        // threads of a trajectory
  const int lane = tid & (seg - 1);                    // the thread's place in its trajectory
  const uint64_t local = (uint64_t)(4 * lane);         // a trajectory starts at local index 0: no tile sign
  uint32_t thr[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) thr[t] = (uint32_t)(__popcll(local & p.zm[t]) & 1) << 31;
  const int r = (int)(g.xl & 3);
  const bool own = (g.xl >> 2) == 0;
  const uint64_t flip = p.xm & ~(uint64_t)3;
  const uint64_t piece = pauli_batch_local(g.f, local) | pauli_batch_traj(g.f, (uint64_t)(tid >> (M - 2))); // (loop-invariant)
  const int per = ARTN_PAULI_TILE_BITS - M;            // log2 trajectories of a virtual tile
  const long vtiles = (long)((g.B + ((long long)1 << per) - 1) >> per);
  for (long w = blockIdx.x; w < vtiles; w += gridDim.x) {
    const long long b = ((long long)w << per) | (tid >> (M - 2));
    double acc[NT + 1];
#pragma unroll
    for (int t = 0; t <= NT; ++t) acc[t] = 0.0;
    if (b < g.B) { // (r = (b << M) | local < n)
      const uint64_t at = pauli_batch_traj(g.f, (uint64_t)w << per) | piece; // (the first trajectory's part: uniform)
      pauli_batch_terms<T, FORM, NT>(a, (long)at, (long)(at ^ flip), own, r, p, thr, 0, acc);
    }
#pragma unroll
    for (int q = 0; q <= NT; ++q) red[tid][q] = acc[q];
    __syncthreads();
    for (int s = seg >> 1; s > 0; s >>= 1) { // born_wg_tree below the segment
      if (lane < s) {
#pragma unroll
        for (int q = 0; q <= NT; ++q) red[tid][q] += red[tid + s][q];
      }
      __syncthreads();
    }
    for (int i = tid; i < (NT + 1) << per; i += ARTN_BORN_THREADS) { // the first lane of every segment holds its sums
      const int sg = i / (NT + 1), q = i - sg * (NT + 1);
      const long long bo = ((long long)w << per) | sg;
      if (bo < g.B) partial[bo * (NT + 1) + q] = red[sg << (M - 2)][q];
    }
    __syncthreads(); // the next virtual tile overwrites red
  }
}

// partial: B rows of C rows of nv doubles (nv - 1 term slots, then sum |a|^2); out: B rows of `row` doubles
static __global__ __launch_bounds__(ARTN_BORN_THREADS) void artn_k_pauli_batch_finish(const double *__restrict__ partial, long long B,
                                                                                       long C, int nv, ArtnPauliFinish f, long row,
                                                                                       double *__restrict__ out) {
  const long long i = (long long)blockIdx.x * ARTN_BORN_THREADS + threadIdx.x;
  const long long b = i / nv;
  const int q = (int)(i - b * nv);
  if (b >= B) return;
  const bool term = q < f.nt, norm = q == nv - 1 && f.norm_index >= 0;
  if (!term && !norm) return;
  const double *__restrict__ pb = partial + (b * C) * nv + q;
  double v = 0.0;
#pragma unroll 8
  for (long c = 0; c < C; ++c) v += pb[c * nv];
  if (term) out[b * row + f.out_index[q]] = (double)f.scale[q] * v;
  else out[b * row + f.norm_index] = v;
}

#endif // ARTN_PAULI_BATCH_KERNEL_H
