// artn_channel_kernel.h -- one quantum-trajectory step of a noise channel on K = 1..5 qubits of an amplitude array on gfx950:
// the draw of an operator on the device and the pass that applies it, in place.
//
//   artn_k_channel_choose   ONE workgroup: the weights w_j of the m operators, the choice, the 32-byte record in the layout of
//                           artn_measure_kernel.h's and, behind it, the CURRENT MATRIX (operator j times scale).
//   artn_k_channel<T, K>    the tile kernel of artn_wgate_kernel.h (its four phases, its LDS layout, its chunk helpers and
//                           gates_term, so the arithmetic is the same function) with three differences, all uniform:
//     (a) record      `rec` (a kernel argument: every read of it is a uniform scalar load) is what the choose kernel wrote.  Where
//                     its j is < 0 (or not below m), and where operator j was flagged an exact identity at pack time and scale ==
//                     1.0, every workgroup returns before its first access to the state.
//     (b) operator    block_mask comes from ops[j], the per-operator array of the table, indexed by the device-side j.
//     (c) matrix      the coefficients are read from the current-matrix slot behind the record, not from the table.
//
// Weights (include/artn.h: FORM).  Each w_j is ONE lane's float64 fma chain from 0.0 in a fixed order -- DIAGONAL: d ascending;
// DENSE: a ascending, inside it b ascending, + Re E Re rho then - Im E Im rho -- so it does not depend on m, on the lane or on the
// launch.  The sums over j (total) and over d (trace) are one lane's ascending additions.
//
// Hazards.  The choose kernel is one workgroup; lane 0 writes the record after a barrier behind the last weight, the lanes write
// disjoint components of the current matrix after the barrier behind the record's LDS copy.  The pass inherits the argument of
// artn_wgate_kernel.h: the tiles of a launch are disjoint, every element is written by the workgroup that loaded it after the
// barrier that follows the last read of the tile's LDS image.  Record and current matrix are only read by the pass; the stream
// orders the launches.  No atomics.
#ifndef ARTN_CHANNEL_KERNEL_H
#define ARTN_CHANNEL_KERNEL_H

#include "artn.h"
#include "artn_gates_kernel.h"
#include "artn_wgate_kernel.h"

#define ARTN_CHANNEL_THREADS 256

struct ArtnChannelRecord { // the head of a step's record: the layout of artn_measure_choose's (include/artn.h), the current matrix behind it
  long long outcome;
  double probability, total, scale;
};

// ---- choice ----------------------------------------------------------------------------------------------------------
static __global__ __launch_bounds__(ARTN_CHANNEL_THREADS) void artn_k_channel_choose(const ArtnChannelTable *__restrict__ tab, int t, int m,
                                                                                     int form, const double *__restrict__ in,
                                                                                     const double *__restrict__ uniform,
                                                                                     int renormalize, ArtnChannelRecord *rec) {
  __shared__ double w[ARTN_CHANNEL_MAX_OPS];
  __shared__ long long chosen;
  __shared__ double scale_s;
  const int tid = threadIdx.x;
  if (blockIdx.x != 0) return;
  // (uniform; a table packed for another channel: nothing can be drawn)
  const bool match = (int)tab->gate.k == t && (int)tab->m == m && (int)tab->form == form && m >= 1 && m <= ARTN_CHANNEL_MAX_OPS;
  const int D = 1 << t, wd = form == ARTN_CHANNEL_FIXED ? 1 : form == ARTN_CHANNEL_DIAGONAL ? D : 2 * D * D;
  const ArtnChannelOp *ops = (const ArtnChannelOp *)(tab + 1);
  const double *__restrict__ weights = (const double *)(ops + m);
  const double *__restrict__ mats = weights + (long)wd * m;
  double *cur = (double *)(rec + 1);
  if (match)
    for (int j = tid; j < m; j += ARTN_CHANNEL_THREADS) {
      const double *__restrict__ e = weights + (long)wd * j;
      double x = 0.0;
      if (form == ARTN_CHANNEL_FIXED) {
        x = e[0];
      } else if (form == ARTN_CHANNEL_DIAGONAL) {
        for (int d = 0; d < D; ++d) x = fma(e[d], in[d], x);
      } else {
        for (int a = 0; a < D; ++a)
          for (int b = 0; b < D; ++b) {
            x = fma(e[2 * (a * D + b)], in[2 * (b * D + a)], x);
            x = fma(-e[2 * (a * D + b) + 1], in[2 * (b * D + a) + 1], x);
          }
      }
      w[j] = x > 0.0 ? x : 0.0; // (negative rounding residue and NaN: 0)
    }
  __syncthreads();
  if (tid == 0) {
    double total = 0.0, trace = 1.0;
    long long o = -1;
    if (match) {
      for (int j = 0; j < m; ++j) total += w[j];
      if (form == ARTN_CHANNEL_DIAGONAL) {
        trace = 0.0;
        for (int d = 0; d < D; ++d) trace += in[d];
      } else if (form == ARTN_CHANNEL_DENSE) {
        trace = 0.0;
        for (int d = 0; d < D; ++d) trace += in[2 * (d * D + d)];
      }
      if (isfinite(total) && total > 0.0 && isfinite(trace) && trace > 0.0) { // the rule of artn_k_measure_choose
        const double thr = uniform[0] * total;
        double run = 0.0;
        long long last = -1;
        for (int j = 0; j < m; ++j) {
          const double x = w[j];
          run += x;
          if (x > 0.0) {
            last = j;
            if (run > thr) {
              o = j;
              break;
            }
          }
        }
        if (o < 0) o = last;
      }
    }
    ArtnChannelRecord r;
    r.outcome = o, r.total = total;
    r.probability = o < 0 ? 0.0 : w[o] / total;
    r.scale = (o < 0 || !renormalize || form == ARTN_CHANNEL_FIXED) ? 1.0 : sqrt(trace / w[o]);
    *rec = r;
    chosen = o, scale_s = r.scale;
  }
  __syncthreads();
  const long long o = chosen;
  const double scale = scale_s;
  const int nm = 2 * D * D;
  for (int e = tid; e < nm; e += ARTN_CHANNEL_THREADS) cur[e] = o < 0 ? 0.0 : mats[(long)nm * o + e] * scale;
}

// ---- the pass ----------------------------------------------------------------------------------------------------------
template <typename T, int K>
__global__ __launch_bounds__(ARTN_BORN_THREADS) void artn_k_channel(T *a, const ArtnChannelTable *__restrict__ ctab,
                                                                    const ArtnChannelRecord *__restrict__ rec, int m) {
  using S = decltype(T::x);
  using W = WgateChunk<T>;
  using C = typename W::type;
  constexpr int NT = ARTN_BORN_THREADS, LOG_NT = 8;
  constexpr int ROWS = 1 << K, R = ROWS < ARTN_WGATE_ROWS ? ROWS : ARTN_WGATE_ROWS, NB = ROWS / R;
  constexpr int LOG_R = K < 3 ? K : 3;
  constexpr int CHUNKS = (1 << W::TB) / W::E / NT; // 16-byte chunks of a full tile per thread
  constexpr int ITEMS = (1 << W::TB) / R / NT;     // items of a full tile per thread
  static_assert(NT == 1 << LOG_NT && R == 1 << LOG_R && CHUNKS >= 1 && ITEMS >= 1, "tile shape");
  const ArtnWgateTable *__restrict__ tab = &ctab->gate;
  if ((int)tab->k != K) return; // (uniform; a table packed for another channel: the launch does nothing)
  // ---- (a) the record (uniform)
  const long long o = rec->outcome;
  if (o < 0 || o >= (long long)m || (int)ctab->m != m) return; // (m: what the host sized the table for)
  const ArtnChannelOp *__restrict__ ops = (const ArtnChannelOp *)(ctab + 1);
  // ---- (b) the operator's block mask and flags
  const uint64_t block_mask = ops[o].block_mask;
  if ((ops[o].flags & ARTN_CHANNEL_OP_IDENTITY) && rec->scale == 1.0) return;
  // ---- (c) the current matrix
  const double *__restrict__ mat = (const double *)(rec + 1);
  T *lds = (T *)artn_wgate_lds;
  const int tid = threadIdx.x;
  const int tb = (int)tab->tile_bits, gb = tb - K, n_loc = 1 << tb;
  const long n_tiles = (long)tab->n_tiles;
  const int seg_bits = tb - (int)tab->n_high;
  const int col0 = (int)tab->lds_col[0];

  // phases 1 and 4: the thread's part of the memory offset and of the LDS index of its chunks
  uint64_t mt = 0;
  int vt = 0;
#pragma unroll
  for (int b = 0; b < LOG_NT; ++b)
    if ((tid >> b) & 1) mt ^= tab->mem_col[b + W::LOG_E], vt ^= (int)tab->lds_col[b + W::LOG_E];
  // phases 2 and 3: the swizzle of the rows inside a block (uniform)
  int swj[R];
#pragma unroll
  for (int j = 0; j < R; ++j) {
    swj[j] = 0;
#pragma unroll
    for (int i = 0; i < LOG_R; ++i)
      if ((j >> i) & 1) swj[j] ^= (int)tab->swizzle[i];
  }
  const int gp = gb > 6 ? gb : 6; // lanes of an item index: a wavefront never spans two row blocks

  for (long q = blockIdx.x; q < n_tiles; q += gridDim.x) {
    uint64_t base = (uint64_t)q << seg_bits;
#pragma unroll
    for (int j = 0; j < ARTN_WGATE_MAX_K; ++j)
      if (j < (int)tab->n_high) { // (uniform)
        const int p = (int)tab->high_bit[j];
        base = ((base >> p) << (p + 1)) | (base & (((uint64_t)1 << p) - 1));
      }
    // ---- 1: memory -> LDS
    C chunk[CHUNKS];
#pragma unroll
    for (int i = 0; i < CHUNKS; ++i) {
      uint64_t mi = 0; // (uniform)
#pragma unroll
      for (int b = 0; (i >> b) != 0; ++b)
        if ((i >> b) & 1) mi ^= tab->mem_col[b + LOG_NT + W::LOG_E];
      if (((i * NT + tid) << W::LOG_E) < n_loc) chunk[i] = *(const C *)(a + (base | (mt ^ mi)));
    }
#pragma unroll
    for (int i = 0; i < CHUNKS; ++i) {
      int vi = 0; // (uniform)
#pragma unroll
      for (int b = 0; (i >> b) != 0; ++b)
        if ((i >> b) & 1) vi ^= (int)tab->lds_col[b + LOG_NT + W::LOG_E];
      if (((i * NT + tid) << W::LOG_E) < n_loc) wgate_to_lds(lds, vt ^ vi, col0, chunk[i]);
    }
    __syncthreads();
    // ---- 2: the outputs of the thread's items
    S outr[ITEMS][R], outi[ITEMS][R];
#pragma unroll
    for (int w = 0; w < ITEMS; ++w) {
      const int it = w * NT + tid;
      const int rb = __builtin_amdgcn_readfirstlane(it >> gp); // (the same in every lane of a wavefront: gp >= 6)
      if (rb >= NB) continue;                                  // (uniform)
      const int g = it & ((1 << gp) - 1);
      const int gs = g < (1 << gb) ? g : 0; // (a state below one tile: lanes beyond its groups read group 0 and write nothing)
      double re[R], im[R];
#pragma unroll
      for (int j = 0; j < R; ++j) re[j] = -0.0, im[j] = -0.0;
#pragma unroll 1
      for (int dh = NB - 1; dh >= 0; --dh) {
        const int cb = rb ^ dh;
        if (!((block_mask >> (rb * NB + cb)) & 1)) continue; // (uniform)
        int swb = 0;
#pragma unroll
        for (int i = LOG_R; i < K; ++i)
          if ((cb >> (i - LOG_R)) & 1) swb ^= (int)tab->swizzle[i];
        S xr[R], xi[R];
#pragma unroll
        for (int j = 0; j < R; ++j) {
          const T x = lds[(((cb * R + j) << gb) | gs) ^ swb ^ swj[j]];
          xr[j] = x.x, xi[j] = x.y;
        }
        const double *__restrict__ mb = mat + 2 * ((long)(rb * R) * ROWS + cb * R);
#pragma unroll
        for (int dl = R - 1; dl >= 0; --dl)
#pragma unroll
          for (int j = 0; j < R; ++j) {
            const int c = j ^ dl;
            gates_term(mb[2 * (j * ROWS + c)], mb[2 * (j * ROWS + c) + 1], xr[c], xi[c], re[j], im[j]);
          }
      }
#pragma unroll
      for (int j = 0; j < R; ++j) outr[w][j] = (S)re[j], outi[w][j] = (S)im[j];
    }
    __syncthreads(); // every thread has read its inputs
    // ---- 3: the outputs to their places
#pragma unroll
    for (int w = 0; w < ITEMS; ++w) {
      const int it = w * NT + tid;
      const int rb = __builtin_amdgcn_readfirstlane(it >> gp);
      if (rb >= NB) continue;
      const int g = it & ((1 << gp) - 1);
      if (g >= (1 << gb)) continue;
      int swb = 0;
#pragma unroll
      for (int i = LOG_R; i < K; ++i)
        if ((rb >> (i - LOG_R)) & 1) swb ^= (int)tab->swizzle[i];
#pragma unroll
      for (int j = 0; j < R; ++j) {
        T y;
        y.x = outr[w][j], y.y = outi[w][j];
        lds[(((rb * R + j) << gb) | g) ^ swb ^ swj[j]] = y;
      }
    }
    __syncthreads();
    // ---- 4: LDS -> memory
#pragma unroll
    for (int i = 0; i < CHUNKS; ++i) {
      uint64_t mi = 0;
      int vi = 0;
#pragma unroll
      for (int b = 0; (i >> b) != 0; ++b)
        if ((i >> b) & 1) mi ^= tab->mem_col[b + LOG_NT + W::LOG_E], vi ^= (int)tab->lds_col[b + LOG_NT + W::LOG_E];
      if (((i * NT + tid) << W::LOG_E) < n_loc) *(C *)(a + (base | (mt ^ mi))) = wgate_from_lds(lds, vt ^ vi, col0);
    }
    __syncthreads(); // the next tile overwrites the image
  }
}

#endif // ARTN_CHANNEL_KERNEL_H
