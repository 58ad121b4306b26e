// artn_batch_kernel.h -- B quantum trajectories in ONE amplitude array on gfx950: measurement, reset and noise channels with an
// outcome, a scale and an operator PER TRAJECTORY.  The batch dimensions are spectators of every unitary operation; here they
// select row b of the records.
//
//   artn_k_measure_batch_choose      one lane per trajectory: q[b, :] + uniform[b] (or forced[b]) -> record[b], the sequential
//                                    arithmetic of artn_k_measure_choose
//   artn_k_measure_batch_collapse<T> the streaming pass of artn_k_measure_collapse; outcome, scale and the `unit` shortcut of a
//                                    vector come from the record of the trajectory that the batch fields of its index name
//   artn_k_measure_batch_move<T>     reset, launch 1, want_hi per trajectory
//   artn_k_measure_batch_clear<T>    reset, launch 2
//   artn_k_channel_batch_choose      one lane per trajectory: the weights w_j, the draw, the 32-byte head of
//                                    artn_k_channel_choose's record (no current matrix: B of them would be large)
//   artn_k_channel_batch<T, K>       the tile kernel of artn_k_channel on a plan whose tile holds no batch bit: a tile lies in
//                                    ONE trajectory, so record, operator, scale and the early return are uniform per tile as
//                                    they are per launch there.  Every coefficient is mats[j][e] * scale, the one float64
//                                    multiply that the current matrix of artn_k_channel_choose holds.
//
// Batch index.  The host merges batch dimensions that are adjacent in memory and in order into FIELDS (shift, width, pos):
// b = OR over the fields of ((index >> shift) & (2^width - 1)) << pos.  Every batch bit lies at or above a 128-byte line, so
// neither a 16-byte vector nor a line spans two trajectories, and the vector index alone names the trajectory.
//
// Hazards.  Collapse and clear write the vector they index and read at most that vector.  Move: destination v has 0 at every
// measured bit, its source is v | want_hi(b).  Batch bits are never measured bits, so source and destination of a lane share b:
// the argument of artn_k_measure_move holds inside every trajectory on its own -- sources {v & mask_hi == want_hi(b)} are only
// read, destinations {v & mask_hi == 0} are only written, by the one lane that read their source; with want_hi(b) != 0 the two
// sets are disjoint, with want_hi(b) == 0 they are the same vector of the same lane -- and no lane of one trajectory touches a
// vector of another.  A trajectory whose outcome is -1 is neither read nor written by any of the three.  The tile kernel
// inherits the argument of artn_wgate_kernel.h: the tiles of a launch are disjoint, an element is written by the workgroup that
// loaded it, after the barrier behind the last read of the tile's LDS image; a skipped tile is left before its first access to
// the state.  Records and table are only read by the passes; the stream orders the launches.  No atomics.
#ifndef ARTN_BATCH_KERNEL_H
#define ARTN_BATCH_KERNEL_H

#include "artn.h"
#include "artn_channel_kernel.h"
#include "artn_measure_kernel.h"

#define ARTN_BATCH_CHOOSE_THREADS 256
#define ARTN_BATCH_MAX_HOLES 16

struct ArtnBatchFields { // a kernel argument: every read of it is uniform
  int32_t n;
  int32_t shift[ARTN_BATCH_MAX_FIELDS]; // lowest memory bit of the field (32-bit entries: an indexed read is a scalar load)
  int32_t width[ARTN_BATCH_MAX_FIELDS];
  int32_t pos[ARTN_BATCH_MAX_FIELDS];   // lowest bit of b that the field fills
};

struct ArtnBatchWalk { // the tile walk of artn_k_channel_batch
  int32_t seg_bits, n_holes;
  int32_t hole[ARTN_BATCH_MAX_HOLES]; // the tile bits at or above seg_bits, ascending
  ArtnBatchFields f;
};

// the trajectory of element index i
__device__ __forceinline__ long long batch_index(const ArtnBatchFields &f, uint64_t i) {
  uint64_t b = 0;
  for (int j = 0; j < f.n; ++j) b |= ((i >> f.shift[j]) & (((uint64_t)1 << f.width[j]) - 1)) << f.pos[j];
  return (long long)b;
}

// ---- measurement: choice ---------------------------------------------------------------------------------------------
// (the rule and the order of additions of artn_k_measure_choose, on row b)
static __global__ __launch_bounds__(ARTN_BATCH_CHOOSE_THREADS) void artn_k_measure_batch_choose(
    const double *__restrict__ q, long B, long D, const double *__restrict__ uniform, const long long *__restrict__ forced_of,
    int renormalize, ArtnMeasureRecord *__restrict__ rec) {
  const long b = (long)blockIdx.x * ARTN_BATCH_CHOOSE_THREADS + threadIdx.x;
  if (b >= B) return;
  const double *__restrict__ qb = q + b * D;
  double total = 0.0;
  for (long i = 0; i < D; ++i) total += qb[i];
  long long o = -1;
  if (isfinite(total) && total > 0.0) {
    if (forced_of) {
      const long long forced = forced_of[b];
      if (forced >= 0 && forced < D && qb[forced] > 0.0) o = forced;
    } else {
      const double t = uniform[b] * total;
      double run = 0.0;
      long long last = -1;
      for (long i = 0; i < D; ++i) {
        const double x = qb[i];
        run += x;
        if (x > 0.0) {
          last = i;
          if (run > t) {
            o = i;
            break;
          }
        }
      }
      if (o < 0) o = last;
    }
  }
  ArtnMeasureRecord r;
  r.outcome = o, r.total = total;
  r.probability = o < 0 ? 0.0 : qb[o] / total;
  r.scale = (o < 0 || !renormalize) ? 1.0 : sqrt(total / qb[o]);
  rec[b] = r;
}

// ---- measurement: collapse -------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(ARTN_MEASURE_THREADS) void artn_k_measure_batch_collapse(T *a, long nvec, ArtnMeasureArgs p, ArtnBatchFields f,
                                                                                      const ArtnMeasureRecord *__restrict__ rec) {
  typedef typename MeasureVec<T>::type V;
  const uint64_t mask_hi = p.mask >> p.vec_shift;
  const bool split = p.vec_shift == 1 && (p.mask & 1);
  V *av = (V *)a;
  const long step = (long)gridDim.x * ARTN_MEASURE_THREADS;
  for (long v = (long)blockIdx.x * ARTN_MEASURE_THREADS + threadIdx.x; v < nvec; v += step) {
    const ArtnMeasureRecord *r = rec + batch_index(f, (uint64_t)v << p.vec_shift);
    const long long o = r->outcome;
    if (o < 0) continue; // (this trajectory is neither read nor written)
    const double scale = r->scale;
    const bool unit = scale == 1.0;
    const uint64_t want = measure_want(p, o);
    const int live = (int)(want & 1);
    if (((uint64_t)v & mask_hi) != (want >> p.vec_shift)) {
      measure_zero(av + v); // (no load: whatever was here is gone)
    } else if (split || !unit) {
      av[v] = measure_keep(av[v], scale, unit, split, live, live);
    } // (a wholly kept vector under scale == 1 stays as it is)
  }
}

// ---- measurement: reset ----------------------------------------------------------------------------------------------
// Launch 1 (the header's hazard argument).  A trajectory with outcome 0..0 under scale == 1 and no split vector keeps its
// destinations as they are, as the whole launch does in artn_k_measure_move.
template <typename T>
__global__ __launch_bounds__(ARTN_MEASURE_THREADS) void artn_k_measure_batch_move(T *a, long nvec_dst, ArtnMeasureArgs p, ArtnBatchFields f,
                                                                                  const ArtnMeasureRecord *__restrict__ rec) {
  typedef typename MeasureVec<T>::type V;
  const bool split = p.vec_shift == 1 && (p.mask & 1);
  V *av = (V *)a;
  const long step = (long)gridDim.x * ARTN_MEASURE_THREADS;
  for (long t = (long)blockIdx.x * ARTN_MEASURE_THREADS + threadIdx.x; t < nvec_dst; t += step) {
    uint64_t v = (uint64_t)t;
    for (int j = 0; j < p.n_hi; ++j) { // a zero at every measured bit, lowest first
      const int b = p.hi_bit[j];
      v = ((v >> b) << (b + 1)) | (v & (((uint64_t)1 << b) - 1));
    }
    const ArtnMeasureRecord *r = rec + batch_index(f, v << p.vec_shift);
    const long long o = r->outcome;
    if (o < 0) continue;
    const double scale = r->scale;
    const bool unit = scale == 1.0;
    const uint64_t want = measure_want(p, o);
    const uint64_t want_hi = want >> p.vec_shift;
    if (unit && want_hi == 0 && !split) continue;
    av[v] = measure_keep(av[v | want_hi], scale, unit, split, (int)(want & 1), 0);
  }
}

// Launch 2 (after launch 1 in stream order): every vector with a measured bit set, of a trajectory that observed something,
// becomes +0.
template <typename T>
__global__ __launch_bounds__(ARTN_MEASURE_THREADS) void artn_k_measure_batch_clear(T *a, long nvec, ArtnMeasureArgs p, ArtnBatchFields f,
                                                                                   const ArtnMeasureRecord *__restrict__ rec) {
  typedef typename MeasureVec<T>::type V;
  const uint64_t mask_hi = p.mask >> p.vec_shift;
  if (mask_hi == 0) return;
  V *av = (V *)a;
  const long step = (long)gridDim.x * ARTN_MEASURE_THREADS;
  for (long v = (long)blockIdx.x * ARTN_MEASURE_THREADS + threadIdx.x; v < nvec; v += step)
    if (((uint64_t)v & mask_hi) && rec[batch_index(f, (uint64_t)v << p.vec_shift)].outcome >= 0) measure_zero(av + v);
}

// ---- channels: choice ------------------------------------------------------------------------------------------------
// One lane per trajectory.  w_j is the fma chain of artn_k_channel_choose; a lane forms it again wherever it needs it (the same
// operations on the same operands: the same bits) instead of keeping m of them.
__device__ __forceinline__ double batch_weight(const double *__restrict__ e, const double *__restrict__ in, int form, int D) {
  double x = 0.0;
  if (form == ARTN_CHANNEL_FIXED) {
    x = e[0];
  } else {
    for (int d = 0; d < D; ++d) x = fma(e[d], in[d], x);
  }
  return x > 0.0 ? x : 0.0; // (negative rounding residue and NaN: 0)
}

static __global__ __launch_bounds__(ARTN_BATCH_CHOOSE_THREADS) void artn_k_channel_batch_choose(
    const ArtnChannelTable *__restrict__ tab, int t, int m, int form, const double *__restrict__ input, const double *__restrict__ uniform,
    long B, int renormalize, ArtnChannelRecord *__restrict__ rec) {
  const long b = (long)blockIdx.x * ARTN_BATCH_CHOOSE_THREADS + threadIdx.x;
  if (b >= B) return;
  // (uniform; a table packed for another channel, or the DENSE form: nothing can be drawn)
  const bool match = (int)tab->gate.k == t && (int)tab->m == m && (int)tab->form == form && m >= 1 && m <= ARTN_CHANNEL_MAX_OPS &&
                     (form == ARTN_CHANNEL_FIXED || form == ARTN_CHANNEL_DIAGONAL);
  const int D = 1 << t, wd = form == ARTN_CHANNEL_FIXED ? 1 : D;
  const ArtnChannelOp *ops = (const ArtnChannelOp *)(tab + 1);
  const double *__restrict__ weights = (const double *)(ops + m);
  const double *__restrict__ in = form == ARTN_CHANNEL_DIAGONAL ? input + b * D : nullptr;
  double total = 0.0, trace = 1.0, wo = 0.0;
  long long o = -1;
  if (match) {
    for (int j = 0; j < m; ++j) total += batch_weight(weights + (long)wd * j, in, form, D);
    if (form == ARTN_CHANNEL_DIAGONAL) {
      trace = 0.0;
      for (int d = 0; d < D; ++d) trace += in[d];
    }
    if (isfinite(total) && total > 0.0 && isfinite(trace) && trace > 0.0) { // the rule of artn_k_measure_choose
      const double thr = uniform[b] * total;
      double run = 0.0, wlast = 0.0;
      long long last = -1;
      for (int j = 0; j < m; ++j) {
        const double x = batch_weight(weights + (long)wd * j, in, form, D);
        run += x;
        if (x > 0.0) {
          last = j, wlast = x;
          if (run > thr) {
            o = j;
            break;
          }
        }
      }
      if (o < 0) o = last;
      wo = wlast; // (o == last on both ways out)
    }
  }
  ArtnChannelRecord r;
  r.outcome = o, r.total = total;
  r.probability = o < 0 ? 0.0 : wo / total;
  r.scale = (o < 0 || !renormalize || form == ARTN_CHANNEL_FIXED) ? 1.0 : sqrt(trace / wo);
  rec[b] = r;
}

// ---- channels: the pass ------------------------------------------------------------------------------------------------
template <typename T, int K>
__global__ __launch_bounds__(ARTN_BORN_THREADS) void artn_k_channel_batch(T *a, const ArtnChannelTable *__restrict__ ctab,
                                                                          const ArtnChannelRecord *__restrict__ rec, int m, ArtnBatchWalk wk) {
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
  if ((int)tab->k != K || (int)ctab->m != m) return; // (uniform; a table packed for another channel: the launch does nothing)
  const ArtnChannelOp *__restrict__ ops = (const ArtnChannelOp *)(ctab + 1);
  const double *__restrict__ mats = (const double *)(ops + m) + (long)ctab->weight_doubles * m;
  const uint64_t block_mask = tab->block_mask; // the OR over the operators: gates_term leaves out what is exactly zero
  T *lds = (T *)artn_wgate_lds;
  const int tid = threadIdx.x;
  const int tb = (int)tab->tile_bits, gb = tb - K, n_loc = 1 << tb;
  const long n_tiles = (long)tab->n_tiles;
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
    // ---- the tile's first element: a 0 at every tile bit above the contiguous part (uniform)
    uint64_t base = (uint64_t)q << wk.seg_bits;
#pragma unroll 1
    for (int j = 0; j < wk.n_holes; ++j) {
      const int p = (int)wk.hole[j];
      base = ((base >> p) << (p + 1)) | (base & (((uint64_t)1 << p) - 1));
    }
    // ---- the tile's trajectory and its record (uniform)
    const ArtnChannelRecord *__restrict__ r = rec + batch_index(wk.f, base);
    const long long o = r->outcome;
    if (o < 0 || o >= (long long)m) continue;
    const double scale = r->scale;
    if ((ops[o].flags & ARTN_CHANNEL_OP_IDENTITY) && scale == 1.0) continue;
    const double *__restrict__ mat = mats + (long)(2 * ROWS * ROWS) * o;
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
      const int gs = g < (1 << gb) ? g : 0; // (a trajectory below one tile: lanes beyond its groups read group 0 and write nothing)
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
            gates_term(mb[2 * (j * ROWS + c)] * scale, mb[2 * (j * ROWS + c) + 1] * scale, xr[c], xi[c], re[j], im[j]);
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

#endif // ARTN_BATCH_KERNEL_H
