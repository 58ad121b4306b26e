// artn_measure_kernel.h -- projective measurement of up to ten qubits of an amplitude array on gfx950, in place: the choice of
// an outcome on the device, the collapse onto it, and the reset that moves the observed branch to |0..0>.
//
//   artn_k_measure_choose        one lane: probabilities + a uniform number (or a forced outcome) -> the 32-byte record
//   artn_k_measure_collapse<T>   streaming pass in memory order: zero-fills what is projected away WITHOUT reading it, scales
//                                what stays
//   artn_k_measure_move<T>       reset, launch 1: reads the vectors whose measured digits spell the outcome, writes the vectors
//                                whose measured digits are all 0
//   artn_k_measure_clear<T>      reset, launch 2: zero-fills every other vector, reading nothing
//
// Every kernel after the choice reads the record from device memory, so a whole measurement is enqueued without the host ever
// seeing the outcome.  A record with outcome -1 (nothing can be observed) makes them return before touching the state.
//
// The streaming kernels work on 16-byte VECTORS (two complex64 elements, one complex128 element) with a persistent grid and a
// grid-stride loop, 64-bit index arithmetic throughout, one 16-byte access per lane and plain vector stores only.  A measured
// dimension of extent 2 and stride 2^b is bit b of the flat memory index; the bits at or above the vector size are bits of the
// vector index (mask_hi), and memory bit 0 of complex64 lies INSIDE a vector: there only the kept half of a loaded vector is
// used and the other half is stored as +0.  A kept component c becomes fl(float64(c) * scale), one rounding; with scale == 1 it
// is stored as loaded (or, where the whole vector stays, not touched at all).
#ifndef ARTN_MEASURE_KERNEL_H
#define ARTN_MEASURE_KERNEL_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "artn.h"

#define ARTN_MEASURE_THREADS 256
#define ARTN_MEASURE_MAX_GRID 2048 /* workgroups of a streaming launch (8 per CU) */

struct ArtnMeasureRecord { // (include/artn.h documents the layout: the caller reads it back as int64 + 3 float64)
  long long outcome;
  double probability, total, scale;
};

struct ArtnMeasureArgs {
  uint64_t mask;      // the measured memory bits
  int32_t k;          // measured dimensions
  int32_t vec_shift;  // log2 elements per vector: 1 (complex64) or 0 (complex128)
  int32_t n_hi;       // measured bits at or above the vector size
  uint8_t bit[ARTN_MEASURE_MAX_DIMS];    // memory bit of measured dimension j, in listed order (j = 0: the most significant digit)
  uint8_t hi_bit[ARTN_MEASURE_MAX_DIMS]; // the n_hi bits of mask_hi as bits of the VECTOR index, ascending
};

// the memory bits that the digits of outcome o set
__device__ __forceinline__ uint64_t measure_want(const ArtnMeasureArgs &p, long long o) {
  uint64_t w = 0;
  for (int j = 0; j < p.k; ++j) w |= (uint64_t)((o >> (p.k - 1 - j)) & 1) << p.bit[j];
  return w;
}

// ---- choice ----------------------------------------------------------------------------------------------------------
// total = q[0] + q[1] + ... in ascending order; the outcome is the smallest o with q[o] > 0 whose inclusive running sum (the same
// sequence of additions) exceeds uniform * total, or the last o with q[o] > 0 where rounding leaves none.  Adding q[o] == 0 does
// not move the running sum, so testing only where q[o] > 0 IS "the smallest o whose sum exceeds", and a zero is never chosen.
static __global__ void artn_k_measure_choose(const double *__restrict__ q, long D, const double *__restrict__ uniform, long long forced,
                                             int renormalize, ArtnMeasureRecord *__restrict__ rec) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  double total = 0.0;
  for (long i = 0; i < D; ++i) total += q[i];
  long long o = -1;
  if (isfinite(total) && total > 0.0) {
    if (forced >= 0) {
      if (forced < D && q[forced] > 0.0) o = forced;
    } else {
      const double t = uniform[0] * total;
      double run = 0.0;
      long long last = -1;
      for (long i = 0; i < D; ++i) {
        const double x = q[i];
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
  r.probability = o < 0 ? 0.0 : q[o] / total;
  r.scale = (o < 0 || !renormalize) ? 1.0 : sqrt(total / q[o]);
  *rec = r;
}

// ---- vectors ---------------------------------------------------------------------------------------------------------
template <typename T> struct MeasureVec;
template <> struct MeasureVec<float2> { typedef float4 type; };
template <> struct MeasureVec<double2> { typedef double2 type; };

__device__ __forceinline__ float measure_scaled(float c, double scale, bool unit) { return unit ? c : (float)((double)c * scale); }
__device__ __forceinline__ double measure_scaled(double c, double scale, bool unit) { return unit ? c : c * scale; }

// What a loaded vector x leaves behind.  `split`: memory bit 0 is measured and lies inside the vector (complex64 only); `live` is
// the half whose digit matches, and it lands in half `to` (collapse: where it was; reset: half 0).
__device__ __forceinline__ float4 measure_keep(const float4 x, double scale, bool unit, bool split, int live, int to) {
  if (!split)
    return make_float4(measure_scaled(x.x, scale, unit), measure_scaled(x.y, scale, unit), measure_scaled(x.z, scale, unit),
                       measure_scaled(x.w, scale, unit));
  const float re = measure_scaled(live ? x.z : x.x, scale, unit), im = measure_scaled(live ? x.w : x.y, scale, unit);
  return to ? make_float4(0.0f, 0.0f, re, im) : make_float4(re, im, 0.0f, 0.0f);
}
__device__ __forceinline__ double2 measure_keep(const double2 x, double scale, bool unit, bool, int, int) {
  return make_double2(measure_scaled(x.x, scale, unit), measure_scaled(x.y, scale, unit));
}
__device__ __forceinline__ void measure_zero(float4 *at) { *at = make_float4(0.0f, 0.0f, 0.0f, 0.0f); }
__device__ __forceinline__ void measure_zero(double2 *at) { *at = make_double2(0.0, 0.0); }

// ---- collapse --------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(ARTN_MEASURE_THREADS) void artn_k_measure_collapse(T *a, long nvec, ArtnMeasureArgs p,
                                                                                const ArtnMeasureRecord *__restrict__ rec) {
  typedef typename MeasureVec<T>::type V;
  const long long o = rec->outcome;
  if (o < 0) return;
  const double scale = rec->scale;
  const bool unit = scale == 1.0;
  const uint64_t want = measure_want(p, o);
  const uint64_t mask_hi = p.mask >> p.vec_shift, want_hi = want >> p.vec_shift;
  const bool split = p.vec_shift == 1 && (p.mask & 1);
  const int live = (int)(want & 1);
  V *av = (V *)a;
  const long step = (long)gridDim.x * ARTN_MEASURE_THREADS;
#pragma unroll 4
  for (long v = (long)blockIdx.x * ARTN_MEASURE_THREADS + threadIdx.x; v < nvec; v += step) {
    if (((uint64_t)v & mask_hi) != want_hi) {
      measure_zero(av + v); // (no load: whatever was here is gone)
    } else if (split || !unit) {
      av[v] = measure_keep(av[v], scale, unit, split, live, live);
    } // (a wholly kept vector under scale == 1 stays as it is)
  }
}

// ---- reset -----------------------------------------------------------------------------------------------------------
// Launch 1.  Destination vector number t (its measured bits 0, the others counting up) is vector v; its source is v | want_hi.
// The sources {v & mask_hi == want_hi} are only read, the destinations {v & mask_hi == 0} are only written, by the one lane that
// read their source: with want_hi != 0 the two sets are disjoint, with want_hi == 0 source and destination are the SAME vector
// of the same lane.  The half of a split destination that is no destination element is stored as +0 here (launch 2 skips these
// vectors); it is a source element only where want_hi == 0, that is, of this very lane.
template <typename T>
__global__ __launch_bounds__(ARTN_MEASURE_THREADS) void artn_k_measure_move(T *a, long nvec_dst, ArtnMeasureArgs p,
                                                                            const ArtnMeasureRecord *__restrict__ rec) {
  typedef typename MeasureVec<T>::type V;
  const long long o = rec->outcome;
  if (o < 0) return;
  const double scale = rec->scale;
  const bool unit = scale == 1.0;
  const uint64_t want = measure_want(p, o);
  const uint64_t want_hi = want >> p.vec_shift;
  const bool split = p.vec_shift == 1 && (p.mask & 1);
  const int live = (int)(want & 1);
  if (unit && want_hi == 0 && !split) return; // outcome 0..0 under scale == 1: every destination already holds its value
  V *av = (V *)a;
  const long step = (long)gridDim.x * ARTN_MEASURE_THREADS;
  for (long t = (long)blockIdx.x * ARTN_MEASURE_THREADS + threadIdx.x; t < nvec_dst; t += step) {
    uint64_t v = (uint64_t)t;
    for (int j = 0; j < p.n_hi; ++j) { // a zero at every measured bit, lowest first
      const int b = p.hi_bit[j];
      v = ((v >> b) << (b + 1)) | (v & (((uint64_t)1 << b) - 1));
    }
    av[v] = measure_keep(av[v | want_hi], scale, unit, split, live, 0);
  }
}

// Launch 2 (after launch 1 in stream order, so every source has been read): every vector with a measured bit set becomes +0.
template <typename T>
__global__ __launch_bounds__(ARTN_MEASURE_THREADS) void artn_k_measure_clear(T *a, long nvec, ArtnMeasureArgs p,
                                                                             const ArtnMeasureRecord *__restrict__ rec) {
  typedef typename MeasureVec<T>::type V;
  if (rec->outcome < 0) return;
  const uint64_t mask_hi = p.mask >> p.vec_shift;
  if (mask_hi == 0) return;
  V *av = (V *)a;
  const long step = (long)gridDim.x * ARTN_MEASURE_THREADS;
#pragma unroll 4
  for (long v = (long)blockIdx.x * ARTN_MEASURE_THREADS + threadIdx.x; v < nvec; v += step)
    if ((uint64_t)v & mask_hi) measure_zero(av + v);
}

#endif // ARTN_MEASURE_KERNEL_H
