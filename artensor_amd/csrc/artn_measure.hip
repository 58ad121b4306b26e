// artn_measure.hip -- host half of the measurement entry points of include/artn.h (kernels: artn_measure_kernel.h).
//
// A translation unit of its own (build/obj/measure.o).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <string>
#include <vector>

#include "artn_host.h"
#include "artn_state_host.h"
#include "artn_measure_kernel.h"

static_assert(sizeof(ArtnMeasureRecord) == ARTN_MEASURE_RECORD_BYTES, "int64 outcome, then probability, total and scale");

// The layout checks of artn_pauli_query (artn_state_host.h), then the measured dimensions -- those with keep[] != 0, in the
// descriptor's order -- as memory bits; what is wrong with them is reported before what the layout does not support.
static int measure_plan(const ArtnMarginalDesc *d, ArtnMeasureInfo *info, ArtnMeasureArgs *args) {
  if (int rc = state_desc(d, "measurement takes", ARTN_MAX_LABELS, false)) return rc;
  StateLayout l;
  if (int rc = state_layout(d, l)) return rc;
  const int64_t n = l.n;
  ArtnMeasureInfo out = {};
  ArtnMeasureArgs a = {};
  for (int j = 0; j < ARTN_MEASURE_MAX_DIMS; ++j) out.mem_bit[j] = -1;
  int k = 0;
  for (int i = 0; i < d->n_dims; ++i) {
    if (!d->keep[i]) continue;
    if (d->extent[i] != 2)
      return fail(ARTN_E_INVALID, "a measured dimension has extent 2; dimension " + std::to_string(i) + " has extent " +
                                      std::to_string(d->extent[i]));
    if (k == ARTN_MEASURE_MAX_DIMS)
      return fail(ARTN_E_INVALID, "at most " + std::to_string(ARTN_MEASURE_MAX_DIMS) + " dimensions are measured in one call");
    const int b = __builtin_ctzll((uint64_t)d->stride[i]); // (dense and extent 2: the stride is a power of two where pow2 holds)
    out.mem_bit[k] = b, a.bit[k] = (uint8_t)b;
    ++k;
  }
  if (k < 1) return fail(ARTN_E_INVALID, "at least one dimension is measured");
  if (int rc = state_bits_only(l, "measurement takes")) return rc;
  const int64_t elem = d->dtype == ARTN_C64 ? 8 : 16;
  a.k = k, a.vec_shift = d->dtype == ARTN_C64 ? 1 : 0;
  for (int j = 0; j < k; ++j) a.mask |= (uint64_t)1 << a.bit[j];
  for (int b = a.vec_shift; b < 40; ++b)
    if (a.mask >> b & 1) a.hi_bit[a.n_hi++] = (uint8_t)(b - a.vec_shift);
  const int64_t nvec = n * elem / 16; // (k >= 1: n >= 2, a whole number of vectors)
  out.k = k, out.dim = (int64_t)1 << k, out.n = n;
  out.grid = (int32_t)std::min<int64_t>((nvec + ARTN_MEASURE_THREADS - 1) / ARTN_MEASURE_THREADS, ARTN_MEASURE_MAX_GRID);
  out.collapse_launches = 1, out.reset_launches = 2;
  out.record_bytes = ARTN_MEASURE_RECORD_BYTES;
  out.bytes_read = (n >> k) * elem, out.bytes_written = n * elem;
  if (info) *info = out;
  if (args) *args = a;
  return ARTN_OK;
}

template <typename T>
static void measure_launch(T *a, const ArtnMeasureInfo &mi, const ArtnMeasureArgs &p, const ArtnMeasureRecord *rec, bool reset, hipStream_t st) {
  const long nvec = (long)(mi.n >> p.vec_shift);
  const dim3 grid((unsigned)mi.grid), block(ARTN_MEASURE_THREADS);
  if (!reset) {
    hipLaunchKernelGGL(artn_k_measure_collapse<T>, grid, block, 0, st, a, nvec, p, rec);
    return;
  }
  const long nvec_dst = nvec >> p.n_hi;
  const unsigned move_grid = (unsigned)std::min<long>((nvec_dst + ARTN_MEASURE_THREADS - 1) / ARTN_MEASURE_THREADS, ARTN_MEASURE_MAX_GRID);
  hipLaunchKernelGGL(artn_k_measure_move<T>, dim3(move_grid), block, 0, st, a, nvec_dst, p, rec);
  hipLaunchKernelGGL(artn_k_measure_clear<T>, grid, block, 0, st, a, nvec, p, rec);
}

extern "C" {

int artn_measure_query(const ArtnMarginalDesc *d, ArtnMeasureInfo *info) {
  if (!info) return fail(ARTN_E_INVALID, "null info");
  return measure_plan(d, info, nullptr);
}

int artn_measure_choose(const double *q, int64_t D, const double *uniform, int64_t forced_outcome, int32_t renormalize, void *record,
                        void *stream) {
  if (artn_device_count() < 1) return fail(ARTN_E_NODEVICE, "no gfx950 device visible");
  if (D < 1 || D > ((int64_t)1 << ARTN_MEASURE_MAX_DIMS)) return fail(ARTN_E_INVALID, "the number of outcomes is out of range");
  if (!q || !record || (forced_outcome < 0 && !uniform)) return fail(ARTN_E_INVALID, "null pointer");
  if (forced_outcome >= D) return fail(ARTN_E_INVALID, "the forced outcome is not below the number of outcomes");
  if ((((uintptr_t)q | (uintptr_t)uniform | (uintptr_t)record) & 7) != 0)
    return fail(ARTN_E_UNSUPPORTED, "artn_measure_choose needs 8-byte aligned arrays");
  hipLaunchKernelGGL(artn_k_measure_choose, dim3(1), dim3(64), 0, (hipStream_t)stream, q, (long)D, uniform, (long long)forced_outcome,
                     (int)renormalize, (ArtnMeasureRecord *)record);
  HIP_TRY(hipGetLastError());
  return ARTN_OK;
}

int artn_measure_collapse(const ArtnMarginalDesc *d, void *a, const void *record, int32_t reset, void *stream) {
  if (artn_device_count() < 1) return fail(ARTN_E_NODEVICE, "no gfx950 device visible");
  ArtnMeasureInfo mi;
  ArtnMeasureArgs p;
  if (int rc = measure_plan(d, &mi, &p)) return rc;
  if (!a || !record) return fail(ARTN_E_INVALID, "null pointer");
  if (int rc = state_array_aligned(a, "artn_measure_collapse")) return rc;
  if (((uintptr_t)record & 7) != 0) return fail(ARTN_E_UNSUPPORTED, "artn_measure_collapse needs an 8-byte aligned record");
  hipStream_t st = (hipStream_t)stream;
  if (d->dtype == ARTN_C64)
    measure_launch<float2>((float2 *)a, mi, p, (const ArtnMeasureRecord *)record, reset != 0, st);
  else
    measure_launch<double2>((double2 *)a, mi, p, (const ArtnMeasureRecord *)record, reset != 0, st);
  HIP_TRY(hipGetLastError());
  return ARTN_OK;
}

} // extern "C"
