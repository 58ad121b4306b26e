// artn_sample_batch.hip -- host half of artn_sample_batch_query / artn_sample_batch of include/artn.h: bitstring sampling per
// trajectory of a batched amplitude array (kernels: artn_sample_batch_kernel.h).
//
// A translation unit of its own (build/obj/sample_batch.o).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <numeric>
#include <string>
#include <vector>

#include "artn_host.h"
#include "artn_state_host.h"
#include "artn_sample_batch_kernel.h"

struct SampleBatchPlan {
  int64_t n = 1, B = 1, nbt = 1; // elements of the tensor, trajectories, blocks of a trajectory
  int local_bits = 0, block_bits = 0, row_bits = 0;
  bool small = false;
  ArtnBatchFields fields = {}; // ascending by shift (what the kernels deposit through)
  ArtnSampleBatchInfo info = {};
};

// The layout checks of the family in the wording "batched sampling takes ...", the batch dimensions (what is wrong with them
// before what the layout does not support), the sample count, the blocks of a trajectory and the launches.
static int sample_batch_plan(const ArtnMarginalDesc *d, int32_t nb, const int32_t *batch_dims, int64_t n_samples, SampleBatchPlan &pl) {
  const char *who = "batched sampling takes";
  if (int rc = state_desc(d, who, ARTN_MARG_MAX_DIMS, false)) return rc;
  if (nb > 0 && !batch_dims) return fail(ARTN_E_INVALID, "null pointer");
  if (nb < 0) return fail(ARTN_E_INVALID, "a negative number of batch dimensions: " + std::to_string(nb));
  if (n_samples < 0) return fail(ARTN_E_INVALID, "negative sample count");
  StateLayout l;
  if (int rc = state_layout(d, l)) return rc;
  if (int rc = state_bits_only(l, who)) return rc;
  std::vector<int32_t> seen;
  BatchDims bd;
  if (int rc = state_batch_dims(d, nb, batch_dims, seen, 0, "sampled", bd)) return rc;
  pl.n = l.n, pl.B = (int64_t)1 << bd.bits;
  if (n_samples > (((int64_t)1 << 28) >> bd.bits))
    return fail(ARTN_E_UNSUPPORTED, "B * n_samples = " + std::to_string(pl.B) + " * " + std::to_string(n_samples) +
                                        " is above 2^28 samples (2 GiB of indices)");
  const int M = pl.local_bits = __builtin_ctzll((uint64_t)l.n) - bd.bits;
  ArtnBornPlan bp;
  if (int rc = artn_born_plan((int64_t)1 << M, d->dtype, &bp)) return rc;
  pl.block_bits = bp.block_bits, pl.nbt = bp.n_blocks, pl.row_bits = __builtin_ctzll((uint64_t)bp.n_blocks);
  pl.small = M < ARTN_SAMPLE_BATCH_SMALL_BITS && pl.B > 1; // (one state below a block: the tiled kernels, a tail of zeros, as unbatched)
  if (pl.small && M < 2) return fail(ARTN_E_UNSUPPORTED, "a trajectory of fewer than 4 elements"); // (the line rule excludes it)
  // the fields: the info lists them as the family does (the order listed), the kernels take them ascending by shift
  ArtnSampleBatchInfo &si = pl.info;
  const size_t nf = bd.shift.size();
  std::vector<size_t> by_shift(nf);
  std::iota(by_shift.begin(), by_shift.end(), (size_t)0);
  std::sort(by_shift.begin(), by_shift.end(), [&](size_t x, size_t y) { return bd.shift[x] < bd.shift[y]; });
  pl.fields.n = (int32_t)nf;
  for (size_t f = 0; f < nf; ++f) {
    si.field_shift[f] = bd.shift[f], si.field_width[f] = bd.width[f], si.field_pos[f] = bd.pos[f];
    const size_t s = by_shift[f];
    pl.fields.shift[f] = bd.shift[s], pl.fields.width[f] = bd.width[s], pl.fields.pos[f] = bd.pos[s];
  }
  si.B = pl.B, si.n = pl.n, si.batch_bits = bd.bits, si.local_bits = M, si.block_bits = pl.block_bits, si.n_fields = (int32_t)nf;
  si.blocks_per_trajectory = pl.nbt;
  si.bytes_read_min = pl.n * (d->dtype == ARTN_C64 ? 8 : 16);
  if (pl.small) {
    const int per = ARTN_SAMPLE_BATCH_SMALL_BITS - M;
    si.form = ARTN_SAMPLE_BATCH_SMALL, si.launches = 1;
    si.grid[0] = (int32_t)std::min<int64_t>((pl.B + ((int64_t)1 << per) - 1) >> per, ARTN_SAMPLE_BATCH_MAX_GRID);
    si.workspace_bytes = 0;
  } else {
    const int64_t units = pl.B * pl.nbt;
    si.form = ARTN_SAMPLE_BATCH_TILED, si.launches = 3;
    si.grid[0] = si.grid[2] = (int32_t)std::min<int64_t>(units, ARTN_SAMPLE_BATCH_MAX_GRID);
    si.grid[1] = (int32_t)(pl.nbt > ARTN_BORN_PREFIX_THREADS ? pl.B : (units + ARTN_BORN_PREFIX_THREADS - 1) / ARTN_BORN_PREFIX_THREADS);
    si.workspace_bytes = units * 2 * (int64_t)sizeof(double);
  }
  return ARTN_OK;
}

template <typename T>
static void sample_batch_launch(const SampleBatchPlan &pl, const T *a, const ArtnSampleBatchArgs &g, const double *uniforms,
                                long long *out_index, double *out_prob, double *out_norm, double *ws, hipStream_t st) {
  const ArtnSampleBatchInfo &si = pl.info;
  const dim3 block(ARTN_BORN_THREADS), wide(ARTN_BORN_PREFIX_THREADS);
  if (pl.small) {
    hipLaunchKernelGGL(artn_k_sample_batch_small<T>, dim3((unsigned)si.grid[0]), block, 0, st, a, g, uniforms, out_index, out_prob, out_norm);
    return;
  }
  const int64_t units = pl.B * pl.nbt;
  double *block_sum = ws, *prefix = ws + units;
  hipLaunchKernelGGL(artn_k_sample_batch_block_sums<T>, dim3((unsigned)si.grid[0]), block, 0, st, a, g, block_sum);
  if (pl.nbt > ARTN_BORN_PREFIX_THREADS)
    hipLaunchKernelGGL(artn_k_sample_batch_prefix_rows, dim3((unsigned)si.grid[1]), wide, 0, st, (const double *)block_sum, prefix,
                       (long)pl.nbt, out_norm);
  else
    hipLaunchKernelGGL(artn_k_sample_batch_prefix_packed, dim3((unsigned)si.grid[1]), wide, 0, st, (const double *)block_sum, prefix,
                       (long)units, (int)pl.row_bits, out_norm);
  hipLaunchKernelGGL(artn_k_sample_batch_pick<T>, dim3((unsigned)si.grid[2]), block, 0, st, a, g, (const double *)prefix, uniforms, out_index,
                     out_prob);
}

extern "C" {

int artn_sample_batch_query(const ArtnMarginalDesc *d, int32_t nb, const int32_t *batch_dims, int64_t n_samples, ArtnSampleBatchInfo *info) {
  if (!info) return fail(ARTN_E_INVALID, "null info");
  SampleBatchPlan pl;
  if (int rc = sample_batch_plan(d, nb, batch_dims, n_samples, pl)) return rc;
  *info = pl.info;
  return ARTN_OK;
}

// (every argument is checked before the device is looked for: a refusal does not depend on the machine)
int artn_sample_batch(const ArtnMarginalDesc *d, const void *a, int32_t nb, const int32_t *batch_dims, const double *uniforms_sorted,
                      int64_t n_samples, int64_t *out_index, double *out_prob, double *out_norm, void *ws, int64_t ws_bytes, void *stream) {
  SampleBatchPlan pl;
  if (int rc = sample_batch_plan(d, nb, batch_dims, n_samples, pl)) return rc;
  if (n_samples == 0) return ARTN_OK; // (nothing to draw: no launch, out_norm is not written)
  if (!a || !uniforms_sorted || !out_index || !out_prob || !out_norm || (!ws && pl.info.workspace_bytes > 0))
    return fail(ARTN_E_INVALID, "null pointer");
  if (ws_bytes < pl.info.workspace_bytes) return fail(ARTN_E_INVALID, "workspace smaller than artn_sample_batch_query reports");
  if (int rc = state_array_aligned(a, "artn_sample_batch")) return rc;
  if ((((uintptr_t)uniforms_sorted | (uintptr_t)out_index | (uintptr_t)out_prob | (uintptr_t)out_norm | (uintptr_t)ws) & 7) != 0)
    return fail(ARTN_E_UNSUPPORTED, "artn_sample_batch needs 8-byte aligned uniforms, outputs and workspace");
  if (artn_device_count() < 1) return fail(ARTN_E_NODEVICE, "no gfx950 device visible");
  hipStream_t st = (hipStream_t)stream;
  const size_t count = (size_t)(pl.B * n_samples);
  HIP_TRY(hipMemsetAsync(out_index, 0xFF, count * sizeof(int64_t), st)); // -1: a target no block claimed
  HIP_TRY(hipMemsetAsync(out_prob, 0, count * sizeof(double), st));
  ArtnSampleBatchArgs g = {};
  g.B = pl.B, g.S = n_samples, g.n = pl.n;
  g.local_bits = pl.local_bits, g.block_bits = pl.block_bits, g.row_bits = pl.row_bits, g.f = pl.fields;
  if (d->dtype == ARTN_C64)
    sample_batch_launch(pl, (const float2 *)a, g, uniforms_sorted, (long long *)out_index, out_prob, out_norm, (double *)ws, st);
  else
    sample_batch_launch(pl, (const double2 *)a, g, uniforms_sorted, (long long *)out_index, out_prob, out_norm, (double *)ws, st);
  HIP_TRY(hipGetLastError());
  return ARTN_OK;
}

} // extern "C"
