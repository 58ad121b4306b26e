// artn_born.hip -- host half of the Born-statistics entry points of include/artn.h (kernels: artn_born_kernel.h).
//
// A translation unit of its own (build/obj/born.o).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <string>
#include <vector>

#include "artn_host.h"
#include "artn_state_host.h"
#include "artn_born_kernel.h"

static int born_plan(int64_t n, int32_t dtype, ArtnBornPlan *p) {
  if (!p) return fail(ARTN_E_INVALID, "null plan");
  if (n < 1 || n > ((int64_t)1 << 40)) return fail(ARTN_E_INVALID, "element count out of range");
  if (dtype != ARTN_C64 && dtype != ARTN_C128) return fail(ARTN_E_UNSUPPORTED, "Born statistics take complex64 or complex128");
  p->block_bits = std::min(ARTN_BORN_MAX_BLOCK_BITS, std::max(ARTN_BORN_MIN_BLOCK_BITS, state_ceil_log2(n) - 16));
  p->n_blocks = (n + ((int64_t)1 << p->block_bits) - 1) >> p->block_bits;
  const int64_t tiles = (n + 4 * ARTN_BORN_THREADS - 1) / (4 * ARTN_BORN_THREADS);
  p->overlap_grid = (int32_t)std::min<int64_t>(tiles, ARTN_BORN_MAX_GRID);
  p->workspace_bytes = (int64_t)p->overlap_grid * 4 * (int64_t)sizeof(double);
  return ARTN_OK;
}

// (the layout checks: artn_state_host.h)
static int marg_plan(const ArtnMarginalDesc *d, ArtnMarginalInfo *info, ArtnMargStream *sp, ArtnMargGeneric *gp) {
  if (int rc = state_desc(d, "marginals take", ARTN_MARG_MAX_DIMS, true)) return rc;
  StateLayout l;
  if (int rc = state_layout(d, l)) return rc;
  if (l.too_big) return fail(ARTN_E_INVALID, "element count out of range");
  const int64_t n = l.n;
  const bool pow2 = l.pow2;
  int64_t n_out = 1;
  for (int i : l.order)
    if (d->keep[i]) n_out *= d->extent[i];
  ArtnMarginalInfo out = {};
  out.out_elems = n_out;
  const int nbits = state_ceil_log2(n), kept_bits = state_ceil_log2(n_out);
  if (pow2 && nbits >= ARTN_MARG_CHUNK_BITS && kept_bits <= ARTN_MARG_MAX_KEPT_BITS) {
    ArtnMargStream s = {};
    // memory bits of every dimension; output bits: kept dimensions in listed order, the last one fastest
    uint64_t kmask = 0;
    int out_of_mem_bit[64];
    int ob = 0;
    for (int i = d->n_dims - 1; i >= 0; --i) {
      if (d->extent[i] == 1 || !d->keep[i]) continue;
      const int e = state_ceil_log2(d->extent[i]), s0 = state_ceil_log2(d->stride[i]);
      for (int b = 0; b < e; ++b) {
        kmask |= (uint64_t)1 << (s0 + b);
        out_of_mem_bit[s0 + b] = ob++;
      }
    }
    int x = 0;
    for (int b = 0; b < nbits; ++b)
      if (kmask >> b & 1) s.out_bit[x++] = (uint8_t)out_of_mem_bit[b];
    const uint64_t all = ((uint64_t)1 << nbits) - 1, in = ((uint64_t)1 << ARTN_MARG_CHUNK_BITS) - 1;
    s.kept_bits = kept_bits;
    s.kmask_in = kmask & in, s.dmask_in = ~kmask & in;
    s.kmask_above = (kmask & all) >> ARTN_MARG_CHUNK_BITS, s.dmask_above = (~kmask & all) >> ARTN_MARG_CHUNK_BITS;
    s.bin_bits = __builtin_popcountll(s.kmask_in);
    s.above_bits = __builtin_popcountll(s.kmask_above);
    s.drop_above_bits = __builtin_popcountll(s.dmask_above);
    s.group_bits = std::min(s.drop_above_bits, std::max(0, 11 - s.above_bits));
    s.item_mask = s.kmask_in;
    uint64_t rest = s.dmask_in;
    for (int have = s.bin_bits; have < 8; ++have) { // spread the lowest dropped bits over the 256 threads
      const uint64_t low = rest & (~rest + 1);
      s.item_mask |= low, rest ^= low;
    }
    s.rest_mask = rest;
    out.kernel = ARTN_MARGINAL_STREAM;
    out.chunk_bits = ARTN_MARG_CHUNK_BITS;
    out.bin_bits = s.bin_bits;
    out.grid = 1 << (s.above_bits + s.group_bits);
    out.workspace_bytes = ((int64_t)out.grid << s.bin_bits) * (int64_t)sizeof(double);
    if (sp) *sp = s;
  } else {
    if (pow2 && nbits >= ARTN_MARG_CHUNK_BITS)
      return fail(ARTN_E_UNSUPPORTED, "the streaming marginal kernel keeps at most 2^24 elements; this one keeps 2^" +
                                          std::to_string(kept_bits));
    ArtnMargGeneric g = {};
    for (int i = 0; i < d->n_dims; ++i)
      if (d->extent[i] > 1 && d->keep[i]) g.extent[g.n_keep] = d->extent[i], g.stride[g.n_keep] = d->stride[i], ++g.n_keep;
    for (int i = 0; i < d->n_dims; ++i)
      if (d->extent[i] > 1 && !d->keep[i])
        g.extent[g.n_keep + g.n_drop] = d->extent[i], g.stride[g.n_keep + g.n_drop] = d->stride[i], ++g.n_drop;
    out.kernel = ARTN_MARGINAL_GENERIC;
    out.grid = (int32_t)std::min<int64_t>((n_out + ARTN_BORN_THREADS - 1) / ARTN_BORN_THREADS, (int64_t)1 << 30);
    out.workspace_bytes = 0;
    if (gp) *gp = g;
  }
  if (info) *info = out;
  return ARTN_OK;
}

extern "C" {

int artn_born_plan(int64_t n, int32_t dtype, ArtnBornPlan *plan) { return born_plan(n, dtype, plan); }

int artn_born_overlap(const void *a, const void *b, int64_t n, int32_t dtype, void *ws, int64_t ws_bytes, double *out4,
                      void *stream) {
  if (artn_device_count() < 1) return fail(ARTN_E_NODEVICE, "no gfx950 device visible");
  ArtnBornPlan p;
  if (int rc = born_plan(n, dtype, &p)) return rc;
  if (!a || !ws || !out4) return fail(ARTN_E_INVALID, "null pointer");
  if (ws_bytes < p.workspace_bytes) return fail(ARTN_E_INVALID, "workspace smaller than artn_born_plan reports");
  if ((((uintptr_t)a | (uintptr_t)b) & 15) != 0) return fail(ARTN_E_UNSUPPORTED, "artn_born_overlap needs 16-byte aligned arrays");
  const bool pair = b && b != a;
  hipStream_t st = (hipStream_t)stream;
  dim3 grid((unsigned)p.overlap_grid), block(ARTN_BORN_THREADS);
  double *part = (double *)ws;
  if (dtype == ARTN_C64) {
    if (pair) hipLaunchKernelGGL((artn_k_born_overlap<float2, true>), grid, block, 0, st, (const float2 *)a, (const float2 *)b, (long)n, part);
    else hipLaunchKernelGGL((artn_k_born_overlap<float2, false>), grid, block, 0, st, (const float2 *)a, (const float2 *)a, (long)n, part);
  } else {
    if (pair) hipLaunchKernelGGL((artn_k_born_overlap<double2, true>), grid, block, 0, st, (const double2 *)a, (const double2 *)b, (long)n, part);
    else hipLaunchKernelGGL((artn_k_born_overlap<double2, false>), grid, block, 0, st, (const double2 *)a, (const double2 *)a, (long)n, part);
  }
  hipLaunchKernelGGL(artn_k_born_finish, dim3(1), block, 0, st, (const double *)part, (int)p.overlap_grid, pair ? 4 : 1, out4);
  HIP_TRY(hipGetLastError());
  return ARTN_OK;
}

int artn_born_block_sums(const void *a, int64_t n, int32_t dtype, double *block_sum, double *prefix, void *stream) {
  if (artn_device_count() < 1) return fail(ARTN_E_NODEVICE, "no gfx950 device visible");
  ArtnBornPlan p;
  if (int rc = born_plan(n, dtype, &p)) return rc;
  if (!a || !block_sum) return fail(ARTN_E_INVALID, "null pointer");
  if (((uintptr_t)a & 15) != 0) return fail(ARTN_E_UNSUPPORTED, "artn_born_block_sums needs a 16-byte aligned array");
  hipStream_t st = (hipStream_t)stream;
  dim3 grid((unsigned)p.n_blocks), block(ARTN_BORN_THREADS);
  if (dtype == ARTN_C64)
    hipLaunchKernelGGL(artn_k_born_block_sums<float2>, grid, block, 0, st, (const float2 *)a, (long)n, (int)p.block_bits, block_sum);
  else
    hipLaunchKernelGGL(artn_k_born_block_sums<double2>, grid, block, 0, st, (const double2 *)a, (long)n, (int)p.block_bits, block_sum);
  if (prefix)
    hipLaunchKernelGGL(artn_k_born_prefix, dim3(1), dim3(ARTN_BORN_PREFIX_THREADS), 0, st, (const double *)block_sum, prefix,
                       (long)p.n_blocks);
  HIP_TRY(hipGetLastError());
  return ARTN_OK;
}

int artn_born_pick(const void *a, int64_t n, int32_t dtype, const double *prefix, const double *targets, int64_t m,
                   int64_t *out_index, double *out_prob, void *stream) {
  if (artn_device_count() < 1) return fail(ARTN_E_NODEVICE, "no gfx950 device visible");
  ArtnBornPlan p;
  if (int rc = born_plan(n, dtype, &p)) return rc;
  if (m < 0) return fail(ARTN_E_INVALID, "negative sample count");
  if (m == 0) return ARTN_OK;
  if (!a || !prefix || !targets || !out_index || !out_prob) return fail(ARTN_E_INVALID, "null pointer");
  if (((uintptr_t)a & 15) != 0) return fail(ARTN_E_UNSUPPORTED, "artn_born_pick needs a 16-byte aligned array");
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(hipMemsetAsync(out_index, 0xFF, (size_t)m * sizeof(int64_t), st)); // -1: a target no block claimed (all-zero input)
  HIP_TRY(hipMemsetAsync(out_prob, 0, (size_t)m * sizeof(double), st));
  dim3 grid((unsigned)p.n_blocks), block(ARTN_BORN_THREADS);
  if (dtype == ARTN_C64)
    hipLaunchKernelGGL(artn_k_born_pick<float2>, grid, block, 0, st, (const float2 *)a, (long)n, (int)p.block_bits, (long)p.n_blocks,
                       prefix, targets, (long)m, (long long *)out_index, out_prob);
  else
    hipLaunchKernelGGL(artn_k_born_pick<double2>, grid, block, 0, st, (const double2 *)a, (long)n, (int)p.block_bits, (long)p.n_blocks,
                       prefix, targets, (long)m, (long long *)out_index, out_prob);
  HIP_TRY(hipGetLastError());
  return ARTN_OK;
}

int artn_marginal_query(const ArtnMarginalDesc *d, ArtnMarginalInfo *info) {
  if (!info) return fail(ARTN_E_INVALID, "null info");
  return marg_plan(d, info, nullptr, nullptr);
}

int artn_marginal(const ArtnMarginalDesc *d, const void *a, double *out, void *ws, int64_t ws_bytes, void *stream) {
  if (artn_device_count() < 1) return fail(ARTN_E_NODEVICE, "no gfx950 device visible");
  ArtnMarginalInfo info;
  ArtnMargStream s;
  ArtnMargGeneric g;
  if (int rc = marg_plan(d, &info, &s, &g)) return rc;
  if (!a || !out) return fail(ARTN_E_INVALID, "null pointer");
  hipStream_t st = (hipStream_t)stream;
  dim3 block(ARTN_BORN_THREADS);
  if (info.kernel == ARTN_MARGINAL_STREAM) {
    if (!ws || ws_bytes < info.workspace_bytes) return fail(ARTN_E_INVALID, "workspace smaller than artn_marginal_query reports");
    if (((uintptr_t)a & 15) != 0) return fail(ARTN_E_UNSUPPORTED, "artn_marginal needs a 16-byte aligned array");
    if (d->dtype == ARTN_C64)
      hipLaunchKernelGGL(artn_k_marginal_stream<float2>, dim3((unsigned)info.grid), block, 0, st, (const float2 *)a, s, (double *)ws);
    else
      hipLaunchKernelGGL(artn_k_marginal_stream<double2>, dim3((unsigned)info.grid), block, 0, st, (const double2 *)a, s, (double *)ws);
    const unsigned fin = (unsigned)((info.out_elems + ARTN_BORN_THREADS - 1) / ARTN_BORN_THREADS);
    hipLaunchKernelGGL(artn_k_marginal_finish, dim3(fin), block, 0, st, (const double *)ws, s, out);
  } else {
    int64_t n_sum = 1;
    for (int i = g.n_keep; i < g.n_keep + g.n_drop; ++i) n_sum *= g.extent[i];
    if ((info.out_elems + ARTN_BORN_THREADS - 1) / ARTN_BORN_THREADS > ((int64_t)1 << 30)) return fail(ARTN_E_UNSUPPORTED, "too many workgroups");
    if (d->dtype == ARTN_C64)
      hipLaunchKernelGGL(artn_k_marginal_generic<float2>, dim3((unsigned)info.grid), block, 0, st, (const float2 *)a, g, (long)info.out_elems,
                         (long)n_sum, out);
    else
      hipLaunchKernelGGL(artn_k_marginal_generic<double2>, dim3((unsigned)info.grid), block, 0, st, (const double2 *)a, g, (long)info.out_elems,
                         (long)n_sum, out);
  }
  HIP_TRY(hipGetLastError());
  return ARTN_OK;
}

} // extern "C"
