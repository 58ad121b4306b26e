// artn_krylov.hip -- host half of the Krylov vector algebra of include/artn.h (kernels: artn_krylov_kernel.h).
//
// A translation unit of its own (build/obj/krylov.o).
#include <hip/hip_runtime.h>
#include <math.h>
#include <string>

#include "artn_host.h"
#include "artn_krylov_kernel.h"

static_assert(ARTN_KRYLOV_BATCH >= 2 && ARTN_KRYLOV_BATCH <= 16 && ARTN_KRYLOV_BATCH % 2 == 0, "groups of four partials hold two vectors");
static_assert(sizeof(ArtnKrylovCombineArgs) == ARTN_KRYLOV_MAX_VECS * 24, "pointers and coefficients by value");

static int krylov_plan(int64_t n, int32_t dtype, int32_t m, ArtnKrylovInfo *info) {
  if (!info) return fail(ARTN_E_INVALID, "null info");
  if (m < 1) return fail(ARTN_E_INVALID, "at least one vector is needed");
  ArtnBornPlan bp;
  if (int rc = artn_born_plan(n, dtype, &bp)) return rc; // (element count, dtype; the grid of artn_born_overlap)
  const int64_t elem = dtype == ARTN_C64 ? 8 : 16, groups = (m + 1) / 2 + 1;
  ArtnKrylovInfo out = {};
  out.grid = bp.overlap_grid;
  out.batch = ARTN_KRYLOV_BATCH;
  out.dots_launches = (m + ARTN_KRYLOV_BATCH - 1) / ARTN_KRYLOV_BATCH;
  out.combine_launches = 1;
  out.dots_workspace_bytes = groups * bp.overlap_grid * 4 * (int64_t)sizeof(double);
  out.combine_workspace_bytes = (int64_t)bp.overlap_grid * (int64_t)sizeof(double);
  out.dots_bytes_read = ((int64_t)m + out.dots_launches) * n * elem; // every V_j once, w once per launch
  out.combine_bytes_read = (int64_t)m * n * elem;
  out.combine_bytes_written = n * elem;
  *info = out;
  return ARTN_OK;
}

template <typename T, int NB>
static void krylov_dots_launch(int nb, const ArtnKrylovDotsArgs &args, const T *w, long n, int first, double *part, double *part_w,
                               unsigned grid, hipStream_t st) {
  if constexpr (NB > 0) {
    if (nb == NB)
      hipLaunchKernelGGL((artn_k_krylov_dots<T, NB>), dim3(grid), dim3(ARTN_BORN_THREADS), 0, st, args, w, n, first, part, part_w);
    else
      krylov_dots_launch<T, NB - 1>(nb, args, w, n, first, part, part_w, grid, st);
  }
}

extern "C" {

int artn_krylov_query(int64_t n, int32_t dtype, int32_t m, ArtnKrylovInfo *info) { return krylov_plan(n, dtype, m, info); }

int artn_krylov_dots(const void *const *vecs, int32_t m, const void *w, int64_t n, int32_t dtype, void *ws, int64_t ws_bytes,
                     double *out, void *stream) {
  if (artn_device_count() < 1) return fail(ARTN_E_NODEVICE, "no gfx950 device visible");
  ArtnKrylovInfo p;
  if (int rc = krylov_plan(n, dtype, m, &p)) return rc;
  if (!vecs || !w || !ws || !out) return fail(ARTN_E_INVALID, "null pointer");
  if (ws_bytes < p.dots_workspace_bytes) return fail(ARTN_E_INVALID, "workspace smaller than artn_krylov_query reports");
  uintptr_t bits = (uintptr_t)w;
  for (int j = 0; j < m; ++j) {
    if (!vecs[j]) return fail(ARTN_E_INVALID, "null pointer (vector " + std::to_string(j) + ")");
    bits |= (uintptr_t)vecs[j];
  }
  if (bits & 15) return fail(ARTN_E_UNSUPPORTED, "artn_krylov_dots needs 16-byte aligned arrays");
  hipStream_t st = (hipStream_t)stream;
  double *part = (double *)ws, *part_w = part + (int64_t)((m + 1) / 2) * p.grid * 4;
  for (int j0 = 0; j0 < m; j0 += ARTN_KRYLOV_BATCH) {
    const int nb = m - j0 < ARTN_KRYLOV_BATCH ? m - j0 : ARTN_KRYLOV_BATCH;
    ArtnKrylovDotsArgs args = {};
    for (int j = 0; j < nb; ++j) args.v[j] = vecs[j0 + j];
    double *at = part + (int64_t)(j0 / 2) * p.grid * 4;
    if (dtype == ARTN_C64)
      krylov_dots_launch<float2, ARTN_KRYLOV_BATCH>(nb, args, (const float2 *)w, (long)n, j0 == 0, at, part_w, (unsigned)p.grid, st);
    else
      krylov_dots_launch<double2, ARTN_KRYLOV_BATCH>(nb, args, (const double2 *)w, (long)n, j0 == 0, at, part_w, (unsigned)p.grid, st);
  }
  hipLaunchKernelGGL(artn_k_krylov_dots_finish, dim3((unsigned)((m + 1) / 2 + 1)), dim3(ARTN_BORN_THREADS), 0, st, (const double *)part,
                     (int)p.grid, (int)m, out);
  HIP_TRY(hipGetLastError());
  return ARTN_OK;
}

int artn_krylov_combine(void *y, const double *coeff, const void *const *xs, int32_t m, int64_t n, int32_t dtype, void *ws,
                        int64_t ws_bytes, double *out4, void *stream) {
  if (artn_device_count() < 1) return fail(ARTN_E_NODEVICE, "no gfx950 device visible");
  ArtnKrylovInfo p;
  if (int rc = krylov_plan(n, dtype, m, &p)) return rc;
  if (m > ARTN_KRYLOV_MAX_VECS)
    return fail(ARTN_E_INVALID, "artn_krylov_combine takes at most " + std::to_string(ARTN_KRYLOV_MAX_VECS) + " vectors, got " +
                                    std::to_string(m));
  if (!y || !coeff || !xs || !ws || !out4) return fail(ARTN_E_INVALID, "null pointer");
  if (ws_bytes < p.combine_workspace_bytes) return fail(ARTN_E_INVALID, "workspace smaller than artn_krylov_query reports");
  uintptr_t bits = (uintptr_t)y;
  for (int j = 0; j < m; ++j) {
    if (!xs[j]) return fail(ARTN_E_INVALID, "null pointer (vector " + std::to_string(j) + ")");
    bits |= (uintptr_t)xs[j];
  }
  if (bits & 15) return fail(ARTN_E_UNSUPPORTED, "artn_krylov_combine needs 16-byte aligned arrays");
  const uintptr_t bytes = (uintptr_t)p.combine_bytes_written, py = (uintptr_t)y;
  ArtnKrylovCombineArgs args = {};
  int used = 0;
  for (int j = 0; j < m; ++j) {
    const uintptr_t px = (uintptr_t)xs[j];
    if (px != py && px < py + bytes && py < px + bytes)
      return fail(ARTN_E_INVALID, "artn_krylov_combine: y overlaps vector " + std::to_string(j) + " without being it");
    const double cr = coeff[2 * j], ci = coeff[2 * j + 1];
    if (!isfinite(cr) || !isfinite(ci)) return fail(ARTN_E_INVALID, "artn_krylov_combine: coefficient " + std::to_string(j) + " is not finite");
    if (cr == 0.0 && ci == 0.0) continue; // (a term that contributes nothing is not read at all)
    args.x[used] = xs[j], args.c[used][0] = cr, args.c[used][1] = ci;
    ++used;
  }
  hipStream_t st = (hipStream_t)stream;
  dim3 grid((unsigned)p.grid), block(ARTN_BORN_THREADS);
  double *part = (double *)ws;
  if (dtype == ARTN_C64)
    hipLaunchKernelGGL(artn_k_krylov_combine<float2>, grid, block, 0, st, args, used, (float2 *)y, (long)n, part);
  else
    hipLaunchKernelGGL(artn_k_krylov_combine<double2>, grid, block, 0, st, args, used, (double2 *)y, (long)n, part);
  hipLaunchKernelGGL(artn_k_born_finish, dim3(1), block, 0, st, (const double *)part, (int)p.grid, 1, out4);
  HIP_TRY(hipGetLastError());
  return ARTN_OK;
}

} // extern "C"
