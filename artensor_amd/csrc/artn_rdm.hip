// artn_rdm.hip -- host half of the reduced-density-matrix entry points of include/artn.h (kernels: artn_rdm_kernel.h).
//
// A translation unit of its own (build/obj/rdm.o).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <string>
#include <vector>

#include "artn_host.h"
#include "artn_state_host.h"
#include "artn_rdm_kernel.h"

// The layout checks of artn_marginal (artn_state_host.h), then the form.
static int rdm_plan(const ArtnMarginalDesc *d, ArtnRdmInfo *info, ArtnRdmStream *sp, ArtnRdmGeneric *gp, int64_t *n_sum) {
  if (int rc = state_desc(d, "reduced density matrices take", ARTN_RDM_MAX_DIMS, true)) return rc;
  StateLayout l;
  if (int rc = state_layout(d, l)) return rc;
  if (l.too_big) return fail(ARTN_E_INVALID, "element count out of range");
  const int64_t n = l.n;
  const bool pow2 = l.pow2;
  int64_t D = 1;
  for (int i : l.order)
    if (d->keep[i]) D *= d->extent[i];
  if (D > ((int64_t)1 << ARTN_RDM_MAX_DIM_BITS))
    return fail(ARTN_E_UNSUPPORTED, "reduced density matrices keep at most 1024 states; this one keeps " + std::to_string(D));
  ArtnRdmInfo out = {};
  out.dim = D;
  const int nbits = state_ceil_log2(n), k = state_ceil_log2(D);
  const int rowb = std::max(k, 4), trb = std::min(rowb, 6), cb = ARTN_RDM_PANEL_BITS - trb;
  if (pow2 && nbits >= ARTN_RDM_MIN_BITS && D >= 2 && nbits - rowb >= cb) {
    ArtnRdmStream s = {};
    // memory bits of the kept dimensions; output row bits: kept dimensions in listed order, the last one fastest
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
    // group bits: the highest dropped bits, until there are four row bits
    uint64_t gmask = 0;
    s.group_bits = rowb - k;
    for (int b = nbits - 1, need = s.group_bits; need > 0; --b)
      if (!(kmask >> b & 1)) gmask |= (uint64_t)1 << b, --need;
    const uint64_t all = ((uint64_t)1 << nbits) - 1, rmask = kmask | gmask;
    for (int b = 0, x = 0, y = 0; b < nbits; ++b) {
      if (!(rmask >> b & 1)) continue;
      if (kmask >> b & 1) s.row_pos[out_of_mem_bit[b]] = (uint8_t)x;
      else s.grp_pos[y++] = (uint8_t)x;
      ++x;
    }
    s.row_mask = rdm_pdep(((uint64_t)1 << trb) - 1, rmask);
    s.tile_mask = rmask & ~s.row_mask;
    s.col_mask = rdm_pdep(((uint64_t)1 << cb) - 1, ~rmask & all);
    s.drop_mask = ~rmask & all & ~s.col_mask;
    s.row_bits = trb, s.col_bits = cb, s.tile_bits = rowb - trb, s.drop_bits = nbits - rowb - cb;
    s.kept_bits = k;
    const int64_t T = (int64_t)1 << s.tile_bits, tiles = T * (T + 1) / 2;
    while (s.split_bits < s.drop_bits && (tiles << s.split_bits) < ARTN_RDM_TARGET_WGS) ++s.split_bits;
    out.kernel = ARTN_RDM_STREAM;
    out.panel_bits = cb;
    out.tiles = (int32_t)tiles;
    out.splits = 1 << s.split_bits;
    out.workspace_bytes = (tiles << s.split_bits) * (((int64_t)1 << (2 * trb)) * 16);
    // one MFMA (2048 FLOP) per block and column of a panel: re and im on two columns each
    const int64_t diag_blocks = trb == 4 ? 1 : trb == 5 ? 3 : 10, blocks = T * diag_blocks + (tiles - T) * 16;
    out.flops = 2048.0 * (double)blocks * (double)((int64_t)1 << (s.drop_bits + cb));
    if (sp) *sp = s;
  } else {
    ArtnRdmGeneric g = {};
    int64_t ns = 1;
    for (int i = 0; i < d->n_dims; ++i)
      if (d->extent[i] > 1 && d->keep[i]) g.extent[g.n_keep] = d->extent[i], g.stride[g.n_keep] = d->stride[i], ++g.n_keep;
    for (int i = 0; i < d->n_dims; ++i)
      if (d->extent[i] > 1 && !d->keep[i])
        g.extent[g.n_keep + g.n_drop] = d->extent[i], g.stride[g.n_keep + g.n_drop] = d->stride[i], ++g.n_drop, ns *= d->extent[i];
    out.kernel = ARTN_RDM_GENERIC;
    if (gp) *gp = g;
    if (n_sum) *n_sum = ns;
  }
  if (info) *info = out;
  return ARTN_OK;
}

template <typename T> static void rdm_launch_stream(const ArtnRdmStream &s, const ArtnRdmInfo &info, const T *a, double *ws, hipStream_t st) {
  const dim3 grid((unsigned)(info.tiles * info.splits)), block(ARTN_RDM_THREADS);
  if (s.row_bits == 4) hipLaunchKernelGGL((artn_k_rdm_stream<T, 4>), grid, block, 0, st, a, s, ws);
  else if (s.row_bits == 5) hipLaunchKernelGGL((artn_k_rdm_stream<T, 5>), grid, block, 0, st, a, s, ws);
  else hipLaunchKernelGGL((artn_k_rdm_stream<T, 6>), grid, block, 0, st, a, s, ws);
}

extern "C" {

int artn_rdm_query(const ArtnMarginalDesc *d, ArtnRdmInfo *info) {
  if (!info) return fail(ARTN_E_INVALID, "null info");
  return rdm_plan(d, info, nullptr, nullptr, nullptr);
}

int artn_rdm_row_offsets(const ArtnMarginalDesc *d, int64_t *offset) {
  ArtnRdmInfo info;
  ArtnRdmStream s;
  ArtnRdmGeneric g;
  if (int rc = rdm_plan(d, &info, &s, &g, nullptr)) return rc;
  if (!offset) return fail(ARTN_E_INVALID, "null pointer");
  for (int64_t i = 0; i < info.dim; ++i) {
    int64_t at = 0;
    if (info.kernel == ARTN_RDM_STREAM) { // what artn_k_rdm_finish and rdm_tile do with row i (group 0)
      uint64_t packed = 0;
      for (int x = 0; x < s.kept_bits; ++x) packed |= (uint64_t)((i >> x) & 1) << s.row_pos[x];
      at = (int64_t)(rdm_pdep(packed & (((uint64_t)1 << s.row_bits) - 1), s.row_mask) | rdm_pdep(packed >> s.row_bits, s.tile_mask));
    } else { // what artn_k_rdm_generic does
      int64_t rem = i;
      for (int k = g.n_keep - 1; k >= 0; --k) at += (rem % g.extent[k]) * g.stride[k], rem /= g.extent[k];
    }
    offset[i] = at;
  }
  return ARTN_OK;
}

int artn_rdm(const ArtnMarginalDesc *d, const void *a, double *out, void *ws, int64_t ws_bytes, void *stream) {
  if (artn_device_count() < 1) return fail(ARTN_E_NODEVICE, "no gfx950 device visible");
  ArtnRdmInfo info;
  ArtnRdmStream s;
  ArtnRdmGeneric g;
  int64_t n_sum = 1;
  if (int rc = rdm_plan(d, &info, &s, &g, &n_sum)) return rc;
  if (!a || !out) return fail(ARTN_E_INVALID, "null pointer");
  if (((uintptr_t)a & 15) != 0) return fail(ARTN_E_UNSUPPORTED, "artn_rdm needs a 16-byte aligned array");
  if (((uintptr_t)out & 15) != 0) return fail(ARTN_E_UNSUPPORTED, "artn_rdm needs a 16-byte aligned output");
  hipStream_t st = (hipStream_t)stream;
  if (info.kernel == ARTN_RDM_STREAM) {
    if (!ws || ws_bytes < info.workspace_bytes) return fail(ARTN_E_INVALID, "workspace smaller than artn_rdm_query reports");
    if (((uintptr_t)ws & 15) != 0) return fail(ARTN_E_UNSUPPORTED, "artn_rdm needs a 16-byte aligned workspace");
    if (d->dtype == ARTN_C64) rdm_launch_stream(s, info, (const float2 *)a, (double *)ws, st);
    else rdm_launch_stream(s, info, (const double2 *)a, (double *)ws, st);
    const unsigned fin = (unsigned)((info.dim * info.dim + ARTN_RDM_THREADS - 1) / ARTN_RDM_THREADS);
    hipLaunchKernelGGL(artn_k_rdm_finish, dim3(fin), dim3(ARTN_RDM_THREADS), 0, st, (const double *)ws, s, out);
  } else {
    const dim3 grid((unsigned)info.dim, (unsigned)info.dim), block(ARTN_RDM_THREADS);
    if (d->dtype == ARTN_C64)
      hipLaunchKernelGGL(artn_k_rdm_generic<float2>, grid, block, 0, st, (const float2 *)a, g, (long)info.dim, (long)n_sum, out);
    else
      hipLaunchKernelGGL(artn_k_rdm_generic<double2>, grid, block, 0, st, (const double2 *)a, g, (long)info.dim, (long)n_sum, out);
  }
  HIP_TRY(hipGetLastError());
  return ARTN_OK;
}

} // extern "C"
