// artn_pauli.hip -- host half of the Pauli-string entry points of include/artn.h (kernels: artn_pauli_kernel.h).
//
// A translation unit of its own (build/obj/pauli.o).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <string>
#include <unordered_map>
#include <vector>

#include "artn_host.h"
#include "artn_pauli_kernel.h"

struct PauliPlan {
  int64_t n = 1;
  std::vector<uint64_t> xm, zm;
  std::vector<int32_t> ny, group;
  std::vector<std::vector<int64_t>> members; // group -> its terms, in the caller's order
  ArtnPauliInfo info = {};
};

// The layout checks of artn_marginal (dense: sorted by stride, every stride is the product of the extents below it), then every
// term's memory-bit masks and the groups of equal xmask in the order they first appear.
static int pauli_plan(const ArtnMarginalDesc *d, const uint8_t *ops, int64_t n_terms, PauliPlan &pl) {
  if (!d) return fail(ARTN_E_INVALID, "null descriptor");
  if (d->dtype != ARTN_C64 && d->dtype != ARTN_C128) return fail(ARTN_E_UNSUPPORTED, "Pauli expectations take complex64 or complex128");
  if (d->n_dims < 0) return fail(ARTN_E_INVALID, "bad number of dimensions");
  if (d->n_dims > ARTN_MARG_MAX_DIMS) return fail(ARTN_E_UNSUPPORTED, "Pauli expectations take at most 96 dimensions");
  if (n_terms < 1) return fail(ARTN_E_INVALID, "at least one Pauli string is needed");
  if (!ops) return fail(ARTN_E_INVALID, "null pointer");
  const int nd = d->n_dims;
  std::vector<int> order;
  bool pow2 = true;
  for (int i = 0; i < nd; ++i) {
    if (d->extent[i] < 1) return fail(ARTN_E_INVALID, "extent below 1");
    if (d->extent[i] == 1) continue; // (carries no index)
    if (d->stride[i] < 1) return fail(ARTN_E_INVALID, "the tensor is not dense: stride below 1");
    if (d->extent[i] & (d->extent[i] - 1)) pow2 = false;
    order.push_back(i);
  }
  std::sort(order.begin(), order.end(), [&](int x, int y) { return d->stride[x] < d->stride[y]; });
  int64_t n = 1;
  bool too_big = false;
  for (int i : order) {
    if (d->stride[i] != n) return fail(ARTN_E_INVALID, "the tensor is not dense: its strides overlap or leave gaps");
    if (d->extent[i] > ((int64_t)1 << 40) / n) {
      too_big = true;
      break;
    }
    n *= d->extent[i];
  }
  if (!pow2) return fail(ARTN_E_UNSUPPORTED, "Pauli expectations take power-of-two extents");
  if (too_big) return fail(ARTN_E_UNSUPPORTED, "Pauli expectations take at most 2^40 elements");
  pl.n = n;
  pl.xm.assign(n_terms, 0), pl.zm.assign(n_terms, 0), pl.ny.assign(n_terms, 0), pl.group.assign(n_terms, 0);
  int bit[ARTN_MARG_MAX_DIMS];
  for (int i = 0; i < nd; ++i) bit[i] = d->extent[i] == 2 ? __builtin_ctzll((uint64_t)d->stride[i]) : -1;
  std::unordered_map<uint64_t, int32_t> group_of;
  for (int64_t t = 0; t < n_terms; ++t) {
    const uint8_t *op = ops + t * nd;
    uint64_t x = 0, z = 0;
    int32_t y = 0;
    for (int i = 0; i < nd; ++i) {
      if (op[i] > 3) return fail(ARTN_E_INVALID, "term " + std::to_string(t) + ": operator code " + std::to_string(op[i]) + " (0..3 = I, X, Y, Z)");
      if (op[i] == 0) continue;
      if (bit[i] < 0)
        return fail(ARTN_E_INVALID, "term " + std::to_string(t) + ": X, Y and Z act on dimensions of extent 2; dimension " +
                                        std::to_string(i) + " has extent " + std::to_string(d->extent[i]));
      const uint64_t b = (uint64_t)1 << bit[i];
      if (op[i] != 3) x |= b;
      if (op[i] != 1) z |= b;
      if (op[i] == 2) ++y;
    }
    pl.xm[t] = x, pl.zm[t] = z, pl.ny[t] = y;
    auto it = group_of.find(x);
    if (it == group_of.end()) {
      it = group_of.emplace(x, (int32_t)pl.members.size()).first;
      pl.members.emplace_back();
    }
    pl.group[t] = it->second;
    pl.members[it->second].push_back(t);
  }
  int64_t launches = 0;
  for (const auto &m : pl.members) launches += ((int64_t)m.size() + ARTN_PAULI_TERMS - 1) / ARTN_PAULI_TERMS;
  if (pl.members.size() > (size_t)INT32_MAX || launches > INT32_MAX) return fail(ARTN_E_UNSUPPORTED, "too many Pauli strings in one call");
  const int64_t tiles = std::max<int64_t>(n >> ARTN_PAULI_TILE_BITS, 1);
  pl.info.n_groups = (int32_t)pl.members.size();
  pl.info.n_launches = (int32_t)launches;
  pl.info.terms_per_launch = ARTN_PAULI_TERMS;
  pl.info.workspace_bytes = std::min<int64_t>(tiles, ARTN_BORN_MAX_GRID) * (ARTN_PAULI_TERMS + 1) * (int64_t)sizeof(double);
  pl.info.bytes_read = launches * n * (d->dtype == ARTN_C64 ? 8 : 16);
  return ARTN_OK;
}

template <typename T, int FORM>
static void pauli_launch_form(int nt, dim3 grid, hipStream_t st, const T *a, long tiles, const ArtnPauliArgs &p, double *part) {
  const dim3 block(ARTN_BORN_THREADS);
  if (nt <= 1) hipLaunchKernelGGL((artn_k_pauli<T, FORM, 1>), grid, block, 0, st, a, tiles, p, part);
  else if (nt <= 4) hipLaunchKernelGGL((artn_k_pauli<T, FORM, 4>), grid, block, 0, st, a, tiles, p, part);
  else hipLaunchKernelGGL((artn_k_pauli<T, FORM, ARTN_PAULI_TERMS>), grid, block, 0, st, a, tiles, p, part);
}

// one launch of the terms m[first .. first + p.nt) of a group, and its finish
template <typename T>
static void pauli_launch(const PauliPlan &pl, const T *a, ArtnPauliArgs &p, const ArtnPauliFinish &f, double *part, double *out, hipStream_t st) {
  const uint64_t in = ((uint64_t)1 << ARTN_PAULI_TILE_BITS) - 1;
  int n_partial = 1, nv = ARTN_PAULI_TERMS + 1;
  if (pl.n <= (int64_t)in) {
    hipLaunchKernelGGL(artn_k_pauli_small<T>, dim3(1), dim3(ARTN_BORN_THREADS), 0, st, a, (long)pl.n, p, part);
  } else {
    const int form = p.xm == 0 ? 0 : (p.xm & ~in) == 0 ? 1 : 2;
    const long tiles = (long)(pl.n >> ARTN_PAULI_TILE_BITS) >> (form == 2 ? 1 : 0);
    const dim3 grid((unsigned)std::min<long>(tiles, ARTN_BORN_MAX_GRID));
    if (form == 0) pauli_launch_form<T, 0>(p.nt, grid, st, a, tiles, p, part);
    else if (form == 1) pauli_launch_form<T, 1>(p.nt, grid, st, a, tiles, p, part);
    else pauli_launch_form<T, 2>(p.nt, grid, st, a, tiles, p, part);
    n_partial = (int)grid.x;
    nv = (p.nt <= 1 ? 1 : p.nt <= 4 ? 4 : ARTN_PAULI_TERMS) + 1;
  }
  hipLaunchKernelGGL(artn_k_pauli_finish, dim3(1), dim3(64), 0, st, (const double *)part, n_partial, nv, f, out);
}

extern "C" {

int artn_pauli_query(const ArtnMarginalDesc *d, const uint8_t *ops, int64_t n_terms, ArtnPauliInfo *info, uint64_t *xmask,
                     uint64_t *zmask, int32_t *n_y, int32_t *group) {
  if (!info) return fail(ARTN_E_INVALID, "null info");
  PauliPlan pl;
  if (int rc = pauli_plan(d, ops, n_terms, pl)) return rc;
  *info = pl.info;
  if (xmask) std::copy(pl.xm.begin(), pl.xm.end(), xmask);
  if (zmask) std::copy(pl.zm.begin(), pl.zm.end(), zmask);
  if (n_y) std::copy(pl.ny.begin(), pl.ny.end(), n_y);
  if (group) std::copy(pl.group.begin(), pl.group.end(), group);
  return ARTN_OK;
}

int artn_pauli_expect(const ArtnMarginalDesc *d, const void *a, const uint8_t *ops, int64_t n_terms, double *out, void *ws,
                      int64_t ws_bytes, void *stream) {
  if (artn_device_count() < 1) return fail(ARTN_E_NODEVICE, "no gfx950 device visible");
  PauliPlan pl;
  if (int rc = pauli_plan(d, ops, n_terms, pl)) return rc;
  if (!a || !out || !ws) return fail(ARTN_E_INVALID, "null pointer");
  if (ws_bytes < pl.info.workspace_bytes) return fail(ARTN_E_INVALID, "workspace smaller than artn_pauli_query reports");
  if (((uintptr_t)a & 15) != 0) return fail(ARTN_E_UNSUPPORTED, "artn_pauli_expect needs a 16-byte aligned array");
  if ((((uintptr_t)out | (uintptr_t)ws) & 7) != 0) return fail(ARTN_E_UNSUPPORTED, "artn_pauli_expect needs 8-byte aligned output and workspace");
  hipStream_t st = (hipStream_t)stream;
  const bool pair_form = pl.n >= ((int64_t)1 << ARTN_PAULI_TILE_BITS);
  bool first = true;
  for (const auto &m : pl.members) {
    const uint64_t xm = pl.xm[m[0]];
    const bool halved = pair_form && (xm >> ARTN_PAULI_TILE_BITS) != 0; // FORM 2: half the index space, weight 2
    for (size_t at = 0; at < m.size(); at += ARTN_PAULI_TERMS) {
      ArtnPauliArgs p = {};
      ArtnPauliFinish f = {};
      p.xm = xm;
      p.nt = f.nt = (int32_t)std::min<size_t>(ARTN_PAULI_TERMS, m.size() - at);
      p.hbit = xm ? 63 - __builtin_clzll(xm) : 0;
      p.norm = first;
      f.norm_index = first ? n_terms : -1;
      for (int t = 0; t < p.nt; ++t) {
        const int64_t term = m[at + t];
        const int32_t ny = pl.ny[term];
        p.zm[t] = pl.zm[term];
        p.sel[t] = (uint8_t)((pl.zm[term] & 3) | (uint64_t)((ny & 1) << 2));
        f.out_index[t] = term;
        f.scale[t] = (int8_t)(((ny & 3) == 1 || (ny & 3) == 2 ? -1 : 1) * (halved ? 2 : 1));
      }
      if (d->dtype == ARTN_C64) pauli_launch(pl, (const float2 *)a, p, f, (double *)ws, out, st);
      else pauli_launch(pl, (const double2 *)a, p, f, (double *)ws, out, st);
      first = false;
    }
  }
  HIP_TRY(hipGetLastError());
  return ARTN_OK;
}

} // extern "C"
