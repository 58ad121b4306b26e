// artn_pauli_batch.hip -- host half of artn_pauli_batch_query / artn_pauli_batch_expect of include/artn.h: Pauli expectation
// values per trajectory of a batched amplitude array (kernels: artn_pauli_batch_kernel.h).
//
// A translation unit of its own (build/obj/pauli_batch.o).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <numeric>
#include <string>
#include <unordered_map>
#include <vector>

#include "artn_host.h"
#include "artn_state_host.h"
#include "artn_pauli_batch_kernel.h"

struct PauliBatchPlan {
  int64_t n = 1, B = 1, tiles = 1; // elements of the tensor, trajectories, local tiles of a trajectory
  int n_bits = 0, batch_bits = 0, local_bits = 0;
  std::vector<uint64_t> xm, zm, xl, zl;
  std::vector<int32_t> ny, group;
  std::vector<std::vector<int64_t>> members; // group -> its terms, in the caller's order
  ArtnBatchFields fields = {};               // ascending by shift (what the kernels deposit through)
  ArtnPauliBatchInfo info = {};
};

// the bits of v under `keep`, packed (the local mask of a global one)
static uint64_t pauli_batch_compress(uint64_t v, uint64_t keep) {
  uint64_t out = 0;
  for (int b = 0, j = 0; b < 64; ++b)
    if ((keep >> b) & 1) out |= ((v >> b) & 1) << j++;
  return out;
}

// The checks of pauli_plan in this family's wording, the batch dimensions (what is wrong with them, a string that acts on one
// included, before what the layout does not support), the masks, the groups and the work split.
static int pauli_batch_plan(const ArtnMarginalDesc *d, const uint8_t *ops, int64_t n_terms, int32_t nb, const int32_t *batch_dims,
                            PauliBatchPlan &pl) {
  const char *who = "batched Pauli expectations take";
  if (int rc = state_desc(d, who, ARTN_MARG_MAX_DIMS, false)) return rc;
  if (n_terms < 1) return fail(ARTN_E_INVALID, "at least one Pauli string is needed");
  if (!ops || (nb > 0 && !batch_dims)) return fail(ARTN_E_INVALID, "null pointer");
  if (nb < 0) return fail(ARTN_E_INVALID, "a negative number of batch dimensions: " + std::to_string(nb));
  const int nd = d->n_dims;
  StateLayout l;
  if (int rc = state_layout(d, l)) return rc;
  if (int rc = state_bits_only(l, who)) return rc;
  const int64_t n = pl.n = l.n;
  pl.n_bits = __builtin_ctzll((uint64_t)n);
  pl.xm.assign(n_terms, 0), pl.zm.assign(n_terms, 0), pl.ny.assign(n_terms, 0), pl.group.assign(n_terms, 0);
  int bit[ARTN_MARG_MAX_DIMS];
  state_dim_bits(d, bit);
  std::unordered_map<uint64_t, int32_t> group_of;
  for (int64_t t = 0; t < n_terms; ++t) {
    uint64_t x = 0, z = 0;
    int32_t y = 0;
    if (int rc = state_string_masks(d, bit, ops + t * nd, t, x, z, y)) return rc;
    pl.xm[t] = x, pl.zm[t] = z, pl.ny[t] = y;
    auto it = group_of.find(x);
    if (it == group_of.end()) {
      it = group_of.emplace(x, (int32_t)pl.members.size()).first;
      pl.members.emplace_back();
    }
    pl.group[t] = it->second;
    pl.members[it->second].push_back(t);
  }
  for (int i = 0; i < nb; ++i) { // (an entry out of range is state_batch_dims' to refuse)
    const int32_t dim = batch_dims[i];
    if (dim < 0 || dim >= nd) continue;
    for (int64_t t = 0; t < n_terms; ++t)
      if (ops[t * nd + dim] != 0)
        return fail(ARTN_E_INVALID, "term " + std::to_string(t) + ": strings carry I on every batch dimension; dimension " +
                                        std::to_string(dim) + " is a batch dimension");
  }
  std::vector<int32_t> seen;
  BatchDims bd;
  if (int rc = state_batch_dims(d, nb, batch_dims, seen, 0, "string", bd)) return rc;
  int64_t launches = 0;
  for (const auto &m : pl.members) launches += ((int64_t)m.size() + ARTN_PAULI_TERMS - 1) / ARTN_PAULI_TERMS;
  if (pl.members.size() > (size_t)INT32_MAX || launches > INT32_MAX) return fail(ARTN_E_UNSUPPORTED, "too many Pauli strings in one call");
  pl.batch_bits = bd.bits, pl.local_bits = pl.n_bits - bd.bits, pl.B = (int64_t)1 << bd.bits;
  if (n_terms + 1 > (((int64_t)1 << 28) >> bd.bits))
    return fail(ARTN_E_UNSUPPORTED, "B * (n_terms + 1) = " + std::to_string(pl.B) + " * " + std::to_string(n_terms + 1) +
                                        " is above 2^28 output values (2 GiB)");
  pl.xl.resize(n_terms), pl.zl.resize(n_terms);
  for (int64_t t = 0; t < n_terms; ++t)
    pl.xl[t] = pauli_batch_compress(pl.xm[t], ~bd.mask), pl.zl[t] = pauli_batch_compress(pl.zm[t], ~bd.mask);
  // the fields: the info lists them as the family does (the order listed), the kernels take them ascending by shift
  ArtnPauliBatchInfo &pi = pl.info;
  const size_t nf = bd.shift.size();
  std::vector<size_t> by_shift(nf);
  std::iota(by_shift.begin(), by_shift.end(), (size_t)0);
  std::sort(by_shift.begin(), by_shift.end(), [&](size_t x, size_t y) { return bd.shift[x] < bd.shift[y]; });
  pl.fields.n = (int32_t)nf;
  for (size_t f = 0; f < nf; ++f) {
    pi.field_shift[f] = bd.shift[f], pi.field_width[f] = bd.width[f], pi.field_pos[f] = bd.pos[f];
    const size_t s = by_shift[f];
    pl.fields.shift[f] = bd.shift[s], pl.fields.width[f] = bd.width[s], pl.fields.pos[f] = bd.pos[s];
  }
  // the work split: C = min(T, max(1, ARTN_BORN_MAX_GRID >> batch_bits)), T halved where the partner lies in another tile
  const int M = pl.local_bits;
  pl.tiles = M >= ARTN_PAULI_TILE_BITS ? (int64_t)1 << (M - ARTN_PAULI_TILE_BITS) : 1;
  const int64_t cap = std::max<int64_t>(1, (int64_t)ARTN_BORN_MAX_GRID >> bd.bits);
  pi.chunks = std::min(pl.tiles, cap);
  pi.chunks_halved = std::min(std::max<int64_t>(pl.tiles >> 1, 1), cap);
  int64_t units = pl.B * pi.chunks;
  if (M < ARTN_PAULI_TILE_BITS) units = pl.B == 1 ? 1 : (pl.B + ((int64_t)1 << (ARTN_PAULI_TILE_BITS - M)) - 1) >> (ARTN_PAULI_TILE_BITS - M);
  pi.n_groups = (int32_t)pl.members.size();
  pi.n_launches = (int32_t)launches;
  pi.terms_per_launch = ARTN_PAULI_TERMS;
  pi.batch_bits = bd.bits, pi.local_bits = M, pi.tile_bits = std::min(ARTN_PAULI_TILE_BITS, M);
  pi.n_fields = (int32_t)nf;
  pi.grid = (int32_t)std::min<int64_t>(units, ARTN_PAULI_BATCH_MAX_GRID);
  pi.B = pl.B, pi.n = n;
  pi.workspace_bytes = pl.B * pi.chunks * (ARTN_PAULI_TERMS + 1) * (int64_t)sizeof(double);
  pi.out_bytes = pl.B * (n_terms + 1) * (int64_t)sizeof(double);
  pi.bytes_read = launches * n * (d->dtype == ARTN_C64 ? 8 : 16);
  return ARTN_OK;
}

static int pauli_batch_log2(int64_t v) { return __builtin_ctzll((uint64_t)v); }

template <typename T, template <typename, int, int> class Launch, int FORM>
static void pauli_batch_launch_nt(int nt, dim3 grid, hipStream_t st, const T *a, const ArtnPauliBatchArgs &g, double *part) {
  if (nt <= 1) Launch<T, FORM, 1>::go(grid, st, a, g, part);
  else if (nt <= 4) Launch<T, FORM, 4>::go(grid, st, a, g, part);
  else Launch<T, FORM, ARTN_PAULI_TERMS>::go(grid, st, a, g, part);
}
template <typename T, int FORM, int NT> struct PauliBatchBig {
  static void go(dim3 grid, hipStream_t st, const T *a, const ArtnPauliBatchArgs &g, double *part) {
    hipLaunchKernelGGL((artn_k_pauli_batch<T, FORM, NT>), grid, dim3(ARTN_BORN_THREADS), 0, st, a, g, part);
  }
};
template <typename T, int FORM, int NT> struct PauliBatchSmall {
  static void go(dim3 grid, hipStream_t st, const T *a, const ArtnPauliBatchArgs &g, double *part) {
    hipLaunchKernelGGL((artn_k_pauli_batch_small<T, FORM, NT>), grid, dim3(ARTN_BORN_THREADS), 0, st, a, g, part);
  }
};

// one pass for the terms of g.p (a group's next at most ARTN_PAULI_TERMS), and its finish
template <typename T>
static void pauli_batch_launch(const PauliBatchPlan &pl, const T *a, ArtnPauliBatchArgs &g, const ArtnPauliFinish &f, int64_t n_terms,
                               double *part, double *out, hipStream_t st) {
  const int M = pl.local_bits, nt = g.p.nt;
  int nv = (nt <= 1 ? 1 : nt <= 4 ? 4 : ARTN_PAULI_TERMS) + 1;
  int64_t C = 1;
  if (M < ARTN_PAULI_TILE_BITS && pl.B == 1) { // one state below one tile: the unbatched kernel, whose order this is to give
    hipLaunchKernelGGL(artn_k_pauli_small<T>, dim3(1), dim3(ARTN_BORN_THREADS), 0, st, a, (long)pl.n, g.p, part);
    nv = ARTN_PAULI_TERMS + 1;
  } else if (M < ARTN_PAULI_TILE_BITS) {
    const int per = ARTN_PAULI_TILE_BITS - M;
    const int64_t vtiles = (pl.B + ((int64_t)1 << per) - 1) >> per;
    const dim3 grid((unsigned)std::min<int64_t>(vtiles, ARTN_PAULI_BATCH_MAX_GRID));
    if (g.xl == 0) pauli_batch_launch_nt<T, PauliBatchSmall, 0>(nt, grid, st, a, g, part);
    else pauli_batch_launch_nt<T, PauliBatchSmall, 1>(nt, grid, st, a, g, part);
  } else {
    const int form = g.xl == 0 ? 0 : (g.xl >> ARTN_PAULI_TILE_BITS) == 0 ? 1 : 2;
    C = form == 2 ? pl.info.chunks_halved : pl.info.chunks;
    g.chunk_bits = pauli_batch_log2(C);
    g.tile_bits = pauli_batch_log2(pl.tiles) - (form == 2 ? 1 : 0);
    const dim3 grid((unsigned)std::min<int64_t>(pl.B * C, ARTN_PAULI_BATCH_MAX_GRID));
    if (form == 0) pauli_batch_launch_nt<T, PauliBatchBig, 0>(nt, grid, st, a, g, part);
    else if (form == 1) pauli_batch_launch_nt<T, PauliBatchBig, 1>(nt, grid, st, a, g, part);
    else pauli_batch_launch_nt<T, PauliBatchBig, 2>(nt, grid, st, a, g, part);
  }
  const int64_t lanes = pl.B * nv;
  hipLaunchKernelGGL(artn_k_pauli_batch_finish, dim3((unsigned)((lanes + ARTN_BORN_THREADS - 1) / ARTN_BORN_THREADS)), dim3(ARTN_BORN_THREADS),
                     0, st, (const double *)part, (long long)pl.B, (long)C, nv, f, (long)(n_terms + 1), out);
}

extern "C" {

int artn_pauli_batch_query(const ArtnMarginalDesc *d, const uint8_t *ops, int64_t n_terms, int32_t nb, const int32_t *batch_dims,
                           ArtnPauliBatchInfo *info, uint64_t *xmask, uint64_t *zmask, int32_t *n_y, int32_t *group,
                           uint64_t *local_xmask, uint64_t *local_zmask) {
  if (!info) return fail(ARTN_E_INVALID, "null info");
  PauliBatchPlan pl;
  if (int rc = pauli_batch_plan(d, ops, n_terms, nb, batch_dims, pl)) return rc;
  *info = pl.info;
  if (xmask) std::copy(pl.xm.begin(), pl.xm.end(), xmask);
  if (zmask) std::copy(pl.zm.begin(), pl.zm.end(), zmask);
  if (n_y) std::copy(pl.ny.begin(), pl.ny.end(), n_y);
  if (group) std::copy(pl.group.begin(), pl.group.end(), group);
  if (local_xmask) std::copy(pl.xl.begin(), pl.xl.end(), local_xmask);
  if (local_zmask) std::copy(pl.zl.begin(), pl.zl.end(), local_zmask);
  return ARTN_OK;
}

// (every argument is checked before the device is looked for: a refusal does not depend on the machine)
int artn_pauli_batch_expect(const ArtnMarginalDesc *d, const void *a, const uint8_t *ops, int64_t n_terms, int32_t nb,
                            const int32_t *batch_dims, double *out, void *ws, int64_t ws_bytes, void *stream) {
  PauliBatchPlan pl;
  if (int rc = pauli_batch_plan(d, ops, n_terms, nb, batch_dims, pl)) return rc;
  if (!a || !out || !ws) return fail(ARTN_E_INVALID, "null pointer");
  if (ws_bytes < pl.info.workspace_bytes) return fail(ARTN_E_INVALID, "workspace smaller than artn_pauli_batch_query reports");
  if (int rc = state_array_aligned(a, "artn_pauli_batch_expect")) return rc;
  if ((((uintptr_t)out | (uintptr_t)ws) & 7) != 0)
    return fail(ARTN_E_UNSUPPORTED, "artn_pauli_batch_expect needs 8-byte aligned output and workspace");
  if (artn_device_count() < 1) return fail(ARTN_E_NODEVICE, "no gfx950 device visible");
  hipStream_t st = (hipStream_t)stream;
  const bool tiled = pl.local_bits >= ARTN_PAULI_TILE_BITS;
  bool first = true;
  for (const auto &m : pl.members) {
    const uint64_t xm = pl.xm[m[0]], xl = pl.xl[m[0]];
    const bool halved = tiled && (xl >> ARTN_PAULI_TILE_BITS) != 0; // FORM 2: half the local index space, weight 2
    for (size_t at = 0; at < m.size(); at += ARTN_PAULI_TERMS) {
      ArtnPauliBatchArgs g = {};
      ArtnPauliFinish f = {};
      ArtnPauliArgs &p = g.p;
      p.xm = xm, g.xl = xl;
      p.nt = f.nt = (int32_t)std::min<size_t>(ARTN_PAULI_TERMS, m.size() - at);
      p.hbit = xl ? 63 - __builtin_clzll(xl) : 0;
      p.norm = first;
      f.norm_index = first ? n_terms : -1;
      for (int t = 0; t < p.nt; ++t) {
        const int64_t term = m[at + t];
        const int32_t ny = pl.ny[term];
        p.zm[t] = pl.zl[term];
        p.sel[t] = (uint8_t)((pl.zl[term] & 3) | (uint64_t)((ny & 1) << 2));
        f.out_index[t] = term;
        f.scale[t] = (int8_t)(((ny & 3) == 1 || (ny & 3) == 2 ? -1 : 1) * (halved ? 2 : 1));
      }
      g.local_bits = pl.local_bits, g.B = pl.B, g.f = pl.fields;
      if (d->dtype == ARTN_C64) pauli_batch_launch(pl, (const float2 *)a, g, f, n_terms, (double *)ws, out, st);
      else pauli_batch_launch(pl, (const double2 *)a, g, f, n_terms, (double *)ws, out, st);
      first = false;
    }
  }
  HIP_TRY(hipGetLastError());
  return ARTN_OK;
}

} // extern "C"
