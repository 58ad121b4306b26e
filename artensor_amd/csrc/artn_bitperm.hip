// artn_bitperm.hip -- host half of the bit-permutation entry points artn_bitperm_* of include/artn.h (kernel:
// artn_bitperm_kernel.h): the cut of a permutation into passes, each pass's tile and hole walk, and the search for an LDS map
// that keeps both phases of the kernel off each other's banks.
//
// A translation unit of its own (build/obj/bitperm.o).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <string>
#include <vector>

#include "artn_host.h"
#include "artn_state_host.h"
#include "artn_bitperm_kernel.h"

struct BitpermPass {
  std::vector<int> map;  // per memory bit: where the pass sends it
  std::vector<int> tile; // tile bits, ascending
  ArtnBitpermPass rec = {};
  int load_degree = 1, store_degree = 1;
};
struct BitpermPlan {
  int n_bits = 0, lb = 0;
  std::vector<BitpermPass> pass;
  ArtnBitpermInfo info = {};
};

// ---- GF(2) helpers: vectors are bit masks
static int bitperm_rank(std::vector<uint64_t> v) {
  int rank = 0;
  for (int bit = 63; bit >= 0; --bit) {
    size_t at = rank;
    while (at < v.size() && !((v[at] >> bit) & 1)) ++at;
    if (at == v.size()) continue;
    std::swap(v[rank], v[at]);
    for (size_t i = 0; i < v.size(); ++i)
      if ((int)i != rank && ((v[i] >> bit) & 1)) v[i] ^= v[rank];
    ++rank;
  }
  return rank;
}
static uint64_t bitperm_xor_cols(const uint64_t *col, uint64_t u) {
  uint64_t x = 0;
  for (int j = 0; u >> j; ++j)
    if ((u >> j) & 1) x ^= col[j];
  return x;
}
// The conflict degree of one LDS phase: `gens` span the tile-local indices of the lanes of one service group (masks over
// tile-local bits), `w` is log2 of the banks' period in elements: 2^(dim - rank of the LDS indices modulo 2^w).
static int bitperm_degree(const uint64_t *col, const std::vector<uint64_t> &gens, int w) {
  std::vector<uint64_t> image;
  for (uint64_t g : gens) image.push_back(bitperm_xor_cols(col, g) & (((uint64_t)1 << w) - 1));
  return 1 << ((int)gens.size() - bitperm_rank(image));
}
// The lanes of a service group as tile-local masks (MI355X: 64-bit writes go 16 consecutive lanes at a time, 64-bit reads 32;
// 128-bit writes 8 consecutive lanes, 128-bit reads the 16 lanes {0-3, 12-15, 20-27} and their cosets); a 16-byte chunk is two
// complex64, so lane bit i is tile-local bit i + 1 there.  Generators that reach beyond a small tile are dropped.
static void bitperm_groups(int32_t dtype, int tb, std::vector<uint64_t> &load, int &wl, std::vector<uint64_t> &store, int &ws) {
  if (dtype == ARTN_C64) {
    load = {2, 4, 8, 16}, wl = 4;
    store = {2, 4, 8, 16, 32}, ws = 5;
  } else {
    load = {1, 2, 4}, wl = 3;
    store = {1, 2, 4 | 8, 4 | 16}, ws = 4;
  }
  const auto beyond = [&](uint64_t g) { return (g >> tb) != 0; };
  load.erase(std::remove_if(load.begin(), load.end(), beyond), load.end());
  store.erase(std::remove_if(store.begin(), store.end(), beyond), store.end());
}

// The LDS map of one pass.  Bit r of L(u) is the parity of f[r] & u; a candidate is ws functionals, completed to an invertible
// map by unit functionals.  Candidates come from a fixed xorshift sequence, so the plan is the same on every call; the first
// with load degree 1 and store degree 1 ends the search, otherwise the best store degree among those with load degree 1 stays.
// (A common complement argument shows that degree 1 on both sides always exists for a full tile: DESIGN section 24.)
static bool bitperm_lds_map(int32_t dtype, int tb, const std::vector<int> &tau_inv, uint64_t *load_col, uint64_t *store_col,
                            int &load_degree, int &store_degree) {
  std::vector<uint64_t> gl, gs;
  int wl = 0, ws = 0;
  bitperm_groups(dtype, tb, gl, wl, gs, ws);
  const uint64_t all = ((uint64_t)1 << tb) - 1;
  uint64_t rng = 0x9E3779B97F4A7C15ull;
  uint64_t best_load[16] = {}, best_store[16] = {};
  int best = 0;
  for (int attempt = 0; attempt < 4096 && best != 1; ++attempt) {
    std::vector<uint64_t> f;
    for (int r = 0; r < std::min(ws, tb); ++r) {
      if (attempt == 0) f.push_back((uint64_t)1 << r); // L(u) = u first
      else {
        rng ^= rng << 13, rng ^= rng >> 7, rng ^= rng << 17;
        f.push_back(rng & all);
      }
    }
    if (bitperm_rank(f) != (int)f.size()) continue;
    for (int j = 0; j < tb && (int)f.size() < tb; ++j) {
      f.push_back((uint64_t)1 << j);
      if (bitperm_rank(f) != (int)f.size()) f.pop_back();
    }
    uint64_t lc[16] = {}, sc[16] = {};
    for (int j = 0; j < tb; ++j)
      for (int r = 0; r < tb; ++r) lc[j] |= ((f[r] >> j) & 1) << r;
    for (int j = 0; j < tb; ++j) sc[j] = lc[tau_inv[j]];
    if (bitperm_degree(lc, gl, wl) != 1) continue;
    const int deg = bitperm_degree(sc, gs, ws);
    if (best == 0 || deg < best) {
      best = deg;
      std::copy(lc, lc + 16, best_load), std::copy(sc, sc + 16, best_store);
    }
  }
  std::copy(best_load, best_load + 16, load_col), std::copy(best_store, best_store + 16, store_col);
  load_degree = bitperm_degree(load_col, gl, wl), store_degree = bitperm_degree(store_col, gs, ws);
  return best != 0;
}

// The layout checks of the bit-indexed families, dst_bit, the passes (include/artn.h: PLAN) and each pass's record.
static int bitperm_plan(const ArtnMarginalDesc *d, const int32_t *dst_bit, int32_t n_bits, BitpermPlan &bp) {
  const char *who = "bit permutations take";
  if (int rc = state_desc(d, who, ARTN_MARG_MAX_DIMS, false)) return rc;
  if (!dst_bit) return fail(ARTN_E_INVALID, "null pointer");
  StateLayout l;
  if (int rc = state_layout(d, l)) return rc;
  if (int rc = state_bits_only(l, who)) return rc;
  const int nb = __builtin_ctzll((uint64_t)l.n);
  if (n_bits != nb)
    return fail(ARTN_E_INVALID, "a state of 2^" + std::to_string(nb) + " elements has " + std::to_string(nb) + " index bits, not " +
                                    std::to_string(n_bits));
  uint64_t seen = 0;
  for (int b = 0; b < nb; ++b) {
    if (dst_bit[b] < 0 || dst_bit[b] >= nb || ((seen >> dst_bit[b]) & 1))
      return fail(ARTN_E_INVALID, "dst_bit is not a permutation of 0 .. " + std::to_string(nb - 1) + ": entry " + std::to_string(b) +
                                      " is " + std::to_string(dst_bit[b]));
    seen |= (uint64_t)1 << dst_bit[b];
  }
  const int lb = d->dtype == ARTN_C64 ? 4 : 3;
  const int tb_max = d->dtype == ARTN_C64 ? ARTN_WGATE_TILE_BITS_C64 : ARTN_WGATE_TILE_BITS_C128;
  const int tb = std::min(tb_max, nb);
  const int low = nb <= tb_max ? nb : lb; // bits below `low` cost a pass nothing: below a line, or the tile is the whole state
  const int room = tb_max - lb;
  const int64_t elem = d->dtype == ARTN_C64 ? 8 : 16;
  bp.n_bits = nb, bp.lb = lb;
  bp.info.n_bits = nb, bp.info.line_bits = lb;
  for (int b = 0; b < nb; ++b)
    if (dst_bit[b] != b) ++bp.info.moved, bp.info.moved_high += b >= lb;

  std::vector<int> left(dst_bit, dst_bit + nb); // what sits at bit p still has to go to left[p]
  for (;;) {
    std::vector<std::vector<int>> cycles;
    uint64_t done = 0;
    for (int b = 0; b < nb; ++b) {
      if (left[b] == b || ((done >> b) & 1)) continue;
      std::vector<int> c;
      for (int p = b; !((done >> p) & 1); p = left[p]) c.push_back(p), done |= (uint64_t)1 << p;
      cycles.push_back(c);
    }
    if (cycles.empty()) break;
    if ((int)bp.pass.size() == ARTN_BITPERM_MAX_PASSES) return fail(ARTN_E_UNSUPPORTED, "bit permutations take at most 8 passes");
    BitpermPass ps;
    ps.map.resize(nb);
    for (int b = 0; b < nb; ++b) ps.map[b] = b;
    const auto high = [&](const std::vector<int> &c) { return (int)std::count_if(c.begin(), c.end(), [&](int p) { return p >= low; }); };
    int free_high = room;
    std::vector<const std::vector<int> *> longer;
    for (const auto &c : cycles) { // whole cycles first
      if (high(c) > free_high) {
        longer.push_back(&c);
        continue;
      }
      free_high -= high(c);
      for (size_t i = 0; i < c.size(); ++i) ps.map[c[i]] = c[(i + 1) % c.size()];
    }
    for (const auto *c : longer) { // then one arc: it takes every free place
      size_t start = 0;
      while (start < c->size() && (*c)[start] >= low) ++start;
      const bool from_low = start < c->size();
      if (free_high < (from_low ? 1 : 2)) break;
      if (!from_low) start = 0;
      std::vector<int> arc;
      int used = 0;
      for (size_t i = 0; i < c->size(); ++i) {
        const int p = (*c)[(start + i) % c->size()];
        if (p >= low && used++ == free_high) break;
        arc.push_back(p);
      }
      for (size_t i = 0; i < arc.size(); ++i) ps.map[arc[i]] = arc[(i + 1) % arc.size()];
      break;
    }
    std::vector<int> next(nb);
    for (int p = 0; p < nb; ++p) next[ps.map[p]] = left[p];
    left = next;

    // ---- the tile, its segment and holes
    uint64_t moved = 0;
    for (int b = 0; b < nb; ++b)
      if (ps.map[b] != b) moved |= (uint64_t)1 << b;
    for (int b = 0; b < nb; ++b)
      if (((moved >> b) & 1) || b < lb) ps.tile.push_back(b);
    if ((int)ps.tile.size() > tb) return fail(ARTN_E_UNSUPPORTED, "bit permutations: a pass does not fit its tile");
    for (int b = lb; b < nb && (int)ps.tile.size() < tb; ++b)
      if (!((moved >> b) & 1)) ps.tile.push_back(b);
    std::sort(ps.tile.begin(), ps.tile.end());
    int seg_bits = 0;
    while (seg_bits < tb && ps.tile[seg_bits] == seg_bits) ++seg_bits;
    ArtnBitpermPass &r = ps.rec;
    r.tile_bits = (uint64_t)tb, r.n_tiles = (uint64_t)(l.n >> tb), r.segment_bits = (uint64_t)seg_bits, r.moved_mask = moved;
    for (int j = seg_bits; j < tb; ++j) r.hole_bit[r.n_holes++] = (uint64_t)ps.tile[j];
    std::vector<int> tau_inv(tb);
    for (int j = 0; j < tb; ++j) {
      r.mem_col[j] = (uint64_t)1 << ps.tile[j];
      const int to = (int)(std::find(ps.tile.begin(), ps.tile.end(), ps.map[ps.tile[j]]) - ps.tile.begin());
      tau_inv[to] = j;
    }
    if (!bitperm_lds_map(d->dtype, tb, tau_inv, r.load_col, r.store_col, ps.load_degree, ps.store_degree))
      return fail(ARTN_E_UNSUPPORTED, "bit permutations: no conflict-free LDS map found for the load phase");
    const int p = (int)bp.pass.size();
    bp.info.tile_bits[p] = tb, bp.info.n_tiles[p] = (int64_t)r.n_tiles, bp.info.moved_mask[p] = moved;
    bp.info.grid[p] = (int32_t)std::min<int64_t>((int64_t)r.n_tiles, ARTN_GATES_MAX_GRID);
    bp.info.load_degree[p] = ps.load_degree, bp.info.store_degree[p] = ps.store_degree;
    bp.pass.push_back(ps);
  }
  bp.info.passes = (int32_t)bp.pass.size();
  bp.info.table_bytes = (int64_t)sizeof(ArtnBitpermTable) + (int64_t)sizeof(ArtnBitpermPass) * bp.info.passes;
  bp.info.lds_bytes = bp.info.passes ? elem << tb : 0;
  bp.info.bytes_moved = 2 * l.n * elem * bp.info.passes;
  return ARTN_OK;
}

extern "C" {

int artn_bitperm_query(const ArtnMarginalDesc *d, const int32_t *dst_bit, int32_t n_bits, ArtnBitpermInfo *info, int32_t *pass_map,
                       int32_t *tiles, uint64_t *load_col, uint64_t *store_col) {
  if (!info) return fail(ARTN_E_INVALID, "null info");
  BitpermPlan bp;
  if (int rc = bitperm_plan(d, dst_bit, n_bits, bp)) return rc;
  *info = bp.info;
  for (size_t p = 0; p < bp.pass.size(); ++p) {
    const BitpermPass &ps = bp.pass[p];
    if (pass_map) std::copy(ps.map.begin(), ps.map.end(), pass_map + p * ARTN_BITPERM_MAX_BITS);
    if (tiles) {
      std::fill(tiles + p * 16, tiles + p * 16 + 16, -1);
      std::copy(ps.tile.begin(), ps.tile.end(), tiles + p * 16);
    }
    if (load_col) std::copy(ps.rec.load_col, ps.rec.load_col + 16, load_col + p * 16);
    if (store_col) std::copy(ps.rec.store_col, ps.rec.store_col + 16, store_col + p * 16);
  }
  return ARTN_OK;
}

int artn_bitperm_pack(const ArtnMarginalDesc *d, const int32_t *dst_bit, int32_t n_bits, void *table, int64_t table_bytes) {
  BitpermPlan bp;
  if (int rc = bitperm_plan(d, dst_bit, n_bits, bp)) return rc;
  if (!table) return fail(ARTN_E_INVALID, "null pointer");
  if (int rc = state_table_fits(table_bytes, bp.info.table_bytes, "artn_bitperm_query")) return rc;
  if (int rc = state_table_aligned(table, "artn_bitperm_pack")) return rc;
  ArtnBitpermTable head = {};
  head.n_passes = (uint64_t)bp.pass.size(), head.n_bits = (uint64_t)bp.n_bits;
  *(ArtnBitpermTable *)table = head;
  ArtnBitpermPass *rec = (ArtnBitpermPass *)((ArtnBitpermTable *)table + 1);
  for (size_t p = 0; p < bp.pass.size(); ++p) rec[p] = bp.pass[p].rec;
  return ARTN_OK;
}

int artn_bitperm_apply(const ArtnMarginalDesc *d, void *a, const int32_t *dst_bit, int32_t n_bits, const void *table,
                       int64_t table_bytes, void *stream) {
  if (artn_device_count() < 1) return fail(ARTN_E_NODEVICE, "no gfx950 device visible");
  BitpermPlan bp;
  if (int rc = bitperm_plan(d, dst_bit, n_bits, bp)) return rc;
  if (!a || !table) return fail(ARTN_E_INVALID, "null pointer");
  if (int rc = state_table_fits(table_bytes, bp.info.table_bytes, "artn_bitperm_query")) return rc;
  if (int rc = state_array_aligned(a, "artn_bitperm_apply")) return rc;
  if (int rc = state_table_aligned(table, "artn_bitperm_apply")) return rc;
  hipStream_t st = (hipStream_t)stream;
  const ArtnBitpermPass *rec = (const ArtnBitpermPass *)((const ArtnBitpermTable *)table + 1);
  const dim3 block(ARTN_BORN_THREADS);
  for (int p = 0; p < bp.info.passes; ++p) {
    const dim3 grid((unsigned)bp.info.grid[p]);
    const size_t lds = (size_t)bp.info.lds_bytes;
    if (d->dtype == ARTN_C64) hipLaunchKernelGGL(artn_k_bitperm<float2>, grid, block, lds, st, (float2 *)a, rec + p);
    else hipLaunchKernelGGL(artn_k_bitperm<double2>, grid, block, lds, st, (double2 *)a, rec + p);
    HIP_TRY(hipGetLastError());
  }
  return ARTN_OK;
}

} // extern "C"
