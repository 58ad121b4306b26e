// artn_state_host.h -- host plumbing shared by the operations on a dense amplitude array (artn_born.hip, artn_rdm.hip,
// artn_pauli.hip, artn_gates.hip, artn_wgate.hip, artn_mgate.hip, artn_cgate.hip, artn_measure.hip, artn_channel.hip,
// artn_batch.hip, artn_cgate_batch.hip, artn_pauli_batch.hip, artn_sample_batch.hip, artn_diag.hip, artn_bitperm.hip): the descriptor and layout checks, the batch dimensions, the max_rank rule and the rank dispatch of the run
// kernels, the matrix scan, the argument checks of the pack / apply entries, the parts of a packed table, the plan, the
// column packer, the table header and the K dispatch of the tile kernels (wide gates, matrix gates, controlled gates,
// channels).  The whole host half of the two dense-gate families is artn_dense_gate_host.h, what the four run-circuit
// families share artn_run_circuit_host.h, both on top of this.  Codes and texts are part of the ABI's behaviour (tests/test_state_layout_cpu.py); each family keeps its own wording (`who`: "gate
// circuits take", ...) and its own precedence between the errors, so the pieces are separate functions.
#pragma once
#include <algorithm>
#include <cmath>
#include <string>
#include <type_traits>
#include <vector>

#include "artn_host.h"

static int state_ceil_log2(int64_t n) {
  int b = 0;
  while (b < 62 && ((int64_t)1 << b) < n) ++b;
  return b;
}

// Descriptor, dtype and number of dimensions.  `fold`: both n_dims errors are one ARTN_E_INVALID (marginals, density matrices).
static int state_desc(const ArtnMarginalDesc *d, const char *who, int max_dims, bool fold) {
  if (!d) return fail(ARTN_E_INVALID, "null descriptor");
  if (d->dtype != ARTN_C64 && d->dtype != ARTN_C128) return fail(ARTN_E_UNSUPPORTED, std::string(who) + " complex64 or complex128");
  if (d->n_dims < 0 || (fold && d->n_dims > max_dims)) return fail(ARTN_E_INVALID, "bad number of dimensions");
  if (d->n_dims > max_dims) return fail(ARTN_E_UNSUPPORTED, std::string(who) + " at most " + std::to_string(max_dims) + " dimensions");
  return ARTN_OK;
}

struct StateLayout {
  int64_t n = 1;          // elements (of the dimensions below the one that passes 2^40, when too_big)
  std::vector<int> order; // the dimensions of extent > 1, by stride
  bool pow2 = true, too_big = false;
};

// Dense: sorted by stride, every stride is the product of the extents below it (extent 1 carries no index).  The walk stops at
// the first dimension that passes 2^40 elements: what the caller reports then, and when, is its own business.
static int state_layout(const ArtnMarginalDesc *d, StateLayout &l) {
  for (int i = 0; i < d->n_dims; ++i) {
    if (d->extent[i] < 1) return fail(ARTN_E_INVALID, "extent below 1");
    if (d->extent[i] == 1) continue;
    if (d->stride[i] < 1) return fail(ARTN_E_INVALID, "the tensor is not dense: stride below 1");
    if (d->extent[i] & (d->extent[i] - 1)) l.pow2 = false;
    l.order.push_back(i);
  }
  std::sort(l.order.begin(), l.order.end(), [&](int x, int y) { return d->stride[x] < d->stride[y]; });
  for (int i : l.order) {
    if (d->stride[i] != l.n) return fail(ARTN_E_INVALID, "the tensor is not dense: its strides overlap or leave gaps");
    if (d->extent[i] > ((int64_t)1 << 40) / l.n) {
      l.too_big = true;
      break;
    }
    l.n *= d->extent[i];
  }
  return ARTN_OK;
}

// the two refusals of the families that index the state by bits, in their order
static int state_bits_only(const StateLayout &l, const char *who) {
  if (!l.pow2) return fail(ARTN_E_UNSUPPORTED, std::string(who) + " power-of-two extents");
  if (l.too_big) return fail(ARTN_E_UNSUPPORTED, std::string(who) + " at most 2^40 elements");
  return ARTN_OK;
}

// Pauli strings (uint8 codes 0..3 = I, X, Y, Z per dimension): the memory bit of every dimension of extent 2 (-1 elsewhere), and
// the masks of term t -- x: the bits under X or Y, z: those under Z or Y, y: the number of Y
static void state_dim_bits(const ArtnMarginalDesc *d, int *bit) {
  for (int i = 0; i < d->n_dims; ++i) bit[i] = d->extent[i] == 2 ? __builtin_ctzll((uint64_t)d->stride[i]) : -1;
}
static int state_string_masks(const ArtnMarginalDesc *d, const int *bit, const uint8_t *op, int64_t t, uint64_t &x, uint64_t &z, int32_t &y) {
  x = z = 0, y = 0;
  for (int i = 0; i < d->n_dims; ++i) {
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
  return ARTN_OK;
}

// max_rank of a circuit query -> the rank the plan cuts at: below -1 is invalid, above the dtype's maximum (`top` for complex64,
// one less for complex128) unsupported, -1 the maximum minus one (64 KiB of LDS per workgroup).  The two-state form is checked
// before the descriptor's dtype: with another dtype it leaves the refusal to the plan.
static int state_max_rank(int32_t dtype, int32_t max_rank, int top, bool two_state, int32_t &rank) {
  const int lib_max = dtype == ARTN_C128 ? top - 1 : top;
  if (max_rank < -1) return fail(ARTN_E_INVALID, "max_rank below -1");
  if (max_rank > lib_max && (dtype == ARTN_C64 || dtype == ARTN_C128))
    return fail(ARTN_E_UNSUPPORTED, "max_rank " + std::to_string(max_rank) + " above the " + (two_state ? "two-state maximum " : "maximum ") +
                                        std::to_string(lib_max) + " of this dtype");
  rank = std::min<int32_t>(max_rank < 0 ? lib_max - 1 : max_rank, lib_max);
  return ARTN_OK;
}

// ... and no more than the state has tiles to pair: 2^rank tiles of 2^tile_bits elements fit into n
static int state_rank_cap(int64_t n, int tile_bits, int rank) {
  int have = 0;
  while (((int64_t)1 << (tile_bits + have + 1)) <= n) ++have;
  return std::min(rank, have);
}

// f(std::integral_constant<int, R>) for the run-time rank: R = 0 .. MAX for 8-byte elements, 0 .. MAX - 1 for 16-byte ones
// (the LDS of a block); any other rank is an invalid value and instantiates nothing.
template <typename T, int MAX, int R = 0, typename F>
static hipError_t state_with_rank(int rank, F &&f) {
  if constexpr (R > MAX || (R == MAX && sizeof(T) != 8)) return hipErrorInvalidValue;
  else return rank == R ? f(std::integral_constant<int, R>()) : state_with_rank<T, MAX, R + 1>(rank, f);
}

// a rows x rows complex matrix: false when an entry is not finite; `diagonal` when nothing off the diagonal is non-zero
static bool state_matrix_scan(const double *m, int rows, bool &diagonal) {
  diagonal = true;
  for (int e = 0; e < 2 * rows * rows; ++e) {
    if (!std::isfinite(m[e])) return false;
    if (m[e] != 0.0 && (e / 2) / rows != (e / 2) % rows) diagonal = false;
  }
  return true;
}

// the argument checks of a pack / apply entry, one text each; the entry calls them in its own order
static int state_table_fits(int64_t table_bytes, int64_t need, const char *query) {
  if (table_bytes < need) return fail(ARTN_E_INVALID, std::string("table smaller than ") + query + " reports");
  return ARTN_OK;
}
static int state_table_aligned(const void *table, const char *entry) {
  if (((uintptr_t)table & 7) != 0) return fail(ARTN_E_UNSUPPORTED, std::string(entry) + " needs an 8-byte aligned table");
  return ARTN_OK;
}
static int state_array_aligned(const void *a, const char *entry) {
  if (((uintptr_t)a & 15) != 0) return fail(ARTN_E_UNSUPPORTED, std::string(entry) + " needs a 16-byte aligned array");
  return ARTN_OK;
}
static int state_disjoint(const void *lam, const void *phi, uintptr_t bytes, const char *entry) {
  const uintptr_t pl = (uintptr_t)lam, pp = (uintptr_t)phi;
  if (pl < pp + bytes && pp < pl + bytes) return fail(ARTN_E_INVALID, std::string(entry) + ": lam overlaps phi");
  return ARTN_OK;
}

// a packed circuit table: the header, then n_runs run records, then the step or gate records
template <typename Header, typename Void, typename Run, typename Rec>
static void state_table_parts(Void *table, size_t n_runs, Run *&runs, Rec *&recs) {
  runs = (Run *)((Header *)table + 1);
  recs = (Rec *)(runs + n_runs);
}

// ---- the tile kernels: artn_k_wgate, artn_k_mgate, artn_k_cgate, artn_k_channel (include/artn.h: PLAN of artn_wgate_query) ----

// One listed dimension of a gate or channel (`what`: "gates", "channels"): in range, of extent 2, not among `seen`, the
// dimensions listed before it -- the n_targets targets first, so a control that repeats one of those gets its own text.
static int state_tile_dim(const ArtnMarginalDesc *d, int32_t dim, const std::vector<int32_t> &seen, size_t n_targets, bool is_control,
                          const char *what) {
  if (dim < 0 || dim >= d->n_dims) return fail(ARTN_E_INVALID, "dimension " + std::to_string(dim) + " out of range");
  if (d->extent[dim] != 2)
    return fail(ARTN_E_INVALID, std::string(what) + " act on dimensions of extent 2; dimension " + std::to_string(dim) + " has extent " +
                                    std::to_string(d->extent[dim]));
  for (size_t i = 0; i < seen.size(); ++i)
    if (seen[i] == dim) {
      if (is_control && i < n_targets)
        return fail(ARTN_E_INVALID, "dimension " + std::to_string(dim) + " is both a target and a control");
      return fail(ARTN_E_INVALID, "the dimensions must differ; dimension " + std::to_string(dim) + " is repeated");
    }
  return ARTN_OK;
}
// the k target dimensions dims[0 .. k-1] of a family without controls -> their memory bits, in the order listed
static int state_tile_targets(const ArtnMarginalDesc *d, int32_t k, const int32_t *dims, const char *what, std::vector<int> &target) {
  std::vector<int32_t> seen;
  for (int j = 0; j < k; ++j) {
    if (int rc = state_tile_dim(d, dims[j], seen, (size_t)k, false, what)) return rc;
    seen.push_back(dims[j]);
    target.push_back(__builtin_ctzll((uint64_t)d->stride[dims[j]]));
  }
  return ARTN_OK;
}

// ---- batch dimensions: B trajectories in one tensor (include/artn.h: BATCHED TRAJECTORIES) ----

struct BatchDims {
  int bits = 0;      // log2 B
  uint64_t mask = 0; // over memory bits
  std::vector<int> shift, width, pos; // the fields, the most significant one first (the order listed)
};

// The nb batch dimensions against `seen`, the dimensions listed before them: its first k are `role` ones ("measured", "target"),
// the rest controls.  What is wrong with them (ARTN_E_INVALID) before what the layout does not support: a batch bit below a
// 128-byte line, more than ARTN_BATCH_MAX_BITS batch bits.  Dimensions adjacent in memory and in order merge into one field.
static int state_batch_dims(const ArtnMarginalDesc *d, int32_t nb, const int32_t *batch_dims, std::vector<int32_t> &seen, size_t k,
                            const char *role, BatchDims &bd) {
  const size_t listed = seen.size();
  const int lb = d->dtype == ARTN_C64 ? 4 : 3; // index bits of a 128-byte line
  for (int i = 0; i < nb; ++i) {
    const int32_t dim = batch_dims[i];
    if (dim < 0 || dim >= d->n_dims) return fail(ARTN_E_INVALID, "batch dimension " + std::to_string(dim) + " out of range");
    for (size_t s = 0; s < seen.size(); ++s)
      if (seen[s] == dim) {
        if (s < k)
          return fail(ARTN_E_INVALID, "dimension " + std::to_string(dim) + " is both a batch dimension and a " + role + " one");
        if (s < listed) return fail(ARTN_E_INVALID, "dimension " + std::to_string(dim) + " is both a batch dimension and a control one");
        return fail(ARTN_E_INVALID, "the batch dimensions must differ; dimension " + std::to_string(dim) + " is repeated");
      }
    seen.push_back(dim);
  }
  int low_dim = -1, low_bit = 0;
  std::vector<int> shift, width, pos; // the last listed dimension first: it fills the lowest bits of b
  for (int i = nb - 1; i >= 0; --i) {
    const int32_t dim = batch_dims[i];
    if (d->extent[dim] == 1) continue; // (no index bit)
    const int e = __builtin_ctzll((uint64_t)d->extent[dim]), s = __builtin_ctzll((uint64_t)d->stride[dim]);
    if (s < lb && (low_dim < 0 || s < low_bit)) low_dim = dim, low_bit = s;
    if (!shift.empty() && s == shift.back() + width.back() && bd.bits == pos.back() + width.back()) {
      width.back() += e; // adjacent in memory and in order: one field
    } else {
      shift.push_back(s), width.push_back(e), pos.push_back(bd.bits);
    }
    bd.bits += e;
    bd.mask |= (((uint64_t)1 << e) - 1) << s;
  }
  if (low_dim >= 0)
    return fail(ARTN_E_UNSUPPORTED, "batch dimension " + std::to_string(low_dim) + " holds memory bit " + std::to_string(low_bit) +
                                        ", below a 128-byte line (bit " + std::to_string(lb) +
                                        " of this dtype): a line would span two trajectories -- move it up with artn_bitperm_apply (relayout_)");
  if (bd.bits > ARTN_BATCH_MAX_BITS)
    return fail(ARTN_E_UNSUPPORTED, "at most " + std::to_string(ARTN_BATCH_MAX_BITS) + " batch bits; these dimensions have " +
                                        std::to_string(bd.bits));
  bd.shift.assign(shift.rbegin(), shift.rend()), bd.width.assign(width.rbegin(), width.rend()), bd.pos.assign(pos.rbegin(), pos.rend());
  return ARTN_OK;
}

struct TilePlan {
  int tb = 0, seg_bits = 0;
  std::vector<int> target; // memory bits in the order listed
  std::vector<int> tile;   // tile bits, ascending
  int64_t elem = 0, n_tiles = 0, segment = 0, lds_bytes = 0;
};

// The tile of a state of 2^sub_bits walked elements: the targets (set before the call) and the lowest bits that are neither
// targets nor `excluded` (the high controls), min(TB, sub_bits) in all, ascending; seg_bits = the leading tile bits j that are
// memory bit j.
static void state_tile_plan(int32_t dtype, int sub_bits, uint64_t excluded, TilePlan &tp) {
  tp.tb = std::min(dtype == ARTN_C64 ? ARTN_WGATE_TILE_BITS_C64 : ARTN_WGATE_TILE_BITS_C128, sub_bits);
  for (int b : tp.target) excluded |= (uint64_t)1 << b;
  tp.tile = tp.target;
  for (int b = 0; (int)tp.tile.size() < tp.tb; ++b)
    if (!((excluded >> b) & 1)) tp.tile.push_back(b);
  std::sort(tp.tile.begin(), tp.tile.end());
  tp.seg_bits = 0;
  while (tp.seg_bits < tp.tb && tp.tile[tp.seg_bits] == tp.seg_bits) ++tp.seg_bits;
  tp.elem = dtype == ARTN_C64 ? 8 : 16;
  tp.n_tiles = (int64_t)1 << (sub_bits - tp.tb), tp.segment = (int64_t)1 << tp.seg_bits, tp.lds_bytes = tp.elem << tp.tb;
}

// The columns of a packed table, per tile-local bit, and the swizzle: the window is the lowest P = min(6, gb) tile-local bits; its
// non-targets are group bits 0 .. P-j-1 and LDS index bits of the same number, its j targets get the LDS index bits P-j .. P-1.
// The r-th non-target tile bit is group bit r: its lds_col is 1 << r.
static void state_tile_cols(const TilePlan &tp, uint64_t *mem_col, uint64_t *lds_col, uint64_t *target_bit, uint64_t *target_pos,
                            uint64_t *swizzle) {
  const int k = (int)tp.target.size(), gb = tp.tb - k, window = std::min(6, gb);
  int low_targets = 0;
  for (int p = 0; p < window; ++p)
    if (std::find(tp.target.begin(), tp.target.end(), tp.tile[p]) != tp.target.end()) ++low_targets;
  int rank = 0, seen = 0; // non-targets / window targets below the position
  for (int p = 0; p < tp.tb; ++p) {
    mem_col[p] = (uint64_t)1 << tp.tile[p];
    const auto at = std::find(tp.target.begin(), tp.target.end(), tp.tile[p]);
    if (at == tp.target.end()) {
      lds_col[p] = (uint64_t)1 << rank++;
      continue;
    }
    const int listed = (int)(at - tp.target.begin()), row_bit = k - 1 - listed; // the LAST listed target is row bit 0
    target_bit[listed] = (uint64_t)tp.tile[p], target_pos[listed] = (uint64_t)p;
    if (p < window) swizzle[row_bit] = (uint64_t)1 << (window - low_targets + seen++);
    lds_col[p] = ((uint64_t)1 << (gb + row_bit)) ^ swizzle[row_bit];
  }
}

// bit rb * nb + cb: block (rb, cb) of ARTN_WGATE_ROWS x ARTN_WGATE_ROWS entries of the rows x rows matrix has a non-zero
static uint64_t state_block_mask(const double *mat, int rows) {
  const int r = std::min(rows, ARTN_WGATE_ROWS), nb = rows / r;
  uint64_t mask = 0;
  for (int row = 0; row < rows; ++row)
    for (int col = 0; col < rows; ++col)
      if (mat[2 * (row * rows + col)] != 0.0 || mat[2 * (row * rows + col) + 1] != 0.0) mask |= (uint64_t)1 << ((row / r) * nb + col / r);
  return mask;
}

// f(std::integral_constant<int, K>) for the run-time k = LO .. HI; the plans admit no other k
template <int LO, int HI, typename F>
static void state_with_k(int k, F &&f) {
  if constexpr (LO <= HI) {
    if (k == LO) f(std::integral_constant<int, LO>());
    else state_with_k<LO + 1, HI>(k, f);
  }
}

// the fields every tile table begins with (ArtnWgateTable, ArtnMgateTable, the `gate` of ArtnChannelTable), from the plan
template <typename Table>
static void state_tile_header(const TilePlan &tp, int k, bool diagonal, Table &t) {
  t.k = (uint64_t)k, t.tile_bits = (uint64_t)tp.tb, t.n_tiles = (uint64_t)tp.n_tiles, t.segment = (uint64_t)tp.segment;
  t.flags = diagonal ? ARTN_GATE_DIAGONAL : 0, t.group_bits = (uint64_t)(tp.tb - k), t.n_high = (uint64_t)(tp.tb - tp.seg_bits);
  for (int j = tp.seg_bits; j < tp.tb; ++j) t.high_bit[j - tp.seg_bits] = (uint64_t)tp.tile[j]; // (all targets: include/artn.h)
  state_tile_cols(tp, t.mem_col, t.lds_col, t.target_bit, t.target_pos, t.swizzle);
}
