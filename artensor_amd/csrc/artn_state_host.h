// artn_state_host.h -- host plumbing shared by the operations on a dense amplitude array (artn_born.hip, artn_rdm.hip,
// artn_pauli.hip, artn_gates.hip, artn_wgate.hip, artn_cgate.hip, artn_measure.hip, artn_channel.hip, artn_diag.hip, artn_bitperm.hip): the descriptor and layout checks, the max_rank rule and the
// rank dispatch of the run kernels, the matrix scan, the argument checks of the pack / apply entries and the parts of a packed
// table.  Codes and texts are part of the ABI's behaviour (tests/test_state_layout_cpu.py); each family keeps its own wording
// (`who`: "gate circuits take", ...) and its own precedence between the errors, so the pieces are separate functions.
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
