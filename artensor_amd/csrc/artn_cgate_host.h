// artn_cgate_host.h -- what the host halves of the two controlled-gate families share (artn_cgate.hip: one gate for the whole
// state; artn_cgate_batch.hip: a gate per trajectory): the plan record, the checks of the head of a plan, the targets and the
// controls with their classes, the holes of the tile walk, and the tile fields of an ArtnCgateTable (include/artn.h: PLAN of
// artn_cgate_query).  `who` is the family's wording ("controlled gates take", "conditional gates take").
#pragma once
#include <algorithm>
#include <string>
#include <vector>

#include "artn_host.h"
#include "artn_state_host.h"

struct CgatePlan : TilePlan {
  int t = 0, c = 0, n_bits = 0, c_high = 0;
  std::vector<int> control; // memory bits in the order listed
  std::vector<int> value;   // the wanted digit of each control
  std::vector<int> hole;    // hole bits, ascending
  uint64_t high_mask = 0, high_want = 0, low_mask = 0, low_want = 0; // over memory bits
  ArtnCgateInfo info = {};
};

// Descriptor, pointers, layout, t and c.  n: the elements of the state.
static int cgate_head(const ArtnMarginalDesc *d, int32_t t, const int32_t *targets, int32_t c, const int32_t *controls, const char *who,
                      const char *what, CgatePlan &cp, int64_t &n) {
  if (int rc = state_desc(d, who, ARTN_MARG_MAX_DIMS, false)) return rc;
  if (!targets || (c > 0 && !controls)) return fail(ARTN_E_INVALID, "null pointer");
  StateLayout l;
  if (int rc = state_layout(d, l)) return rc;
  if (int rc = state_bits_only(l, who)) return rc;
  n = l.n;
  if (t < 1 || t > ARTN_WGATE_MAX_K)
    return fail(ARTN_E_UNSUPPORTED, std::string(what) + " act on one to five target dimensions, not " + std::to_string(t));
  if (c < 0) return fail(ARTN_E_INVALID, "a negative number of controls: " + std::to_string(c));
  cp.t = t, cp.c = c, cp.n_bits = __builtin_ctzll((uint64_t)n);
  return ARTN_OK;
}

// The targets, then the controls: a control at or above a 128-byte line is HIGH, one below it LOW.  `seen` collects the
// dimensions in the order listed.
static int cgate_dims(const ArtnMarginalDesc *d, const int32_t *targets, const int32_t *controls, const int32_t *values, CgatePlan &cp,
                      std::vector<int32_t> &seen) {
  const int t = cp.t, c = cp.c;
  const int lb = d->dtype == ARTN_C64 ? 4 : 3; // index bits of a 128-byte line
  for (int j = 0; j < t; ++j) {
    if (int rc = state_tile_dim(d, targets[j], seen, (size_t)t, false, "gates")) return rc;
    seen.push_back(targets[j]);
    cp.target.push_back(__builtin_ctzll((uint64_t)d->stride[targets[j]]));
  }
  for (int j = 0; j < c; ++j) {
    if (int rc = state_tile_dim(d, controls[j], seen, (size_t)t, true, "gates")) return rc;
    seen.push_back(controls[j]);
    const int v = values ? values[j] : 1;
    if (v != 0 && v != 1)
      return fail(ARTN_E_INVALID, "a control value is 0 or 1; control " + std::to_string(j) + " has " + std::to_string(v));
    const int b = __builtin_ctzll((uint64_t)d->stride[controls[j]]);
    cp.control.push_back(b), cp.value.push_back(v);
    if (b >= lb) cp.high_mask |= (uint64_t)1 << b, cp.high_want |= (uint64_t)v << b, ++cp.c_high;
    else cp.low_mask |= (uint64_t)1 << b, cp.low_want |= (uint64_t)v << b;
  }
  return ARTN_OK;
}

// After state_tile_plan: the holes are the tile bits above the contiguous part and the high controls, ascending.
static int cgate_holes(CgatePlan &cp, const char *who) {
  for (int j = cp.seg_bits; j < cp.tb; ++j) cp.hole.push_back(cp.tile[j]);
  for (int b = 0; b < cp.n_bits; ++b)
    if ((cp.high_mask >> b) & 1) cp.hole.push_back(b);
  std::sort(cp.hole.begin(), cp.hole.end());
  if ((int)cp.hole.size() > ARTN_CGATE_MAX_HOLES) return fail(ARTN_E_UNSUPPORTED, std::string(who) + " at most 2^40 elements");
  return ARTN_OK;
}

// Every field of the table but flags and block_mask, which belong to the matrix.
static void cgate_tile_fields(const CgatePlan &cp, ArtnCgateTable &tab) {
  const int t = cp.t, gb = cp.tb - t;
  tab.t = (uint64_t)t, tab.tile_bits = (uint64_t)cp.tb, tab.n_tiles = (uint64_t)cp.n_tiles, tab.segment = (uint64_t)cp.segment;
  tab.group_bits = (uint64_t)gb, tab.segment_bits = (uint64_t)cp.seg_bits;
  tab.n_holes = (uint64_t)cp.hole.size(), tab.high_want = cp.high_want, tab.high_mask = cp.high_mask;
  for (size_t j = 0; j < cp.hole.size(); ++j) tab.hole_bit[j] = (uint64_t)cp.hole[j];
  state_tile_cols(cp, tab.mem_col, tab.lds_col, tab.target_bit, tab.target_pos, tab.swizzle);
  for (int p = 0; p < cp.tb; ++p) // a low control is a non-target tile bit, so a group bit: the one its lds_col names
    if ((cp.low_mask >> cp.tile[p]) & 1) {
      tab.group_mask |= tab.lds_col[p];
      if ((cp.low_want >> cp.tile[p]) & 1) tab.group_want |= tab.lds_col[p];
    }
}
