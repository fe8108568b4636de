// tracer_set.h -- a tracer set and the sets of a context as tracers.hip (their life and their advance) and
// tracer_moments.hip (their moments and maps, include/xpic_tracer_moments.h) both see them.  Host code only.
#pragma once

#include <algorithm>
#include <memory>
#include <string>
#include <vector>

#include "batch.h"
#include "common.h"
#include "trace_open.h"

namespace xpic {

// A map of a set: the accumulator the set's moment is added into at every step that is a multiple of `every`
struct TracerMap {
  int id = 0, kind = 0, dof = 0;
  double q = 0, m = 0, weight = 0;
  bool whole = true;    // no region6 was given
  int region6[6] = {};
  int64_t every = 1;
  int64_t deposits = 0; // deposits made since the map was created or last reset
  DevScratch<double> acc;               // [dof][nz][ny][nx]
  DevScratch<unsigned long long> count; // the particle-deposits counted since then
};

struct TracerSet {
  int id = 0, kind = 0;
  int64_t n = 0;
  xpic_fo_params fo{};
  xpic_dk_params dk{};
  OpenRegion R{};        // the region as given; without one: a box every finite position passes
  bool tracked = false;  // a region was given: the removed count is read back after every launch (the live list's input)
  int policy = XPIC_COMPACT_NEVER;
  int gradB = -1;        // drift kinetic: a field id, -1 or XPIC_GRADB_AUTO
  int64_t every = 0, cap = 0; // sample_every (0: none) and the rows the buffer holds
  int64_t done = 0;      // steps since creation
  int64_t base = 0;      // sample rows that were due before the buffer's row 0
  int64_t dropped = 0;   // rows lost to a full buffer before `base`
  bool attached = false;
  DevScratch<double> s, sm;      // the state [6][n], the sample rows [cap][6][n]
  DevScratch<int64_t> ex, tot, al, rm; // exit_step [n], iteration sums [n], alive [cap], the removed count
  DevScratch<int> mx;            // iteration maxima [n]
  LiveList L;
  std::vector<std::unique_ptr<TracerMap>> maps; // in creation order; empty: the set advances as it did without maps
  int next_map = 0;

  bool counters() const { return kind == XPIC_TRACERS_DRIFT_KINETIC || fo.scheme == XPIC_FO_CN; }
  int64_t due() const { return every > 0 ? done / every : 0; }           // rows due since creation
  int64_t held() const { return std::min(due() - base, cap); }          // rows in the buffer
  int64_t lost() const { return dropped + (due() - base - held()); }    // rows dropped since creation
};

struct TracerSets {
  std::vector<std::unique_ptr<TracerSet>> sets; // in creation order
  int next_id = 0;
  double* gradB = nullptr; // XPIC_GRADB_AUTO: grad |B|, allocated by the first advance that needs it; no field id names it
};

// tracers.hip: the set `id` of ctx, or an error whose message `who` heads
int tracers_find(xpic_ctx* ctx, const std::string& who, int id, TracerSet** out);
// tracer_moments.hip: the set has just reached step T.done; every map that is due there takes its deposit
int tracer_maps_deposit(xpic_ctx* ctx, TracerSet& T);

}  // namespace xpic
