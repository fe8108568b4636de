// trace_open.h -- what the traces of full_orbit.hip, drift_kinetic.hip and model_trace.hip share on the device: the region
// rule of RemoveParticles (src/commands/remove_particles.cpp:22-38) for one particle, and the workgroup's tally of the
// lanes that are still alive at each sample of a launch and of the lanes the launch removed.  The list of live particles
// and its compaction are trace_open.hip's, the host driver is batch.h's batch_trace.
#pragma once

#include "common.h"
#include "device_common.h"

namespace xpic {

struct OpenRegion {
  int kind;        // XPIC_GEOM_BOX, XPIC_GEOM_CYLINDER; < 0 (XPIC_GEOM_NONE): no region, the closed trace
  double a[7];     // within()'s
  long long step0; // steps the batch has been traced before this call
};

constexpr int kOpenRows = 64; // sample rows one launch can reach: its steps, at most XPIC_FO_ / XPIC_DK_LAUNCH_STEPS

// the checks of an xpic_trace_region.  allow_none: XPIC_GEOM_NONE, "no region", is a geometry (the model traces);
// read_compact: the call compacts its list, so `compact` is checked (the grid traces)
inline int trace_region(const std::string& who, const xpic_trace_region* in, bool allow_none, bool read_compact, OpenRegion* R)
{
  XPIC_CHECK(in, who + ": region is null");
  XPIC_CHECK((allow_none && in->geometry == XPIC_GEOM_NONE) || in->geometry == XPIC_GEOM_BOX ||
      in->geometry == XPIC_GEOM_CYLINDER, who + ": unknown geometry kind");
  XPIC_CHECK(!read_compact || (in->compact >= XPIC_COMPACT_AUTO && in->compact <= XPIC_COMPACT_ALWAYS),
    who + ": compact must be 0 (auto), 1 (never) or 2 (always)");
  XPIC_CHECK(in->step0 >= 0, who + ": step0 is negative");
  R->kind = in->geometry;
  for (int i = 0; i < 7; ++i) R->a[i] = in->geom[i];
  R->step0 = in->step0;
  return 0;
}

// RemoveParticles keeps a cell iff its corner passes the test; the cell of r is FLOOR_STEP's (src/utils/utils.h:78), of
// the unfolded position.  A position that is not a number has no cell: it fails either geometry.
__device__ inline bool open_keep(const GridDev& g, const OpenRegion& R, const double* r)
{
  double pn[3];
  if (g.pow2) scaled_position<true>(g, r[0], r[1], r[2], pn);
  else scaled_position<false>(g, r[0], r[1], r[2], pn);
  return within(R.kind, R.a, floor(pn[0]) * g.dx, floor(pn[1]) * g.dy, floor(pn[2]) * g.dz);
}

// Called once by EVERY thread of a workgroup of BLOCK threads, after its lane's step loop (it synchronises).  live: the
// lane held a particle that was alive when the launch began; reached: first + the steps that particle completed; gone: the
// launch removed it.  The launch covers steps first + 1 .. first + ns; row r of `alive` belongs to step (r + 1) every, and
// a particle is alive at that sample iff it has completed the step.  Integer atomics: the sums do not depend on timing.
template <int BLOCK>
__device__ inline void open_tally(bool live, bool gone, long reached, long first, int ns, long every, long nsamp,
  unsigned long long* alive, unsigned long long* removed)
{
  __shared__ int sm[kOpenRows + 1][BLOCK / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int nrows = 0;
  long r0 = 0;
  if (alive) {
    r0 = first / every;                  // the first row whose step lies behind `first`
    long r1 = (first + ns) / every;      // one past the last row whose step the launch reaches
    r1 = r1 < nsamp ? r1 : nsamp;
    nrows = r1 > r0 ? (int)(r1 - r0) : 0;
    nrows = nrows < kOpenRows ? nrows : kOpenRows;
  }
  for (int t = 0; t < nrows; ++t) {
    const long step = (r0 + t + 1) * every;
    const int cnt = __popcll(__ballot(live && reached >= step));
    if (lane == 0) sm[t][wave] = cnt;
  }
  const int cg = __popcll(__ballot(gone));
  if (lane == 0) sm[kOpenRows][wave] = cg;
  __syncthreads();
  if ((int)threadIdx.x <= nrows) {
    const int t = (int)threadIdx.x == nrows ? kOpenRows : (int)threadIdx.x;
    int sum = 0;
#pragma unroll
    for (int w = 0; w < BLOCK / 64; ++w) sum += sm[t][w];
    if (sum) atomicAdd(t == kOpenRows ? removed : alive + r0 + t, (unsigned long long)sum);
  }
}

}  // namespace xpic
