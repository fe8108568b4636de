// full_orbit.hip -- full orbits of a batch of particles on the context's static E and B, the companion of
// drift_kinetic.hip (the reference's grid tests run the two side by side):
//   process_<id> for the 17 Chin ids     tests/boris_push/boris_push.h:20-198   (BorisPush, src/algorithms/boris_push.cpp)
//   CrankNicolsonPush::process           src/algorithms/crank_nicolson_push.cpp:31-71
// with the gathers of basic::Particles::push (src/impls/basic/particles.cpp:32-37) and ImplicitEsirkepov::interpolate
// (src/algorithms/implicit_esirkepov.cpp:63-91).  One lane per particle, fp64, no cross-lane operation, no atomics, no
// deposition: a lane reads the field vectors and writes its own six state slots, its own sample rows and its own
// iteration counters.  The state {x, y, z, px, py, pz} lives in structure-of-arrays device buffers (s[k * n + q]).
// Positions are not folded into the box: the gathers wrap their node indices (ie_node).  Single z-slab contexts only
// (G == 0: every index wraps, so no position, however far out, reads outside a field vector).
// Every loop is bounded by a constant or by an argument the entry points have range-checked: at most 4 nodes per axis,
// maxit <= XPIC_FO_MAXIT iterations, at most XPIC_FO_LAUNCH_STEPS steps per launch.  The staging of the host records, the
// push and trace drivers and the sample buffer's size are batch.h's, the trace's checks and its call trace_call.h's, shared
// with drift_kinetic.hip and model_trace.hip.
#include <algorithm>
#include <cmath>

#include "batch.h"
#include "common.h"
#include "device_common.h"
#include "ie_shape.h"
#include "trace_call.h"
#include "trace_open.h"

// contracted per source expression only (not across statements), so k_fo_push and k_fo_trace, which inline the same
// fo_step / fo_cn_process, round identically whatever surrounds the call
#pragma clang fp contract(on)

#include "full_orbit_step.h"

namespace xpic {

namespace {

constexpr int kBlock = kLaneBlock; // batch.h: lane_grid launches workgroups of this size
constexpr int kLaunchSteps = XPIC_FO_LAUNCH_STEPS;

// one step of P.scheme; CN: CrankNicolsonPush::process from the guess pn = p0, -> its iteration number
template <bool CN>
__device__ inline int fo_one(const GridDev& g, const double* __restrict__ E, const double* __restrict__ B,
  const xpic_fo_params& P, FOPoint& pn)
{
  if (CN) {
    const FOPoint p0 = pn;
    return fo_cn_process(g, E, B, P.qm, P.dt, P.atol, P.rtol, P.maxit, pn, p0);
  }
  fo_step(P.scheme, g, E, B, P.qm, P.dt, pn);
  return 0;
}

// iterations: written by the CN instance only
template <bool CN>
__global__ void __launch_bounds__(kBlock) k_fo_push(GridDev g, const double* __restrict__ E, const double* __restrict__ B,
  xpic_fo_params P, long n, const double* __restrict__ s0, double* __restrict__ sn, int* __restrict__ iterations)
{
  const long q = (long)blockIdx.x * kBlock + threadIdx.x;
  if (q >= n) return;
  FOPoint pn;
  fo_load(s0, n, q, pn);
  const int it = fo_one<CN>(g, E, B, P, pn);
  if (CN) iterations[q] = it;
  fo_store(sn, n, q, pn);
}

// steps first + 1 .. first + nsteps of a trace, in place; nsteps <= kLaunchSteps.  Step k (counted from 1) is sampled
// when sample_every divides it: sample k / sample_every - 1 of samples[sample][6][n], < nsamp by construction and
// checked again here.
template <bool CN>
__global__ void __launch_bounds__(kBlock) k_fo_trace(GridDev g, const double* __restrict__ E, const double* __restrict__ B,
  xpic_fo_params P, long n, double* __restrict__ s, long first, int nsteps, long sample_every, long nsamp,
  double* __restrict__ samples, long long* __restrict__ it_sum, int* __restrict__ it_max)
{
  const long q = (long)blockIdx.x * kBlock + threadIdx.x;
  if (q >= n) return;
  FOPoint pn;
  fo_load(s, n, q, pn);
  long long total = CN ? it_sum[q] : 0;
  int most = CN ? it_max[q] : 0;
  const int ns = nsteps < kLaunchSteps ? nsteps : kLaunchSteps;
  for (int k = 1; k <= ns; ++k) {
    const int it = fo_one<CN>(g, E, B, P, pn);
    total += it;
    most = it > most ? it : most;
    const long step = first + k;
    if (samples && step % sample_every == 0) {
      const long row = step / sample_every - 1;
      if (row < nsamp) fo_store(samples + row * 6 * n, n, q, pn);
    }
  }
  fo_store(s, n, q, pn);
  if (CN) { it_sum[q] = total; it_max[q] = most; }
}

// k_fo_trace with the region rule of an open trace (trace_open.h) over the m entries of `list` (null:
// the particles 0 .. m - 1).  A lane whose particle is alive tests the corner of its cell at the top of every step and
// leaves the loop when the test fails: exit_step = step0 + the steps completed, the state as it was.  The step itself is
// fo_one, as in k_fo_push and k_fo_trace.  Every thread reaches open_tally.  The two traces stay two texts: folded as
// k_dk_trace is (drift_kinetic.hip), the closed Crank-Nicolson instance would run one wave per SIMD where it runs two
// (DESIGN.md 5q).
static_assert(kLaunchSteps <= kOpenRows, "open_tally holds one row per step of a launch");
template <bool CN>
__global__ void __launch_bounds__(kBlock) k_fo_trace_open(GridDev g, const double* __restrict__ E,
  const double* __restrict__ B, xpic_fo_params P, OpenRegion R, long n, double* __restrict__ s,
  const long long* __restrict__ list, long m, long first, int nsteps, long sample_every, long nsamp,
  double* __restrict__ samples, long long* __restrict__ it_sum, int* __restrict__ it_max, long long* __restrict__ exit_step,
  unsigned long long* alive, unsigned long long* removed)
{
  const long j = (long)blockIdx.x * kBlock + threadIdx.x;
  const long q = j < m ? (list ? (long)list[j] : j) : -1;
  const bool live = q >= 0 && q < n && exit_step[q] < 0;
  const int ns = nsteps < kLaunchSteps ? nsteps : kLaunchSteps;
  int done = 0;
  bool gone = false;
  if (live) {
    FOPoint pn;
    fo_load(s, n, q, pn);
    long long total = CN ? it_sum[q] : 0;
    int most = CN ? it_max[q] : 0;
    for (; done < ns; ++done) {
      if (!open_keep(g, R, pn.r)) { gone = true; break; }
      const int it = fo_one<CN>(g, E, B, P, pn);
      total += it;
      most = it > most ? it : most;
      const long step = first + done + 1;
      if (samples && step % sample_every == 0) {
        const long row = step / sample_every - 1;
        if (row < nsamp) fo_store(samples + row * 6 * n, n, q, pn);
      }
    }
    fo_store(s, n, q, pn);
    if (CN) { it_sum[q] = total; it_max[q] = most; }
    if (gone) exit_step[q] = R.step0 + first + done;
  }
  open_tally<kBlock>(live, gone, first + done, first, ns, sample_every, nsamp, alive, removed);
}

// the checks the three calls share
int fo_check(xpic_ctx* ctx, int64_t n, const xpic_fo_params* P)
{
  XPIC_CHECK(ctx != nullptr, "null context");
  XPIC_CHECK(n >= 0, "full_orbit: n is negative");
  XPIC_CHECK(n <= ((int64_t)1 << 36), "full_orbit: n is larger than 2^36");
  XPIC_CHECK(ctx->geom.nranks == 1 && ctx->g.G == 0,
    "full_orbit: a context of several z-slabs (or a self_ring one) is not supported: the gathers wrap z in the kernel");
  XPIC_CALL(fo_check_params("full_orbit", P));
  XPIC_CHECK(ctx->field[XPIC_E] && ctx->field[XPIC_B], "full_orbit: the context has no E or B");
  return 0;
}

// both traces, after fo_check; region: null for the closed trace.  A Chin id has no iterations: its launches get null
// counters
int fo_trace(xpic_ctx* ctx, const TraceEntry& E, const xpic_fo_params& P, const TraceArrays& A, const xpic_trace_region* region)
{
  const bool cn = A.counters;
  const long n = (long)A.n, every = (long)A.sample_every;
  OpenRegion R{XPIC_GEOM_NONE, {}, 0};
  if (!E.closed) XPIC_CALL(trace_region(E.who, region, false, true, &R));
  return trace_call(ctx, E, kLaunchSteps, A, R, E.closed ? XPIC_COMPACT_NEVER : region->compact, nullptr,
    [&](const TraceDev& d) {
      if (E.closed) // its text takes no region: the driver's stand-ins for exit_step and removed stay unused
        hipLaunchKernelGGL(cn ? k_fo_trace<true> : k_fo_trace<false>, lane_grid(n), dim3(kBlock), 0, ctx->stream, ctx->g,
          ctx->field[XPIC_E], ctx->field[XPIC_B], P, n, d.s, d.first, d.ns, every, d.nsamp, d.samples, d.it_sum, d.it_max);
      else fo_launch_open(ctx, P, R, n, every, d);
    });
}

}  // namespace

// one launch of the open trace (trace_call.h): the entry point above and the tracer sets of tracers.hip start it here
void fo_launch_open(xpic_ctx* ctx, const xpic_fo_params& P, const OpenRegion& R, long n, long every, const TraceDev& d)
{
  hipLaunchKernelGGL(P.scheme == XPIC_FO_CN ? k_fo_trace_open<true> : k_fo_trace_open<false>, lane_grid(d.m), dim3(kBlock), 0,
    ctx->stream, ctx->g, ctx->field[XPIC_E], ctx->field[XPIC_B], P, R, n, d.s, d.list, d.m, d.first, d.ns, every, d.nsamp,
    d.samples, d.it_sum, d.it_max, d.exit_step, d.alive, d.removed);
}

}  // namespace xpic

using namespace xpic;

extern "C" {

int xpic_full_orbit_push(xpic_ctx* ctx, int64_t n, const xpic_fo_params* params, const double* p0_6, double* pn_6,
  int* iterations)
{ // process_<id>, tests/boris_push/boris_push.h:20-198; CrankNicolsonPush::process, crank_nicolson_push.cpp:31-71
  XPIC_CALL(fo_check(ctx, n, params));
  const bool cn = params->scheme == XPIC_FO_CN;
  XPIC_CHECK(p0_6, "full_orbit_push: p0_6 is null");
  XPIC_CHECK(pn_6, "full_orbit_push: pn_6 is null");
  XPIC_CHECK(iterations || !cn, "full_orbit_push: iterations is null");
  if (n == 0) return 0;
  XPIC_CALL(batch_push(ctx, "fo_push", n, cn, p0_6, pn_6, iterations, [&](const double* s0, double* sn, int* it) {
    hipLaunchKernelGGL(cn ? k_fo_push<true> : k_fo_push<false>, lane_grid(n), dim3(kBlock), 0, ctx->stream, ctx->g,
      ctx->field[XPIC_E], ctx->field[XPIC_B], *params, (long)n, s0, sn, it);
  }));
  if (!cn && iterations) std::fill(iterations, iterations + n, 0);
  return 0;
}

int xpic_full_orbit_trace(xpic_ctx* ctx, int64_t n, const xpic_fo_params* params, int64_t steps, int64_t sample_every,
  double* p_6, double* samples, int64_t* iterations_sum, int* iterations_max)
{ // the time loops of boris_push_ex1.cpp:51-60 and crank_nicolson_push_ex2.cpp:43-56
  XPIC_CALL(fo_check(ctx, n, params));
  const bool cn = params->scheme == XPIC_FO_CN;
  return fo_trace(ctx, {"full_orbit_trace", "p_6", "iterations_sum", "iterations_max", true, "fo_trace", "fo_trace"}, *params,
    {n, steps, sample_every, p_6, samples, iterations_sum, iterations_max, nullptr, nullptr, nullptr, cn, nullptr}, nullptr);
}

int xpic_full_orbit_trace_open(xpic_ctx* ctx, int64_t n, const xpic_fo_params* params, int64_t steps, int64_t sample_every,
  double* p_6, double* samples, int64_t* iterations_sum, int* iterations_max, const xpic_trace_region* region,
  int64_t* exit_step, int64_t* alive, int64_t* removed)
{ // xpic_full_orbit_trace with RemoveParticles::execute (remove_particles.cpp:22-38) at the top of every step
  XPIC_CALL(fo_check(ctx, n, params));
  const bool cn = params->scheme == XPIC_FO_CN;
  return fo_trace(ctx,
    {"full_orbit_trace_open", "p_6", "iterations_sum", "iterations_max", false, "fo_trace_open", "fo_trace_open_compact"},
    *params, {n, steps, sample_every, p_6, samples, iterations_sum, iterations_max, exit_step, alive, removed, cn, nullptr},
    region);
}

}  // extern "C"
