// drift_kinetic.hip -- the reference's drift-kinetic (guiding-centre) pusher with its grid interpolation:
//   DriftKineticEsirkepov::interpolate   src/algorithms/drift_kinetic_implicit.cpp:11-31
//   DriftKineticPush::process            src/algorithms/drift_kinetic_push.cpp:48-160
//   PointByField                         src/interfaces/point.h:37-58
// One lane per particle, fp64, no cross-lane operation: the lanes of a wave leave the Picard loop independently.  The
// state {x, y, z, p_parallel, p_perp, mu_p} lives in structure-of-arrays device buffers (s[k * n + q]).  Positions are
// not folded into the box: the gathers wrap their node indices (ie_node), folding is the caller's business as
// correct_coordinates is in the reference.  Single z-slab contexts only (G == 0: every index wraps, so no position,
// however far out, reads outside a field vector).  The C entry points and their argument checks are at the end of the
// file; the staging of the host records, the push and trace drivers and the sample buffer's size are batch.h's, the
// trace's checks and its call trace_call.h's.
#include "batch.h"
#include "common.h"
#include "device_common.h"
#include "ie_shape.h"
#include "trace_call.h"
#include "trace_open.h"

// The pusher's own expressions are contracted per source expression only (not across statements), so k_dk_push and
// k_dk_trace, which inline the same dk_process, round identically whatever surrounds the call.  (The segment shape in
// ie_shape.h keeps the build's default, as in eccapfim.hip: the E gather here returns k_ie_interpolate's bits.)
#pragma clang fp contract(on)

#include "drift_kinetic_step.h"

namespace xpic {

namespace {

constexpr int kBlock = kLaneBlock; // batch.h: lane_grid launches workgroups of this size

template <bool GRAD>
__global__ void __launch_bounds__(kBlock) k_dk_interpolate(GridDev g, const double* __restrict__ E,
  const double* __restrict__ B, const double* __restrict__ gB, long n, const double* rn3, const double* r03, double* Ep3,
  double* Bp3, double* gBp3)
{
  const long q = (long)blockIdx.x * kBlock + threadIdx.x;
  if (q >= n) return;
  const double rn[3] = {rn3[3 * q], rn3[3 * q + 1], rn3[3 * q + 2]}, r0[3] = {r03[3 * q], r03[3 * q + 1], r03[3 * q + 2]};
  double Ep[3], Bp[3], gBp[3];
  dk_fields<GRAD>(g, E, B, gB, rn, r0, Ep, Bp, gBp);
#pragma unroll
  for (int c = 0; c < 3; ++c) { Ep3[3 * q + c] = Ep[c]; Bp3[3 * q + c] = Bp[c]; gBp3[3 * q + c] = gBp[c]; }
}

template <bool GRAD>
__global__ void __launch_bounds__(kBlock) k_dk_push(GridDev g, const double* __restrict__ E, const double* __restrict__ B,
  const double* __restrict__ gB, xpic_dk_params P, long n, const double* __restrict__ s0, double* __restrict__ sn,
  int* __restrict__ iterations)
{
  const long q = (long)blockIdx.x * kBlock + threadIdx.x;
  if (q >= n) return;
  DKPoint p0, pn;
  dk_load(s0, n, q, p0);
  pn = p0;
  iterations[q] = dk_process<GRAD>(g, E, B, gB, P, p0, pn);
  dk_store(sn, n, q, pn);
}

// steps first + 1 .. first + nsteps of a trace, in place.  Step k (counted from 1) is sampled when sample_every divides
// it: sample k / sample_every - 1 of samples[sample][6][n].
template <bool GRAD>
__global__ void __launch_bounds__(kBlock) k_dk_trace(GridDev g, const double* __restrict__ E, const double* __restrict__ B,
  const double* __restrict__ gB, xpic_dk_params P, long n, double* __restrict__ s, long first, int nsteps, long sample_every,
  double* __restrict__ samples, long long* __restrict__ it_total, int* __restrict__ it_max)
{
  const long q = (long)blockIdx.x * kBlock + threadIdx.x;
  if (q >= n) return;
  DKPoint p0, pn;
  dk_load(s, n, q, pn);
  long long total = it_total[q];
  int most = it_max[q];
  for (int k = 1; k <= nsteps; ++k) {
    p0 = pn;
    const int it = dk_process<GRAD>(g, E, B, gB, P, p0, pn);
    total += it;
    most = it > most ? it : most;
    const long step = first + k;
    if (samples && step % sample_every == 0) dk_store(samples + (step / sample_every - 1) * 6 * n, n, q, pn);
  }
  dk_store(s, n, q, pn);
  it_total[q] = total;
  it_max[q] = most;
}

// k_dk_trace with the region rule of an open trace (trace_open.h) over the m entries of `list` (null: the
// particles 0 .. m - 1): as k_fo_trace_open, the step being dk_process as in k_dk_push and k_dk_trace.  The two traces
// stay two texts: folded as k_model_dk_trace is, the closed trace measured 0.8 - 1.1 % slower, outside the margin
// (DESIGN.md 5q).
static_assert(XPIC_DK_LAUNCH_STEPS <= kOpenRows, "open_tally holds one row per step of a launch");
template <bool GRAD>
__global__ void __launch_bounds__(kBlock) k_dk_trace_open(GridDev g, const double* __restrict__ E,
  const double* __restrict__ B, const double* __restrict__ gB, xpic_dk_params P, OpenRegion R, long n, double* __restrict__ s,
  const long long* __restrict__ list, long m, long first, int nsteps, long sample_every, long nsamp,
  double* __restrict__ samples, long long* __restrict__ it_total, int* __restrict__ it_max, long long* __restrict__ exit_step,
  unsigned long long* alive, unsigned long long* removed)
{
  const long j = (long)blockIdx.x * kBlock + threadIdx.x;
  const long q = j < m ? (list ? (long)list[j] : j) : -1;
  const bool live = q >= 0 && q < n && exit_step[q] < 0;
  const int ns = nsteps < XPIC_DK_LAUNCH_STEPS ? nsteps : XPIC_DK_LAUNCH_STEPS;
  int done = 0;
  bool gone = false;
  if (live) {
    DKPoint p0, pn;
    dk_load(s, n, q, pn);
    long long total = it_total[q];
    int most = it_max[q];
    for (; done < ns; ++done) {
      if (!open_keep(g, R, pn.r)) { gone = true; break; }
      p0 = pn;
      const int it = dk_process<GRAD>(g, E, B, gB, P, p0, pn);
      total += it;
      most = it > most ? it : most;
      const long step = first + done + 1;
      if (samples && step % sample_every == 0) {
        const long row = step / sample_every - 1;
        if (row < nsamp) dk_store(samples + row * 6 * n, n, q, pn);
      }
    }
    dk_store(s, n, q, pn);
    it_total[q] = total;
    it_max[q] = most;
    if (gone) exit_step[q] = R.step0 + first + done;
  }
  open_tally<kBlock>(live, gone, first + done, first, ns, sample_every, nsamp, alive, removed);
}

// the checks the three calls share; *gradB: the vector of gradB_field, null for -1 (grad B = 0)
int dk_check(xpic_ctx* ctx, int64_t n, int gradB_field, const double** gradB)
{
  XPIC_CHECK(ctx != nullptr, "null context");
  XPIC_CHECK(n >= 0, "drift_kinetic: n is negative");
  XPIC_CHECK(ctx->geom.nranks == 1 && ctx->g.G == 0,
    "drift_kinetic: a context of several z-slabs (or a self_ring one) is not supported: the gathers wrap z in the kernel");
  XPIC_CHECK(gradB_field == -1 || (gradB_field >= 0 && gradB_field < XPIC_NFIELDS && ctx->field[gradB_field]),
    "drift_kinetic: gradB_field is neither -1 nor an allocated field id");
  *gradB = gradB_field == -1 ? nullptr : ctx->field[gradB_field];
  return 0;
}

// both traces, after dk_check; region: null for the closed trace
int dk_trace(xpic_ctx* ctx, const TraceEntry& E, const xpic_dk_params* params, const double* gradB, const TraceArrays& A,
  const xpic_trace_region* region)
{
  XPIC_CALL(dk_check_params("drift_kinetic", params, 0));
  const long n = (long)A.n, every = (long)A.sample_every;
  OpenRegion R{XPIC_GEOM_NONE, {}, 0};
  if (!E.closed) XPIC_CALL(trace_region(E.who, region, false, true, &R));
  return trace_call(ctx, E, XPIC_DK_LAUNCH_STEPS, A, R, E.closed ? XPIC_COMPACT_NEVER : region->compact, nullptr,
    [&](const TraceDev& d) {
      if (E.closed) // its text takes no region: the driver's stand-ins for exit_step and removed stay unused
        hipLaunchKernelGGL(gradB ? k_dk_trace<true> : k_dk_trace<false>, lane_grid(n), dim3(kBlock), 0, ctx->stream, ctx->g,
          ctx->field[XPIC_E], ctx->field[XPIC_B], gradB, *params, n, d.s, d.first, d.ns, every, d.samples, d.it_sum, d.it_max);
      else dk_launch_open(ctx, *params, gradB, R, n, every, d);
    });
}

}  // namespace

// one launch of the open trace (trace_call.h): the entry point above and the tracer sets of tracers.hip start it here
void dk_launch_open(xpic_ctx* ctx, const xpic_dk_params& P, const double* gradB, const OpenRegion& R, long n, long every,
  const TraceDev& d)
{
  hipLaunchKernelGGL(gradB ? k_dk_trace_open<true> : k_dk_trace_open<false>, lane_grid(d.m), dim3(kBlock), 0, ctx->stream,
    ctx->g, ctx->field[XPIC_E], ctx->field[XPIC_B], gradB, P, R, n, d.s, d.list, d.m, d.first, d.ns, every, d.nsamp, d.samples,
    d.it_sum, d.it_max, d.exit_step, d.alive, d.removed);
}

}  // namespace xpic

using namespace xpic;

extern "C" {

int xpic_drift_kinetic_interpolate(xpic_ctx* ctx, int64_t n, const double* rn3, const double* r03, int gradB_field,
  double* Ep3, double* Bp3, double* gradBp3)
{ // DriftKineticEsirkepov::interpolate, drift_kinetic_implicit.cpp:11-31
  const double* gradB;
  XPIC_CALL(dk_check(ctx, n, gradB_field, &gradB));
  XPIC_CHECK(rn3, "drift_kinetic_interpolate: rn3 is null");
  XPIC_CHECK(r03, "drift_kinetic_interpolate: r03 is null");
  XPIC_CHECK(Ep3, "drift_kinetic_interpolate: Ep3 is null");
  XPIC_CHECK(Bp3, "drift_kinetic_interpolate: Bp3 is null");
  XPIC_CHECK(gradBp3, "drift_kinetic_interpolate: gradBp3 is null");
  if (n == 0) return 0;
  DevScratch<double> a, b, o;
  XPIC_CALL(a.alloc(3 * n)); XPIC_CALL(b.alloc(3 * n)); XPIC_CALL(o.alloc(9 * n));
  XPIC_CALL(upload(a, rn3, 3 * n, ctx->stream));
  XPIC_CALL(upload(b, r03, 3 * n, ctx->stream));
  {
    Timed t(ctx, "dk_interpolate");
    hipLaunchKernelGGL(gradB ? k_dk_interpolate<true> : k_dk_interpolate<false>, lane_grid(n), dim3(kBlock), 0, ctx->stream,
      ctx->g, ctx->field[XPIC_E], ctx->field[XPIC_B], gradB, (long)n, (const double*)a.p, (const double*)b.p, o.p, o.p + 3 * n,
      o.p + 6 * n);
    XPIC_HIP(hipGetLastError());
  }
  XPIC_CALL(download(Ep3, o, 3 * n, ctx->stream));
  XPIC_CALL(download(Bp3, o, 3 * n, ctx->stream, 3 * n));
  XPIC_CALL(download(gradBp3, o, 3 * n, ctx->stream, 6 * n));
  XPIC_HIP(hipStreamSynchronize(ctx->stream));
  return 0;
}

int xpic_drift_kinetic_push(xpic_ctx* ctx, int64_t n, const xpic_dk_params* params, int gradB_field, const double* p0_6,
  double* pn_6, int* iterations)
{ // DriftKineticPush::process, drift_kinetic_push.cpp:48-108
  const double* gradB;
  XPIC_CALL(dk_check(ctx, n, gradB_field, &gradB));
  XPIC_CALL(dk_check_params("drift_kinetic", params, 0));
  XPIC_CHECK(p0_6, "drift_kinetic_push: p0_6 is null");
  XPIC_CHECK(pn_6, "drift_kinetic_push: pn_6 is null");
  XPIC_CHECK(iterations, "drift_kinetic_push: iterations is null");
  if (n == 0) return 0;
  return batch_push(ctx, "dk_push", n, true, p0_6, pn_6, iterations, [&](const double* s0, double* sn, int* it) {
    hipLaunchKernelGGL(gradB ? k_dk_push<true> : k_dk_push<false>, lane_grid(n), dim3(kBlock), 0, ctx->stream, ctx->g,
      ctx->field[XPIC_E], ctx->field[XPIC_B], gradB, *params, (long)n, s0, sn, it);
  });
}

int xpic_drift_kinetic_trace(xpic_ctx* ctx, int64_t n, const xpic_dk_params* params, int gradB_field, int64_t steps,
  int64_t sample_every, double* state_6, double* samples, int64_t* iterations_total, int* iterations_max)
{
  const double* gradB;
  XPIC_CALL(dk_check(ctx, n, gradB_field, &gradB));
  return dk_trace(ctx, {"drift_kinetic_trace", "state_6", "iterations_total", "iterations_max", true, "dk_trace", "dk_trace"},
    params, gradB,
    {n, steps, sample_every, state_6, samples, iterations_total, iterations_max, nullptr, nullptr, nullptr, true, nullptr},
    nullptr);
}

int xpic_drift_kinetic_trace_open(xpic_ctx* ctx, int64_t n, const xpic_dk_params* params, int gradB_field, int64_t steps,
  int64_t sample_every, double* state_6, double* samples, int64_t* iterations_total, int* iterations_max,
  const xpic_trace_region* region, int64_t* exit_step, int64_t* alive, int64_t* removed)
{ // xpic_drift_kinetic_trace with RemoveParticles::execute (remove_particles.cpp:22-38) at the top of every step
  const double* gradB;
  XPIC_CALL(dk_check(ctx, n, gradB_field, &gradB));
  const TraceEntry E{"drift_kinetic_trace_open", "state_6", "iterations_total", "iterations_max", false, "dk_trace_open",
    "dk_trace_open_compact"};
  return dk_trace(ctx, E, params, gradB,
    {n, steps, sample_every, state_6, samples, iterations_total, iterations_max, exit_step, alive, removed, true, nullptr},
    region);
}

}  // extern "C"
