// model_trace.hip -- the tracers on an analytic field model instead of the context's grid: the
// reference's examples that feed their pusher through set_fields_callback with a closed-form field,
//   tests/drift_kinetic_push/drift_kinetic_push_ex1 .. ex5, ex9.cpp     DriftKineticPush (callback at rn)
//   tests/boris_push/boris_push_ex*.cpp, drift_kinetic_push_ex9.cpp     process_<id> (fields at the particle's r)
//   tests/crank_nicolson_push/crank_nicolson_push_ex1, ex2.cpp, ex9     CrankNicolsonPush (ex9.cpp:75-78: at (r1 + r0) / 2)
// for a batch, and the same traces with a time envelope on the model's E: the one pusher example whose
// callback captures the step index,
//   tests/crank_nicolson_push/crank_nicolson_push_ex3.cpp:39-58         E_p = E0 * (t * dt); B_p = B0;
// with the running sums of its two checks (:51-57) kept on the device.  The models are field_model.h's; the step
// arithmetic is full_orbit_step.h's and drift_kinetic_step.h's own text, instantiated with a field source that evaluates
// the model in registers where the grid source gathers.  The drift-kinetic kernel is one text for both: its Clock yields
// the field source of a step, ModelSource (model_source.h) for the static clock and TimedModelSource (timed_source.h)
// with the factor of step R.step0 + first + done for the envelope clock.  The full-orbit kernel has two texts,
// k_model_fo_trace<CN> and k_timed_fo_trace<CN, SUMS>, which forms the same source at the top of every step (DESIGN.md
// 5o has the measurement that keeps them apart).  Either way every field evaluation inside a step sees the
// same factor.  One lane per particle, fp64, no cross-lane operation but open_tally's.  Each kernel serves the closed
// trace, the open trace and the one-step push: the region rule (trace_open.h) is skipped for XPIC_GEOM_NONE, which the
// host passes as R.kind < 0.  No grid vector is read, so no index is formed from a position and any context will do.
// Every loop is bounded by a constant or by an argument the entry points have range-checked: fo maxit <= XPIC_FO_MAXIT,
// 1 <= dk maxit <= XPIC_MODEL_DK_MAXIT, at most XPIC_MODEL_LAUNCH_STEPS steps per launch.  Every global index is formed
// under q < n, row < nsamp, i < nown or i < nsteps.  The trace's checks and its call are trace_call.h's, shared with the
// grid traces; the staging is batch.h's batch_trace with the "never" policy; sums_4 travels as [4][n] beside it.
#include <algorithm>
#include <cmath>
#include <vector>

#include "batch.h"
#include "common.h"
#include "device_common.h"
#include "field_model.h"
#include "ie_shape.h"
#include "trace_call.h"
#include "trace_open.h"

// as in full_orbit.hip and drift_kinetic.hip: contracted per source expression only
#pragma clang fp contract(on)

#include "full_orbit_step.h"
#include "drift_kinetic_step.h"
#include "model_source.h"
#include "timed_source.h"

namespace xpic {

namespace {

constexpr int kBlock = kLaneBlock; // batch.h: lane_grid launches workgroups of this size
constexpr int kLaunchSteps = XPIC_MODEL_LAUNCH_STEPS;
static_assert(kLaunchSteps <= kOpenRows, "open_tally holds one row per step of a launch");

// What yields the field source of a step (counted from the start of the whole trace).  k_model_dk_trace takes its clock
// by value where the model stood in the argument list.  The static clock: the model as it is.
struct StaticClock {
  xpic_field_model M;
  __device__ inline ModelSource at(long long, double) const { return ModelSource{M}; }
};
// The envelope clock: the model with the step's factor on E; a constant envelope multiplies nothing (on == false)
struct EnvelopeClock {
  xpic_field_model M;
  xpic_field_envelope V;
  __device__ inline TimedModelSource at(long long step, double dt) const
  {
    return TimedModelSource{{M}, V.kind != XPIC_ENV_CONSTANT, envelope_factor(V, step, dt)};
  }
};

__global__ void __launch_bounds__(kBlock) k_model_fields(xpic_field_model M, long n, const double* __restrict__ r3,
  double* __restrict__ out)
{
  const long q = (long)blockIdx.x * kBlock + threadIdx.x;
  if (q >= n) return;
  const double r[3] = {r3[3 * q], r3[3 * q + 1], r3[3 * q + 2]};
  double E[3], B[3], gB[3];
  model_fields(M, r, E, B, gB);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    out[3 * q + c] = E[c];
    out[3 * n + 3 * q + c] = B[c];
    out[6 * n + 3 * q + c] = gB[c];
  }
}

// FieldContext::initialize (drift_kinetic_push.h:191-199), one thread per owned node as k_mirror (commands.hip): all
// three components of node (x, y, z) are the model at (x dx, y dy, z dz); a null vector is skipped
__global__ void __launch_bounds__(kBlock) k_set_model_field(GridDev g, xpic_field_model M, double* E, double* B, double* gB)
{
  const long i = (long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= g.nown) return;
  const int x = (int)(i % g.nx), y = (int)((i / g.nx) % g.ny), zl = (int)(i / g.plane);
  const int z = g.z0 + zl;
  const long nd = g.node(x, y, g.wz(zl));
  const double r[3] = {x * g.dx, y * g.dy, z * g.dz};
  double Ep[3], Bp[3], gBp[3];
  model_fields(M, r, Ep, Bp, gBp);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    if (E) E[c * g.cstride + nd] = Ep[c];
    if (B) B[c * g.cstride + nd] = Bp[c];
    if (gB) gB[c * g.cstride + nd] = gBp[c];
  }
}

// k_fo_trace_open (full_orbit.hip) on the model, without a list; R.kind < 0: no region rule
template <bool CN>
__global__ void __launch_bounds__(kBlock) k_model_fo_trace(GridDev g, xpic_field_model M, xpic_fo_params P, OpenRegion R,
  long n, double* __restrict__ s, long first, int nsteps, long sample_every, long nsamp, double* __restrict__ samples,
  long long* __restrict__ it_sum, int* __restrict__ it_max, long long* __restrict__ exit_step, unsigned long long* alive,
  unsigned long long* removed)
{
  const long q = (long)blockIdx.x * kBlock + threadIdx.x;
  const bool live = q < n && exit_step[q] < 0;
  const int ns = nsteps < kLaunchSteps ? nsteps : kLaunchSteps;
  const ModelSource src{M};
  int done = 0;
  bool gone = false;
  if (live) {
    FOPoint pn;
    fo_load(s, n, q, pn);
    long long total = CN ? it_sum[q] : 0;
    int most = CN ? it_max[q] : 0;
    for (; done < ns; ++done) {
      if (R.kind >= 0 && !open_keep(g, R, pn.r)) { gone = true; break; }
      int it = 0;
      if (CN) {
        const FOPoint p0 = pn;
        it = fo_cn_process(src, P.qm, P.dt, P.atol, P.rtol, P.maxit, pn, p0);
      }
      else fo_step(P.scheme, src, P.qm, P.dt, pn);
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

// the terms of ex3's two checks for the step p0 -> pn (ex3.cpp:51-57), added to the lane's sums: the energy balance
// with the work of the step's E at the midpoint, and vh.transverse_to(B_s) (Vector3::parallel_to / transverse_to,
// src/utils/vector3.h:195-205, statement by statement)
__device__ inline void ex3_sums(const TimedModelSource& src, double qm, double dt, const FOPoint& pn, const FOPoint& p0,
  double* sum)
{
  double vh[3], Es[3], Bs[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) vh[c] = 0.5 * (pn.p[c] + p0.p[c]);
  src.segment(pn.r, p0.r, Es, Bs);
  sum[0] += 0.5 * (dot3(pn.p, pn.p) - dot3(p0.p, p0.p)) - qm * dt * dot3(vh, Es);
  const double vb = dot3(vh, Bs), bb = dot3(Bs, Bs);
#pragma unroll
  for (int c = 0; c < 3; ++c) sum[1 + c] += vh[c] - (vb * Bs[c]) / bb;
}

// k_model_fo_trace<CN> with the step's factor; SUMS: sums [4][n], read and written.  It keeps its own text: merged with
// k_model_fo_trace under a clock, the Chin instance without sums measured 3 % slower
template <bool CN, bool SUMS>
__global__ void __launch_bounds__(kBlock) k_timed_fo_trace(GridDev g, xpic_field_model M, xpic_field_envelope V,
  xpic_fo_params P, OpenRegion R, long n, double* __restrict__ s, long first, int nsteps, long sample_every, long nsamp,
  double* __restrict__ samples, long long* __restrict__ it_sum, int* __restrict__ it_max, long long* __restrict__ exit_step,
  unsigned long long* alive, unsigned long long* removed, double* __restrict__ sums)
{
  const long q = (long)blockIdx.x * kBlock + threadIdx.x;
  const bool live = q < n && exit_step[q] < 0;
  const int ns = nsteps < kLaunchSteps ? nsteps : kLaunchSteps;
  const bool on = V.kind != XPIC_ENV_CONSTANT;
  int done = 0;
  bool gone = false;
  if (live) {
    FOPoint pn;
    fo_load(s, n, q, pn);
    long long total = CN ? it_sum[q] : 0;
    int most = CN ? it_max[q] : 0;
    double sum[4] = {0.0, 0.0, 0.0, 0.0};
    if (SUMS) {
#pragma unroll
      for (int k = 0; k < 4; ++k) sum[k] = sums[k * n + q];
    }
    for (; done < ns; ++done) {
      if (R.kind >= 0 && !open_keep(g, R, pn.r)) { gone = true; break; }
      const TimedModelSource src{{M}, on, envelope_factor(V, R.step0 + first + done, P.dt)};
      const FOPoint p0 = pn;
      int it = 0;
      if (CN) it = fo_cn_process(src, P.qm, P.dt, P.atol, P.rtol, P.maxit, pn, p0);
      else fo_step(P.scheme, src, P.qm, P.dt, pn);
      if (SUMS) ex3_sums(src, P.qm, P.dt, pn, p0, sum);
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
    if (SUMS) {
#pragma unroll
      for (int k = 0; k < 4; ++k) sums[k * n + q] = sum[k];
    }
    if (gone) exit_step[q] = R.step0 + first + done;
  }
  open_tally<kBlock>(live, gone, first + done, first, ns, sample_every, nsamp, alive, removed);
}

// k_dk_trace_open (drift_kinetic.hip) on the model of the step's clock, without a list
template <class Clock>
__global__ void __launch_bounds__(kBlock) k_model_dk_trace(GridDev g, Clock C, xpic_dk_params P, OpenRegion R, long n,
  double* __restrict__ s, long first, int nsteps, long sample_every, long nsamp, double* __restrict__ samples,
  long long* __restrict__ it_total, int* __restrict__ it_max, long long* __restrict__ exit_step, unsigned long long* alive,
  unsigned long long* removed)
{
  const long q = (long)blockIdx.x * kBlock + threadIdx.x;
  const bool live = q < n && exit_step[q] < 0;
  const int ns = nsteps < kLaunchSteps ? nsteps : kLaunchSteps;
  int done = 0;
  bool gone = false;
  if (live) {
    DKPoint p0, pn;
    dk_load(s, n, q, pn);
    long long total = it_total[q];
    int most = it_max[q];
    for (; done < ns; ++done) {
      if (R.kind >= 0 && !open_keep(g, R, pn.r)) { gone = true; break; }
      const auto src = C.at(R.step0 + first + done, P.dt);
      p0 = pn;
      const int it = dk_process(src, P, p0, pn);
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

// the factors of steps step0 .. step0 + nsteps - 1 by the device function the traces call
__global__ void __launch_bounds__(kBlock) k_envelope_factors(xpic_field_envelope V, double dt, long long step0, long nsteps,
  double* __restrict__ out)
{
  const long i = (long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= nsteps) return;
  out[i] = envelope_factor(V, step0 + i, dt);
}

// the envelope a call runs with: a null one is the constant one
int timed_envelope(const std::string& who, const xpic_field_envelope* in, xpic_field_envelope* V)
{
  const char* bad = envelope_check(in);
  XPIC_CHECK(!bad, who + ": " + (bad ? bad : ""));
  *V = xpic_field_envelope{};
  if (in) *V = *in;
  return 0;
}

// the drift-kinetic trace of either clock, after the checks: `label` names the profile entry
template <class Clock>
int dk_trace(xpic_ctx* ctx, const std::string& who, const char* label, const xpic_dk_params& P, const Clock& C,
  const TraceArrays& A, const OpenRegion& R)
{
  return trace_call(ctx, model_entry(who, label), kLaunchSteps, A, R, XPIC_COMPACT_NEVER, nullptr, [&](const TraceDev& d) {
    hipLaunchKernelGGL(k_model_dk_trace<Clock>, lane_grid(A.n), dim3(kBlock), 0, ctx->stream, ctx->g, C, P, R, (long)A.n, d.s,
      d.first, d.ns, (long)A.sample_every, d.nsamp, d.samples, d.it_sum, d.it_max, d.exit_step, d.alive, d.removed);
  });
}

}  // namespace

}  // namespace xpic

using namespace xpic;

extern "C" {

int xpic_model_fields(xpic_ctx* ctx, const xpic_field_model* model, int64_t n, const double* r3, double* E3, double* B3,
  double* gradB3)
{
  XPIC_CHECK(ctx != nullptr, "null context");
  XPIC_CALL(model_ok("model_fields", model));
  XPIC_CHECK(n >= 0, "model_fields: n is negative");
  XPIC_CHECK(n <= ((int64_t)1 << 36), "model_fields: n is larger than 2^36");
  XPIC_CHECK(r3 && E3 && B3 && gradB3, "model_fields: a null array");
  if (n == 0) return 0;
  DevScratch<double> a, o;
  XPIC_CALL(a.alloc(3 * n)); XPIC_CALL(o.alloc(9 * n));
  XPIC_CALL(upload(a, r3, 3 * n, ctx->stream));
  {
    Timed t(ctx, "model_fields");
    hipLaunchKernelGGL(k_model_fields, lane_grid(n), dim3(kBlock), 0, ctx->stream, *model, (long)n, (const double*)a.p, o.p);
    XPIC_HIP(hipGetLastError());
  }
  XPIC_CALL(download(E3, o, 3 * n, ctx->stream));
  XPIC_CALL(download(B3, o, 3 * n, ctx->stream, 3 * n));
  XPIC_CALL(download(gradB3, o, 3 * n, ctx->stream, 6 * n));
  XPIC_HIP(hipStreamSynchronize(ctx->stream));
  return 0;
}

int xpic_set_model_field(xpic_ctx* ctx, const xpic_field_model* model, int E_field, int B_field, int gradB_field)
{ // FieldContext::initialize, tests/drift_kinetic_push/drift_kinetic_push.h:176-209
  XPIC_CHECK(ctx != nullptr, "null context");
  XPIC_CALL(model_ok("set_model_field", model));
  double* v[3];
  const int id[3] = {E_field, B_field, gradB_field};
  for (int k = 0; k < 3; ++k) {
    XPIC_CHECK(id[k] < 0 || (id[k] < XPIC_NFIELDS && ctx->field[id[k]]), "set_model_field: not an allocated field id");
    v[k] = id[k] < 0 ? nullptr : ctx->field[id[k]];
  }
  XPIC_CHECK(!(v[0] && v[0] == v[1]) && !(v[0] && v[0] == v[2]) && !(v[1] && v[1] == v[2]),
    "set_model_field: the same field id twice");
  Timed t(ctx, "set_model_field");
  hipLaunchKernelGGL(k_set_model_field, lane_grid(std::max<int64_t>(ctx->g.nown, 1)), dim3(kBlock), 0, ctx->stream, ctx->g,
    *model, v[0], v[1], v[2]);
  XPIC_HIP(hipGetLastError());
  XPIC_HIP(hipStreamSynchronize(ctx->stream));
  return 0;
}

int xpic_model_full_orbit_trace(xpic_ctx* ctx, int64_t n, const xpic_fo_params* params, const xpic_field_model* model,
  int64_t steps, int64_t sample_every, double* p_6, double* samples, int64_t* iterations_sum, int* iterations_max,
  const xpic_trace_region* region, int64_t* exit_step, int64_t* alive, int64_t* removed)
{
  const std::string who = "model_full_orbit_trace";
  XPIC_CALL(model_checks(who, ctx, n, params, model));
  OpenRegion R;
  XPIC_CALL(trace_region(who, region, true, false, &R));
  const bool cn = params->scheme == XPIC_FO_CN;
  return trace_call(ctx, model_entry(who, "model_fo_trace"), kLaunchSteps,
    {n, steps, sample_every, p_6, samples, iterations_sum, iterations_max, exit_step, alive, removed, cn, nullptr}, R,
    XPIC_COMPACT_NEVER, nullptr, [&](const TraceDev& d) {
      hipLaunchKernelGGL(cn ? k_model_fo_trace<true> : k_model_fo_trace<false>, lane_grid(n), dim3(kBlock), 0, ctx->stream,
        ctx->g, *model, *params, R, (long)n, d.s, d.first, d.ns, (long)sample_every, d.nsamp, d.samples, d.it_sum, d.it_max,
        d.exit_step, d.alive, d.removed);
    });
}

int xpic_model_drift_kinetic_trace(xpic_ctx* ctx, int64_t n, const xpic_dk_params* params, const xpic_field_model* model,
  int64_t steps, int64_t sample_every, double* state_6, double* samples, int64_t* iterations_total, int* iterations_max,
  const xpic_trace_region* region, int64_t* exit_step, int64_t* alive, int64_t* removed)
{
  const std::string who = "model_drift_kinetic_trace";
  XPIC_CALL(model_checks(who, ctx, n, params, model));
  OpenRegion R;
  XPIC_CALL(trace_region(who, region, true, false, &R));
  return dk_trace(ctx, who, "model_dk_trace", *params, StaticClock{*model},
    {n, steps, sample_every, state_6, samples, iterations_total, iterations_max, exit_step, alive, removed, true, nullptr}, R);
}

int xpic_model_full_orbit_trace_timed(xpic_ctx* ctx, int64_t n, const xpic_fo_params* params, const xpic_field_model* model,
  const xpic_field_envelope* envelope, int64_t steps, int64_t sample_every, double* p_6, double* samples,
  int64_t* iterations_sum, int* iterations_max, const xpic_trace_region* region, int64_t* exit_step, int64_t* alive,
  int64_t* removed, double* sums_4)
{
  const std::string who = "model_full_orbit_trace_timed";
  XPIC_CALL(model_checks(who, ctx, n, params, model));
  xpic_field_envelope V;
  XPIC_CALL(timed_envelope(who, envelope, &V));
  OpenRegion R;
  XPIC_CALL(trace_region(who, region, true, false, &R));
  const bool cn = params->scheme == XPIC_FO_CN, sums = sums_4 != nullptr;
  auto kernel = cn ? (sums ? k_timed_fo_trace<true, true> : k_timed_fo_trace<true, false>)
                   : (sums ? k_timed_fo_trace<false, true> : k_timed_fo_trace<false, false>);
  return trace_call(ctx, model_entry(who, "timed_fo_trace"), kLaunchSteps,
    {n, steps, sample_every, p_6, samples, iterations_sum, iterations_max, exit_step, alive, removed, cn, sums_4}, R,
    XPIC_COMPACT_NEVER, nullptr, [&](const TraceDev& d) {
      hipLaunchKernelGGL(kernel, lane_grid(n), dim3(kBlock), 0, ctx->stream, ctx->g, *model, V, *params, R, (long)n, d.s,
        d.first, d.ns, (long)sample_every, d.nsamp, d.samples, d.it_sum, d.it_max, d.exit_step, d.alive, d.removed, d.extra);
    });
}

int xpic_model_drift_kinetic_trace_timed(xpic_ctx* ctx, int64_t n, const xpic_dk_params* params,
  const xpic_field_model* model, const xpic_field_envelope* envelope, int64_t steps, int64_t sample_every, double* state_6,
  double* samples, int64_t* iterations_total, int* iterations_max, const xpic_trace_region* region, int64_t* exit_step,
  int64_t* alive, int64_t* removed)
{
  const std::string who = "model_drift_kinetic_trace_timed";
  XPIC_CALL(model_checks(who, ctx, n, params, model));
  xpic_field_envelope V;
  XPIC_CALL(timed_envelope(who, envelope, &V));
  OpenRegion R;
  XPIC_CALL(trace_region(who, region, true, false, &R));
  return dk_trace(ctx, who, "timed_dk_trace", *params, EnvelopeClock{*model, V},
    {n, steps, sample_every, state_6, samples, iterations_total, iterations_max, exit_step, alive, removed, true, nullptr}, R);
}

int xpic_envelope_factors(xpic_ctx* ctx, const xpic_field_envelope* envelope, double dt, int64_t step0, int64_t nsteps,
  double* out)
{
  const std::string who = "envelope_factors";
  XPIC_CHECK(ctx != nullptr, "null context");
  xpic_field_envelope V;
  XPIC_CALL(timed_envelope(who, envelope, &V));
  XPIC_CHECK(step0 >= 0, who + ": step0 is negative");
  XPIC_CHECK(nsteps >= 0 && nsteps <= ((int64_t)1 << 31), who + ": nsteps must be within 0 .. 2^31");
  XPIC_CHECK(out || nsteps == 0, who + ": out is null");
  if (nsteps == 0) return 0;
  DevScratch<double> o;
  XPIC_CALL(o.alloc(nsteps));
  {
    Timed t(ctx, "envelope_factors");
    hipLaunchKernelGGL(k_envelope_factors, lane_grid(nsteps), dim3(kBlock), 0, ctx->stream, V, dt, (long long)step0,
      (long)nsteps, o.p);
    XPIC_HIP(hipGetLastError());
  }
  XPIC_CALL(download(out, o, nsteps, ctx->stream));
  XPIC_HIP(hipStreamSynchronize(ctx->stream));
  return 0;
}

}  // extern "C"
