// collide_trace.hip -- the model traces with Coulomb scattering off Maxwellian backgrounds: after the push
// of a step a test particle collides with one partner drawn from each background species, by the Takizuka-Abe pair
// collision of collide.hip (collide_pair.h).  AN EXTENSION, as xpic_collide is: the reference has no collision operator;
// include/xpic_hip.h (xpic_trace_collisions) is the definition, tests/collisional_trace_ref.py states it a second time
// in numpy float64.
//
// k_coll_fo_trace<CN> and k_coll_dk_trace are the texts of model_trace.hip's k_model_fo_trace<CN> and
// k_model_dk_trace<StaticClock> with the collision between the push and the sample; full_orbit_step.h,
// drift_kinetic_step.h and model_source.h are instantiated unchanged, under the same contraction as there, and the
// collision carries its own (off: it is rounded operation by operation).  One lane per particle, fp64, no LDS, no
// cross-lane operation but open_tally's; plain vector loads and stores.  A guiding centre is given a gyrophase, collided as
// a velocity and projected back on the field direction at its own position: velocity-space scattering only, the guiding
// centre is not displaced.  Every loop is bounded as in model_trace.hip, the loop over the backgrounds by
// XPIC_TRACE_BG_MAX; every global index is formed under q < n.  The four tallies travel per lane in tally [4][n] from
// launch to launch and leave through block_reduce_store / reduce_to_host in a fixed order.  The host side is trace_call.h's
// with the "never" policy, as the model traces'.
#include <cmath>
#include <string>

#include "batch.h"
#include "common.h"
#include "device_common.h"
#include "field_model.h"
#include "ie_shape.h"
#include "trace_call.h"
#include "trace_open.h"
#include "collide_pair.h"

// as in model_trace.hip: contracted per source expression only (the collision's functions switch it off in their bodies)
#pragma clang fp contract(on)

#include "full_orbit_step.h"
#include "drift_kinetic_step.h"
#include "model_source.h"

namespace xpic {

namespace {

constexpr int kBlock = kLaneBlock; // batch.h: lane_grid launches workgroups of this size
constexpr int kLaunchSteps = XPIC_MODEL_LAUNCH_STEPS;
static_assert(kLaunchSteps <= kOpenRows, "open_tally holds one row per step of a launch");
constexpr int kTally = 4;

// what the kernels know of one background: cdt = S q_a^2 q_b^2 n_b (every dt) / m_ab^2, fa = m_ab / m_a
struct CollBg {
  double cdt, fa, vth, drift[3];
};
struct CollDev {
  int nbg, every;
  uint64_t seed;
  long long particle0;
  CollBg bg[XPIC_TRACE_BG_MAX];
};

// a1 .. a4 of the stream -> the partner's velocity w = drift + vth (g1, g2, g3)
__device__ inline void coll_partner(const CollBg& b, uint64_t& st, double* w)
{
#pragma clang fp contract(off)
  const double a1 = u01(st), a2 = u01(st), a3 = u01(st), a4 = u01(st);
  const double r1 = sqrt(-2.0 * log(a1)), r3 = sqrt(-2.0 * log(a3));
  const double g1 = r1 * cos(2.0 * M_PI * a2), g2 = r1 * sin(2.0 * M_PI * a2), g3 = r3 * cos(2.0 * M_PI * a4);
  w[0] = b.drift[0] + b.vth * g1;
  w[1] = b.drift[1] + b.vth * g2;
  w[2] = b.drift[2] + b.vth * g3;
}

// the collisions of one full-orbit step: v is the record's p
__device__ inline void coll_fo(const CollDev& C, uint64_t step_key, long long particle, double* v, double* t)
{
  for (int b = 0; b < C.nbg && b < XPIC_TRACE_BG_MAX; ++b) {
    uint64_t st = trace_stream(step_key, particle, b);
    double w[3];
    coll_partner(C.bg[b], st, w);
    (void)u01(st); // a5: the gyrophase a guiding centre draws here
    collide_pair(C.bg[b].fa, 0.0, C.bg[b].cdt, st, v, w, t);
  }
}

// b = B / |B| and the basis across it: e1 = normalize(b x e_c), e_c the axis with the smallest |b_c| (a tie: the lowest
// index), e2 = b x e1 -> |B|
__device__ inline double coll_basis(const double* B, double* b, double* e1, double* e2)
{
#pragma clang fp contract(off)
  const double lenB = sqrt(B[0] * B[0] + B[1] * B[1] + B[2] * B[2]);
  if (lenB == 0.0) return 0.0;
  b[0] = B[0] / lenB; b[1] = B[1] / lenB; b[2] = B[2] / lenB;
  int c = 0;
  double least = fabs(b[0]);
  if (fabs(b[1]) < least) { c = 1; least = fabs(b[1]); }
  if (fabs(b[2]) < least) c = 2;
  double x[3]; // b x e_c
  if (c == 0) { x[0] = 0.0; x[1] = b[2]; x[2] = -b[1]; }
  else if (c == 1) { x[0] = -b[2]; x[1] = 0.0; x[2] = b[0]; }
  else { x[0] = b[1]; x[1] = -b[0]; x[2] = 0.0; }
  const double l = sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
  e1[0] = x[0] / l; e1[1] = x[1] / l; e1[2] = x[2] / l;
  e2[0] = b[1] * e1[2] - b[2] * e1[1];
  e2[1] = b[2] * e1[0] - b[0] * e1[2];
  e2[2] = b[0] * e1[1] - b[1] * e1[0];
  return lenB;
}

// the collisions of one guiding-centre step; B: the model at pn.r.  |B| == 0: the step's collisions are skipped and counted
__device__ inline void coll_dk(const CollDev& C, uint64_t step_key, long long particle, const double* B, double mp, DKPoint& pn,
  double* t)
{
#pragma clang fp contract(off)
  double b[3], e1[3], e2[3];
  const double lenB = coll_basis(B, b, e1, e2);
  if (lenB == 0.0) {
    t[1] += (double)C.nbg;
    return;
  }
  for (int k = 0; k < C.nbg && k < XPIC_TRACE_BG_MAX; ++k) {
    uint64_t st = trace_stream(step_key, particle, k);
    double w[3], v[3];
    coll_partner(C.bg[k], st, w);
    const double psi = 2.0 * M_PI * u01(st);
    const double cs = cos(psi), sn = sin(psi);
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = pn.ppar * b[c] + pn.pperp * (cs * e1[c] + sn * e2[c]);
    const double made = t[0];
    collide_pair(C.bg[k].fa, 0.0, C.bg[k].cdt, st, v, w, t);
    if (t[0] == made) continue; // (|u| == 0: skipped, the record keeps its bits)
    const double par = v[0] * b[0] + v[1] * b[1] + v[2] * b[2];
    const double x = v[0] - par * b[0], y = v[1] - par * b[1], z = v[2] - par * b[2];
    const double perp = sqrt(x * x + y * y + z * z);
    pn.ppar = par;
    pn.pperp = perp;
    pn.mu = mp * perp * perp / (2.0 * lenB);
  }
}

// k_model_fo_trace (model_trace.hip) with the collisions of step R.step0 + first + done + 1 after its push
template <bool CN>
__global__ void __launch_bounds__(kBlock) k_coll_fo_trace(GridDev g, xpic_field_model M, xpic_fo_params P, OpenRegion R,
  CollDev C, long n, double* __restrict__ s, long first, int nsteps, long sample_every, long nsamp, double* __restrict__ samples,
  long long* __restrict__ it_sum, int* __restrict__ it_max, long long* __restrict__ exit_step, unsigned long long* alive,
  unsigned long long* removed, double* __restrict__ tally)
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
    double t[kTally];
#pragma unroll
    for (int k = 0; k < kTally; ++k) t[k] = tally[k * n + q];
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
      const long long k = R.step0 + step;
      if (k % C.every == 0) coll_fo(C, trace_step_key(C.seed, k), C.particle0 + q, pn.p, t);
      if (samples && step % sample_every == 0) {
        const long row = step / sample_every - 1;
        if (row < nsamp) fo_store(samples + row * 6 * n, n, q, pn);
      }
    }
    fo_store(s, n, q, pn);
    if (CN) { it_sum[q] = total; it_max[q] = most; }
#pragma unroll
    for (int k = 0; k < kTally; ++k) tally[k * n + q] = t[k];
    if (gone) exit_step[q] = R.step0 + first + done;
  }
  open_tally<kBlock>(live, gone, first + done, first, ns, sample_every, nsamp, alive, removed);
}

// k_model_dk_trace<StaticClock> (model_trace.hip) with the collisions after the push, on the model at pn.r
__global__ void __launch_bounds__(kBlock) k_coll_dk_trace(GridDev g, xpic_field_model M, xpic_dk_params P, OpenRegion R,
  CollDev C, long n, double* __restrict__ s, long first, int nsteps, long sample_every, long nsamp, double* __restrict__ samples,
  long long* __restrict__ it_total, int* __restrict__ it_max, long long* __restrict__ exit_step, unsigned long long* alive,
  unsigned long long* removed, double* __restrict__ tally)
{
  const long q = (long)blockIdx.x * kBlock + threadIdx.x;
  const bool live = q < n && exit_step[q] < 0;
  const int ns = nsteps < kLaunchSteps ? nsteps : kLaunchSteps;
  const ModelSource src{M};
  int done = 0;
  bool gone = false;
  if (live) {
    DKPoint p0, pn;
    dk_load(s, n, q, pn);
    long long total = it_total[q];
    int most = it_max[q];
    double t[kTally];
#pragma unroll
    for (int k = 0; k < kTally; ++k) t[k] = tally[k * n + q];
    for (; done < ns; ++done) {
      if (R.kind >= 0 && !open_keep(g, R, pn.r)) { gone = true; break; }
      p0 = pn;
      const int it = dk_process(src, P, p0, pn);
      total += it;
      most = it > most ? it : most;
      const long step = first + done + 1;
      const long long k = R.step0 + step;
      if (k % C.every == 0) {
        double Ep[3], Bp[3], gBp[3];
        src.dk(pn.r, pn.r, Ep, Bp, gBp);
        coll_dk(C, trace_step_key(C.seed, k), C.particle0 + q, Bp, P.mp, pn, t);
      }
      if (samples && step % sample_every == 0) {
        const long row = step / sample_every - 1;
        if (row < nsamp) dk_store(samples + row * 6 * n, n, q, pn);
      }
    }
    dk_store(s, n, q, pn);
    it_total[q] = total;
    it_max[q] = most;
#pragma unroll
    for (int k = 0; k < kTally; ++k) tally[k * n + q] = t[k];
    if (gone) exit_step[q] = R.step0 + first + done;
  }
  open_tally<kBlock>(live, gone, first + done, first, ns, sample_every, nsamp, alive, removed);
}

// first stage of the tallies' reduction: each thread sums its particles q, q + stride, ... in that order
__global__ void __launch_bounds__(kBlock) k_coll_tally(long n, const double* __restrict__ tally, double* partial)
{
  double t[kTally] = {0.0, 0.0, 0.0, 0.0};
  const long stride = (long)gridDim.x * kBlock;
  for (long q = (long)blockIdx.x * kBlock + threadIdx.x; q < n; q += stride) {
#pragma unroll
    for (int k = 0; k < kTally; ++k) t[k] += tally[k * n + q];
  }
  block_reduce_store<kTally, kBlock>(t, partial, gridDim.x, blockIdx.x);
}

// the checks of an xpic_trace_collisions (null: no collisions) -> on: the call collides; C: what the kernels get
int coll_setup(const std::string& who, const xpic_trace_collisions* in, double qm, double dt, bool* on, CollDev* C)
{
  *on = false;
  *C = CollDev{};
  if (!in) return 0;
  XPIC_CHECK(in->nbg >= 0 && in->nbg <= XPIC_TRACE_BG_MAX, who + ": nbg must be within 0 .. XPIC_TRACE_BG_MAX");
  XPIC_CHECK(in->every >= 1, who + ": collisions->every must be >= 1");
  XPIC_CHECK(in->particle0 >= 0, who + ": particle0 is negative");
  XPIC_CHECK(std::isfinite(in->strength) && in->strength >= 0.0, who + ": the strength must be finite and not negative");
  XPIC_CHECK(std::isfinite(in->mass) && in->mass > 0.0, who + ": the test particle's mass must be finite and > 0");
  for (int b = 0; b < in->nbg; ++b) {
    const xpic_trace_background& g = in->bg[b];
    XPIC_CHECK(std::isfinite(g.m) && g.m > 0.0, who + ": a background's mass must be finite and > 0");
    XPIC_CHECK(g.n >= 0.0, who + ": a background's density is negative");
    XPIC_CHECK(g.vth >= 0.0, who + ": a background's thermal speed is negative");
  }
  if (in->nbg == 0 || in->strength == 0.0) return 0;
  *on = true;
  C->nbg = in->nbg;
  C->every = in->every;
  C->seed = in->seed;
  C->particle0 = in->particle0;
  const double qa = qm * in->mass, dtc = (double)in->every * dt;
  for (int b = 0; b < in->nbg; ++b) {
    const xpic_trace_background& g = in->bg[b];
    const double mab = in->mass * g.m / (in->mass + g.m);
    const double c0 = in->strength * (qa * qa) * (g.q * g.q) / (mab * mab);
    C->bg[b].cdt = c0 * g.n * dtc;
    C->bg[b].fa = mab / in->mass;
    C->bg[b].vth = g.vth;
    for (int k = 0; k < 3; ++k) C->bg[b].drift[k] = g.drift[k];
  }
  return 0;
}

// the per-lane tallies of a call: zeroed before the first launch, summed into coll_4 after the last
struct Tally {
  DevScratch<double> d;
  int begin(xpic_ctx* ctx, int64_t n)
  {
    XPIC_CALL(d.alloc((size_t)kTally * n));
    return zero(d, (size_t)kTally * n, ctx->stream);
  }
  int end(xpic_ctx* ctx, int64_t n, double* coll_4)
  {
    long nb = lane_grid(n).x;
    if (nb > kRedBlocks) nb = kRedBlocks;
    hipLaunchKernelGGL(k_coll_tally, dim3((unsigned)nb), dim3(kBlock), 0, ctx->stream, (long)n, (const double*)d.p,
      ctx->red_partial);
    XPIC_HIP(hipGetLastError());
    double res[kTally];
    XPIC_CALL(reduce_to_host(ctx, kTally, (int)nb, 1, false, res));
    if (coll_4)
      for (int k = 0; k < kTally; ++k) coll_4[k] = res[k];
    return 0;
  }
};

TraceEntry coll_entry(const std::string& who)
{
  return {who.c_str(), "the particle array", "an iteration counter", "an iteration counter", false};
}

}  // namespace

}  // namespace xpic

using namespace xpic;

extern "C" {

int xpic_model_full_orbit_trace_collisional(xpic_ctx* ctx, int64_t n, const xpic_fo_params* params,
  const xpic_field_model* model, int64_t steps, int64_t sample_every, double* p_6, double* samples, int64_t* iterations_sum,
  int* iterations_max, const xpic_trace_region* region, int64_t* exit_step, int64_t* alive, int64_t* removed,
  const xpic_trace_collisions* collisions, double* coll_4)
{
  const std::string who = "model_full_orbit_trace_collisional";
  XPIC_CHECK(ctx != nullptr, "null context");
  XPIC_CHECK(n >= 0, who + ": n is negative");
  XPIC_CALL(fo_check_params(who, params));
  const char* bad = model_check(model);
  XPIC_CHECK(!bad, who + ": " + (bad ? bad : ""));
  bool on;
  CollDev Cd;
  XPIC_CALL(coll_setup(who, collisions, params->qm, params->dt, &on, &Cd));
  if (!on) { // the model trace itself, bit for bit
    XPIC_CALL(xpic_model_full_orbit_trace(ctx, n, params, model, steps, sample_every, p_6, samples, iterations_sum,
      iterations_max, region, exit_step, alive, removed));
    if (coll_4)
      for (int k = 0; k < kTally; ++k) coll_4[k] = 0.0;
    return 0;
  }
  OpenRegion R;
  XPIC_CALL(trace_region(who, region, true, false, &R));
  const bool cn = params->scheme == XPIC_FO_CN;
  const bool runs = n > 0 && steps > 0;
  Tally tally;
  if (runs) XPIC_CALL(tally.begin(ctx, n));
  XPIC_CALL(trace_call(ctx, coll_entry(who), "coll_fo_trace", "coll_fo_trace", kLaunchSteps, n, cn, steps, sample_every, p_6,
    samples, iterations_sum, iterations_max, R, XPIC_COMPACT_NEVER, exit_step, alive, removed, nullptr,
    [&](double* s, const long long*, long, long first, int ns, long nsamp, double* sm, long long* sum, int* mx, long long* ex,
      unsigned long long* al, unsigned long long* rm, double*) {
      hipLaunchKernelGGL(cn ? k_coll_fo_trace<true> : k_coll_fo_trace<false>, lane_grid(n), dim3(kBlock), 0, ctx->stream,
        ctx->g, *model, *params, R, Cd, (long)n, s, first, ns, (long)sample_every, nsamp, sm, sum, mx, ex, al, rm, tally.d.p);
    }));
  if (coll_4)
    for (int k = 0; k < kTally; ++k) coll_4[k] = 0.0;
  if (runs) XPIC_CALL(tally.end(ctx, n, coll_4));
  return 0;
}

int xpic_model_drift_kinetic_trace_collisional(xpic_ctx* ctx, int64_t n, const xpic_dk_params* params,
  const xpic_field_model* model, int64_t steps, int64_t sample_every, double* state_6, double* samples,
  int64_t* iterations_total, int* iterations_max, const xpic_trace_region* region, int64_t* exit_step, int64_t* alive,
  int64_t* removed, const xpic_trace_collisions* collisions, double* coll_4)
{
  const std::string who = "model_drift_kinetic_trace_collisional";
  XPIC_CHECK(ctx != nullptr, "null context");
  XPIC_CHECK(n >= 0, who + ": n is negative");
  XPIC_CALL(dk_check_params(who, params, XPIC_MODEL_DK_MAXIT));
  const char* bad = model_check(model);
  XPIC_CHECK(!bad, who + ": " + (bad ? bad : ""));
  bool on;
  CollDev Cd;
  XPIC_CALL(coll_setup(who, collisions, params->qm, params->dt, &on, &Cd));
  if (!on) { // the model trace itself, bit for bit
    XPIC_CALL(xpic_model_drift_kinetic_trace(ctx, n, params, model, steps, sample_every, state_6, samples, iterations_total,
      iterations_max, region, exit_step, alive, removed));
    if (coll_4)
      for (int k = 0; k < kTally; ++k) coll_4[k] = 0.0;
    return 0;
  }
  OpenRegion R;
  XPIC_CALL(trace_region(who, region, true, false, &R));
  const bool runs = n > 0 && steps > 0;
  Tally tally;
  if (runs) XPIC_CALL(tally.begin(ctx, n));
  XPIC_CALL(trace_call(ctx, coll_entry(who), "coll_dk_trace", "coll_dk_trace", kLaunchSteps, n, true, steps, sample_every,
    state_6, samples, iterations_total, iterations_max, R, XPIC_COMPACT_NEVER, exit_step, alive, removed, nullptr,
    [&](double* s, const long long*, long, long first, int ns, long nsamp, double* sm, long long* sum, int* mx, long long* ex,
      unsigned long long* al, unsigned long long* rm, double*) {
      hipLaunchKernelGGL(k_coll_dk_trace, lane_grid(n), dim3(kBlock), 0, ctx->stream, ctx->g, *model, *params, R, Cd, (long)n,
        s, first, ns, (long)sample_every, nsamp, sm, sum, mx, ex, al, rm, tally.d.p);
    }));
  if (coll_4)
    for (int k = 0; k < kTally; ++k) coll_4[k] = 0.0;
  if (runs) XPIC_CALL(tally.end(ctx, n, coll_4));
  return 0;
}

}  // extern "C"
