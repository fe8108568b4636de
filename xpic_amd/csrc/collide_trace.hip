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
//
// The same kernel text serves the collisional grid traces (xpic_full_orbit_trace_collisional,
// xpic_drift_kinetic_trace_collisional): it is written over the field source (the model, or the context's grid through
// FOGrid / DKGrid), the background source (the struct's uniform backgrounds, or the context's per-cell profiles of
// background.hip) and the lanes (all particles, or the list of live ones, so the grid traces' compaction is honoured).
// tests/collisional_grid_trace_ref.py states that form a second time.
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

// ---- the three things a kernel is written over: the field source, the background source, the lanes' particles.
//
// A field source is a kernel argument with src(g), the source the step functions take (full_orbit_step.h,
// drift_kinetic_step.h): the analytic model, or the context's grid.
struct ModelField {
  xpic_field_model M;
  __device__ inline ModelSource src(const GridDev&) const { return ModelSource{M}; }
};
struct FOGridField {
  const double *E, *B;
  __device__ inline FOGrid src(const GridDev& g) const { return FOGrid{g, E, B}; }
};
template <bool GRAD>
struct DKGridField {
  const double *E, *B, *gB;
  __device__ inline DKGrid<GRAD> src(const GridDev& g) const { return DKGrid<GRAD>{g, E, B, gB}; }
};

// A background source says what a particle at r meets of background b: cell(g, r) once per colliding step, then
// get(C, b, cell, own) per background fills what coll_partner and collide_pair read; false: no collision for that
// background, nothing is drawn and neither tally moves.  UniformBg: the struct's own backgrounds, as the host formed them
// (kUniform: the callers read C.bg[b] where it lies, the kernel argument, and get is never called).
struct UniformBg {
  static constexpr bool kUniform = true;
  __device__ inline long cell(const GridDev&, const double*) const { return 0; }
  __device__ inline bool get(const CollDev&, int, long, CollBg&) const { return true; }
};
// ProfileBg: background b reads n, vth and the drift of slot[b] ([5][ncell], background.hip) at the cell of r --
// floor(r / d) per axis, folded onto the grid by the true modulus (positions are not folded in the traces), piecewise
// constant -- and forms sigma^2's factor ((c0 n) dt_c) here, rounded operation by operation as the host rounds the
// uniform one's: a constant profile gives the uniform background's bits.  slot[b] null: the uniform one of the struct.
// A position that is not a number, or further out than an int counts cells, has no cell (fo_in_range): no index is
// formed from it and it meets nobody.  n == 0: nobody to meet.
struct ProfileBg {
  static constexpr bool kUniform = false;
  const double* slot[XPIC_TRACE_BG_MAX];
  double c0[XPIC_TRACE_BG_MAX]; // S q_a^2 q_b^2 / m_ab^2
  double dtc;                   // every * dt
  long ncell;
  __device__ inline long cell(const GridDev& g, const double* r) const
  {
#pragma clang fp contract(off)
    if (!fo_in_range(g, r)) return -1;
    const int x = GridDev::wrap((int)floor(r[0] / g.dx), g.nx), y = GridDev::wrap((int)floor(r[1] / g.dy), g.ny),
              z = GridDev::wrap((int)floor(r[2] / g.dz), g.nzl);
    return ((long)z * g.ny + y) * g.nx + x;
  }
  __device__ inline bool get(const CollDev& C, int b, long cell, CollBg& own) const
  {
#pragma clang fp contract(off)
    own = C.bg[b]; // (by value: a pointer that may lead to the kernel argument or to `own` would put both in scratch)
    const double* p = slot[b];
    if (!p) return true;
    if (cell < 0 || cell >= ncell) return false;
    const double n = p[cell];
    if (!(n > 0.0)) return false;
    own.cdt = (c0[b] * n) * dtc;
    own.vth = p[ncell + cell];
    own.drift[0] = p[2 * ncell + cell];
    own.drift[1] = p[3 * ncell + cell];
    own.drift[2] = p[4 * ncell + cell];
    return true;
  }
};

// The particle *q of lane j of a launch; false: none.  AllLanes: particle j (the model traces: every launch covers all n);
// ListedLanes: entry j of the list of live particles (trace_open.hip; null: the particles 0 .. m - 1), the grid traces'.
struct AllLanes {
  __device__ inline bool pick(long j, long n, long* q) const
  {
    *q = j;
    return j < n;
  }
};
struct ListedLanes {
  const long long* list;
  long m;
  __device__ inline bool pick(long j, long n, long* q) const
  {
    *q = j < m ? (list ? (long)list[j] : j) : -1;
    return *q >= 0 && *q < n;
  }
};

// one full-orbit collision with background b
__device__ inline void coll_fo_one(const CollBg& bg, uint64_t step_key, long long particle, int b, double* v, double* t)
{
  uint64_t st = trace_stream(step_key, particle, b);
  double w[3];
  coll_partner(bg, st, w);
  (void)u01(st); // a5: the gyrophase a guiding centre draws here
  collide_pair(bg.fa, 0.0, bg.cdt, st, v, w, t);
}

// the collisions of one full-orbit step at r: v is the record's p
template <class BG>
__device__ inline void coll_fo(const BG& bgs, const GridDev& g, const CollDev& C, uint64_t step_key, long long particle,
  const double* r, double* v, double* t)
{
  const long cell = bgs.cell(g, r);
  for (int b = 0; b < C.nbg && b < XPIC_TRACE_BG_MAX; ++b) {
    if constexpr (BG::kUniform) coll_fo_one(C.bg[b], step_key, particle, b, v, t);
    else {
      CollBg own;
      if (bgs.get(C, b, cell, own)) coll_fo_one(own, step_key, particle, b, v, t);
    }
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

// one guiding-centre collision with background k, in the basis b, e1, e2 across B
__device__ inline void coll_dk_one(const CollBg& bg, uint64_t step_key, long long particle, int k, const double* b,
  const double* e1, const double* e2, double lenB, double mp, DKPoint& pn, double* t)
{
#pragma clang fp contract(off)
  uint64_t st = trace_stream(step_key, particle, k);
  double w[3], v[3];
  coll_partner(bg, st, w);
  const double psi = 2.0 * M_PI * u01(st);
  const double cs = cos(psi), sn = sin(psi);
#pragma unroll
  for (int c = 0; c < 3; ++c) v[c] = pn.ppar * b[c] + pn.pperp * (cs * e1[c] + sn * e2[c]);
  const double made = t[0];
  collide_pair(bg.fa, 0.0, bg.cdt, st, v, w, t);
  if (t[0] == made) return; // (|u| == 0: skipped, the record keeps its bits)
  const double par = v[0] * b[0] + v[1] * b[1] + v[2] * b[2];
  const double x = v[0] - par * b[0], y = v[1] - par * b[1], z = v[2] - par * b[2];
  const double perp = sqrt(x * x + y * y + z * z);
  pn.ppar = par;
  pn.pperp = perp;
  pn.mu = mp * perp * perp / (2.0 * lenB);
}

// the collisions of one guiding-centre step; B: the field source at pn.r.  |B| == 0: the step's collisions are skipped and
// counted (on a profile: those of the backgrounds that have somebody to meet in the cell)
template <class BG>
__device__ inline void coll_dk(const BG& bgs, const GridDev& g, const CollDev& C, uint64_t step_key, long long particle,
  const double* B, double mp, DKPoint& pn, double* t)
{
#pragma clang fp contract(off)
  double b[3], e1[3], e2[3];
  const double lenB = coll_basis(B, b, e1, e2);
  if (BG::kUniform && lenB == 0.0) {
    t[1] += (double)C.nbg;
    return;
  }
  const long cell = bgs.cell(g, pn.r);
  for (int k = 0; k < C.nbg && k < XPIC_TRACE_BG_MAX; ++k) {
    if constexpr (BG::kUniform) coll_dk_one(C.bg[k], step_key, particle, k, b, e1, e2, lenB, mp, pn, t);
    else {
      CollBg own;
      if (!bgs.get(C, k, cell, own)) continue;
      if (lenB == 0.0) t[1] += 1.0;
      else coll_dk_one(own, step_key, particle, k, b, e1, e2, lenB, mp, pn, t);
    }
  }
}

// k_model_fo_trace (model_trace.hip) with the collisions of step R.step0 + first + done + 1 after its push, written once
// over the field source, the background source and the lanes: <ModelField, UniformBg, AllLanes> is the model trace's
// kernel, <FOGridField, ProfileBg, ListedLanes> k_fo_trace_open's (full_orbit.hip) with the collisions, R.kind < 0 its
// closed form.  The per-lane tallies are the particle's, tally[k * n + q]: a list of live particles changes the lane, not
// the slot.  The policies come last in the argument list, so what the model instance read before them lies where it lay.
template <bool CN, class FIELD, class BG, class LANES>
__global__ void __launch_bounds__(kBlock) k_coll_fo_trace(GridDev g, FIELD F, xpic_fo_params P, OpenRegion R,
  CollDev C, long n, double* __restrict__ s, long first, int nsteps, long sample_every, long nsamp, double* __restrict__ samples,
  long long* __restrict__ it_sum, int* __restrict__ it_max, long long* __restrict__ exit_step, unsigned long long* alive,
  unsigned long long* removed, double* __restrict__ tally, BG bgs, LANES lanes)
{
  long q;
  const bool live = lanes.pick((long)blockIdx.x * kBlock + threadIdx.x, n, &q) && exit_step[q] < 0;
  const int ns = nsteps < kLaunchSteps ? nsteps : kLaunchSteps;
  const auto src = F.src(g);
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
      if (k % C.every == 0) coll_fo(bgs, g, C, trace_step_key(C.seed, k), C.particle0 + q, pn.r, pn.p, t);
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

// k_model_dk_trace<StaticClock> (model_trace.hip) with the collisions after the push, in the field the source gives for
// the segment (pn.r, pn.r): the model at pn.r, or what xpic_drift_kinetic_interpolate returns there on the grid.
// <DKGridField<GRAD>, ProfileBg, ListedLanes> is k_dk_trace_open's (drift_kinetic.hip) with the collisions.
template <class FIELD, class BG, class LANES>
__global__ void __launch_bounds__(kBlock) k_coll_dk_trace(GridDev g, FIELD F, xpic_dk_params P, OpenRegion R,
  CollDev C, long n, double* __restrict__ s, long first, int nsteps, long sample_every, long nsamp, double* __restrict__ samples,
  long long* __restrict__ it_total, int* __restrict__ it_max, long long* __restrict__ exit_step, unsigned long long* alive,
  unsigned long long* removed, double* __restrict__ tally, BG bgs, LANES lanes)
{
  long q;
  const bool live = lanes.pick((long)blockIdx.x * kBlock + threadIdx.x, n, &q) && exit_step[q] < 0;
  const int ns = nsteps < kLaunchSteps ? nsteps : kLaunchSteps;
  const auto src = F.src(g);
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
        coll_dk(bgs, g, C, trace_step_key(C.seed, k), C.particle0 + q, Bp, P.mp, pn, t);
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

// the test particle of `in` (charge qm * mass) against background g -> S q_a^2 q_b^2 / m_ab^2; *mab: the reduced mass
double coll_c0(const xpic_trace_collisions* in, const xpic_trace_background& g, double qm, double* mab)
{
  const double qa = qm * in->mass;
  *mab = in->mass * g.m / (in->mass + g.m);
  return in->strength * (qa * qa) * (g.q * g.q) / (*mab * *mab);
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
  const double dtc = (double)in->every * dt;
  for (int b = 0; b < in->nbg; ++b) {
    const xpic_trace_background& g = in->bg[b];
    double mab;
    const double c0 = coll_c0(in, g, qm, &mab);
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

// no tally has moved: a call that did not collide (rc: what the trace it was handed to returned), or one yet to be summed
int coll_none(int rc, double* coll_4)
{
  if (rc == 0 && coll_4)
    for (int k = 0; k < kTally; ++k) coll_4[k] = 0.0;
  return rc;
}

// what the four colliding entry points do around trace_call: the tallies before the first launch, coll_4 after the last.
// launch: trace_call's, with the tallies as TraceDev's extra
template <class Launch>
int coll_trace(xpic_ctx* ctx, const TraceEntry& E, const TraceArrays& A, const OpenRegion& R, int policy, double* coll_4,
  Launch launch)
{
  const bool runs = A.n > 0 && A.steps > 0;
  Tally tally;
  if (runs) XPIC_CALL(tally.begin(ctx, A.n));
  XPIC_CALL(coll_none(trace_call(ctx, E, kLaunchSteps, A, R, policy, tally.d.p, launch), coll_4));
  if (runs) XPIC_CALL(tally.end(ctx, A.n, coll_4));
  return 0;
}

// ---- the collisional grid traces
static_assert(XPIC_FO_LAUNCH_STEPS == kLaunchSteps && XPIC_DK_LAUNCH_STEPS == kLaunchSteps,
  "the grid instances of the kernels take the grid traces' launches");

// the grid tracers' checks of the context, under the entry point's name
int grid_check(xpic_ctx* ctx, const std::string& who, int64_t n)
{
  XPIC_CHECK(ctx != nullptr, "null context");
  XPIC_CHECK(n >= 0, who + ": n is negative");
  XPIC_CHECK(ctx->geom.nranks == 1 && ctx->g.G == 0,
    who + ": a context of several z-slabs (or a self_ring one) is not supported: the gathers wrap z in the kernel");
  XPIC_CHECK(ctx->field[XPIC_E] && ctx->field[XPIC_B], who + ": the context has no E or B");
  return 0;
}

// the checks of `profile` (null: every background is the struct's uniform one) -> what the kernels get.  Called after
// coll_setup has accepted `in`
int profile_setup(xpic_ctx* ctx, const std::string& who, const xpic_trace_collisions* in, const int32_t* profile, double qm,
  double dt, ProfileBg* B)
{
  *B = ProfileBg{};
  B->ncell = ctx->ncell;
  if (!in) return 0;
  B->dtc = (double)in->every * dt;
  for (int b = 0; b < in->nbg; ++b) {
    const int s = profile ? profile[b] : -1;
    XPIC_CHECK(s >= -1 && s < XPIC_TRACE_BG_MAX, who + ": a profile entry must be within -1 .. XPIC_TRACE_BG_MAX - 1");
    XPIC_CHECK(s < 0 || ctx->bg_profile[s], who + ": a profile entry names an empty slot");
    double mab;
    B->c0[b] = coll_c0(in, in->bg[b], qm, &mab);
    B->slot[b] = s < 0 ? nullptr : ctx->bg_profile[s];
  }
  return 0;
}

// The two entry points on a model, either pusher's, after model_checks.  plain: the entry point of the model trace
// itself, which a call that does not collide is handed to, bit for bit; launch(d, R, C) starts the kernel.
template <class Params, class Plain, class Launch>
int coll_model_trace(xpic_ctx* ctx, const TraceEntry& E, const Params* params, const xpic_field_model* model,
  const TraceArrays& A, const xpic_trace_region* region, const xpic_trace_collisions* collisions, double* coll_4, Plain plain,
  Launch launch)
{
  bool on;
  CollDev Cd;
  XPIC_CALL(coll_setup(E.who, collisions, params->qm, params->dt, &on, &Cd));
  if (!on)
    return coll_none(plain(ctx, A.n, params, model, A.steps, A.sample_every, A.state_6, A.samples, A.it_sum, A.it_max, region,
      A.exit_step, A.alive, A.removed), coll_4);
  OpenRegion R;
  XPIC_CALL(trace_region(E.who, region, true, false, &R));
  return coll_trace(ctx, E, A, R, XPIC_COMPACT_NEVER, coll_4, [&](const TraceDev& d) { launch(d, R, Cd); });
}

// The two entry points on the grid, either pusher's, after grid_check and the pusher's checks.  XPIC_GEOM_NONE is the
// closed trace, and `compact` is read.  plain(open): the open or the closed entry point of the grid trace itself, which a
// call that does not collide is handed to, bit for bit; launch(d, R, C, B) starts the kernel.
template <class Params, class Plain, class Launch>
int coll_grid_trace(xpic_ctx* ctx, const TraceEntry& E, const Params& P, const TraceArrays& A, const xpic_trace_region* region,
  const xpic_trace_collisions* collisions, const int32_t* profile, double* coll_4, Plain plain, Launch launch)
{
  const std::string who = E.who;
  bool on;
  CollDev Cd;
  ProfileBg Bg;
  OpenRegion R;
  XPIC_CALL(coll_setup(who, collisions, P.qm, P.dt, &on, &Cd));
  XPIC_CALL(profile_setup(ctx, who, collisions, profile, P.qm, P.dt, &Bg));
  XPIC_CALL(trace_region(who, region, true, true, &R));
  const int policy = R.kind < 0 ? (int)XPIC_COMPACT_NEVER : region->compact;
  if (!on && (R.kind >= 0 || !A.exit_step)) {
    const int rc = plain(R.kind >= 0);
    if (rc != 0) set_error(who + ": " + xpic_last_error()); // the grid trace's refusal, under this entry point's name too
    else if (R.kind < 0) { // the closed trace: alive and removed as a model trace under XPIC_GEOM_NONE reports them
      if (A.alive && A.sample_every >= 1)
        for (int64_t k = 0; k < A.steps / A.sample_every; ++k) A.alive[k] = A.n;
      if (A.removed) *A.removed = 0;
    }
    return coll_none(rc, coll_4);
  }
  if (!on) Cd.every = 1; // (no region, but an exit_step to honour: the kernel with no background)
  return coll_trace(ctx, E, A, R, policy, coll_4, [&](const TraceDev& d) { launch(d, R, Cd, Bg); });
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
  XPIC_CALL(model_checks(who, ctx, n, params, model));
  const bool cn = params->scheme == XPIC_FO_CN;
  return coll_model_trace(ctx, model_entry(who, "coll_fo_trace"), params, model,
    {n, steps, sample_every, p_6, samples, iterations_sum, iterations_max, exit_step, alive, removed, cn, nullptr}, region,
    collisions, coll_4, xpic_model_full_orbit_trace, [&](const TraceDev& d, const OpenRegion& R, const CollDev& Cd) {
      hipLaunchKernelGGL((cn ? k_coll_fo_trace<true, ModelField, UniformBg, AllLanes>
                             : k_coll_fo_trace<false, ModelField, UniformBg, AllLanes>),
        lane_grid(n), dim3(kBlock), 0, ctx->stream, ctx->g, ModelField{*model}, *params, R, Cd, (long)n, d.s, d.first, d.ns,
        (long)sample_every, d.nsamp, d.samples, d.it_sum, d.it_max, d.exit_step, d.alive, d.removed, d.extra, UniformBg{},
        AllLanes{});
    });
}

int xpic_model_drift_kinetic_trace_collisional(xpic_ctx* ctx, int64_t n, const xpic_dk_params* params,
  const xpic_field_model* model, int64_t steps, int64_t sample_every, double* state_6, double* samples,
  int64_t* iterations_total, int* iterations_max, const xpic_trace_region* region, int64_t* exit_step, int64_t* alive,
  int64_t* removed, const xpic_trace_collisions* collisions, double* coll_4)
{
  const std::string who = "model_drift_kinetic_trace_collisional";
  XPIC_CALL(model_checks(who, ctx, n, params, model));
  return coll_model_trace(ctx, model_entry(who, "coll_dk_trace"), params, model,
    {n, steps, sample_every, state_6, samples, iterations_total, iterations_max, exit_step, alive, removed, true, nullptr},
    region, collisions, coll_4, xpic_model_drift_kinetic_trace, [&](const TraceDev& d, const OpenRegion& R, const CollDev& Cd) {
      hipLaunchKernelGGL((k_coll_dk_trace<ModelField, UniformBg, AllLanes>), lane_grid(n), dim3(kBlock), 0, ctx->stream, ctx->g,
        ModelField{*model}, *params, R, Cd, (long)n, d.s, d.first, d.ns, (long)sample_every, d.nsamp, d.samples, d.it_sum,
        d.it_max, d.exit_step, d.alive, d.removed, d.extra, UniformBg{}, AllLanes{});
    });
}

int xpic_full_orbit_trace_collisional(xpic_ctx* ctx, int64_t n, const xpic_fo_params* params, int64_t steps,
  int64_t sample_every, double* p_6, double* samples, int64_t* iterations_sum, int* iterations_max,
  const xpic_trace_region* region, int64_t* exit_step, int64_t* alive, int64_t* removed,
  const xpic_trace_collisions* collisions, const int32_t* profile, double* coll_4)
{
  const std::string who = "full_orbit_trace_collisional";
  XPIC_CALL(grid_check(ctx, who, n));
  XPIC_CALL(fo_check_params(who, params));
  const bool cn = params->scheme == XPIC_FO_CN;
  const FOGridField F{ctx->field[XPIC_E], ctx->field[XPIC_B]};
  return coll_grid_trace(ctx, model_entry(who, "coll_fo_grid_trace", "coll_fo_grid_trace_compact"), *params,
    {n, steps, sample_every, p_6, samples, iterations_sum, iterations_max, exit_step, alive, removed, cn, nullptr}, region,
    collisions, profile, coll_4,
    [&](bool open) {
      return open ? xpic_full_orbit_trace_open(ctx, n, params, steps, sample_every, p_6, samples, iterations_sum,
                      iterations_max, region, exit_step, alive, removed)
                  : xpic_full_orbit_trace(ctx, n, params, steps, sample_every, p_6, samples, iterations_sum, iterations_max);
    },
    [&](const TraceDev& d, const OpenRegion& R, const CollDev& Cd, const ProfileBg& Bg) {
      hipLaunchKernelGGL((cn ? k_coll_fo_trace<true, FOGridField, ProfileBg, ListedLanes>
                             : k_coll_fo_trace<false, FOGridField, ProfileBg, ListedLanes>),
        lane_grid(d.m), dim3(kBlock), 0, ctx->stream, ctx->g, F, *params, R, Cd, (long)n, d.s, d.first, d.ns,
        (long)sample_every, d.nsamp, d.samples, d.it_sum, d.it_max, d.exit_step, d.alive, d.removed, d.extra, Bg,
        ListedLanes{d.list, d.m});
    });
}

int xpic_drift_kinetic_trace_collisional(xpic_ctx* ctx, int64_t n, const xpic_dk_params* params, int gradB_field,
  int64_t steps, int64_t sample_every, double* state_6, double* samples, int64_t* iterations_total, int* iterations_max,
  const xpic_trace_region* region, int64_t* exit_step, int64_t* alive, int64_t* removed,
  const xpic_trace_collisions* collisions, const int32_t* profile, double* coll_4)
{
  const std::string who = "drift_kinetic_trace_collisional";
  XPIC_CALL(grid_check(ctx, who, n));
  XPIC_CHECK(gradB_field == -1 || (gradB_field >= 0 && gradB_field < XPIC_NFIELDS && ctx->field[gradB_field]),
    who + ": gradB_field is neither -1 nor an allocated field id");
  XPIC_CALL(dk_check_params(who, params, 0));
  const double* gB = gradB_field == -1 ? nullptr : ctx->field[gradB_field];
  return coll_grid_trace(ctx, model_entry(who, "coll_dk_grid_trace", "coll_dk_grid_trace_compact"), *params,
    {n, steps, sample_every, state_6, samples, iterations_total, iterations_max, exit_step, alive, removed, true, nullptr},
    region, collisions, profile, coll_4,
    [&](bool open) {
      return open ? xpic_drift_kinetic_trace_open(ctx, n, params, gradB_field, steps, sample_every, state_6, samples,
                      iterations_total, iterations_max, region, exit_step, alive, removed)
                  : xpic_drift_kinetic_trace(ctx, n, params, gradB_field, steps, sample_every, state_6, samples,
                      iterations_total, iterations_max);
    },
    [&](const TraceDev& d, const OpenRegion& R, const CollDev& Cd, const ProfileBg& Bg) {
      auto go = [&](auto F) {
        hipLaunchKernelGGL((k_coll_dk_trace<decltype(F), ProfileBg, ListedLanes>), lane_grid(d.m), dim3(kBlock), 0,
          ctx->stream, ctx->g, F, *params, R, Cd, (long)n, d.s, d.first, d.ns, (long)sample_every, d.nsamp, d.samples, d.it_sum,
          d.it_max, d.exit_step, d.alive, d.removed, d.extra, Bg, ListedLanes{d.list, d.m});
      };
      if (gB) go(DKGridField<true>{ctx->field[XPIC_E], ctx->field[XPIC_B], gB});
      else go(DKGridField<false>{ctx->field[XPIC_E], ctx->field[XPIC_B], gB});
    });
}

}  // extern "C"
