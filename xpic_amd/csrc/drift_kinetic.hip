// drift_kinetic.hip -- the reference's drift-kinetic (guiding-centre) pusher with its grid interpolation:
//   DriftKineticEsirkepov::interpolate   src/algorithms/drift_kinetic_implicit.cpp:11-31
//   DriftKineticPush::process            src/algorithms/drift_kinetic_push.cpp:48-160
//   PointByField                         src/interfaces/point.h:37-58
// One lane per particle, fp64, no cross-lane operation: the lanes of a wave leave the Picard loop independently.  The
// state {x, y, z, p_parallel, p_perp, mu_p} lives in structure-of-arrays device buffers (s[k * n + q]).  Positions are
// not folded into the box: the gathers wrap their node indices (ie_node), folding is the caller's business as
// correct_coordinates is in the reference.  Single z-slab contexts only (G == 0: every index wraps, so no position,
// however far out, reads outside a field vector).  The C entry points and their argument checks are at the end of the
// file; the staging of the host records, the push and trace drivers and the sample buffer's size are batch.h's.
#include "batch.h"
#include "common.h"
#include "device_common.h"
#include "ie_shape.h"
#include "trace_open.h"

// The pusher's own expressions are contracted per source expression only (not across statements), so k_dk_push and
// k_dk_trace, which inline the same dk_process, round identically whatever surrounds the call.  (The segment shape in
// ie_shape.h keeps the build's default, as in eccapfim.hip: the E gather here returns k_ie_interpolate's bits.)
#pragma clang fp contract(on)

namespace xpic {

namespace {

constexpr int kBlock = kLaneBlock; // batch.h: lane_grid launches workgroups of this size

struct DKPoint {
  double r[3], ppar, pperp, mu;
};

// Vector3::length (src/utils/vector3.h:160-164) is std::hypot of three arguments
__device__ inline double len3(const double* a) { return norm3d(a[0], a[1], a[2]); }
__device__ inline double dot3(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
// Vector3::cross (:212-219)
__device__ inline void cross3(const double* a, const double* b, double* o)
{
  o[0] = +(a[1] * b[2] - a[2] * b[1]);
  o[1] = -(a[0] * b[2] - a[2] * b[0]);
  o[2] = +(a[0] * b[1] - a[1] * b[0]);
}
// Vector3::normalized (:150-158)
__device__ inline void normalized3(const double* a, double* o)
{
  const double l = len3(a);
  if (l > 0) { o[0] = a[0] / l; o[1] = a[1] / l; o[2] = a[2] / l; }
  else { o[0] = o[1] = o[2] = 0.0; }
}

// DriftKineticEsirkepov::interpolate(E_p, B_p, gradB_p, rn, r0): E_p with the segment shape of (rn, r0)
// (ImplicitEsirkepov::interpolate, implicit_esirkepov.cpp:71-90), B_p and gradB_p with Shape::setup(rn, 1.5,
// spline_of_2nd_order) (src/utils/shape.cpp:31-41) and SimpleInterpolation's magnetic products (shape.h:65-72): one set
// of weights, one pass over the nodes.  GRAD = false is the reference's gradB_g == nullptr: gradB_p = 0.
template <bool GRAD>
__device__ inline void dk_fields(const GridDev& g, const double* __restrict__ E, const double* __restrict__ B,
  const double* __restrict__ gB, const double* rn, const double* r0, double* Ep, double* Bp, double* gBp)
{
  const double d[3] = {g.dx, g.dy, g.dz};
  // a position that is not a number, or further out than an int counts cells, has no node: its fields are NaN and no
  // index is formed from it
  bool ok = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) ok = ok && fabs(rn[a]) <= 1e9 * d[a] && fabs(r0[a]) <= 1e9 * d[a];
  if (!ok) {
    const double nan = __builtin_nan("");
#pragma unroll
    for (int a = 0; a < 3; ++a) { Ep[a] = nan; Bp[a] = nan; gBp[a] = GRAD ? nan : 0.0; }
    return;
  }
  {
    IEShape sh;
    sh.setup(g, rn, r0);
    Ep[0] = Ep[1] = Ep[2] = 0.0;
#pragma unroll
    for (int cx = 0; cx < 3; cx++) {
      const int cy = (cx + 1) % 3, cz = (cx + 2) % 3;
#pragma unroll
      for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 3; j++)
#pragma unroll
          for (int k = 0; k < 3; k++) { // i[cx], i[cy], i[cz] of the reference's loop nest, m = its running index
            int o[3];
            o[cx] = i; o[cy] = j; o[cz] = k;
            const int m = ((cx * 2 + i) * 3 + j) * 3 + k;
            Ep[cx] += E[cx * g.cstride + ie_node(g, sh.start[0] + o[0], sh.start[1] + o[1], sh.start[2] + o[2])] * sh.cache[m];
          }
    }
  }
  Bp[0] = Bp[1] = Bp[2] = 0.0;
  gBp[0] = gBp[1] = gBp[2] = 0.0;
  // x and y weights in registers, the z pair formed plane by plane: the plane loop stays rolled, which keeps the 96 loads
  // of a plane in flight without holding all 384 of the footprint in registers
  int st[3], sz[3];
  double No[2][4], Sh[2][4], prz = 0.0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double pr = rn[a] / d[a];
    st[a] = (int)round(pr - 1.5);
    sz[a] = (int)floor(pr + 1.5) + 1 - st[a]; // 3 or 4
    if (a == 2) { prz = pr; break; }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const double gx = (double)(st[a] + t);
      No[a][t] = spline2_ref(pr - gx);
      Sh[a][t] = spline2_ref(pr - (gx + 0.5));
    }
  }
#pragma unroll 1
  for (int kz = 0; kz < sz[2]; ++kz) {
    const double gz = (double)(st[2] + kz);
    const double Noz = spline2_ref(prz - gz), Shz = spline2_ref(prz - (gz + 0.5));
#pragma unroll
    for (int jy = 0; jy < 4; ++jy) {
      if (jy < sz[1]) {
#pragma unroll
        for (int ix = 0; ix < 4; ++ix) {
          if (ix < sz[0]) {
            const long o = ie_node(g, st[0] + ix, st[1] + jy, st[2] + kz);
            const double wx = Shz * Sh[1][jy] * No[0][ix];
            const double wy = Shz * No[1][jy] * Sh[0][ix];
            const double wz = Noz * Sh[1][jy] * Sh[0][ix];
            Bp[0] += B[o] * wx;
            Bp[1] += B[g.cstride + o] * wy;
            Bp[2] += B[2 * g.cstride + o] * wz;
            if (GRAD) {
              gBp[0] += gB[o] * wx;
              gBp[1] += gB[g.cstride + o] * wy;
              gBp[2] += gB[2 * g.cstride + o] * wz;
            }
          }
        }
      }
    }
  }
}

// DriftKineticPush::get_Vd (drift_kinetic_push.cpp:111-119)
__device__ inline void dk_get_Vd(const xpic_dk_params& P, const DKPoint& p0, const double* h, double Vh, double Bh,
  const double* gradBh, const double* Eh, double* Vd)
{
  if (Bh < 1e-12) { Vd[0] = Vd[1] = Vd[2] = 0.0; return; }
  double Exh[3], gb[3], hxg[3];
  cross3(Eh, h, Exh);
#pragma unroll
  for (int c = 0; c < 3; ++c) gb[c] = gradBh[c] / Bh;
  cross3(h, gb, hxg);
  const double f = 1.0 / P.qm * (Vh * Vh / Bh + p0.mu / P.mp);
#pragma unroll
  for (int c = 0; c < 3; ++c) Vd[c] = Exh[c] / Bh + f * hxg[c];
}

// the right-hand side that update_v_parallel (:133-142) assigns and get_residue_v (:150-160) compares with:
// dt qm (Eh . h + term) - mu_term
__device__ inline void dk_v_terms(const xpic_dk_params& P, const DKPoint& p0, double Vh, const double* h, const double* Vd,
  double lenBp, double lenB0, const double* Eh, double* drive, double* mu_term)
{
  const bool small = fabs(Vh) < 1e-12;
  const double term = small ? 0.0 : (dot3(Eh, Vd) / Vh);
  const double dB = lenBp - lenB0;
  *mu_term = small ? 0.0 : (p0.mu / P.mp) * (dB / Vh);
  *drive = P.dt * P.qm * (dot3(Eh, h) + term);
}

// DriftKineticPush::process(dt, pn, p0) (:48-108), statement by statement; pn enters as the initial guess.  Returns the
// reference's `it`: the number of updates made, maxit for a lane that did not meet the tolerances (the reference's
// trailing PetscCheckAbort is the caller's to make).
template <bool GRAD>
__device__ inline int dk_process(const GridDev& g, const double* __restrict__ E, const double* __restrict__ B,
  const double* __restrict__ gB, const xpic_dk_params& P, const DKPoint& p0, DKPoint& pn)
{
  double Eh[3], Bp[3], gradBp[3];
  dk_fields<GRAD>(g, E, B, gB, pn.r, p0.r, Eh, Bp, gradBp); // set_fields(p0.r, pn.r, Eh, Bp, gradBp)
  double Vd[3], Vhh[3], B0[3], Bh[3], gradB0[3], gradBh[3], b0[3], bp[3], h[3];
  double Vh = 0.0, R1 = 0.0, R2 = 0.0;
#pragma unroll
  for (int c = 0; c < 3; ++c) { B0[c] = Bh[c] = Bp[c]; gradB0[c] = gradBh[c] = gradBp[c]; }
  normalized3(Bp, b0);
#pragma unroll
  for (int c = 0; c < 3; ++c) bp[c] = h[c] = b0[c];
  const double lenB0 = len3(B0);
  double lenBp = lenB0;
  int it;
  for (it = 0; it < P.maxit; ++it) {
    Vh = 0.5 * (pn.ppar + p0.ppar);
    dk_get_Vd(P, p0, h, Vh, len3(Bh), gradBh, Eh, Vd);
    double res[3], drive, mu_term;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      Vhh[c] = Vh * h[c];
      res[c] = pn.r[c] - p0.r[c] - P.dt * (Vhh[c] + Vd[c]);
    }
    R1 = len3(res);                                                         // get_residue_r :144-148
    dk_v_terms(P, p0, Vh, h, Vd, lenBp, lenB0, Eh, &drive, &mu_term);
    R2 = fabs((pn.ppar - p0.ppar) - drive + mu_term);                       // get_residue_v :150-160
    if ((R1 < P.eps) && (R2 < P.delta) && it) break;
#pragma unroll
    for (int c = 0; c < 3; ++c) pn.r[c] = p0.r[c] + P.dt * (Vhh[c] + Vd[c]); // update_r :121-125
    dk_fields<GRAD>(g, E, B, gB, pn.r, p0.r, Eh, Bp, gradBp);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      Bh[c] = 0.5 * (Bp[c] + B0[c]);
      gradBh[c] = 0.5 * (gradBp[c] + gradB0[c]);
    }
    normalized3(Bp, bp);
#pragma unroll
    for (int c = 0; c < 3; ++c) h[c] = 0.5 * (bp[c] + b0[c]);
    lenBp = len3(Bp);
    pn.pperp = p0.pperp * sqrt(lenBp / lenB0);                              // update_v_perp :127-131
    dk_v_terms(P, p0, Vh, h, Vd, lenBp, lenB0, Eh, &drive, &mu_term);
    pn.ppar = p0.ppar + drive - mu_term;                                    // update_v_parallel :133-142
  }
  return it;
}

__device__ inline void dk_load(const double* __restrict__ s, long n, long q, DKPoint& p)
{
  p.r[0] = s[q]; p.r[1] = s[n + q]; p.r[2] = s[2 * n + q];
  p.ppar = s[3 * n + q]; p.pperp = s[4 * n + q]; p.mu = s[5 * n + q];
}
__device__ inline void dk_store(double* __restrict__ s, long n, long q, const DKPoint& p)
{
  s[q] = p.r[0]; s[n + q] = p.r[1]; s[2 * n + q] = p.r[2];
  s[3 * n + q] = p.ppar; s[4 * n + q] = p.pperp; s[5 * n + q] = p.mu;
}

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
// particles 0 .. m - 1): as k_fo_trace_open, the step being dk_process as in k_dk_push and k_dk_trace.
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

int dk_check_params(const xpic_dk_params* P)
{
  XPIC_CHECK(P, "drift_kinetic: params is null");
  XPIC_CHECK(P->maxit >= 1, "drift_kinetic: maxit must be >= 1");
  XPIC_CHECK(P->mp != 0.0, "drift_kinetic: mp must not be 0");
  return 0;
}

}  // namespace

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
  XPIC_CALL(dk_check_params(params));
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
  XPIC_CALL(dk_check_params(params));
  XPIC_CHECK(steps >= 0, "drift_kinetic_trace: steps is negative");
  XPIC_CHECK(!samples || sample_every >= 1, "drift_kinetic_trace: sample_every must be >= 1 when samples are asked for");
  XPIC_CHECK(state_6, "drift_kinetic_trace: state_6 is null");
  XPIC_CHECK(iterations_total, "drift_kinetic_trace: iterations_total is null");
  XPIC_CHECK(iterations_max, "drift_kinetic_trace: iterations_max is null");
  int64_t nsamp;
  XPIC_CHECK(trace_sample_bytes(n, steps, sample_every, samples != nullptr, &nsamp) >= 0,
    "drift_kinetic_trace: the sample buffer (48 n steps / sample_every bytes) is too large");
  if (n == 0) return 0;
  return batch_trace(ctx, "dk_trace", XPIC_DK_LAUNCH_STEPS, n, steps, nsamp, true, state_6, samples, iterations_total,
    iterations_max, [&](double* s, long first, int ns, double* sm, long long* it_sum, int* it_max) {
      hipLaunchKernelGGL(gradB ? k_dk_trace<true> : k_dk_trace<false>, lane_grid(n), dim3(kBlock), 0, ctx->stream, ctx->g,
        ctx->field[XPIC_E], ctx->field[XPIC_B], gradB, *params, (long)n, s, first, ns, (long)sample_every, sm, it_sum, it_max);
    });
}

int xpic_drift_kinetic_trace_open(xpic_ctx* ctx, int64_t n, const xpic_dk_params* params, int gradB_field, int64_t steps,
  int64_t sample_every, double* state_6, double* samples, int64_t* iterations_total, int* iterations_max,
  const xpic_trace_region* region, int64_t* exit_step, int64_t* alive, int64_t* removed)
{ // xpic_drift_kinetic_trace with RemoveParticles::execute (remove_particles.cpp:22-38) at the top of every step
  const double* gradB;
  XPIC_CALL(dk_check(ctx, n, gradB_field, &gradB));
  XPIC_CALL(dk_check_params(params));
  OpenRegion R;
  XPIC_CALL(open_region("drift_kinetic_trace_open", region, &R));
  XPIC_CHECK(steps >= 0, "drift_kinetic_trace_open: steps is negative");
  XPIC_CHECK((!samples && !alive) || sample_every >= 1,
    "drift_kinetic_trace_open: sample_every must be >= 1 when samples or alive are asked for");
  XPIC_CHECK(state_6, "drift_kinetic_trace_open: state_6 is null");
  XPIC_CHECK(exit_step, "drift_kinetic_trace_open: exit_step is null");
  XPIC_CHECK(removed, "drift_kinetic_trace_open: removed is null");
  XPIC_CHECK(iterations_total, "drift_kinetic_trace_open: iterations_total is null");
  XPIC_CHECK(iterations_max, "drift_kinetic_trace_open: iterations_max is null");
  int64_t nsamp;
  XPIC_CHECK(trace_sample_bytes(samples ? n : 0, steps, sample_every, samples || alive, &nsamp) >= 0,
    "drift_kinetic_trace_open: the sample buffer (48 n steps / sample_every bytes) is too large");
  *removed = 0;
  if (n == 0 || steps == 0) return 0;
  return batch_trace_open(ctx, "dk_trace_open", "dk_trace_open_compact", XPIC_DK_LAUNCH_STEPS, n, steps, sample_every, nsamp,
    true, region->compact, region->step0, state_6, samples, iterations_total, iterations_max, exit_step, alive, removed,
    [&](double* s, const int64_t* list, long m, long first, int ns, double* sm, long long* it_sum, int* it_max, long long* ex,
      unsigned long long* al, unsigned long long* rm) {
      hipLaunchKernelGGL(gradB ? k_dk_trace_open<true> : k_dk_trace_open<false>, lane_grid(m), dim3(kBlock), 0, ctx->stream,
        ctx->g, ctx->field[XPIC_E], ctx->field[XPIC_B], gradB, *params, R, (long)n, s, (const long long*)list, m, first, ns,
        (long)sample_every, (long)nsamp, sm, it_sum, it_max, ex, al, rm);
    });
}

}  // extern "C"
