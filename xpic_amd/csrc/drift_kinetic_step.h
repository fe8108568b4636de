// drift_kinetic_step.h -- the device functions of drift_kinetic.hip: the gather and one step of the drift-kinetic pusher,
// the twin of full_orbit_step.h.  They are in a header so that compare_trace.hip, which advances a guiding centre beside a
// full orbit in one lane, inlines the same text as k_dk_push and k_dk_trace.  Included with `#pragma clang fp contract(on)`
// in force: contraction per source expression only, so every caller rounds alike; shape2.h (Shape2, segment_gather_E,
// len3 / dot3 / cross3) comes in here, under that pragma.
//   DriftKineticEsirkepov::interpolate   src/algorithms/drift_kinetic_implicit.cpp:11-31
//   DriftKineticPush::process            src/algorithms/drift_kinetic_push.cpp:48-160
//   PointByField                         src/interfaces/point.h:37-58
#pragma once

#include "shape2.h"

namespace xpic {

namespace {

struct DKPoint {
  double r[3], ppar, pperp, mu;
};

// Vector3::normalized (src/utils/vector3.h:150-158)
__device__ inline void normalized3(const double* a, double* o)
{
  const double l = len3(a);
  if (l > 0) { o[0] = a[0] / l; o[1] = a[1] / l; o[2] = a[2] / l; }
  else { o[0] = o[1] = o[2] = 0.0; }
}

// DriftKineticEsirkepov::interpolate(E_p, B_p, gradB_p, rn, r0): E_p with the segment shape of (rn, r0)
// (segment_gather_E), B_p and gradB_p with Shape2::setup(rn) and SimpleInterpolation's magnetic products
// (shape.h:65-72): one set of weights, one pass over the nodes.  GRAD = false is the reference's gradB_g == nullptr:
// gradB_p = 0.
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
  IEShape seg;
  seg.setup(g, rn, r0);
  segment_gather_E(g, E, seg, Ep);
  Bp[0] = Bp[1] = Bp[2] = 0.0;
  gBp[0] = gBp[1] = gBp[2] = 0.0;
  Shape2 sh;
  sh.setup(g, rn);
  sh.nodes([&](int gx, int gy, int gz, double Noz, double Shz, double Noy, double Shy, double Nox, double Shx) {
    const long o = ie_node(g, gx, gy, gz);
    const double wx = Shz * Shy * Nox;
    const double wy = Shz * Noy * Shx;
    const double wz = Noz * Shy * Shx;
    Bp[0] += B[o] * wx;
    Bp[1] += B[g.cstride + o] * wy;
    Bp[2] += B[2 * g.cstride + o] * wz;
    if (GRAD) {
      gBp[0] += gB[o] * wx;
      gBp[1] += gB[g.cstride + o] * wy;
      gBp[2] += gB[2 * g.cstride + o] * wz;
    }
  });
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

// The field source of dk_process: what the reference's set_fields_callback is to DriftKineticPush.  A source has
//   void dk(const double* rn, const double* r0, double* Ep, double* Bp, double* gBp) const
// DKGrid is the grid of the context (dk_fields); model_source.h has the analytic one.
template <bool GRAD>
struct DKGrid {
  const GridDev& g;
  const double* __restrict__ E;
  const double* __restrict__ B;
  const double* __restrict__ gB;
  __device__ inline void dk(const double* rn, const double* r0, double* Ep, double* Bp, double* gBp) const
  {
    dk_fields<GRAD>(g, E, B, gB, rn, r0, Ep, Bp, gBp);
  }
};

// DriftKineticPush::process(dt, pn, p0) (:48-108), statement by statement; pn enters as the initial guess.  Returns the
// reference's `it`: the number of updates made, maxit for a lane that did not meet the tolerances (the reference's
// trailing PetscCheckAbort is the caller's to make).
template <class SRC>
__device__ inline int dk_process(const SRC& src, const xpic_dk_params& P, const DKPoint& p0, DKPoint& pn)
{
  double Eh[3], Bp[3], gradBp[3];
  src.dk(pn.r, p0.r, Eh, Bp, gradBp); // set_fields(p0.r, pn.r, Eh, Bp, gradBp)
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
    src.dk(pn.r, p0.r, Eh, Bp, gradBp);
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

// dk_process on the context's grid
template <bool GRAD>
__device__ inline int dk_process(const GridDev& g, const double* __restrict__ E, const double* __restrict__ B,
  const double* __restrict__ gB, const xpic_dk_params& P, const DKPoint& p0, DKPoint& pn)
{
  return dk_process(DKGrid<GRAD>{g, E, B, gB}, P, p0, pn);
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

}  // namespace

}  // namespace xpic
