// full_orbit_step.h -- the device functions of full_orbit.hip: the gathers and one step of every scheme.  They are in a
// header so that tools/full_orbit_host.cpp can compile the same text for the host and run it against the numpy
// restatement (tests/full_orbit_ref.py) without a GPU.  Included with `#pragma clang fp contract(on)` in force:
// contraction per source expression only, so every caller rounds alike; shape2.h (Shape2, segment_gather_E, len3 / dot3 /
// cross3) comes in here, under that pragma.
//   BorisPush                                   src/algorithms/boris_push.cpp:19-91
//   process_<id>                                tests/boris_push/boris_push.h:20-198
//   CrankNicolsonPush::process                  src/algorithms/crank_nicolson_push.cpp:31-71
//   ImplicitEsirkepov::interpolate              src/algorithms/implicit_esirkepov.cpp:63-91
// A lane whose |B_p| is exactly 0 keeps its v in update_vM / vB / vC1 / vC2: the reference's update_v_impl forms
// v.parallel_to(B_p.normalized()) there, which divides by zero.
#pragma once

#include "shape2.h"

namespace xpic {

struct FOPoint {
  double r[3], p[3];
};

// a lane's point in the [6][n] state of the traces
__device__ inline void fo_load(const double* __restrict__ s, long n, long q, FOPoint& p)
{
  p.r[0] = s[q]; p.r[1] = s[n + q]; p.r[2] = s[2 * n + q];
  p.p[0] = s[3 * n + q]; p.p[1] = s[4 * n + q]; p.p[2] = s[5 * n + q];
}
__device__ inline void fo_store(double* __restrict__ s, long n, long q, const FOPoint& p)
{
  s[q] = p.r[0]; s[n + q] = p.r[1]; s[2 * n + q] = p.r[2];
  s[3 * n + q] = p.p[0]; s[4 * n + q] = p.p[1]; s[5 * n + q] = p.p[2];
}

// a position that is not a number, or further out than an int counts cells, has no node: no index is formed from it
__device__ inline bool fo_in_range(const GridDev& g, const double* r)
{
  return fabs(r[0]) <= 1e9 * g.dx && fabs(r[1]) <= 1e9 * g.dy && fabs(r[2]) <= 1e9 * g.dz;
}

// E_p and B_p at r: one Shape2::setup(r), one pass over its nodes with the electric products (E_x: No_z No_y Sh_x,
// E_y: No_z Sh_y No_x, E_z: Sh_z No_y No_x) and the magnetic ones (B_x: Sh_z Sh_y No_x, B_y: Sh_z No_y Sh_x,
// B_z: No_z Sh_y Sh_x).  WITH_E = false: the magnetic half only (Ep untouched).
template <bool WITH_E>
__device__ inline void fo_gather(const GridDev& g, const double* __restrict__ E, const double* __restrict__ B,
  const double* r, double* Ep, double* Bp)
{
  if (!fo_in_range(g, r)) {
    const double nan = __builtin_nan("");
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      if (WITH_E) Ep[a] = nan;
      Bp[a] = nan;
    }
    return;
  }
  if (WITH_E) Ep[0] = Ep[1] = Ep[2] = 0.0;
  Bp[0] = Bp[1] = Bp[2] = 0.0;
  Shape2 sh;
  sh.setup(g, r);
  sh.nodes([&](int gx, int gy, int gz, double Noz, double Shz, double Noy, double Shy, double Nox, double Shx) {
    const long o = ie_node(g, gx, gy, gz);
    if (WITH_E) {
      Ep[0] += E[o] * (Noz * Noy * Shx);
      Ep[1] += E[g.cstride + o] * (Noz * Shy * Nox);
      Ep[2] += E[2 * g.cstride + o] * (Shz * Noy * Nox);
    }
    Bp[0] += B[o] * (Shz * Shy * Nox);
    Bp[1] += B[g.cstride + o] * (Shz * Noy * Shx);
    Bp[2] += B[2 * g.cstride + o] * (Noz * Shy * Shx);
  });
}

// ImplicitEsirkepov::interpolate(E_p, B_p, rn, r0): B_p with Shape(0.5 (rn + r0)) and the magnetic products, E_p with the
// 54 weights of the segment (ie_shape.h; segment_gather_E)
__device__ inline void fo_gather_segment(const GridDev& g, const double* __restrict__ E, const double* __restrict__ B,
  const double* rn, const double* r0, double* Ep, double* Bp)
{
  if (!fo_in_range(g, rn) || !fo_in_range(g, r0)) {
    const double nan = __builtin_nan("");
#pragma unroll
    for (int a = 0; a < 3; ++a) { Ep[a] = nan; Bp[a] = nan; }
    return;
  }
  const double rm[3] = {0.5 * (rn[0] + r0[0]), 0.5 * (rn[1] + r0[1]), 0.5 * (rn[2] + r0[2])};
  fo_gather<false>(g, E, B, rm, Ep, Bp);
  IEShape sh;
  sh.setup(g, rn, r0);
  segment_gather_E(g, E, sh, Ep);
}

// BorisPush::update_r (boris_push.cpp:19-22)
__device__ inline void fo_update_r(double dt, FOPoint& pt)
{
#pragma unroll
  for (int c = 0; c < 3; ++c) pt.r[c] += pt.p[c] * dt;
}

enum { FO_VM = 0, FO_VB = 1, FO_VC1 = 2, FO_VC2 = 3, FO_VEB = 4 };

// update_vM / vB / vC1 / vC2 (boris_push.cpp:24-46): the angle pair of get_theta_* (:60-83), then update_v_impl (:85-91)
__device__ inline void fo_update_v_magnetic(int kind, double dt, double qm, const double* Bp, double* v)
{
  const double lenB = len3(Bp);
  const double theta = (-1.0) * qm * lenB * dt;
  double first, second; // the AnglePair: "sine" and "cosine"
  if (kind == FO_VM) { first = sin(theta); second = cos(theta); }
  else if (kind == FO_VB) {
    const double d = (1.0 + 0.25 * (theta * theta));
    first = theta / d;
    second = (1.0 - 0.25 * (theta * theta)) / d;
  }
  else if (kind == FO_VC1) {
    first = theta * sqrt(1.0 - 0.25 * (theta * theta));
    second = 1 - 0.5 * (theta * theta);
  }
  else {
    first = theta;
    second = sqrt(1.0 - (theta * theta));
  }
  if (lenB == 0.0) return; // v is left as it is (see the top of this file)
  double b[3], vp[3], vt[3], bxvt[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) b[c] = Bp[c] / lenB; // Vector3::normalized (vector3.h:150-158)
  const double vb = dot3(v, b), bb = dot3(b, b);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    vp[c] = (vb * b[c]) / bb; // parallel_to (:195-199)
    vt[c] = v[c] - vp[c];     // transverse_to (:201-205)
  }
  cross3(b, vt, bxvt);
#pragma unroll
  for (int c = 0; c < 3; ++c) v[c] = vp[c] + second * vt[c] + first * bxvt[c];
}

// BorisPush::update_vEB (boris_push.cpp:48-57), with the reference's division
__device__ inline void fo_update_vEB(double dt, double qm, const double* Ep, const double* Bp, double* v)
{
  const double alpha = dt * qm;
  double a[3], b[3], w[3], bw[3], bbw[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    a[c] = +alpha * Ep[c];
    b[c] = -alpha * Bp[c];
    w[c] = v[c] + 0.5 * a[c];
  }
  cross3(b, w, bw);
  cross3(b, bw, bbw);
  const double den = 1.0 + 0.25 * dot3(b, b);
#pragma unroll
  for (int c = 0; c < 3; ++c) v[c] += a[c] + (bw[c] + 0.5 * bbw[c]) / den;
}

// The field source of fo_step and fo_cn_process: what `interpolate` is to process_<id> and the set_fields_callback to
// CrankNicolsonPush.  A source has
//   void at(const double* r, double* Ep, double* Bp) const                            the fields of a kick at r
//   void segment(const double* rn, const double* r0, double* Ep, double* Bp) const    those of a step r0 -> rn
// FOGrid is the grid of the context (fo_gather, fo_gather_segment); model_source.h has the analytic one.
struct FOGrid {
  const GridDev& g;
  const double* __restrict__ E;
  const double* __restrict__ B;
  __device__ inline void at(const double* r, double* Ep, double* Bp) const { fo_gather<true>(g, E, B, r, Ep, Bp); }
  __device__ inline void segment(const double* rn, const double* r0, double* Ep, double* Bp) const
  {
    fo_gather_segment(g, E, B, rn, r0, Ep, Bp);
  }
};

// interpolate(point.r, E_p, B_p); push.set_fields(E_p, B_p); push.update_v<kind>(h, point)
template <class SRC>
__device__ inline void fo_kick(const SRC& src, int kind, double h, double qm, FOPoint& pt)
{
  double Ep[3], Bp[3];
  src.at(pt.r, Ep, Bp);
  if (kind == FO_VEB) fo_update_vEB(h, qm, Ep, Bp, pt.p);
  else fo_update_v_magnetic(kind, h, qm, Bp, pt.p);
}

// process_<id>(push, point, interpolate) for the 17 Chin ids (boris_push.h:20-198).  The one switch names, for every id,
// the velocity update it uses and which of the four orders of statements it is; the statements below are those of the
// process_ functions, in their order and with their dt / 2 arguments.  `scheme` is uniform over a launch.
template <class SRC>
__device__ inline void fo_step(int scheme, const SRC& src, double qm, double dt, FOPoint& pt)
{
  enum { O_1A, O_1B, O_2A, O_2B };
  int kind = FO_VM, order = O_1A;
  switch (scheme) {
    case XPIC_FO_M1A: kind = FO_VM; order = O_1A; break;
    case XPIC_FO_M1B: case XPIC_FO_MLF: kind = FO_VM; order = O_1B; break;   // process_MLF is process_M1B
    case XPIC_FO_B1A: kind = FO_VB; order = O_1A; break;
    case XPIC_FO_B1B: case XPIC_FO_BLF: kind = FO_VB; order = O_1B; break;
    case XPIC_FO_C1A: kind = FO_VC1; order = O_1A; break;
    case XPIC_FO_C1B: case XPIC_FO_CLF: kind = FO_VC1; order = O_1B; break;
    case XPIC_FO_M2A: kind = FO_VM; order = O_2A; break;
    case XPIC_FO_M2B: kind = FO_VM; order = O_2B; break;
    case XPIC_FO_C2A: kind = FO_VC2; order = O_2A; break;
    case XPIC_FO_B2B: kind = FO_VB; order = O_2B; break;
    case XPIC_FO_EB1A: kind = FO_VEB; order = O_1A; break;
    case XPIC_FO_EB1B: case XPIC_FO_EBLF: kind = FO_VEB; order = O_1B; break;
    case XPIC_FO_EB2B: kind = FO_VEB; order = O_2B; break;
    default: return; // refused on the host
  }
  if (order == O_1B) fo_update_r(dt, pt);                  // 1B: r first
  if (order == O_2B) fo_update_r(dt / 2.0, pt);            // 2B: r_0 + (dt / 2) v_0 -> r_{1/2}
  fo_kick(src, kind, order == O_2A ? dt / 2.0 : dt, qm, pt);
  if (order == O_1A || order == O_2A) fo_update_r(dt, pt); // 1A: r last; 2A: r_0 + dt v_{1/2} -> r_1
  if (order == O_2B) fo_update_r(dt / 2.0, pt);            // 2B: r_{1/2} + (dt / 2) v_1 -> r_1
  if (order == O_2A) fo_kick(src, kind, dt / 2.0, qm, pt); // 2A: v_B(r_1, v_{1/2}, dt / 2) -> v_1
}
// fo_step on the context's grid
__device__ inline void fo_step(int scheme, const GridDev& g, const double* __restrict__ E, const double* __restrict__ B,
  double qm, double dt, FOPoint& pt)
{
  fo_step(scheme, FOGrid{g, E, B}, qm, dt, pt);
}

// calc_residue of CrankNicolsonPush::process (:41-43)
__device__ inline double fo_cn_residue(double dt, double qm, const FOPoint& pn, const FOPoint& p0, const double* vh,
  const double* Ep, const double* Bp)
{
  double vxB[3], res[3];
  cross3(vh, Bp, vxB);
#pragma unroll
  for (int c = 0; c < 3; ++c) res[c] = (pn.p[c] - p0.p[c]) - dt * qm * (Ep[c] + vxB[c]);
  return len3(res);
}

// CrankNicolsonPush::process(dt, pn, p0) (:31-71), statement by statement; pn enters as the initial guess.  Returns the
// reference's `it`: the index of the iteration whose residual met the tolerances, maxit for a lane that ran out of
// iterations (the reference's trailing PetscCheckAbort is the caller's to make).  maxit <= XPIC_FO_MAXIT on the host.
template <class SRC>
__device__ inline int fo_cn_process(const SRC& src, double qm, double dt, double atol, double rtol, int maxit, FOPoint& pn,
  const FOPoint& p0)
{
  double vh[3], Ep[3], Bp[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    vh[c] = 0.5 * (pn.p[c] + p0.p[c]);
    pn.r[c] = p0.r[c] + dt * vh[c];
  }
  src.segment(pn.r, p0.r, Ep, Bp); // set_fields(pn.r, p0.r, E_p, B_p)
  const double r0 = fo_cn_residue(dt, qm, pn, p0, vh, Ep, Bp);
  double rn = 0;
  const double alpha = 0.5 * dt * qm;
  for (int it = 0; it < maxit; ++it) {
    double a[3], b[3], w[3], wxb[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      a[c] = alpha * Ep[c];
      b[c] = alpha * Bp[c];
      w[c] = p0.p[c] + a[c];
    }
    cross3(w, b, wxb);
    const double wb = dot3(w, b), den = (1.0 + dot3(b, b));
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      vh[c] = (w[c] + wxb[c] + b[c] * wb) / den;
      pn.r[c] = p0.r[c] + dt * vh[c];
      pn.p[c] = 2.0 * vh[c] - p0.p[c];
    }
    rn = fo_cn_residue(dt, qm, pn, p0, vh, Ep, Bp);
    if (rn < atol + rtol * r0) return it;
    src.segment(pn.r, p0.r, Ep, Bp);
  }
  return maxit;
}
// fo_cn_process on the context's grid
__device__ inline int fo_cn_process(const GridDev& g, const double* __restrict__ E, const double* __restrict__ B, double qm,
  double dt, double atol, double rtol, int maxit, FOPoint& pn, const FOPoint& p0)
{
  return fo_cn_process(FOGrid{g, E, B}, qm, dt, atol, rtol, maxit, pn, p0);
}

}  // namespace xpic
