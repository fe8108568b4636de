// field_line_step.h -- one lane of the field-line tracer (include/xpic_field_lines.h): the accumulators of a
// line, the tests that stop it and one RK4 step of dr/dl = s F / |F| at a fixed arc-length step.  Templated on the field
// source as fo_step is (full_orbit_step.h): a source has
//   void at(const double* r, double* F) const      the vector at r
// field_lines.hip has the grid source (fo_gather) and the analytic one (ModelSource).  Plain C++: no HIP type appears, so
// a host compiler compiles this text too.  Contraction is off inside every function here, whatever the including file
// has in force, as in k_grad_abs and field_model.h: tests/field_lines_ref.py states the same operations in the same
// order, and only the source's own sums can round differently.
#pragma once

#include <float.h>
#include <math.h>

#include "../../include/xpic_hip.h"

#ifdef __HIPCC__
#define XPIC_FL_FN __host__ __device__ inline
#else
#define XPIC_FL_FN inline
#endif
#ifdef __clang__
#define XPIC_FL_FP _Pragma("clang fp contract(off)")
#else
#define XPIC_FL_FP
#endif

namespace xpic {

struct FLState {
  double r[3], length, volume, fmin, smin, fmax;
  long long steps;
};

// |F|, in plain arithmetic (norm3d and hypot scale their arguments and round differently)
XPIC_FL_FN double fl_abs(const double* F)
{
  XPIC_FL_FP
  return sqrt((F[0] * F[0] + F[1] * F[1]) + F[2] * F[2]);
}

// a line can be followed through a point with this |F|
XPIC_FL_FN bool fl_usable(double f, double f_floor) { return f >= f_floor && f > 0.0 && f <= DBL_MAX; }

// the running extrema at a point the line has reached (L.length is its arc length); a value that is not a number
// compares false and leaves them alone, and so does a point seen twice
XPIC_FL_FN void fl_extrema(FLState& L, double f)
{
  if (f < L.fmin) { L.fmin = f; L.smin = L.length; }
  if (f > L.fmax) L.fmax = f;
}

XPIC_FL_FN double fl_distance(const double* a, const double* b)
{
  XPIC_FL_FP
  const double x = a[0] - b[0], y = a[1] - b[1], z = a[2] - b[2];
  return sqrt((x * x + y * y) + z * z);
}

// One step from L.r, where the field is F0 and |F0| = f0 is usable.  false: |F| at a stage or at the new point is not
// usable, and nothing has changed.  true: L is the state after the step, F0 and f0 are the field there (the next step's
// first stage) and the extrema have seen it.  The four evaluations run in one rolled loop: stage k forms the point the
// k-th direction leads to (r + h/2 t1, r + h/2 t2, r + h t3, r + h/6 (((t1 + 2 t2) + 2 t3) + t4)) and evaluates there.
template <class SRC>
XPIC_FL_FN bool fl_step(const SRC& src, double s, double h, double f_floor, FLState& L, double* F0, double& f0)
{
  XPIC_FL_FP
  const double hh = h / 2.0, h6 = h / 6.0;
  double t[3], acc[3] = {0.0, 0.0, 0.0}, rs[3] = {0.0, 0.0, 0.0}, F[3] = {F0[0], F0[1], F0[2]};
  double f = f0;
#pragma unroll 1
  for (int stage = 0; stage < 4; ++stage) {
    const double w = stage == 1 || stage == 2 ? 2.0 : 1.0;
    const double a = stage < 2 ? hh : (stage == 2 ? h : h6);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      t[c] = s * (F[c] / f);
      acc[c] = stage == 0 ? t[c] : acc[c] + w * t[c];
      rs[c] = L.r[c] + a * (stage < 3 ? t[c] : acc[c]);
    }
    src.at(rs, F);
    f = fl_abs(F);
    if (!fl_usable(f, f_floor)) return false;
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) { L.r[c] = rs[c]; F0[c] = F[c]; }
  L.length = L.length + h;
  L.volume = L.volume + hh * (1.0 / f0 + 1.0 / f);
  L.steps += 1;
  f0 = f;
  fl_extrema(L, f);
  return true;
}

// The steps of one lane in one launch: at most ns steps from L, whose field is evaluated afresh (the same bits the last
// launch carried).  keep(r): the region's test.  sample(L): called after every step.  -> the lane's code, or
// XPIC_LINE_RUNNING when the launch ended first.
template <class SRC, class KEEP, class SAMPLE>
XPIC_FL_FN int fl_advance(const SRC& src, const KEEP& keep, const SAMPLE& sample, double s, double h, double f_floor,
  double close_tol, long long max_steps, int ns, const double* seed, FLState& L)
{
  double F0[3];
  src.at(L.r, F0);
  double f0 = fl_abs(F0);
  fl_extrema(L, f0);
  for (int k = 0; k < ns; ++k) {
    if (L.steps >= max_steps) return XPIC_LINE_MAXSTEPS;
    if (!keep(L.r)) return XPIC_LINE_LEFT;
    // back at the seed: this step, which passes it, closes the line (a test of the start point, so a launch can repeat it)
    const bool closing = close_tol > 0.0 && L.steps >= 2 && fl_distance(L.r, seed) <= close_tol;
    if (!fl_usable(f0, f_floor) || !fl_step(src, s, h, f_floor, L, F0, f0)) return XPIC_LINE_NULL;
    sample(L);
    if (closing) return XPIC_LINE_CLOSED;
  }
  return L.steps >= max_steps ? XPIC_LINE_MAXSTEPS : XPIC_LINE_RUNNING;
}

}  // namespace xpic
