// timed_source.h -- the time envelope of the model's E (include/xpic_hip.h: xpic_field_envelope) and the field source
// that carries one step's factor: ModelSource (model_source.h) for a callback that captures the loop index,
//   tests/crank_nicolson_push/crank_nicolson_push_ex3.cpp:39-58     E_p = E0 * (t * dt); B_p = B0;
// envelope_factor and envelope_check are plain C++ as field_model.h is (a host compiler compiles them); contraction is
// off inside envelope_factor, so the ramp and the harmonic's argument round as the numpy restatement's do and only cos
// can differ.  TimedModelSource is device code.
#pragma once

#include <cmath>

#include "field_model.h"
#ifdef __HIPCC__
#include "model_source.h"
#endif

namespace xpic {

// the factor of step `step` (counted from the start of the whole trace): t = (double)step * dt is one product, the
// reference's `t * dt` with its integer t.  XPIC_ENV_CONSTANT (and an unknown kind, refused by envelope_check): 1.
XPIC_MODEL_FN double envelope_factor(const xpic_field_envelope& e, long long step, double dt)
{
  XPIC_MODEL_FP
  const double t = (double)step * dt;
  if (e.kind == XPIC_ENV_RAMP) return e.a + e.b * t;
  if (e.kind == XPIC_ENV_HARMONIC) return cos(e.omega * t + e.phase);
  return 1.0;
}

// the argument checks of an envelope: nullptr when it is usable (a null envelope is the constant one)
inline const char* envelope_check(const xpic_field_envelope* e)
{
  if (!e) return nullptr;
  if (e->kind < 0 || e->kind >= XPIC_ENV_NKINDS) return "unknown envelope kind";
  if (e->kind == XPIC_ENV_RAMP && !(std::isfinite(e->a) && std::isfinite(e->b))) return "ramp envelope: a and b must be finite";
  if (e->kind == XPIC_ENV_HARMONIC && !(std::isfinite(e->omega) && std::isfinite(e->phase)))
    return "harmonic envelope: omega and phase must be finite";
  return nullptr;
}

#ifdef __HIPCC__

namespace {

// ModelSource with the step's factor on E: E_p = E_model * f component by component (Vector3R * scalar), B_p and
// gradB_p untouched.  on == false (XPIC_ENV_CONSTANT): no factor at all, ModelSource's values as they are.
struct TimedModelSource {
  ModelSource src;
  bool on;
  double f;
  __device__ inline void scale(double* Ep) const
  {
    if (on) { Ep[0] = Ep[0] * f; Ep[1] = Ep[1] * f; Ep[2] = Ep[2] * f; }
  }
  __device__ inline void dk(const double* rn, const double* r0, double* Ep, double* Bp, double* gBp) const
  {
    src.dk(rn, r0, Ep, Bp, gBp);
    scale(Ep);
  }
  __device__ inline void at(const double* r, double* Ep, double* Bp) const
  {
    src.at(r, Ep, Bp);
    scale(Ep);
  }
  __device__ inline void segment(const double* rn, const double* r0, double* Ep, double* Bp) const
  {
    src.segment(rn, r0, Ep, Bp);
    scale(Ep);
  }
};

}  // namespace

#endif  // __HIPCC__

}  // namespace xpic
