// model_source.h -- the analytic field source of the step functions (full_orbit_step.h: FOGrid, drift_kinetic_step.h:
// DKGrid): where the grid sources gather, this one evaluates a model of field_model.h in registers, at the position the
// reference's set_fields_callback is given.  Shared by model_trace.hip, compare_trace.hip and
// timed_source.h, whose TimedModelSource puts a step's factor on this one's E.  Device code only.
#pragma once

#include "field_model.h"

namespace xpic {

namespace {

// the analytic field source of the step functions (full_orbit_step.h: FOGrid, drift_kinetic_step.h: DKGrid)
struct ModelSource {
  const xpic_field_model& m;
  __device__ inline void dk(const double* rn, const double*, double* Ep, double* Bp, double* gBp) const
  {
    model_fields(m, rn, Ep, Bp, gBp);
  }
  __device__ inline void at(const double* r, double* Ep, double* Bp) const
  {
    double gBp[3];
    model_fields(m, r, Ep, Bp, gBp);
  }
  __device__ inline void segment(const double* rn, const double* r0, double* Ep, double* Bp) const
  {
    const double rm[3] = {(r0[0] + rn[0]) / 2, (r0[1] + rn[1]) / 2, (r0[2] + rn[2]) / 2};
    double gBp[3];
    model_fields(m, rm, Ep, Bp, gBp);
  }
};

}  // namespace

}  // namespace xpic
