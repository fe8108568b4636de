// pair_compare.h -- what the two kernels of compare_trace.hip share on the device: the guiding-centre / full-orbit half of
// the reference's update_comparison_stats (tests/drift_kinetic_push/drift_kinetic_push.h:311-328) and the wave maximum of
// their curves.  Included after full_orbit_step.h and drift_kinetic_step.h, with `#pragma clang fp contract(on)` in force.
#pragma once

namespace xpic {

namespace {

// update_comparison_stats (drift_kinetic_push.h:311-328), statement by statement; Bg is its `B`, mp its `m`.
// e = {err_z, err_parallel, err_mu, err_energy}
__device__ inline void pair_errors(const DKPoint& gc, const FOPoint& fo, const double* Bg, double mp, double* e)
{
  e[0] = fabs(gc.r[2] - fo.r[2]);
  // Vector3::parallel_to (vector3.h:195-199): (dot(ref) * ref) / ref.squared(); transverse_to (:201-205)
  const double pb = dot3(fo.p, Bg), bb = dot3(Bg, Bg);
  double par[3], tr[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    par[c] = (pb * Bg[c]) / bb;
    tr[c] = fo.p[c] - par[c];
  }
  const double v_par = len3(par);
  e[1] = fabs(gc.ppar - v_par);
  const double p_perp = len3(tr);
  const double mu = 0.5 * mp * (p_perp * p_perp) / len3(Bg);
  e[2] = fabs(gc.mu - mu);
  const double energy_drift = 0.5 * (gc.pperp * gc.pperp + gc.ppar * gc.ppar); // get_kinetic_energy :270-278
  const double energy_boris = 0.5 * dot3(fo.p, fo.p);
  e[3] = fabs(energy_drift - energy_boris);
}

// the largest v of a wave in lane 0, by the rule of the running maxima; no v is NaN here
__device__ inline double wave_max(double v)
{
  for (int o = 32; o > 0; o >>= 1) {
    const double t = __shfl_down(v, o, 64);
    v = (v < t) ? t : v;
  }
  return v;
}

}  // namespace

}  // namespace xpic
