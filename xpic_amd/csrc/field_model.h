// field_model.h -- the closed set of analytic field models (include/xpic_hip.h: xpic_field_model) evaluated at one
// position: the reference's set_fields_callback functions restated statement by statement.
//   XPIC_MODEL_UNIFORM            tests/drift_kinetic_push/drift_kinetic_push_ex1.cpp:9-13, ex2.cpp:11-16,
//                                 tests/crank_nicolson_push/crank_nicolson_push_ex1.cpp:74-77, ex2.cpp:78-83
//   XPIC_MODEL_LINEAR             tests/drift_kinetic_push/drift_kinetic_push_ex3.cpp:12-17
//   XPIC_MODEL_QUADRATIC_MIRROR   quadratic_magnetic_mirror, tests/drift_kinetic_push/drift_kinetic_push.h:24-70, with the
//                                 rotating E of drift_kinetic_push_ex4.cpp:12-22
//   XPIC_MODEL_GAUSSIAN_MIRROR    gaussian_magnetic_mirror, drift_kinetic_push.h:72-157
// Plain C++: no HIP type appears, so a host compiler compiles this file too (tests and tools restate nothing twice).
// Under hipcc every function is __host__ __device__.  POW2(A) is (A) * (A) and POW3(A) is (A) * (A) * (A)
// (src/utils/utils.h:67-68), written out.  Contraction is off inside these functions, whatever the including file has in
// force: the reference's build forms no fused multiply-add here, and neither does the numpy restatement the tests compare
// with, so sums and products agree to the bit and only exp, sin and hypot can differ.
#pragma once

#include <cmath>

#include "../../include/xpic_hip.h"

#ifdef __HIPCC__
#define XPIC_MODEL_FN __host__ __device__ inline
#else
#define XPIC_MODEL_FN inline
#endif
#ifdef __clang__
#define XPIC_MODEL_FP _Pragma("clang fp contract(off)")
#else
#define XPIC_MODEL_FP
#endif

namespace xpic {

// ---- quadratic_magnetic_mirror (drift_kinetic_push.h:24-70); Rc = W / 2, L = D / 2 (:30-31)
XPIC_MODEL_FN void model_quadratic(const xpic_field_model& m, const double* pos, double* E, double* B, double* gradB)
{
  XPIC_MODEL_FP
  const double Rc = m.W / 2, L = m.D / 2;
  const double x = pos[0] - Rc;
  const double y = pos[1] - Rc;
  const double z = pos[2] - L;
  const double r = hypot(x, y);
  const double Bz = m.B_min + (m.B_max - m.B_min) * ((z / m.D) * (z / m.D));   // get_Bz :33-36
  const double Bm = Bz * (1.0 + 0.5 * ((r / m.W) * (r / m.W)));                // get_B :38-41
  B[0] = 0.0; B[1] = 0.0; B[2] = Bm;
  const double dBz_dz = 2 * (m.B_max - m.B_min) * z / (m.D * m.D);             // get_dBz_dz :43-46
  const double dB_dz = dBz_dz * (1.0 + 0.5 * ((r / m.D) * (r / m.D)));         // (r / D here, r / W in get_B: as written)
  const double dB_dr = Bz * r / (m.D * m.D);
  if (r > 1e-10) { gradB[0] = x / r * dB_dr; gradB[1] = y / r * dB_dr; gradB[2] = dB_dz; }
  else { gradB[0] = 0.0; gradB[1] = 0.0; gradB[2] = dB_dz; }
  // drift_kinetic_push_ex4.cpp:17-21; E_phi == 0 and phi == 0: the callback of the other examples, which leaves E_p alone
  if (m.E_phi != 0.0 || m.phi != 0.0) {
    E[0] = +m.E_phi * (pos[1] - Rc);
    E[1] = -m.E_phi * (pos[0] - Rc);
    E[2] = +m.phi * M_PI / m.D * sin(M_PI * (pos[2] - L) / m.D);
  }
  else { E[0] = E[1] = E[2] = 0.0; }
}

// ---- gaussian_magnetic_mirror (drift_kinetic_push.h:72-157); S = W^2, Rc = L (:78-79)
XPIC_MODEL_FN void model_gaussian(const xpic_field_model& m, const double* pos, double* E, double* B, double* gradB)
{
  XPIC_MODEL_FP
  const double L = m.L, S = m.W * m.W, Rc = m.L, dB = m.B_max - m.B_min;
  const double x = pos[0] - Rc;
  const double y = pos[1] - Rc;
  const double z = pos[2] - L;
  const double r2 = x * x + y * y;
  const double r = sqrt(r2);
  // exp(z, -L) and exp(z, +L) (:81-84): every get_ function below forms the same two values
  const double t1 = (z + L), t2 = (z - L);
  const double e1 = exp(-(t1 * t1) / S), e2 = exp(-(t2 * t2) / S);
  const double Bz = m.B_min + dB * (e1 + e2);                                                      // get_Bz :87-90
  const double dBz_dz = dB * ((-2.0 * t1 / S * e1) + (-2.0 * t2 / S * e2));                        // get_dBz_dz :92-97
  const double d2Bz_dz2 =                                                                          // get_d2Bz_dz2 :99-106
    dB * ((-2.0 / S + 4.0 * ((t1 / S) * (t1 / S))) * e1 + (-2.0 / S + 4.0 * ((t2 / S) * (t2 / S))) * e2);
  const double d3Bz_dz3 = dB *                                                                     // get_d3Bz_dz3 :108-115
    ((12.0 * t1 / (S * S) - 8.0 * ((t1 / S) * (t1 / S) * (t1 / S))) * e1 +
      (12.0 * t2 / (S * S) - 8.0 * ((t2 / S) * (t2 / S) * (t2 / S))) * e2);
  B[0] = -0.5 * x * dBz_dz;
  B[1] = -0.5 * y * dBz_dz;
  B[2] = Bz - 0.25 * r2 * d2Bz_dz2;
  const double dB_dr = -0.5 * r * d2Bz_dz2;
  const double dB_dz = dBz_dz - 0.25 * r2 * d3Bz_dz3;
  if (r > 1e-12) { gradB[0] = x / r * dB_dr; gradB[1] = y / r * dB_dr; gradB[2] = dB_dz; }
  else { gradB[0] = 0; gradB[1] = 0; gradB[2] = dB_dz; }
  E[0] = E[1] = E[2] = 0.0;
}

// the callback's (E_p, B_p, gradB_p) at pos.  An unknown kind (refused by model_check) gives zeros.
XPIC_MODEL_FN void model_fields(const xpic_field_model& m, const double* pos, double* E, double* B, double* gradB)
{
  XPIC_MODEL_FP
  if (m.kind == XPIC_MODEL_QUADRATIC_MIRROR) { model_quadratic(m, pos, E, B, gradB); return; }
  if (m.kind == XPIC_MODEL_GAUSSIAN_MIRROR) { model_gaussian(m, pos, E, B, gradB); return; }
  E[0] = m.E0[0]; E[1] = m.E0[1]; E[2] = m.E0[2];
  B[0] = m.B0[0]; B[1] = m.B0[1]; B[2] = m.B0[2];
  gradB[0] = gradB[1] = gradB[2] = 0.0;
  if (m.kind != XPIC_MODEL_LINEAR) return;
  // B_p = B0 + (rn - r0).dot(gradB0) * gradB0.normalized(); gradB_p = gradB0 (ex3.cpp:15-16); Vector3::length is
  // std::hypot of three arguments, normalized() of a null vector is null (src/utils/vector3.h:150-164)
#ifdef __HIP_DEVICE_COMPILE__
  const double l = norm3d(m.g[0], m.g[1], m.g[2]);
#else
  const double l = std::hypot(m.g[0], m.g[1], m.g[2]);
#endif
  const double s = (pos[0] - m.r0[0]) * m.g[0] + (pos[1] - m.r0[1]) * m.g[1] + (pos[2] - m.r0[2]) * m.g[2];
  const bool has = l > 0;
  B[0] = m.B0[0] + s * (has ? m.g[0] / l : 0.0);
  B[1] = m.B0[1] + s * (has ? m.g[1] / l : 0.0);
  B[2] = m.B0[2] + s * (has ? m.g[2] / l : 0.0);
  gradB[0] = m.g[0]; gradB[1] = m.g[1]; gradB[2] = m.g[2];
}

// the argument checks of a model: nullptr when it is usable, otherwise what is wrong with it
inline const char* model_check(const xpic_field_model* m)
{
  if (!m) return "model is null";
  if (m->kind < 0 || m->kind >= XPIC_MODEL_NKINDS) return "unknown model kind";
  if (m->kind == XPIC_MODEL_QUADRATIC_MIRROR && (m->W == 0.0 || m->D == 0.0)) return "quadratic mirror: W and D must not be 0";
  if (m->kind == XPIC_MODEL_GAUSSIAN_MIRROR && m->W == 0.0) return "gaussian mirror: W must not be 0";
  return nullptr;
}

}  // namespace xpic
