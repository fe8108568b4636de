// krylov.hip -- the Krylov drivers behind xpic_solve: restarted GMRES(30) with classical Gram-Schmidt
// (what PETSc's default KSPGMRES runs for the reference, src/impls/ecsim/simulation.cpp:558-567, minus the
// ILU(0) preconditioner that lives in PETSc) and CG for the SPD matM.  The operator applies and the
// fused multi-dot / multi-axpy kernels are in fields.hip; the (m+1) x m Hessenberg least-squares problem
// is tiny and stays on the host, fed by one device->host copy of the iteration's dot products.
#include <cmath>

#include "common.h"

namespace xpic {

namespace {

constexpr int kRestart = 30;

int apply_op(xpic_ctx* c, int op, double* x, double* y)
{
  // the VecScatter inside MatMult: matL reaches 2 planes, matM 1.  On slabs the exchange runs beside the interior rows.
  if (c->g.G > 0 && c->overlap) return op_apply_overlapped(c, op == XPIC_OP_MATA_GMRES, x, y);
  XPIC_CALL(halo_fill(c, x, op == XPIC_OP_MATA_GMRES ? 2 : 1));
  if (op == XPIC_OP_MATA_GMRES) return matA_apply(c, x, y);
  return matM_apply(c, x, y, false);
}

// z = P v: the polynomial in matM + <matL> (abar) or the one in matM, at the degree of the solve on `op`
int precond_vector(xpic_ctx* c, int op, bool abar, const double* v, double* z)
{
  if (abar) return cheb_abar_inverse(c, v, z);
  return cheb_matM_inverse(c, v, z, op == XPIC_OP_MATM_GMRES ? c->cheb_degree_M : c->cheb_degree);
}

// which of the two a solve on `op` starts with: kinds 3 - 5 rebuild their surrogate from the matL the solve runs on
int precond_choose(xpic_ctx* c, int op, bool* abar)
{
  *abar = c->precond >= 3 && op == XPIC_OP_MATA_GMRES;
  if (*abar) {
    XPIC_CALL(abar_update(c));
    // (sums that are not finite: nothing to build a surrogate from)
    if (!c->abar_valid) { *abar = false; if (c->profiling) c->prof["precond_fallback"].launches += 1; }
  }
  return 0;
}

// Right-preconditioned restarted GMRES in its flexible form: z_j = P v_j is kept (kry_Z), the Arnoldi relation is
// A Z = V H and x = x0 + Z y.  The recurrence residual is the TRUE residual |b - A x|, so the stopping rule is the
// same with and without P -- and, the z_j being whatever P returned, it stays so when P is applied in reduced
// precision (fields.hip: cheb_matM_inverse works on fp32 copies).  Compared with x = P (V y) this also saves the
// preconditioner application that closes every cycle.
int gmres(xpic_ctx* c, int op, const double* b, double* x, double rtol, double atol, int maxit, int* its_out,
  int* reason, double* rnorm_out)
{
  const int m = kRestart;
  // both GMRES solves are right-preconditioned by the Chebyshev polynomial in matM: for the "correct" solve on matM
  // itself it is an approximate inverse (1-2 iterations instead of ~25)
  const bool pc = (op == XPIC_OP_MATA_GMRES || op == XPIC_OP_MATM_GMRES) && c->precond != 0;
  // kry_Z is sized with the context (xpic_create / xpic_set_preconditioner): an allocation here, in the middle of a step,
  // could fail on one slab alone and leave the others waiting in the solve's collectives
  XPIC_CHECK(!pc || c->kry_Z, "flexible GMRES workspace missing (xpic_set_preconditioner allocates it)");
  // kinds 3, 4: the predict solve's polynomial is in matM + <matL> (4: rows scaled by the local density), rebuilt from the
  // matL this solve runs on
  bool pc_abar = false;
  if (pc) XPIC_CALL(precond_choose(c, op, &pc_abar));
  // A surrogate whose spectral interval is not proven (precond.hip: abar_proven) runs on PROBATION: every iteration must at
  // least halve the residual (a sound one divides it by 70 - 200; the matM polynomial it would fall back to by 1.5) and
  // return finite numbers, or the solve continues with the matM polynomial -- the GMRES is flexible, its preconditioner may
  // change between two iterations.  The decision rests on all-reduced numbers: every slab takes it alike.
  bool probation = pc_abar && !c->abar_proven;
  if (probation && c->profiling) c->prof["precond_probation"].launches += 1;
  double* Z = c->kry_Z;
  double* V = c->kry_V;
  double* w = c->kry_w;
  std::vector<double> H((m + 1) * m, 0.0), cs(m), sn(m), gg(m + 1), h(m + 2), yv(m);
  XPIC_CALL(vec_set(c, x, 0.0));
  double bb;
  XPIC_CALL(vec_dot_host(c, b, b, &bb));
  // (an infinite |b| would pass for converged below, inf <= rtol inf; the sum is all-reduced: every slab refuses alike)
  XPIC_CHECK(std::isfinite(bb), "solve: the right-hand side is not finite");
  const double bnorm = std::sqrt(bb);
  // The preconditioned "correct" solve costs next to nothing per iteration: it is run two orders beyond the
  // requested tolerance, so its result does not depend on where inside the tolerance the iteration happens to stop
  // (the reference's tables pin 7 digits of the field energy).
  // `tol` drives the iteration; convergence is JUDGED against the requested tolerance `tol_req` (the extra two
  // orders are best effort: running out of iterations between the two is still a converged solve).
  const double tol_req = std::max(rtol * bnorm, atol);
  const double tol = tol_req * (pc && op == XPIC_OP_MATM_GMRES ? 1e-2 : 1.0);
  double rnorm = bnorm;
  int its = 0;
  *reason = 0;
  if (rnorm <= tol) {
    *its_out = 0; *reason = 1; *rnorm_out = rnorm;
    return 0;
  }
  // r = b (x0 = 0)
  const double* r = b;
  while (its < maxit) {
    XPIC_CALL(vec_scale_to(c, V, 1.0 / rnorm, r)); // V_0 = r / |r|
    std::fill(gg.begin(), gg.end(), 0.0);
    gg[0] = rnorm;
    int j = 0;
    for (; j < m && its < maxit; ++j) {
      double* Vj = V + (long)j * c->nvec;
      if (pc) {
        double* Zj = Z + (long)j * c->nvec;
        XPIC_CALL(precond_vector(c, op, pc_abar, Vj, Zj));
        XPIC_CALL(apply_op(c, op, Zj, w));
      }
      else XPIC_CALL(apply_op(c, op, Vj, w));
      // Classical Gram-Schmidt with ONE reduction (one all-reduce on slabs) per iteration: the dot products w . V_i and
      // w . w travel together, and |w - sum h_i V_i|^2 = w.w - sum h_i^2 for an orthonormal V.  V is orthonormal only up
      // to CGS's loss of orthogonality, which grows like eps / (relative residual) as GMRES converges (measured: 1e-10
      // at a relative residual of 1e-6, 1e-7 at 1e-9, and the recurrence then stagnates a decade above the true
      // residual): the identity is used while the residual entering the iteration is above 1e-6 |b| and the
      // subtraction keeps 4 digits; after that the norm is taken explicitly, as PETSc's VecNorm behind VecMAXPY (a
      // second reduction).  At the reference's tolerances (1e-7) that is the last iteration of a solve.  The errors the
      // identity leaves in H (1e-10 relative) also bound what the recurrence can resolve: for a requested tolerance
      // below 1e-8 |b| every norm is explicit (measured: rtol 1e-9 took 12 instead of 10 iterations, 1e-11 a restart).
      const bool pythagoras = tol >= 1e-8 * bnorm && rnorm > 1e-6 * bnorm;
      double ww = 0.0;
      XPIC_CALL(vec_mdot_ww_host(c, w, V, j + 1, h.data(), pythagoras ? &ww : nullptr)); // VecMDot (+ the norm's w . w)
      double hh = 0.0;
      for (int i = 0; i <= j; ++i) hh += h[i] * h[i];
      if (probation && !(std::isfinite(hh) && std::isfinite(ww))) {
        // the surrogate's polynomial blew up: this column is discarded and the iteration taken again with the matM polynomial
        probation = false; pc_abar = false;
        if (c->profiling) c->prof["precond_fallback"].launches += 1;
        --j;
        continue;
      }
      double nrm2 = pythagoras ? ww - hh : 0.0;
      double* Vn = V + (long)(j + 1) * c->nvec;
      if (!pythagoras || !(nrm2 > 1e-4 * ww)) {
        XPIC_CALL(vec_maxpy_norm_host(c, w, V, j + 1, h.data(), &nrm2)); // VecMAXPY + VecNorm
        h[j + 1] = std::sqrt(nrm2);
        if (h[j + 1] != 0.0) XPIC_CALL(vec_scale_to(c, Vn, 1.0 / h[j + 1], w));
      }
      else {
        h[j + 1] = std::sqrt(nrm2);
        XPIC_CALL(vec_maxpy_scaled(c, w, V, j + 1, h.data(), Vn, 1.0 / h[j + 1], nullptr)); // VecMAXPY + VecScale
      }
      for (int i = 0; i < j; ++i) {
        const double t = cs[i] * h[i] + sn[i] * h[i + 1];
        h[i + 1] = -sn[i] * h[i] + cs[i] * h[i + 1];
        h[i] = t;
      }
      const double den = std::hypot(h[j], h[j + 1]);
      if (den == 0.0) { cs[j] = 1.0; sn[j] = 0.0; } // A P V_j = 0: the column adds nothing (singular direction)
      else { cs[j] = h[j] / den; sn[j] = h[j + 1] / den; }
      h[j] = den;
      const double gj_before = gg[j];
      gg[j + 1] = -sn[j] * gg[j];
      gg[j] = cs[j] * gg[j];
      for (int i = 0; i <= j; ++i) H[i * m + j] = h[i];
      ++its;
      const double rprev = rnorm;
      rnorm = std::abs(gg[j + 1]);
      if (probation && !(rnorm <= 0.5 * rprev)) {
        // the column is dropped with the surrogate that built it (a direction that poor costs the Krylov space more than
        // the iteration it took: measured 36 iterations with it kept against 26 for the matM polynomial from the start):
        // the iteration is taken again with the matM polynomial
        probation = false; pc_abar = false;
        if (c->profiling) c->prof["precond_fallback"].launches += 1;
        gg[j] = gj_before; gg[j + 1] = 0.0;
        rnorm = rprev;
        --its; --j;
        continue;
      }
      if (rnorm <= tol) { ++j; break; }
    }
    for (int i = j - 1; i >= 0; --i) {
      double t = gg[i];
      for (int k = i + 1; k < j; ++k) t -= H[i * m + k] * yv[k];
      yv[i] = H[i * m + i] != 0.0 ? t / H[i * m + i] : 0.0;
    }
    XPIC_CALL(vec_maxpy(c, x, pc ? Z : V, j, yv.data())); // x += Z y  (x += V y without P)
    if (rnorm <= tol) break;
    if (its >= maxit) break;
    // restart: r = b - A x, kept in w
    XPIC_CALL(apply_op(c, op, x, w));
    XPIC_CALL(vec_axpby(c, w, 1.0, -1.0, b)); // w = b - w
    double rr;
    XPIC_CALL(vec_dot_host(c, w, w, &rr));
    rnorm = std::sqrt(rr);
    // V_0 is rebuilt from w; park r in the last basis slot so that V_0 may be overwritten
    double* park = V + (long)m * c->nvec;
    XPIC_CALL(vec_copy(c, park, w));
    r = park;
    if (rnorm <= tol) break;
  }
  *its_out = its;
  *rnorm_out = rnorm;
  *reason = rnorm <= tol_req ? 2 : -3; // KSP_CONVERGED_RTOL-like / KSP_DIVERGED_ITS
  return 0;
}

// CG on the SPD matM with fused kernels (fields.hip): per iteration one stencil apply that also yields p . Ap (2 V),
// one pass that updates x and r and yields r . r (6 V) and the direction update (3 V): 11 V, two small reductions.
int cg(xpic_ctx* c, int op, const double* b, double* x, double rtol, double atol, int maxit, int* its_out,
  int* reason, double* rnorm_out)
{
  XPIC_CHECK(op == XPIC_OP_MATM_CG, "CG runs on matM only");
  double* r = c->kry_V;
  double* p = c->kry_V + c->nvec;
  double* Ap = c->kry_w;
  XPIC_CALL(vec_set(c, x, 0.0));
  XPIC_CALL(vec_copy(c, r, b));
  XPIC_CALL(vec_copy(c, p, b));
  double rr;
  XPIC_CALL(vec_dot_host(c, r, r, &rr));
  XPIC_CHECK(std::isfinite(rr), "solve: the right-hand side is not finite");
  const double tol = std::max(rtol * std::sqrt(rr), atol);
  int its = 0;
  while (std::sqrt(rr) > tol && its < maxit) {
    XPIC_CALL(halo_fill(c, p, 1)); // the VecScatter inside MatMult: matM reaches 1 plane
    double pAp;
    XPIC_CALL(cg_apply_dot_host(c, p, Ap, &pAp));
    const double alpha = rr / pAp;
    double rr1;
    XPIC_CALL(cg_update_host(c, alpha, p, Ap, x, r, &rr1));
    const double beta = rr1 / rr;
    rr = rr1;
    XPIC_CALL(vec_axpby(c, p, 1.0, beta, r)); // p = r + beta p
    ++its;
  }
  *its_out = its;
  *rnorm_out = std::sqrt(rr);
  *reason = std::sqrt(rr) <= tol ? 2 : -3;
  return 0;
}

}  // namespace

int precond_apply(xpic_ctx* c, int op, double* r, double* out)
{
  XPIC_CHECK((op == XPIC_OP_MATA_GMRES || op == XPIC_OP_MATM_GMRES) && c->precond != 0, "no preconditioner is applied to this solve");
  XPIC_CHECK(c->kry_Z, "flexible GMRES workspace missing (xpic_set_preconditioner allocates it)");
  bool abar = false;
  XPIC_CALL(precond_choose(c, op, &abar));
  return precond_vector(c, op, abar, r, out);
}

int solve(xpic_ctx* c, int op, const double* rhs, double* x, double rtol, double atol, int maxit, int* its,
  int* reason, double* rnorm)
{
  int rc;
  if (op == XPIC_OP_MATM_CG) rc = cg(c, op, rhs, x, rtol, atol, maxit, its, reason, rnorm);
  else rc = gmres(c, op, rhs, x, rtol, atol, maxit, its, reason, rnorm);
  if (rc) return rc;
  if (*reason < 0) {
    // KSPSetErrorIfNotConverged(ksp, PETSC_TRUE), src/impls/ecsim/simulation.cpp:562
    set_error("KSP did not converge: " + std::to_string(*its) + " iterations, |r| = " + std::to_string(*rnorm));
    return 4;
  }
  return 0;
}

}  // namespace xpic
