/* xpic_gauss.h -- Gauss's law div E = rho on the device: its residual, and a cleaner that restores it with a scalar
 * Poisson solve (an extension: the reference has no Gauss-law cleaner).  Included by xpic_hip.h, which
 * defines xpic_ctx and the field ids; include that header.  (The entry points stand here and in the package's
 * GAUSS_PROTOTYPES, as those of xpic_field_lines.h stand in FIELD_LINE_PROTOTYPES; tests/test_abi_gauss.py holds the two
 * to each other.)
 *
 * All in float64 on the nodes of the periodic box, indices wrapped; d = (dx, dy, dz):
 *     (D F)[x,y,z]   = (Fx[x] - Fx[x-1]) / dx + (Fy[y] - Fy[y-1]) / dy + (Fz[z] - Fz[z-1]) / dz
 *                      the reference's negative-shift divergence (src/utils/operators.cpp:275-333);
 *     (G phi)_x[x]   = (phi[x+1] - phi[x]) / dx, likewise y and z: the gradient on the edges where E lives.  D G is the
 *                      symmetric 7-point Laplacian and rot(+) G = 0.  At an extent of 2 the nodes x-1 and x+1 are one
 *                      node and the stencil folds onto it (off-diagonal weight 2 / d^2), as the wrapped matrices do;
 *     rho            = the sum of xpic_charge_density over the sorts in creation order, then + the background
 *                      (xpic_gauss_background) where one is set;
 *     rho~           = rho - mean(rho), the mean over the whole box: a periodic box is solvable only for a mean-free
 *                      right-hand side, and the mean taken out is the uniform neutralising background.  It is returned;
 *     res            = D F - rho~.
 * Clean: solve D G phi = res for the mean-free phi by unpreconditioned conjugate gradients from phi = 0, then
 * F <- F - G phi.  rot(+) F and the sum of each component of F do not change.  (A context may choose the direct solve of
 * xpic_poisson.h instead of CG; `iterations` then counts its applications.  CG is the default.)
 * Stopping rule: |r|_2 <= max(rtol |rho~|_2, atol) -- relative to the charge, not to the entering residual.  When CG's
 * recurrence meets it the residual res - D G phi is formed explicitly once and the iteration goes on from it if that one
 * does not.  An entering residual that meets the rule: 0 iterations, F is not written.  No convergence within maxit
 * iterations: non-zero return with a message, F is not written.  A field or a charge that is not finite: an error.
 *
 * field: XPIC_E, XPIC_EP, or any allocated vector filled like E -- except XPIC_W2, which the charge deposit uses as
 * scratch (as xpic_charge_density does): the calls overwrite XPIC_W2 and write nothing else but `field` (the clean) and
 * their outputs.  The solve's own vectors are allocated by the first call; a context that never calls these entry points
 * allocates and launches nothing for them.  Scalars in and out are [nzl][ny][nx] of this slab.
 * Z-slabs: ghost planes by the halo exchange, sums by the all-reduce of xpic_solve's CG; pinned on a self_ring context,
 * unpinned on distinct ranks.
 *
 * xpic_set_gauss_clean(every = k > 0): every xpic_step whose count (calls of xpic_step on this context, from 1) is a
 * multiple of k cleans XPIC_E after the step's last field update and before the attached tracer sets ride, with the
 * charge of the positions the step leaves behind; a clean that fails fails the step.  every = 0 (the default): off. */
#ifndef XPIC_GAUSS_H
#define XPIC_GAUSS_H
#ifdef __cplusplus
extern "C" {
#endif
/* rho_zyx: a static charge density added to the sorts' (immobile ions, say); NULL clears it */
int xpic_gauss_background(xpic_ctx* ctx, const double* rho_zyx);
/* res_zyx: the residual, or NULL; out4 = { |res|_1, |res|_2, mean rho removed, |rho~|_2 } */
int xpic_gauss_residual(xpic_ctx* ctx, int field, double* res_zyx, double* out4);
/* phi_zyx: the potential, or NULL; iterations: required; out4 = { |res|_2 before, |res|_2 after (formed from the
 * corrected field, not CG's recurrence), mean rho removed, |G phi|_2 } */
int xpic_gauss_clean(xpic_ctx* ctx, int field, double rtol, double atol, int maxit, double* phi_zyx, int* iterations,
  double* out4);
int xpic_set_gauss_clean(xpic_ctx* ctx, int every, double rtol, double atol, int maxit);
/* out6 = { cleans done (0-iteration ones included), iterations total, last |res|_2 before, last after, last mean,
 * last iterations } */
int xpic_gauss_info(xpic_ctx* ctx, double* out6);
#ifdef __cplusplus
}
#endif
#endif
