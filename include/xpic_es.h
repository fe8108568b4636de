/* xpic_es.h -- the electrostatic scheme XPIC_ES ("es" in the package): Boris push, fused charge deposit and a Poisson
 * solve for E (an extension: the reference has no electrostatic scheme).  Included by
 * xpic_hip.h, which defines xpic_ctx, enum xpic_scheme and the field ids; include that header.  (The entry point stands
 * here and in the package's ES_PROTOTYPES; tests/test_abi_es.py holds the two to each other.)
 *
 * Staggering in time: on entry of xpic_step the positions are r^n (cell-sorted), the velocities are taken as v^{n-1/2},
 * XPIC_E holds E^n, and XPIC_B is an external static field that no step writes.  One xpic_step, in this order:
 *   1. gather   per sort and particle E_p, B_p at r^n with the second-order shape of the basic scheme (Shape::setup(r) +
 *               SimpleInterpolation::process: the node ranges, weight types per component and summation order of the
 *               basic push's gather);
 *   2. kick and move   update_vEB(dt): v^{n-1/2} -> v^{n+1/2}; update_r(dt): r^{n+1} = r^n + dt v^{n+1/2}.  A full
 *               leapfrog step, not the basic scheme's two half moves;
 *   3. deposit  rho of r^{n+1} (not yet folded into the box) by xpic_charge_density's rule: first node
 *               ceil(r / d - 1.5), three nodes per axis, the reference's three-branch spline, value q n / Np, indices
 *               wrapped -- into a scalar accumulator of the context, fused into the push (es.hip: k_es_push).  A particle
 *               may move any number of cells in a step, across the periodic wrap too;
 *   4. re-bin   positions folded into the box, cells updated, as the basic step does;
 *   5. rho      after all sorts: the ghost planes' share added to its owners, + xpic_gauss_background where one is set,
 *               the mean taken out (the uniform neutralising background);
 *   6. solve    xpic_gauss_clean's own path on XPIC_E with this rho: D G phi = D E - rho~, E <- E - G phi (xpic_gauss.h).
 *               E^n is the warm start; rot(+) E and the sum of each component of E are not changed, so a uniform external
 *               field and a caller's solenoidal field persist;
 *   7. report   ksp_iterations = the CG iterations.  No convergence: non-zero return with a message, XPIC_E untouched
 *               (the particles have moved).  A position or velocity that is not finite, or a particle outside its cell: an
 *               error, XPIC_E untouched; the sorts in front of the failing one have been moved and re-binned, the failing
 *               sort's other particles moved: the context's particles are then no consistent state.
 * Tolerances are xpic_set_tolerances'; an XPIC_ES context is created with rtol = 1e-10, atol = 1e-14, maxit = 10000 (the
 * other schemes' default of 100 iterations is a preconditioned GMRES's and would always fail an unpreconditioned CG on the
 * Laplacian).  The stopping rule is xpic_gauss_clean's: |r|_2 <= max(rtol |rho~|_2, atol); an entering residual that
 * meets it costs 0 iterations and E is not written.  xpic_gauss_info counts the steps' solves as cleans.
 *
 * Extents: every grid extent and every z-slab at least 6 cells (the 6-node tiles of the push); smaller is refused by
 * xpic_create.  Allocated: XPIC_E, XPIC_B, XPIC_W0 .. XPIC_W2, the Gauss vectors and the charge accumulator -- no current
 * vector, no XPIC_B0, no Krylov workspace, no round table.
 * Refused on an XPIC_ES context, with a message: xpic_set_gauss_clean (the step already solves Gauss's law), xpic_solve,
 * xpic_precond_apply, the ecsim / ecsimcorr / basic phase entry points, xpic_matL_*, xpic_matA_apply,
 * xpic_sort_current_get, xpic_charge_columns, and any call that names a field the scheme does not hold.
 * Work as on any other context, tested (tests/test_gpu_es.py): xpic_gauss_residual, xpic_gauss_clean (the start:
 * E = 0, clean, then step -- with one caveat: the plain clean takes the mean of rho in a single pass, which leaves a constant
 * of some sqrt(N) eps |rho| in its residual; on a quiet start whose rho~ is 1e-4 of rho (the two-stream of BASELINE
 * configs[1]: 2e-14 against the default atol = 1e-14) it does not converge with the context's default tolerances.  Give that
 * clean an atol above the floor (the test takes 1e-12); the step's own solve refines the mean and meets the defaults),
 * xpic_gauss_background, xpic_energy, xpic_charge_density, xpic_update_cells,
 * xpic_sort_add_particles / _get_particles, xpic_set_tolerances, self_ring z-slabs.  Expected to work, not tested here:
 * moments, attached tracer sets, collisions, the remove / inject / set_particles commands; distinct z-slab ranks are
 * unpinned (a particle that leaves the neighbouring slabs' ghost planes in one step is an error there).
 *
 * xpic_es_push is phases 1 - 3 for one sort alone: it pushes the sort on the context's E and B and returns that sort's rho
 * [nzl][ny][nx] (ghost planes added to their owners; no background, mean not removed).  No re-bin and no solve: the
 * positions it leaves are not folded and the cells are stale until xpic_update_cells. */
#ifndef XPIC_ES_H
#define XPIC_ES_H
#ifdef __cplusplus
extern "C" {
#endif
int xpic_es_push(xpic_ctx* ctx, int sort, double* rho_zyx);
#ifdef __cplusplus
}
#endif
#endif
