/* xpic_poisson.h -- a direct solve of the scalar periodic 7-point Poisson problem D G phi = res of xpic_gauss.h, by a
 * separable discrete Hartley transform on the device (an extension: the reference has no such solver, and no Poisson solve
 * at all).  Included by xpic_hip.h, which defines xpic_ctx; include that header.  (The entry points stand
 * here and in the package's POISSON_PROTOTYPES; tests/test_abi_poisson.py holds the two to each other.)
 *
 * D G is a sum of three Kronecker terms, each a symmetric circulant along one axis.  The discrete Hartley matrix
 *     H_n[k][j] = (cos(2 pi k j / n) + sin(2 pi k j / n)) / sqrt(n)
 * is real, symmetric and its own inverse, and diagonalises every symmetric circulant of extent n; the eigenvalues of the
 * term of axis a are lam_a[k] = -4 sin^2(pi k / n_a) / d_a^2 (the folded stencil of an extent of 2 and the empty one of an
 * extent of 1 included).  Hence
 *     phi = Hx Hy Hz [ (Hx Hy Hz res) / (lam_x[kx] + lam_y[ky] + lam_z[kz]) ],  the (0, 0, 0) mode set to 0:
 * the mean-free phi.  All float64, no complex arithmetic, any extent: six dense passes C = H . X along one axis each on the
 * matrix cores (v_mfma_f64_16x16x4_f64), the division folded into the third.  The summation order is fixed: two calls on
 * the same data return the same bits.
 * Tables: the library builds H_n per distinct extent and the three lam on the host, once, at the first direct solve of a
 * context -- in long double, k j reduced modulo n in integers before the angle is formed, rounded to double -- uploads
 * them and frees them with the context.  A context that never solves directly allocates and launches nothing for it.  The
 * work planes are two of the Gauss vectors' (those CG keeps its direction and its product in): no second workspace.
 *
 * xpic_set_poisson_solver: the solve that xpic_gauss_clean, the clean that rides with xpic_step (xpic_set_gauss_clean) and
 * the XPIC_ES step take on this context.  XPIC_POISSON_CG is the default of every context, XPIC_ES included; with it every
 * call launches what it launched before this header existed and returns the same bits.  With XPIC_POISSON_DIRECT the solve
 * is: one application of the transform solve to r (= res at first), added to phi; r = res - D G phi formed explicitly; done
 * when |r|_2 meets xpic_gauss_clean's stopping rule, else another application to the new r (iterative refinement).
 * `iterations`, wherever a clean or a step reports it, then counts the applications (1 where float64 allows the tolerance
 * in one).  No convergence -- maxit applications, or one that did not halve the residual it was given -- is reported as
 * CG's is: non-zero return, the same message, the field untouched.  Everything around the solve is the same code for both
 * kinds: the charge, its mean, the stopping rule, the 0-iteration case, the correction, the `after` norm, xpic_gauss_info.
 * Refused, with a message, the kind left as it was: an unknown kind; XPIC_POISSON_DIRECT on a context with ghost planes
 * (z-slabs, self_ring included) -- the direct solve is for single-slab contexts only, a transform along z needs every plane
 * -- or with an extent above XPIC_POISSON_MAX_EXTENT = 1024 (an 8 MB table).
 *
 * xpic_poisson_apply: one application of the transform solve to rhs - mean(rhs), without refinement, whatever the
 * context's kind: phi [nz][ny][nx] from rhs [nz][ny][nx].  The hook that pins the kernels, as xpic_precond_apply pins the
 * preconditioner.  The same refusals; a right-hand side that is not finite is an error.  Overwrites the Gauss vectors.
 *
 * xpic_poisson_solve: the refinement itself on rhs - mean(rhs), whatever the context's kind -- the function the clean
 * calls with XPIC_POISSON_DIRECT, phi from 0, the stopping rule |r|_2 <= tol -> phi, the count of applications and the last
 * explicitly formed |r|_2.  The hook that pins the second and later applications (the += epilogue, the residual between
 * them, the "did not halve" exit): not converging is no error here, since the caller asked for a count -- tol = 0,
 * maxit = k gives exactly k applications while each one halves the residual it was given, and maxit = 1 returns
 * xpic_poisson_apply's bits.  xpic_poisson_apply's refusals; tol must be finite and >= 0, maxit >= 1.  Overwrites the
 * Gauss vectors; leaves the kind and xpic_gauss_info's counters as they were. */
#ifndef XPIC_POISSON_H
#define XPIC_POISSON_H
#define XPIC_POISSON_MAX_EXTENT 1024
enum xpic_poisson_solver { XPIC_POISSON_CG = 0, XPIC_POISSON_DIRECT = 1 };
#ifdef __cplusplus
extern "C" {
#endif
int xpic_set_poisson_solver(xpic_ctx* ctx, int kind);
int xpic_get_poisson_solver(xpic_ctx* ctx, int* kind);
int xpic_poisson_apply(xpic_ctx* ctx, const double* rhs_zyx, double* phi_zyx);
int xpic_poisson_solve(xpic_ctx* ctx, const double* rhs_zyx, double tol, int maxit, double* phi_zyx, int* applications,
                       double* rnorm);
#ifdef __cplusplus
}
#endif
#endif
