/*
 * xpic_hip.h -- C ABI of the MI355X (gfx950) implementation of xpic's per-timestep hot path.
 *
 * The reference (vakurshakov/xpic) has no FFI: its hot path is reached through the C++ virtual
 * `interfaces::Simulation::timestep_implementation()` (src/interfaces/simulation.h:71-72) and the
 * public members of `interfaces::Simulation` / `interfaces::Particles`.  This header is the boundary a
 * `impls/` backend binds UNDERNEATH those classes: every entry point names the reference function it
 * replaces (file:line relative to the reference checkout).  INTEGRATION.md shows the subclass a
 * maintainer would add on the reference side.
 *
 * Conventions
 *   - every function returns 0 on success, non-zero on error (slots into `PetscCall`); the message
 *     of the last error of the calling thread is returned by xpic_last_error().
 *   - field vectors cross the boundary in the reference's DMDA layout: double[nz][ny][nx][3]
 *     (x fastest, 3 components interleaved; src/utils/vector3.h:233, src/utils/world.h:35-43).
 *   - particles cross the boundary as `struct Point` records: double[6] = {x,y,z,px,py,pz}
 *     (src/interfaces/point.h:7-35).  Inside, both are re-laid out.
 *   - pointers are HOST pointers unless the parameter is called `dptr` (device pointer).
 *   - all boundaries are periodic (every BASELINE config); anything else is rejected at create.
 */
#ifndef XPIC_HIP_H
#define XPIC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct xpic_ctx xpic_ctx;

/* Geometry: globals dx,dy,dz,dt,geom_n* (src/constants.h:10-28) + World (src/utils/world.h:11-61). */
typedef struct xpic_geometry {
  int32_t n[3];     /* global cells geom_nx, geom_ny, geom_nz */
  double d[3];      /* dx, dy, dz */
  double dt;
  int32_t periodic[3]; /* must be {1,1,1}: DM_BOUNDARY_PERIODIC */
  int32_t rank;     /* z-slab index of this context (DMDA da_processors_z) */
  int32_t nranks;   /* number of z-slabs */
  int32_t device;   /* HIP device ordinal */
  int32_t self_ring; /* nranks == 1 only: keep the ghost planes and run the exchange layer with the slab as its own
                        lower and upper neighbour (exercises the RCCL transport on one GPU); 0 in production */
} xpic_geometry;

/* SortParameters (src/interfaces/sort_parameters.h:7-19) */
typedef struct xpic_sort_params {
  int32_t Np;
  double n, q, m;
} xpic_sort_params;

/* named global vectors of interfaces::Simulation / ecsim::Simulation / ecsimcorr::Simulation
 * (src/interfaces/simulation.h:33-48, src/impls/ecsim/simulation.h:27-28, ecsimcorr/simulation.h:17-18) */
enum xpic_field {
  XPIC_E = 0, XPIC_B = 1, XPIC_B0 = 2, XPIC_J = 3, XPIC_EP = 4, XPIC_EC = 5, XPIC_CURRI = 6,
  XPIC_CURRJE = 7, XPIC_W0 = 8, XPIC_W1 = 9, XPIC_W2 = 10, XPIC_NFIELDS = 11
};

enum xpic_scheme { XPIC_BASIC = 0, XPIC_ECSIM = 1, XPIC_ECSIMCORR = 2, XPIC_ES = 3 /* electrostatic: xpic_es.h */ };

/* operator / method selector of xpic_solve */
enum xpic_solve_op {
  XPIC_OP_MATA_GMRES = 0, /* (matL + matM) x = b, GMRES(30): KSP "predict" (ecsim/simulation.cpp:197-201,266) */
  XPIC_OP_MATM_GMRES = 1, /* matM x = b, GMRES(30): KSP "correct" (ecsimcorr/simulation.cpp:133) */
  XPIC_OP_MATM_CG = 2     /* matM x = b, CG (matM is SPD on periodic boundaries) */
};

#define XPIC_LSTENCIL 123 /* couplings per matL row: 27 same-component + 48 + 48 */

const char* xpic_last_error(void);
/* XPIC_VERSION, with XPIC_VERSION_EXPERIMENT_BIT set when any object of the library was built with -DXPIC_EXPERIMENT
 * (ablation switches and in-kernel timers of the kernels; some produce wrong physics by design): refuse such a library
 * for production runs. */
#define XPIC_VERSION 7
#define XPIC_VERSION_EXPERIMENT_BIT 0x40000000
int xpic_version(void);

/* World::initialize + Simulation::initialize_implementation (world.cpp:11-48; ecsim/simulation.cpp:122-143,
 * 517-567; basic/simulation.cpp:8-28): allocates E,B,B0,J,(Ep,Ec,currI,currJe), operators and solver state. */
int xpic_create(const xpic_geometry* geom, int scheme, xpic_ctx** out);
int xpic_destroy(xpic_ctx* ctx); /* Simulation::finalize (ecsim/simulation.cpp:569-590) */
int xpic_synchronize(xpic_ctx* ctx);

/* init_particles -> PartSpec(sim, SortParameters) (src/interfaces/simulation.tpp:43); capacity in particles */
int xpic_add_sort(xpic_ctx* ctx, const xpic_sort_params* p, int64_t capacity, int* sort_out);
/* Particles::add_particle (src/interfaces/particles.cpp:47-67) for n Points: binned by FLOOR_STEP, points
 * outside the local box are dropped; *added = number kept. Appends to what the sort already holds. */
int xpic_sort_add_particles(xpic_ctx* ctx, int sort, int64_t n, const double* points6, int64_t* added);
int xpic_sort_count(xpic_ctx* ctx, int sort, int64_t* count);
/* storage read-back in cell order: points6[count][6], cell_of[count] = local cell index g (world.s_g) */
int xpic_sort_get_particles(xpic_ctx* ctx, int sort, double* points6, int32_t* cell_of);
int xpic_sort_clear(xpic_ctx* ctx, int sort);
/* synthetic plasma generated on the device (bench/smoke only): ppc * (local cells) particles, Maxwellian velocities of
 * thermal spread vth (then v /= sqrt(1+v^2), "tov").  regular == 0: positions uniform over the slab, i.e. Poisson
 * occupancy of the cells, the load CoordinateInBox + SetParticles produce (src/utils/particles_load.cpp:11-18,
 * src/commands/set_particles.cpp:19-43; the device RNG is its own, not mt19937); regular != 0: exactly ppc particles
 * in every cell.  Collective over the z-slabs like xpic_update_cells. */
int xpic_sort_fill_synthetic(xpic_ctx* ctx, int sort, int ppc, double vth, uint64_t seed, int regular);
/* The same with a drift and a density profile.  drift = SortParameters::px, py, pz as MaxwellianMomentum adds them
 * (src/utils/particles_load.cpp:57-76: to the thermal momentum, before `tov`; in units of m c with m = 1).  The
 * reference's JSON surface never reads px / py / pz (src/interfaces/simulation.tpp:24-41), so a drifting Maxwellian -- the
 * two counter-streaming beams of BASELINE configs[1] -- is an EXTENSION of this build's loaders, not reference behaviour.
 * profile: XPIC_LOAD_UNIFORM / XPIC_LOAD_REGULAR as above; XPIC_LOAD_GRADIENT: density falling linearly along x from
 * profile_param[0] : 1 at x = 0 to 1 at x = Lx (same particle total); XPIC_LOAD_BLOB: the fraction profile_param[0] of
 * the particles in a Gaussian clump of sigma = profile_param[1] cells at the centre of the slab, the rest uniform (cells
 * of many times the mean occupancy: the bucket / third-pass / colour-balance fall-backs of the particle kernels). */
#define XPIC_LOAD_UNIFORM 0
#define XPIC_LOAD_REGULAR 1
#define XPIC_LOAD_GRADIENT 2
#define XPIC_LOAD_BLOB 3
typedef struct xpic_load_params {
  int32_t ppc;
  int32_t profile;
  double vth;
  double drift[3];
  double profile_param[4];
  uint64_t seed;
} xpic_load_params;
int xpic_sort_load_synthetic(xpic_ctx* ctx, int sort, const xpic_load_params* params);
/* Occupancy of the local cells (`storage[g].size()`, src/interfaces/particles.h:32, any distribution): out8 = {largest
 * cell, cells of more than 64 particles (a second staging pass in the assembly), of more than 128 (a third), of more than
 * a bucket of the deferred scatter holds (the step then takes the index pass), largest and smallest population of an
 * x-pencil (one workgroup each in the particle kernels: the balance of a colour launch), empty cells, bucket capacity}. */
int xpic_sort_occupancy(xpic_ctx* ctx, int sort, int64_t* out8);

/* Vec access (DMDAVecGetArray / VecGetArray): copies in/out in the [z][y][x][3] layout, local slab */
int xpic_field_set(xpic_ctx* ctx, int field, const double* v);
int xpic_field_get(xpic_ctx* ctx, int field, double* v);
int xpic_sort_current_get(xpic_ctx* ctx, int sort, int which /* XPIC_J | XPIC_CURRI | XPIC_CURRJE */, double* v);

/* ---- BLAS-1 on named vectors (VecSet/VecAXPY/VecAXPBY/VecDot/VecNorm; K14) */
int xpic_vec_set(xpic_ctx* ctx, int y, double alpha);
int xpic_vec_axpy(xpic_ctx* ctx, int y, double alpha, int x);                 /* y += alpha x */
int xpic_vec_axpby(xpic_ctx* ctx, int y, double alpha, double beta, int x);  /* y = alpha x + beta y */
int xpic_vec_dot(xpic_ctx* ctx, int x, int y, double* out);
int xpic_vec_norm2(xpic_ctx* ctx, int x, double* out);

/* ---- operators (K11-K13) on named vectors; `add` != 0 gives MatMultAdd (y += ...) */
/* Rotor (src/utils/operators.cpp:155-215): y (+)= alpha * rot(sign) x; sign +1 = rotE, -1 = rotB */
int xpic_rot_apply(xpic_ctx* ctx, int sign, double alpha, int x, int y, int add);
/* matM = 2 I + 0.5 dt^2 rotB rotE (src/impls/ecsim/simulation.cpp:544-551) */
int xpic_matM_apply(xpic_ctx* ctx, int x, int y, int add);
/* matL as filled by xpic_ecsim_fill_current (MatMultAdd(matL,...) ecsimcorr/simulation.cpp:78) */
int xpic_matL_apply(xpic_ctx* ctx, int x, int y, int add);
/* matA = matL + matM (ecsim/simulation.cpp:197-198) */
int xpic_matA_apply(xpic_ctx* ctx, int x, int y);
/* matL read-back as double[3N][XPIC_LSTENCIL], row = ((z*ny+y)*nx+x)*3+c, k as xpic_lstencil_decode */
int xpic_matL_get(xpic_ctx* ctx, double* out);
void xpic_lstencil_decode(int c1, int k, int* c2, int* d3);

/* ---- per-phase entry points */
/* ecsim::Particles::first_push (src/impls/ecsim/particles.cpp:21-31): r += dt*p */
int xpic_ecsim_first_push(xpic_ctx* ctx, int sort);
/* Particles::update_cells_seq / correct_coordinates (src/interfaces/particles.cpp:79-116,329-339):
 * periodic wrap, re-bin by FLOOR_STEP, drop what falls outside; *count = particles left */
int xpic_update_cells(xpic_ctx* ctx, int sort, int64_t* count);
/* ecsim::Simulation::fill_ecsim_current + Particles::fill_ecsim_current/decompose_ecsim_current
 * (src/impls/ecsim/simulation.cpp:336-368,471-484; particles.cpp:33-173): zeroes then fills currI
 * (per sort and total) and matL from all sorts, gathering B */
int xpic_ecsim_fill_current(xpic_ctx* ctx);
/* ecsim::Particles::second_push (src/impls/ecsim/particles.cpp:175-192): CIC gather of Ep and B, update_vEB(dt) */
int xpic_ecsim_second_push(xpic_ctx* ctx, int sort);
/* basic::Particles::push (src/impls/basic/particles.cpp:17-53): half move, 2nd-order gather, Boris, half move,
 * Esirkepov into the sort's J and the simulation's J */
int xpic_basic_push(xpic_ctx* ctx, int sort);
/* ecsimcorr::Particles::{first_push, second_push, final_update, calculate_energy}
 * (src/impls/ecsimcorr/particles.cpp:27-50, 52-91, 93-126, 134-150) */
int xpic_ecsimcorr_first_push(xpic_ctx* ctx, int sort);
int xpic_ecsimcorr_second_push(xpic_ctx* ctx, int sort);
int xpic_ecsimcorr_final_update(xpic_ctx* ctx, int sort);
int xpic_calculate_energy(xpic_ctx* ctx, int sort, double* energy);
/* pred_w, corr_w, lambda_dK, pred_dK, corr_dK, energy (ecsimcorr/particles.h:44-49) */
int xpic_ecsimcorr_scalars(xpic_ctx* ctx, int sort, double* out6);

/* KSPSolve (src/impls/ecsim/simulation.cpp:266): x0 = 0, preconditioner as set by xpic_set_preconditioner (both GMRES
 * operators; CG is unpreconditioned), converged when the residual ||b - A x|| <= max(rtol ||b||, atol) (the cheap
 * preconditioned XPIC_OP_MATM_GMRES is run to 1e-2 of that).  The norm tested (and returned in *rnorm) is GMRES's
 * RECURRENCE value of the unpreconditioned residual -- right / flexible preconditioning keeps it the residual of A x = b
 * itself, not of a preconditioned system -- as in PETSc's KSPGMRES; no explicit b - A x is formed at exit (one more apply
 * per solve).  It equals the true residual up to the orthogonality of the basis: iterations whose entering residual is
 * above 1e-6 ||b|| take |w - sum h_i v_i| from w.w - sum h_i^2 (one reduction per iteration), later ones and every solve
 * with a tolerance below 1e-8 ||b|| take the norm explicitly (krylov.hip).  *iterations >= 0; *reason > 0 converged,
 * < 0 diverged (maxit).
 * A non-converged solve RETURNS NON-ZERO, like KSPSetErrorIfNotConverged (:562). */
int xpic_solve(xpic_ctx* ctx, int op, int rhs, int x, double rtol, double atol, int maxit, int* iterations,
  int* reason, double* rnorm);
/* KSPSetTolerances used by the step drivers (src/impls/ecsim/simulation.h:15-18: 1e-7,1e-7,100) */
int xpic_set_tolerances(xpic_ctx* ctx, double rtol, double atol, int maxit);

/* PCSetType for the "predict" and "correct" KSPs.  The reference runs PETSc's default ILU(0) (not part of its tree, not a GPU
 * algorithm); here: kind 0 = none, kind 1 / 2 = a fixed Chebyshev polynomial in matM applied from the right
 * (matM = 2 I + 0.5 dt^2 rotB rotE dominates matA and its spectral interval is known in closed form), its work vectors
 * kept in fp32 (kind 1) or fp64 (kind 2); kind 3 = the polynomial in matM + <matL>, the translation average of the assembled
 * mass matrix as one constant-coefficient 123-point stencil (fp32), for the predict solve (the correct solve on matM keeps
 * kind 1); kind 4 = kind 3 with the rows of <matL> scaled by the local density (the ratio of the row's own diagonal
 * entry of matL to the average's): three times the convergence rate per iteration at 64 particles per cell, at twice the
 * polynomial's cost (at the reference's tolerance both need 4 iterations on the uniform 256^3 box: kind 3 is the faster one
 * there; with the density falling 4 : 1 across the box kind 3 needs 6 and kind 4 four); kind 5 (default) = kind 3 or kind 4,
 * chosen per solve from the relative spread of matL's diagonal (above 0.2: kind 4; a uniform Poisson load of 64 per cell
 * has 0.1).  The GMRES around it is the flexible variant (x = x0 + sum y_j P v_j with the
 * P v_j stored): the result does not depend on how exactly P is applied, only the iteration count could.
 * degree <= 0 returns to the automatic choice.  The stopping rule of xpic_solve is unchanged (the residual of A x = b).
 * Kinds 3, 4 and 5 check their surrogate per solve: where 2 + the Gershgorin lower bound of <matL> (times the largest density
 * ratio) is positive the polynomial's interval is proven; otherwise the surrogate runs on probation -- an iteration that does
 * not halve the residual, or is not finite, ends it and the solve goes on with kind 1. */
int xpic_set_preconditioner(xpic_ctx* ctx, int kind, int degree);
/* Test hooks of the preconditioner (read-only: a solve after them returns the bits it returned before).
 * xpic_precond_apply: out = P r, as the next xpic_solve(ctx, op, ...) would apply P to a Krylov vector: the same choice
 * between the polynomial in matM and the one in matM + <matL>, the same degree (XPIC_OP_MATM_GMRES: the "correct" solve's),
 * the surrogate rebuilt first where a solve rebuilds it (and, as there, dropped for the matM polynomial where it is not
 * finite).  No probation runs.  r and out are distinct vectors (r's ghost planes are refreshed on z-slabs); collective over
 * the z-slabs.  Kind 0 and XPIC_OP_MATM_CG have no P: an error.
 * xpic_precond_get: the surrogate as the last build left it (a solve or xpic_precond_apply with kind >= 3 on
 * XPIC_OP_MATA_GMRES).  info[XPIC_PRECOND_NINFO] = {interval bottom, interval top, 2 + Gershgorin bound of <matL>, degree
 * of the next apply on XPIC_OP_MATA_GMRES, rows scaled (0 / 1), interval proven, surrogate valid, largest density ratio
 * (1 where the rows are not scaled), relative variance <d^2> / <d>^2 - 1 of matL's diagonal per component (kind 5 only; the
 * other kinds do not sum d^2)}.  abar (or NULL): double[3][XPIC_LSTENCIL + 1], matM + <matL> in xpic_lstencil_decode's
 * order, all taps (slot XPIC_LSTENCIL: <d^2>).  rscale (or NULL): the density ratios of the rows, widened to double, in
 * xpic_field_get's layout over the local slab; meaningful only where info[4] is set. */
#define XPIC_PRECOND_NINFO 11
int xpic_precond_apply(xpic_ctx* ctx, int op, int r, int out);
int xpic_precond_get(xpic_ctx* ctx, double* info, double* abar, double* rscale);
/* The mass-matrix assembly (fill_ecsim_current) has two bodies: kind 0 (default) the classic 4-wave kernel (all grids);
 * kind 1 the warp-specialised kernel (one 16-wave workgroup per CU: a producer wave per SIMD runs the per-particle algebra,
 * two consumer waves the matrix-core accumulation, a flusher the window's read-modify-write), available where nx is a
 * multiple of 4 and no extent is below 3, measured slower.  Same matrix up to the summation order of a
 * cell's neighbours.  xpic_get_fill_variant: out3 = {power-of-two spacings, full-chunk body, warp-specialised body} as the
 * next assembly of this context will run. */
int xpic_set_fill_kernel(xpic_ctx* ctx, int kind);
/* update_cells (src/interfaces/particles.cpp:79-116) re-bins the particles in two passes (keys, then an out-of-place
 * scatter).  on = 1 (default) leaves the scatter to the next kernel that reads every particle anyway: in the ecsim step
 * (ecsim/simulation.cpp:174-189) and for the first re-binning of the ecsimcorr step that is the mass-matrix assembly, in the
 * basic step (basic/simulation.cpp:45-72) the next step's push; it gathers the records through source indices, applies the
 * move and the periodic wrap and writes the sorted copy on its way.  on = 2 (ecsim): the assembly only reads through the
 * index and second_push -- which is bound by memory anyway -- writes the sorted copy with the new velocities.  Same
 * particles, same cells, same arithmetic as on = 0 (scatter first); any other reader of a sort (diagnostics, downloads,
 * the phase entry points) resolves a pending deferral by the plain scatter.  On z-slabs the assembly's form is used as well
 * (records received from the neighbours are gathered out of the receive buffer); the basic step and on = 2 defer on a single
 * slab only. */
int xpic_set_fused_rebin(xpic_ctx* ctx, int on);
int xpic_get_fill_variant(xpic_ctx* ctx, int* out3);
/* Test hooks for two size limits of the gathering assembly that no test-sized box reaches on its own (results are the same
 * for every value; only the code path changes).  XPIC_DEBUG_GATHER_WINDOW: old-order records within `value` slots of an
 * x-pencil's first slot are fetched by 32-bit offsets, the others -- at 256^3 x 64 what crossed the periodic z boundary --
 * by 64-bit addresses (default and maximum 2^28).  XPIC_DEBUG_PENCIL_LIMIT: a sort with an x-pencil of `value` particles or
 * more scatters first instead of deferring (default and maximum 2^29, the reach of the sorted copy's 32-bit offsets). */
#define XPIC_DEBUG_GATHER_WINDOW 0
#define XPIC_DEBUG_PENCIL_LIMIT 1
/* XPIC_DEBUG_SURROGATE_SCALE: the preconditioner's surrogate is built from `value` / 1000 times <matL> (1000 = as it is): a
 * deliberately wrong surrogate, to see the probation of an unproven one end in the fall-back (results are unchanged: the
 * stopping rule is the true residual). */
#define XPIC_DEBUG_SURROGATE_SCALE 2
int xpic_debug_set(xpic_ctx* ctx, int what, int64_t value);
/* MatMult on a z-slab with neighbours: on = 1 posts the ghost exchange of the operand (VecScatterBegin), applies
 * the rows of the interior planes meanwhile and the rows of the boundary planes after it (VecScatterEnd), as PETSc's
 * MPIAIJ MatMult does (the reference's KSPSolve, src/impls/ecsim/simulation.cpp:266); on = 0 exchanges first. Same result.
 * Bit 1 of `on` (on = 3) also posts the assembly's ghost-row exchange of matL behind the boundary colours, beside the
 * interior colour launches (off by default: measured slower).
 * Default: 0 -- on the one-GPU self-ring (the only hardware these paths have run on) both overlaps cost more than the
 * exchanges they hide, and over RCCL with more than one rank the second-stream path has not yet run
 * on two distinct GPUs.  XPIC_RCCL_OVERLAP=1 turns bit 0 on at xpic_comm_init_rccl.
 * bit 2: the matL ghost rows by copy engine (see xpic_comm_peer_import below). */
int xpic_set_overlap(xpic_ctx* ctx, int on);

/* timestep_implementation of the context's scheme (basic/simulation.cpp:30-43, ecsim/simulation.cpp:145-155,
 * ecsimcorr/simulation.cpp:21-32); *ksp_iterations = Krylov iterations spent in this step */
int xpic_step(xpic_ctx* ctx, int* ksp_iterations);

/* Energy::calculate_field/calculate_kinetic (src/diagnostics/energy.cpp:43-108):
 * out = {wE, wB, sE, sB, wK_0, sK_0, wK_1, sK_1, ...} */
int xpic_energy(xpic_ctx* ctx, double* out);

/* MomentumConservation::calculate (src/diagnostics/momentum_conservation.cpp:77-131): per sort
 * out[6 i ..] = {Px, Py, Pz, QEx, QEy, QEz}, P = sum (m/Np) v ns and QE = sum (q/Np) E Es over the particle's
 * 2nd-order shape nodes */
int xpic_momentum(xpic_ctx* ctx, double* out);

/* ParticlesChargeDensity::collect of one sort (src/diagnostics/charge_conservation.cpp:67-97) -> rho[z][y][x] */
int xpic_charge_density(xpic_ctx* ctx, int sort, double* rho_zyx);
/* DistributionMoment::collect with moment "density" (src/diagnostics/distribution_moment.cpp:125-216): cell-centred
 * first-order deposit of n/Np -> out[z][y][x].  Uses the scratch vector XPIC_W2. */
int xpic_moment_density(xpic_ctx* ctx, int sort, double* out_zyx);
/* DistributionMoment::collect of one sort with any of its six moments (src/diagnostics/distribution_moment.cpp:157-298,
 * builder builders/distribution_moment_builder.cpp:16-23): cell-centred first-order deposit of moment(p) * n/Np from
 * round(r/d - 1) over 2 x 2 x 2 cells.  region6 = {start x, y, z, size x, y, z} in global cells (NULL: the whole box).  The
 * reference's region rule (:59-108, :157-210): a particle counts iff its storage cell lies in the region; a deposit lands
 * iff its cell lies in the region, after a periodic wrap on each axis the region spans in full.  out[nzl][ny][nx][dof]
 * over the local slab (the reference's DOF layout), zero outside the region; dof = 1, 3, 6, 3, 6, 3 in the order of
 * enum xpic_moment_kind.  Collective over the z-slabs (ghost-plane deposits go to their owner).  Uses the scratch vector
 * XPIC_W2, and XPIC_W1 as well for the 6-component moments. */
enum xpic_moment_kind {
  XPIC_MOMENT_DENSITY = 0,            /* get_density (:212-216), dof 1 */
  XPIC_MOMENT_CURRENT = 1,            /* get_current (:218-224): q v, dof 3 */
  XPIC_MOMENT_MOMENTUM_FLUX = 2,      /* get_momentum_flux (:226-239): m v_i v_j, i <= j, dof 6 */
  XPIC_MOMENT_MOMENTUM_FLUX_DIAG = 3, /* get_momentum_flux_diag (:241-251): m v_i v_i, dof 3 */
  XPIC_MOMENT_MOMENTUM_FLUX_CYL = 4,  /* get_momentum_flux_cyl (:279-292): (r, phi, z) about (geom_x/2, geom_y/2), dof 6 */
  XPIC_MOMENT_MOMENTUM_FLUX_DIAG_CYL = 5 /* get_momentum_flux_diag_cyl (:294-304), dof 3 */
};
int xpic_moment(xpic_ctx* ctx, int sort, int kind, const int region6[6], double* out);
/* VelocityDistribution::collect (src/diagnostics/velocity_distribution.cpp:112-163; builder
 * builders/velocity_distribution_builder.cpp:13-115): a cell counts iff it lies in the geometry's AABB (FLOOR_STEP of the
 * bounds) and its centre (g + 0.5) d passes WithinBox / WithinCylinder (src/utils/geometries.cpp:3-19); each of its
 * particles adds n/Np to bin (ROUND_STEP(v1, dvx), ROUND_STEP(v2, dvy)) (std::round: half away from zero), bins outside the
 * histogram are dropped.  geom = {min x, y, z, max x, y, z} (box) or {center x, y, z, radius, height} (cylinder);
 * vreg = {vx_min, vy_min, vx_max, vy_max, dvx, dvy}.  As the reference's set_regions (:57-68) WRITES it, both axes start
 * at ROUND_STEP(vx_min, dvx) and have ROUND_STEP(vx_max - vx_min, dvx) bins: vy_min, vy_max never enter (dvy does, as the
 * bin width of v2).  vgrid4 = {vsize_x, vsize_y, vstart_x, vstart_y}: column i of out holds the bin vstart_x + i (vstart
 * = ROUND_STEP(vx_min, dvx), half away from zero); out[vsize_y][vsize_x] (NULL: the sizes and starts only), the whole
 * histogram on every z-slab (collective: the VecScatter ADD, :159-160).  At most 2^15 bins per axis.  Uses the scratch
 * vector XPIC_W0; a histogram of more bins than a field vector holds (a fine histogram on a small grid) takes a device
 * buffer of its own for the call. */
enum xpic_projector {
  XPIC_PROJ_VX_VY = 0,  /* get_vx_vy (:166-169) */
  XPIC_PROJ_VZ_VXY = 1, /* get_vz_vxy (:171-175): (vz, |(vx, vy)|) */
  XPIC_PROJ_VR_VPHI = 2 /* get_vr_vphi (:177-193): about (geom_x/2, geom_y/2) */
};
enum xpic_vgeometry { XPIC_GEOM_BOX = 0, XPIC_GEOM_CYLINDER = 1 };
int xpic_velocity_distribution(xpic_ctx* ctx, int sort, int projector, int geometry, const double geom[7],
  const double vreg[6], int* vgrid4, double* out);
/* ---- the per-step commands of an open system (src/commands/).  geometry / geom as in xpic_velocity_distribution.  Every
 * call is collective over the z-slabs: the counts and energies it returns are summed over them. */
/* RemoveParticles::execute (src/commands/remove_particles.cpp:11-40): every local cell whose CORNER (start + g) d fails
 * WithinBox (half-open) / WithinCylinder (strict |z - center z| < height / 2) (src/utils/geometries.cpp:3-19) is emptied
 * (VelocityDistribution tests the cell centre instead).  *removed = records removed, *energy = sum of 0.5 m v^2 n/Np over
 * them (Energy::get_kinetic, src/diagnostics/energy.cpp:188-191).  The other cells keep their records in their order; when
 * no failing cell holds a record, no record is touched. */
int xpic_remove_particles(xpic_ctx* ctx, int sort, int geometry, const double geom[7], int64_t* removed, double* energy);
/* FieldsDamping::execute (src/commands/fields_damping.cpp:15-111): on E and on B - B0 (B0 added back), every node whose
 * point (x + 0.5, y + 0.5, z + 0.5) d -- the cell centre, for all three components -- lies outside the geometry is scaled
 * by DampForBox / DampForCylinder (:71-111) as written; *energy = sum of 0.5 |f|^2 (1 - damping^2) over both fields (no
 * cell volume, as Energy::get_field).  As written, the box's factor on the lower side is 1 - c at the wall and 1 at the
 * interface, on the upper side 1 - c at the interface and 1 at the wall; the cylinder's width is center x - radius and
 * its factor is 0 from delta0 = width (1 + 1/sqrt(c)) outwards. */
int xpic_fields_damping(xpic_ctx* ctx, int E, int B, int B0, int geometry, const double geom[7], double coefficient,
  double* energy);
/* InjectParticles::execute (src/commands/inject_particles.cpp:26-63) for `pairs` pairs: each draws one coordinate
 * (PreciseCoordinate / CoordinateInBox / CoordinateInCylinder, src/utils/particles_load.cpp:6-30), then the momentum of
 * the ionized and then of the ejected sort (PreciseMomentum / MaxwellianMomentum with `tov`, :46-76; T in the reference's
 * keV, mec2 = 511).  The draws come from a counter-based stream keyed by (seed, step, pair): this build's own RNG, not the
 * reference's mt19937, and every z-slab draws the same pairs and keeps those in its planes.  A pair is added to both sorts
 * iff its coordinate lies in the local box (Particles::add_particle, src/interfaces/particles.cpp:47-67); new records
 * follow the old ones of their cell.  *added = pairs added, energy2 = kinetic energy added to the ionized, the ejected
 * sort.  The two sorts must differ.  More records than a sort's capacity fail with an error on every slab, before any
 * sort is changed. */
enum xpic_coordinate_kind {
  XPIC_COORD_PRECISE = 0, XPIC_COORD_IN_BOX = 1, XPIC_COORD_IN_CYLINDER = 2,
  XPIC_COORD_ON_ANNULUS = 3 /* xpic_set_particles only */
};
enum xpic_momentum_kind {
  XPIC_MOMENTUM_PRECISE = 0, XPIC_MOMENTUM_MAXWELLIAN = 1,
  XPIC_MOMENTUM_COSINE_PERTURBATION = 2, XPIC_MOMENTUM_ANGULAR = 3 /* xpic_set_particles only */
};
typedef struct xpic_momentum_params {
  int32_t kind;     /* enum xpic_momentum_kind */
  int32_t tov;      /* MaxwellianMomentum: p /= sqrt(m^2 + p^2) */
  double value[3];  /* PreciseMomentum: the value; MaxwellianMomentum: the drift px, py, pz (SortParameters) */
  double T[3];      /* MaxwellianMomentum: Tx, Ty, Tz (SortParameters) */
} xpic_momentum_params;
typedef struct xpic_inject_params {
  int32_t coordinate; /* enum xpic_coordinate_kind */
  int32_t reserved;
  double geom[7];     /* the point (precise), {min xyz, max xyz} (box), {center xyz, radius, height} (cylinder) */
  xpic_momentum_params momentum[2]; /* ionized, ejected */
  uint64_t seed;
} xpic_inject_params;
int xpic_inject_particles(xpic_ctx* ctx, int ionized, int ejected, const xpic_inject_params* params, int64_t pairs,
  int64_t step, int64_t* added, double energy2[2]);
/* The parameters of xpic_set_particles (include/xpic_set_particles.h, where the command is defined). */
#define XPIC_SET_PARTICLES_CHUNK 16777216 /* particles per internal chunk when `chunk` is 0 */
typedef struct xpic_set_particles_params {
  int32_t coordinate;    /* enum xpic_coordinate_kind */
  int32_t momentum;      /* enum xpic_momentum_kind */
  int32_t tov;           /* MaxwellianMomentum: p /= sqrt(m^2 + p^2) */
  int32_t reserved;
  double geom[7];        /* the point (precise), {min xyz, max xyz} (box), {center xyz, radius, height} (cylinder),
                            {center xyz, inner_r, outer_r, height} (annulus) */
  double value[3];       /* PreciseMomentum: the value; Maxwellian, angular: px, py, pz of SortParameters */
  double T[3];           /* Tx, Ty, Tz of SortParameters (all generators but the precise one) */
  double amplitude[3];   /* MaxwellCosinePerturbation: a */
  double wave_number[3]; /* MaxwellCosinePerturbation: m */
  double box6[6];        /* MaxwellCosinePerturbation: its box {min xyz, max xyz}; only the extents enter */
  double center[3];      /* AngularMomentum: the axis (its z is not read) */
  uint64_t seed;
  int64_t chunk;         /* particles per internal chunk; 0: XPIC_SET_PARTICLES_CHUNK */
} xpic_set_particles_params;
/* Binary Coulomb collisions between the records of one cell (Takizuka and Abe, J. Comput. Phys. 25, 205, 1977),
 * non-relativistic.  AN EXTENSION: the reference has no collision operator, so no file:line of it is cited here.
 * A call collides sort_a with sort_b (the same sort: intra-species) inside every local cell, independently of every other
 * cell; positions and the order of the records are never touched.  The two sorts must carry the same weight n / Np.
 * Per cell: Na, Nb from cell_start; n_L = (n / Np) min(Na, Nb).  One stream key per (seed, step, sort_a, sort_b, GLOBAL
 * cell ((z0 + cz) ny + cy) nx + cx) -- z-slabs and the single box draw the same numbers -- with sub-streams for the
 * permutation of a, of b, and the draws of pair p.  Record i of the cell gets a 64-bit key; the permutation pi orders the
 * records by (key, i).  Intra-species pairs: (pi0, pi1), (pi2, pi3), ... (p = 0, 1, ...); an odd N >= 3 starts with
 * (pi0, pi1), (pi1, pi2), (pi2, pi0), one after the other with dt / 2 each (p = 0, 1, 2), then (pi3, pi4), ... (p = 3, ...);
 * N < 2: nothing.  Inter-species: the sort with fewer records in the cell is the short side (equal counts: sort_b); record
 * pi_long[j] meets pi_short[j mod N_short], p = j, the meetings of one short record in increasing j; an empty side: nothing.
 * One collision of a-record and b-record (the call's order; intra-species: first and second of the pair):
 * u = v_a - v_b, m_ab = m_a m_b / (m_a + m_b), sigma^2 = strength q_a^2 q_b^2 n_L dt / (m_ab^2 |u|^3);
 * delta = sigma sqrt(-2 ln u1) cos(2 pi u2), Phi = 2 pi u3; sin Theta = 2 delta / (1 + delta^2),
 * 1 - cos Theta = 2 delta^2 / (1 + delta^2); the relative velocity is rotated by (Theta, Phi) (Takizuka-Abe's eq. 4a-4c;
 * for u_perp == 0: du = (u sin Theta cos Phi, u sin Theta sin Phi, -u_z (1 - cos Theta))), v_a += (m_ab / m_a) du,
 * v_b -= (m_ab / m_b) du.  A pair with |u| == 0 is skipped and counted.  Momentum and energy of every pair are conserved.
 * strength: in the reference's units (velocities in c, time in 1 / w_pe, densities in n0) it is ln Lambda / (8 pi) times the
 * inverse number of particles in a skin-depth cube, 1 / (n0 (c / w_pe)^3).
 * out4 = {pairs collided, pairs skipped (|u| == 0), sum of sigma^2 over the collided pairs, pairs with sigma^2 > 1}, summed
 * over the z-slabs (the call is collective): the mean sigma^2 and the count above 1 say whether the small-angle step is
 * resolved.  Works for all three schemes (it reads nothing but the sorts).  Argument errors (a bad sort, unequal weights, a
 * null pointer, a negative strength) are refused on every slab before anything changes.  A pair so slow that sigma^2 or
 * delta^2 exceeds 1e300 (or overflows) scatters by Theta = pi (the limit: sin Theta = 0, 1 - cos Theta = 2); an overflowed sigma^2
 * is counted above 1 and left out of the sum.  Cells of more than XPIC_COLLIDE_LDS_CELL records of a sort take a second
 * path that uses the sort's binning scratch.
 * xpic_collide_info: out2 = {XPIC_COLLIDE_LDS_CELL as the library was built, the LOCAL cells of the context's last
 * xpic_collide that took the second path (not summed over the slabs)}. */
#define XPIC_COLLIDE_LDS_CELL 256
typedef struct xpic_collision_params {
  double strength;   /* S above; 0: the call changes nothing, bit for bit */
  double dt;         /* collision time step; <= 0: the context's dt */
  uint64_t seed;
} xpic_collision_params;
int xpic_collide(xpic_ctx* ctx, int sort_a, int sort_b, const xpic_collision_params* p, int64_t step, double out4[4]);
int xpic_collide_info(xpic_ctx* ctx, int64_t out2[2]);
/* Binary collisions between two sorts of UNEQUAL weight (Nanbu and Yonemura, J. Comput. Phys. 145, 639, 1998; the density
 * factor for repeated meetings after Higginson et al., J. Comput. Phys. 413, 109450, 2020).  AN EXTENSION, as xpic_collide
 * is.  Everything xpic_collide's comment says holds, except the following.
 * Weights: w_a = n_a / Np_a and w_b = n_b / Np_b may differ; both must be finite and positive.  w_max = max(w_a, w_b) and
 * r = min(w_a, w_b) / w_max are formed once on the host in fp64 and passed to the kernel; r is never recomputed on the device.
 * Density factor: n_L = w_max N_short.  (With a the lighter-weighted sort: an a-record is always updated and must see
 * n_b = w_b N_b over a step; a b-record is updated with probability w_a / w_b per meeting and must see n_a = w_a N_a.  The
 * long side's record j meets the short side's j mod N_short, so a short record has N_long / N_short meetings: both
 * conditions give n_L = w_b N_short, whichever side is long.)  At w_a == w_b this is (n / Np) min(N_a, N_b), xpic_collide's
 * factor, formed by the same operations in the same order.
 * Pairing and streams: xpic_collide's, the call key of (seed, step, sort_a, sort_b) included.  A fourth draw u4 is taken
 * from the pair's stream state after u3; a skipped pair (|u| == 0) draws nothing.
 * Update: the collision is evaluated as written; the lighter-weighted record takes its new velocity; the heavier-weighted
 * record takes its new velocity iff u4 < r, otherwise its three components keep their bits (r == 1: both are updated at
 * every meeting, u4 < 1 always; equal weights: sort_b counts as the heavier side).  A rejected update still counts as a
 * collision made and its sigma^2 is tallied.  When the heavier-weighted side is the short side, each meeting of its record
 * sees the velocity the meetings before it left, updated or not.
 * sort_a == sort_b forwards to xpic_collide's path and gives its bits.  Two different sorts of equal weight: the records
 * and out6[0..3] equal xpic_collide's bit for bit.
 * out6 = xpic_collide's out4, the heavier-side updates made, the heavier-side updates rejected; all six summed over the
 * z-slabs.  Equal weights (and sort_a == sort_b): out6[4] == out6[0], out6[5] == 0.
 * Refused on every slab before anything changes: a bad sort, a null pointer, a negative or non-finite strength, a sort
 * without mass, Np or positive n.  strength == 0 launches nothing.  xpic_collide_info also reports this call's
 * second-path cells.
 * Momentum and energy are conserved in expectation only (w_a . 1 . dp - w_b (w_a / w_b) dp = 0 for a pair); a single
 * pair does not conserve them, and there is no per-cell repair step. */
int xpic_collide_weighted(xpic_ctx* ctx, int sort_a, int sort_b, const xpic_collision_params* p, int64_t step,
  double out6[6]);
/* SetCoilsField::operator() (src/commands/set_magnetic_field.cpp:38-150): field += the field of the coils {z0, R, I}
 * (coils3[3 i ..]) about the axis (geom_x / 2, geom_y / 2), by the reference's 2000-point quadrature with its
 * denominator_tolerance, at the positions it writes: Bx at (x, y + 1/2, z + 1/2) d, By at (x + 1/2, y, z + 1/2) d,
 * Bz at (x + 1/2, y + 1/2, z) d.  A Bx or By node on the axis (r = 0) is 0 / 0 there as in the reference: NaN. */
int xpic_set_coils_field(xpic_ctx* ctx, int field, int ncoils, const double* coils3);
/* SetApproximateMirrorField::operator() (src/commands/set_magnetic_field.cpp:142-191) as written: field += the paraxial
 * field of two coils of radius R and current I at z = -D / 2 and z = +D / 2, with B0(z, s) = I R^2 / 2 /
 * (R^2 + (z + s D / 2)^2)^1.5 and B1(z, s) = (z + s D / 2) / (R^2 + (z + s D / 2)^2) for s = +1, -1.  The X component
 * takes BOTH transverse terms, B0 B1 1.5 (x dx - geom_x / 2) and B0 B1 1.5 (y dy - geom_y / 2), at (z + 1/2) dz; the Y
 * component takes nothing; the Z component takes B0 at z dz.  (The reference's JSON builder does not offer this setter,
 * set_magnetic_field_builder.cpp:13-17; neither does the host executable.) */
int xpic_set_mirror_field(xpic_ctx* ctx, int field, double D, double R, double I);
/* ChargeConservation (charge_conservation.cpp:117-171): xpic_charge_collect() = initialize(); then once per step
 * xpic_charge_columns(): out = {N1dQ_0, N2dQ_0, ..., N1dQ_tot, N2dQ_tot} of (rho_new - rho_old)/dt + div(-) J.
 * Uses the scratch vectors XPIC_W0..W2. */
int xpic_charge_collect(xpic_ctx* ctx);
int xpic_charge_columns(xpic_ctx* ctx, double* out);

/* ---- inner kernels of the `eccapfim` scheme, batch form over n path segments r0 -> rn (host arrays,
 * 3 doubles per point).  The scheme's outer loops are not part of this library.
 * cell_traversal (src/impls/eccapfim/cell_traversal.cpp:3-77): for every segment the points start, face crossings of the
 * node-centred cells, end -> pts[(q * max_pts + i) * 3 ..], counts[q] (may exceed max_pts: then the tail is dropped and
 * counts[q] is still the full count; pts behind the points of a segment is zero).  The points are the reference's bit for
 * bit (the kernel is compiled without contraction).  A guard the reference does not have: after 64 crossings the walk
 * stops and the end is appended, so counts[q] <= 66, and counts[q] == 66 marks a walk cut short.  That is a move of more
 * than 64 crossings, or one of the exact ties on which the reference's ladder (z before y before x) steps an axis whose
 * end coordinate lies on a face and rounds back into its cell, and never returns; the points of such a walk run on past
 * the end.
 * These three calls are single-slab calls (nranks == 1, no self_ring): there every node index is folded into the box on
 * all three axes, so positions may lie any distance outside it.  On a z-slab of several the z index is not folded and
 * positions are not checked against the ghost planes. */
int xpic_cell_traversal(xpic_ctx* ctx, int64_t n, const double* end3, const double* start3, int max_pts, double* pts,
  int* counts);
/* ImplicitEsirkepov::interpolate (src/algorithms/implicit_esirkepov.cpp:60-90): E_p with the segment's 54-weight shape,
 * B_p with Shape(midpoint) + SimpleInterpolation, from the context's XPIC_E / XPIC_B. */
int xpic_implicit_esirkepov_interpolate(xpic_ctx* ctx, int64_t n, const double* rn3, const double* r03, double* Ep3,
  double* Bp3);
/* ImplicitEsirkepov::decompose (:92-117): field += alpha[q] * v[q] * shape(q), ghost contributions folded like
 * DMLocalToGlobal(ADD_VALUES).  Uses the scratch vector XPIC_W2. */
int xpic_implicit_esirkepov_decompose(xpic_ctx* ctx, int64_t n, const double* alpha, const double* v3, const double* rn3,
  const double* r03, int field);

/* ---- drift-kinetic (guiding-centre) pusher on the context's static fields, batch form over n particles (host arrays).
 * A particle is six doubles {x, y, z, p_parallel, p_perp, mu_p} (PointByField, src/interfaces/point.h:37-58).
 * gradB_field: any xpic_field id whose vector the caller has filled with grad |B| (a scratch vector such as XPIC_W0), or
 * -1 for the reference's gradB_g == nullptr (grad B = 0).  Positions are not folded into the box: the gathers wrap
 * their node indices, folding is the caller's business as correct_coordinates is in the reference.  Single z-slab
 * contexts only (nranks == 1, no self_ring).  n == 0 succeeds and touches nothing.
 * xpic_drift_kinetic_interpolate: DriftKineticEsirkepov::interpolate (src/algorithms/drift_kinetic_implicit.cpp:11-31):
 * E_p with the segment shape of (rn, r0) as xpic_implicit_esirkepov_interpolate, B_p and gradB_p with Shape(rn) (radius
 * 1.5, 2nd-order spline) + SimpleInterpolation's magnetic products -- at rn, not at the midpoint. */
typedef struct xpic_dk_params {
  double qm, mp;     /* DriftKineticPush::set_qm / set_mp */
  double dt;
  double eps, delta; /* set_tolerances: residual bounds of the position and of p_parallel (reference default 1e-12) */
  int maxit;         /* >= 1 (reference default 30) */
} xpic_dk_params;
int xpic_drift_kinetic_interpolate(xpic_ctx* ctx, int64_t n, const double* rn3, const double* r03, int gradB_field,
  double* Ep3, double* Bp3, double* gradBp3);
/* DriftKineticPush::process (src/algorithms/drift_kinetic_push.cpp:48-108) from the initial guess pn = p0, with the fields
 * of xpic_drift_kinetic_interpolate(p0.r -> pn.r).  iterations[q] is the reference's get_iteration_number(): the updates
 * made, >= 1; == maxit for a particle that did not meet the tolerances (the reference aborts there; here the caller
 * decides). */
int xpic_drift_kinetic_push(xpic_ctx* ctx, int64_t n, const xpic_dk_params* params, int gradB_field, const double* p0_6,
  double* pn_6, int* iterations);
/* `steps` pushes in a row with the particles kept on the device, in launches of at most XPIC_DK_LAUNCH_STEPS steps:
 * state_6 is read and overwritten with the result, bit for bit that of `steps` calls of xpic_drift_kinetic_push.  samples
 * (or NULL): the state after every sample_every-th step (>= 1), samples[(k * n + q) * 6 ..] for k < steps / sample_every.
 * iterations_total[q] / iterations_max[q]: sum and maximum of the particle's iteration counts over the steps. */
#define XPIC_DK_LAUNCH_STEPS 64
int xpic_drift_kinetic_trace(xpic_ctx* ctx, int64_t n, const xpic_dk_params* params, int gradB_field, int64_t steps,
  int64_t sample_every, double* state_6, double* samples, int64_t* iterations_total, int* iterations_max);

/* ---- full-orbit pusher on the context's static XPIC_E / XPIC_B, batch form over n particles (host arrays).  A particle
 * is a `Point` record: six doubles {x, y, z, px, py, pz} (src/interfaces/point.h:7-35).  The companion of the
 * drift-kinetic calls above: the reference's grid tests (tests/drift_kinetic_push/drift_kinetic_grid_boris_ex1..4) run
 * the two side by side on the same grid fields.  Positions are not folded into the box: the gathers wrap their node
 * indices.  Single z-slab contexts only (nranks == 1, no self_ring).  n == 0 succeeds and touches nothing.
 * Schemes 0..16 are the Chin ids of BorisPush as tests/boris_push/boris_push.h:20-228 composes them (process_<id>):
 * update_r (src/algorithms/boris_push.cpp:19-22), a gather at the particle with Shape::setup(r) (radius 1.5, 2nd-order
 * spline) and SimpleInterpolation's electric and magnetic products -- what basic::Particles::push gathers
 * (src/impls/basic/particles.cpp:32-37) --, and update_vM / vB / vC1 / vC2 / vEB (boris_push.cpp:24-91).  update_v_impl
 * normalises B_p: where |B_p| is 0 the reference divides by zero; here such a particle keeps its v in the magnetic ids.
 * The LF ids are the 1B step: the half step back that starts a leap-frog run is the caller's.
 * XPIC_FO_CN is CrankNicolsonPush::process (src/algorithms/crank_nicolson_push.cpp:31-71) from the initial guess
 * pn = p0, with the gather of ImplicitEsirkepov::interpolate (src/algorithms/implicit_esirkepov.cpp:63-91). */
enum xpic_fo_scheme {
  XPIC_FO_M1A = 0, XPIC_FO_M1B = 1, XPIC_FO_MLF = 2, XPIC_FO_B1A = 3, XPIC_FO_B1B = 4, XPIC_FO_BLF = 5, XPIC_FO_C1A = 6,
  XPIC_FO_C1B = 7, XPIC_FO_CLF = 8, XPIC_FO_M2A = 9, XPIC_FO_M2B = 10, XPIC_FO_C2A = 11, XPIC_FO_B2B = 12,
  XPIC_FO_EB1A = 13, XPIC_FO_EB1B = 14, XPIC_FO_EBLF = 15, XPIC_FO_EB2B = 16, XPIC_FO_CN = 17, XPIC_FO_NSCHEMES = 18
};
typedef struct xpic_fo_params {
  double qm, dt;
  double atol, rtol; /* XPIC_FO_CN: CrankNicolsonPush::set_tolerances (reference default 1e-7, 1e-7) */
  int32_t scheme;    /* enum xpic_fo_scheme */
  int32_t maxit;     /* XPIC_FO_CN: 1 .. XPIC_FO_MAXIT (reference default 30); ignored by the other schemes */
} xpic_fo_params;
#define XPIC_FO_MAXIT 64
#define XPIC_FO_LAUNCH_STEPS 64
/* One step: process_<id> (tests/boris_push/boris_push.h:20-198) or CrankNicolsonPush::process
 * (crank_nicolson_push.cpp:31-71).  iterations (XPIC_FO_CN: required; otherwise it may be NULL and is zeroed if given):
 * the reference's get_iteration_number(), the index of the iteration whose residual met atol + rtol * r0, or maxit for a
 * particle that ran out of iterations (the reference aborts there; here the caller decides). */
int xpic_full_orbit_push(xpic_ctx* ctx, int64_t n, const xpic_fo_params* params, const double* p0_6, double* pn_6,
  int* iterations);
/* `steps` pushes in a row with the particles kept on the device, in launches of at most XPIC_FO_LAUNCH_STEPS steps (the
 * time loops of tests/boris_push/boris_push_ex1.cpp:51-60 and tests/crank_nicolson_push/crank_nicolson_push_ex2.cpp:43-56):
 * p_6 is read and overwritten with the result, bit for bit that of `steps` calls of xpic_full_orbit_push.  samples (or
 * NULL): the state after every sample_every-th step (>= 1), samples[(k * n + q) * 6 ..] for k < steps / sample_every, so
 * sample 0 is the state after step sample_every, as in xpic_drift_kinetic_trace.  iterations_sum[q] / iterations_max[q]
 * (XPIC_FO_CN: required; otherwise optional and zeroed): sum and maximum of the particle's iteration counts. */
int xpic_full_orbit_trace(xpic_ctx* ctx, int64_t n, const xpic_fo_params* params, int64_t steps, int64_t sample_every,
  double* p_6, double* samples, int64_t* iterations_sum, int* iterations_max);

/* ---- open-trap traces: the two traces above with RemoveParticles' region rule inside the step loop
 * (RemoveParticles::execute, src/commands/remove_particles.cpp:22-38, applied to one particle).  At the top of every step
 * the corner of the particle's cell, (floor(x / dx) dx, floor(y / dy) dy, floor(z / dz) dz) -- FLOOR_STEP as in
 * Particles::add_particle (src/interfaces/particles.cpp:47-67) -- of its UNFOLDED position is tested with WithinBox /
 * WithinCylinder (src/utils/geometries.cpp:3-19), the test of xpic_remove_particles.  A particle that fails is removed:
 * exit_step[q] = step0 + the steps it has completed in this call, its state stays what it was, it takes no further step
 * and adds nothing to the iteration counters.  Positions are not folded, so a particle that runs out of the box fails a
 * box that lies inside the domain: the open end.  The state after the last step is not tested (the next call's first step
 * tests it), so a call of s1 + s2 steps equals a call of s1 steps followed by one of s2 steps with step0 advanced by s1
 * and the first call's exit_step, bit for bit.  A particle that stays runs the step functions of the closed trace: its
 * result is the closed trace's, bit for bit.
 * exit_step (required, in and out, one entry per particle): -1 alive; k >= 0 removed after completing k steps in total; a
 * particle that enters with k >= 0 is returned untouched.  alive (or NULL; needs sample_every >= 1): alive[k] = particles
 * still alive when sample k is taken, k < steps / sample_every.  *removed (required): particles removed by this call.  In
 * samples, a removed particle's state is repeated in every later row.  Iteration counters as in the closed traces.
 * compact: what happens to the list of live particles between the launches (each of at most XPIC_FO_LAUNCH_STEPS /
 * XPIC_DK_LAUNCH_STEPS steps).  The results are bit-identical for all three values. */
enum xpic_trace_compact {
  XPIC_COMPACT_AUTO = 0,  /* rebuild the list, in order, when fewer than half of its entries are alive */
  XPIC_COMPACT_NEVER = 1, /* every launch covers all n particles */
  XPIC_COMPACT_ALWAYS = 2 /* rebuild the list after every launch that removed a particle */
};
typedef struct xpic_trace_region {
  int32_t geometry; /* XPIC_GEOM_BOX, XPIC_GEOM_CYLINDER */
  int32_t compact;  /* enum xpic_trace_compact */
  double geom[7];   /* as xpic_remove_particles': {min xyz, max xyz} (box), {center xyz, radius, height} (cylinder) */
  int64_t step0;    /* steps this batch has been traced already (>= 0) */
} xpic_trace_region;
int xpic_full_orbit_trace_open(xpic_ctx* ctx, int64_t n, const xpic_fo_params* params, int64_t steps, int64_t sample_every,
  double* p_6, double* samples, int64_t* iterations_sum, int* iterations_max, const xpic_trace_region* region,
  int64_t* exit_step, int64_t* alive, int64_t* removed);
int xpic_drift_kinetic_trace_open(xpic_ctx* ctx, int64_t n, const xpic_dk_params* params, int gradB_field, int64_t steps,
  int64_t sample_every, double* state_6, double* samples, int64_t* iterations_total, int* iterations_max,
  const xpic_trace_region* region, int64_t* exit_step, int64_t* alive, int64_t* removed);

/* ---- paired trace: a guiding centre beside the full orbit of the same particle, advanced in lock-step on the device, and
 * the reference's comparison of the two reduced there -- the time loop of the grid tests
 * tests/drift_kinetic_push/drift_kinetic_grid_boris_ex1..4.cpp (ex1.cpp:79-98: process, boris_step, interpolate,
 * update_comparison_stats) for n pairs.  Pair q is the Point record p_6[6 q ..] (fo: its scheme and tolerances) and the
 * PointByField record state_6[6 q ..] (dk, gradB_field as in xpic_drift_kinetic_trace); both are read and overwritten.
 * After every step the grid / Boris half of update_comparison_stats (tests/drift_kinetic_push/drift_kinetic_push.h:293-329;
 * there is no analytical member here) is formed statement by statement, with Bg = the B_p of
 * DriftKineticEsirkepov::interpolate(rn = the guiding centre after the step, r0 = before it) (ex1.cpp:92-93), which is
 * xpic_drift_kinetic_interpolate's Bp3 for that segment, and Vector3::parallel_to / transverse_to / length
 * (src/utils/vector3.h:160-205):
 *   err_z      = |gc.z - fo.z|                                                       (:311)
 *   err_par    = |gc.p_parallel - |fo.p.parallel_to(Bg)||     (a length: the sign is lost, as in the reference)  (:316-317)
 *   err_mu     = |gc.mu_p - 0.5 mp |fo.p.transverse_to(Bg)|^2 / |Bg||               (:320-322)
 *   err_energy = |0.5 (gc.p_perp^2 + gc.p_parallel^2) - 0.5 fo.p^2|                  (:270-278, :325-327)
 * Every maximum is m = (m < e) ? e : m, the reference's std::max(m, e): an error that is not a number leaves the maximum
 * alone, an infinite one is kept; |Bg| = 0 gets no special case.
 * stats_4 [n][4] (required, in and out): the running maxima {z, p_parallel, mu, energy} of each pair over the steps; the
 * entries are read as the maxima so far (zeros to start; a negative entry or a NaN is not checked, the rule above says what
 * becomes of it).  curve_4 [steps / sample_every][4] (or NULL; needs sample_every >= 1): curve_4[k][j] = the maximum over
 * the pairs of error j at step (k + 1) sample_every of this call, 0 where no pair has an error > 0; written, not
 * accumulated.  dk_iterations_total / dk_iterations_max (required) and fo_iterations_sum / fo_iterations_max (XPIC_FO_CN:
 * required; otherwise optional and zeroed) are the counters of the two closed traces.
 * Checks: those of xpic_full_orbit_trace and xpic_drift_kinetic_trace, dk->maxit <= XPIC_PAIR_DK_MAXIT, and
 * fo->dt == dk->dt, fo->qm == dk->qm.  n == 0 succeeds and touches nothing; steps == 0 returns the inputs.  Single z-slab
 * contexts only.  Launches of at most XPIC_PAIR_LAUNCH_STEPS steps.  The region rule of the open traces is not part of
 * this call: a pair is never removed.
 * Guarantees: (a) p_6, state_6 and the four counters are bit for bit those of xpic_full_orbit_trace and
 * xpic_drift_kinetic_trace over the same steps; (b) a call of s1 + s2 steps equals a call of s1 steps followed by one of
 * s2 steps fed the first call's p_6, state_6 and stats_4, bit for bit in the states and stats_4; (c) curve_4[k][j] is, bit
 * for bit, the maximum over q of the error a run of pair q alone has at that step. */
#define XPIC_PAIR_LAUNCH_STEPS 64
#define XPIC_PAIR_DK_MAXIT 1024
int xpic_paired_trace(xpic_ctx* ctx, int64_t n, const xpic_fo_params* fo, const xpic_dk_params* dk, int gradB_field,
  int64_t steps, int64_t sample_every, double* p_6, double* state_6, double* stats_4, double* curve_4,
  int64_t* fo_iterations_sum, int* fo_iterations_max, int64_t* dk_iterations_total, int* dk_iterations_max);

/* ---- analytic field models: a second field source for the tracers, evaluated on the device at the position the
 * reference's set_fields_callback is given, instead of gathered from the context's grid.  A closed set of kinds, each the
 * restatement of one family of the reference's callbacks (xpic_amd/csrc/field_model.h):
 *   XPIC_MODEL_UNIFORM           E = E0, B = B0, grad |B| = 0 (tests/drift_kinetic_push/drift_kinetic_push_ex1.cpp:9-13,
 *                                ex2.cpp:11-16, tests/crank_nicolson_push/crank_nicolson_push_ex1.cpp, ex2.cpp)
 *   XPIC_MODEL_LINEAR            E = E0, B = B0 + ((r - r0) . g) g / |g|, grad |B| = g (drift_kinetic_push_ex3.cpp:12-17)
 *   XPIC_MODEL_QUADRATIC_MIRROR  quadratic_magnetic_mirror::get_fields (tests/drift_kinetic_push/drift_kinetic_push.h:24-70)
 *                                with B_min, B_max, W, D; axis at (W / 2, W / 2), midplane z = D / 2.  E_phi and phi: the
 *                                E of drift_kinetic_push_ex4.cpp:12-22, {E_phi (y - W / 2), -E_phi (x - W / 2),
 *                                phi pi / D sin(pi (z - D / 2) / D)}; both 0: E = 0
 *   XPIC_MODEL_GAUSSIAN_MIRROR   gaussian_magnetic_mirror::get_fields (drift_kinetic_push.h:72-157) with B_min, B_max, L,
 *                                W; axis at (L, L), throats at z = 0 and z = 2 L; E = 0
 * Members a kind does not name are ignored.  W (and the quadratic mirror's D) must not be 0. */
enum xpic_model_kind {
  XPIC_MODEL_UNIFORM = 0, XPIC_MODEL_LINEAR = 1, XPIC_MODEL_QUADRATIC_MIRROR = 2, XPIC_MODEL_GAUSSIAN_MIRROR = 3,
  XPIC_MODEL_NKINDS = 4
};
typedef struct xpic_field_model {
  int32_t kind; /* enum xpic_model_kind */
  int32_t reserved;
  double E0[3];
  double B0[3];
  double r0[3];
  double g[3];
  double B_min;
  double B_max;
  double W;
  double D;
  double L;
  double E_phi;
  double phi;
} xpic_field_model;
/* The model at n positions r3[3 q ..] (host arrays) -> E3, B3, gradB3 (3 doubles per position each). */
int xpic_model_fields(xpic_ctx* ctx, const xpic_field_model* model, int64_t n, const double* r3, double* E3, double* B3,
  double* gradB3);
/* Fills grid vectors from a model as the reference's FieldContext::initialize does (drift_kinetic_push.h:176-209 with the
 * fill functions of drift_kinetic_grid_boris_ex1..4.cpp): all three components of node (i, j, k) are the model at
 * (i dx, j dy, k dz).  A field id < 0 is skipped.  Any context; on z-slabs every rank fills its owned planes (ghost planes
 * are the next exchange's). */
int xpic_set_model_field(xpic_ctx* ctx, const xpic_field_model* model, int E_field, int B_field, int gradB_field);
/* xpic_full_orbit_trace_open and xpic_drift_kinetic_trace_open with the model in the grid's place.  The model is evaluated
 * where the reference's callback is: at rn for the drift-kinetic pusher (E_p too: no segment shape), at the particle's r in
 * the kick of a Chin scheme, at the midpoint (r1 + r0) / 2 for Crank-Nicolson (drift_kinetic_push_ex9.cpp:75-78).  The
 * step arithmetic is the grid traces' own text (full_orbit_step.h, drift_kinetic_step.h).  steps == 1 is the one-step push.
 * region: as in the open traces, with two differences.  geometry may be XPIC_GEOM_NONE: no particle is ever tested or
 * removed, the call is the closed trace, and exit_step, alive and removed may be NULL.  `compact` is not read: every launch
 * covers all n particles (XPIC_COMPACT_NEVER).  dx, dy, dz of the region rule are the context's.  Calls compose through
 * step0 and exit_step as the open traces do, bit for bit.  No grid vector is read, so any context is accepted, z-slabs
 * included.  n == 0 succeeds and touches nothing.  Launches of at most XPIC_MODEL_LAUNCH_STEPS steps; the drift-kinetic
 * maxit is within 1 .. XPIC_MODEL_DK_MAXIT, the Crank-Nicolson one within 1 .. XPIC_FO_MAXIT. */
#define XPIC_GEOM_NONE (-1)
#define XPIC_MODEL_LAUNCH_STEPS 64
#define XPIC_MODEL_DK_MAXIT 1024
int xpic_model_full_orbit_trace(xpic_ctx* ctx, int64_t n, const xpic_fo_params* params, const xpic_field_model* model,
  int64_t steps, int64_t sample_every, double* p_6, double* samples, int64_t* iterations_sum, int* iterations_max,
  const xpic_trace_region* region, int64_t* exit_step, int64_t* alive, int64_t* removed);
int xpic_model_drift_kinetic_trace(xpic_ctx* ctx, int64_t n, const xpic_dk_params* params, const xpic_field_model* model,
  int64_t steps, int64_t sample_every, double* state_6, double* samples, int64_t* iterations_total, int* iterations_max,
  const xpic_trace_region* region, int64_t* exit_step, int64_t* alive, int64_t* removed);

/* ---- time-dependent analytic fields: the model traces with a time envelope on the model's E, the callback of
 * tests/crank_nicolson_push/crank_nicolson_push_ex3.cpp:39-58 that captures the loop index, `E_p = E0 * (t * dt)`,
 * `B_p = B0`.  A closed set of kinds again:
 *   XPIC_ENV_CONSTANT   no factor is applied at all: the call is the model trace, bit for bit (a NULL envelope too)
 *   XPIC_ENV_RAMP       f = a + b * t        ex3 is a = 0, b = 1; then f is exactly t, contracted or not
 *   XPIC_ENV_HARMONIC   f = cos(omega * t + phase)     AN EXTENSION: the reference has no such callback
 * Time: t = (double)(region->step0 + k) * dt, one product, k = the steps this call has completed before the step in
 * question -- the reference's `t * dt` with its integer loop index; dt is params->dt.  One factor per step: every field
 * evaluation inside the step (all kicks of a Chin scheme, every Picard / Crank-Nicolson iteration, the drift-kinetic
 * callback) sees the same f, as a callback that captures t does.  E of the step is E_model(r) * f, component by component
 * (Vector3R * scalar); B and grad |B| are untouched.  a + b * t and omega * t + phase are formed without contraction, one
 * rounding per operation.  The parameters the kind reads (a, b for the ramp, omega, phase for the harmonic) must be finite;
 * the others are ignored. */
enum xpic_envelope_kind { XPIC_ENV_CONSTANT = 0, XPIC_ENV_RAMP = 1, XPIC_ENV_HARMONIC = 2, XPIC_ENV_NKINDS = 3 };
typedef struct xpic_field_envelope {
  int32_t kind; /* enum xpic_envelope_kind */
  int32_t reserved;
  double a;
  double b;
  double omega;
  double phase;
} xpic_field_envelope;
/* xpic_model_full_orbit_trace and xpic_model_drift_kinetic_trace with an envelope: everything else is theirs -- region
 * semantics with XPIC_GEOM_NONE, samples, counters, checks, launches of at most XPIC_MODEL_LAUNCH_STEPS steps, any context,
 * z-slabs included.  step0, which the model traces read even under XPIC_GEOM_NONE, also fixes the clock here: a call of
 * s1 + s2 steps equals a call of s1 steps followed by one of s2 steps with step0 advanced by s1 (and the first call's
 * exit_step and sums_4), bit for bit, for every envelope.
 * sums_4 [n][4] (or NULL; the full-orbit trace only; read and written, so calls compose through it): the running sums of
 * ex3's two checks (ex3.cpp:51-57), kept on the device so that a long run needs no samples.  After each completed step
 * p0 -> pn of a live particle, with vh = 0.5 (pn.p + p0.p) and (E_s, B_s) = the model at (r0 + rn) / 2 with the step's factor:
 *   sums_4[q][0]    += 0.5 (|pn.p|^2 - |p0.p|^2) - qm dt (vh . E_s)    (qm = -1, uniform E0: ex3's term before its / geom_nt)
 *   sums_4[q][1..3] += vh.transverse_to(B_s)                            (Vector3::transverse_to, src/utils/vector3.h:195-205)
 * The sums are not divided: the caller divides by its step count.  A removed particle adds nothing after its exit.  With
 * sums_4 the step costs one more model evaluation; without it, nothing. */
int xpic_model_full_orbit_trace_timed(xpic_ctx* ctx, int64_t n, const xpic_fo_params* params, const xpic_field_model* model,
  const xpic_field_envelope* envelope, int64_t steps, int64_t sample_every, double* p_6, double* samples,
  int64_t* iterations_sum, int* iterations_max, const xpic_trace_region* region, int64_t* exit_step, int64_t* alive,
  int64_t* removed, double* sums_4);
int xpic_model_drift_kinetic_trace_timed(xpic_ctx* ctx, int64_t n, const xpic_dk_params* params,
  const xpic_field_model* model, const xpic_field_envelope* envelope, int64_t steps, int64_t sample_every, double* state_6,
  double* samples, int64_t* iterations_total, int* iterations_max, const xpic_trace_region* region, int64_t* exit_step,
  int64_t* alive, int64_t* removed);
/* out[i] = the factor of step step0 + i for i < nsteps (0 <= nsteps <= 2^31, step0 >= 0; a host array), evaluated on the
 * device by the device function the two traces call: what a test holds against a host cos. */
int xpic_envelope_factors(xpic_ctx* ctx, const xpic_field_envelope* envelope, double dt, int64_t step0, int64_t nsteps,
  double* out);

/* ---- collisional traces: xpic_model_full_orbit_trace and xpic_model_drift_kinetic_trace with Coulomb scattering of the
 * test particles off Maxwellian background species, by xpic_collide's pair collision (Takizuka and Abe).  AN EXTENSION, as
 * xpic_collide is: the reference has no collision operator, so no file:line of it is cited.  Everything that is not said
 * here is the model traces': region semantics with XPIC_GEOM_NONE, samples, counters, checks, launches of at most
 * XPIC_MODEL_LAUNCH_STEPS steps, any context.  The grid traces' collisional form follows below
 * (xpic_full_orbit_trace_collisional); the envelope traces and the paired and triplet traces have none.
 * When: after the push of step k and before that step's sample is stored, where k = region->step0 + the steps this call
 * has completed + 1 is the step's global index; the step collides iff k % every == 0, with dt_c = every * dt (dt is
 * params->dt), against the backgrounds b = 0 .. nbg - 1 in this order.  A removed particle collides no more.
 * Streams (splitmix / u01 as everywhere in this library): one per (seed, particle0 + q, k, b), q the particle's index in
 * the batch.  step key: x = seed; splitmix(x); x ^= k * 0xD1342543DE82EF95; key = splitmix(x) (xpic_collide's first two
 * mixes).  particle key: y = key ^ ((particle0 + q) * 0xD6E8FEB86659FD93); splitmix(y).  stream state: z = particle key ^
 * ((b + 1) * 0xA0761D6478BD642F); st = splitmix(z).  From st come seven u01 draws in this order: a1 a2 a3 a4, a5, u1 u2 u3.
 * Partner: w = drift + vth (g1, g2, g3), g1 = sqrt(-2 ln a1) cos(2 pi a2), g2 = sqrt(-2 ln a1) sin(2 pi a2),
 * g3 = sqrt(-2 ln a3) cos(2 pi a4); vth is the background's thermal speed per component, sqrt(T_b / m_b).
 * Collision: xpic_collide's text with v_a = v, v_b = w, q_a = qm * mass, m_a = mass, n_L = bg.n, dt = dt_c and (u1, u2, u3)
 * as its three draws; only the test particle is updated, v += (m_ab / m_a) du.  The partner's side is not stored.  |u| == 0
 * is skipped and counted, and leaves the record's bits.  The Theta = pi limit and the overflow rule are xpic_collide's.
 * All of this is rounded operation by operation (no contraction), sigma^2's factor as
 * ((S (q_a q_a) (q_b q_b) / (m_ab m_ab)) n_L) dt_c with dt_c = (double)every * dt.
 * Full orbit: v is the record's p; a5 is drawn and discarded.  The staggered LF ids collide their p as it stands.
 * Guiding centre: B = the model at the pushed position, |B| = sqrt(Bx Bx + By By + Bz Bz), b = B / |B|; |B| == 0 skips the
 * step's collisions for that particle and counts nbg skipped.  e1 = normalize(b x e_c), e_c the coordinate axis with the
 * smallest |b_c| (a tie: the lowest index), e2 = b x e1; for every background psi = 2 pi a5,
 * v = p_parallel b + p_perp (cos psi e1 + sin psi e2), collided as above to v'; then p_parallel' = v' . b,
 * p_perp' = |v' - p_parallel' b|, mu_p' = mp p_perp'^2 / (2 |B|).  The position is NOT moved: the displacement of the
 * guiding centre in a collision is left out, so this is velocity-space scattering (pitch-angle and energy), not classical
 * cross-field transport.
 * coll_4 (or NULL) = {collisions made, skipped, sum of sigma^2 over the collisions made, collisions with sigma^2 > 1} of this
 * call; written, not accumulated.
 * Refused before anything changes: nbg outside 0 .. XPIC_TRACE_BG_MAX, every < 1, particle0 < 0, a negative (or not finite)
 * strength, mass <= 0, a background with m <= 0, n < 0 or vth < 0.
 * Guarantees: (a) collisions == NULL, nbg == 0 or strength == 0 is the model trace, bit for bit -- state, samples, counters,
 * exit_step, alive and removed -- and coll_4 is zeros; (b) a call of s1 + s2 steps equals a call of s1 steps followed by
 * one of s2 steps with step0 advanced by s1 (and the first call's exit_step), bit for bit; (c) a batch split in two, the
 * second part with particle0 advanced by the first part's size, gives the bits of the whole batch; (d) momentum and energy
 * of every test-particle / partner pair are conserved (the partner's side is not stored: tests/collisional_trace_ref.py
 * checks it). */
#define XPIC_TRACE_BG_MAX 4
typedef struct xpic_trace_background { double q, m, n, vth, drift[3]; } xpic_trace_background;
typedef struct xpic_trace_collisions {
  int32_t nbg;        /* 0 .. XPIC_TRACE_BG_MAX; 0: no collisions */
  int32_t every;      /* >= 1: collide after the steps whose global index is a multiple of it, with dt_c = every * dt */
  uint64_t seed;
  int64_t particle0;  /* the batch's first particle has the global index particle0 (>= 0) */
  double strength;    /* S of xpic_collide; 0: no collisions */
  double mass;        /* m_a of the test particle; q_a = qm * mass */
  xpic_trace_background bg[XPIC_TRACE_BG_MAX];
} xpic_trace_collisions;
int xpic_model_full_orbit_trace_collisional(xpic_ctx* ctx, int64_t n, const xpic_fo_params* params,
  const xpic_field_model* model, int64_t steps, int64_t sample_every, double* p_6, double* samples, int64_t* iterations_sum,
  int* iterations_max, const xpic_trace_region* region, int64_t* exit_step, int64_t* alive, int64_t* removed,
  const xpic_trace_collisions* collisions, double* coll_4);
int xpic_model_drift_kinetic_trace_collisional(xpic_ctx* ctx, int64_t n, const xpic_dk_params* params,
  const xpic_field_model* model, int64_t steps, int64_t sample_every, double* state_6, double* samples,
  int64_t* iterations_total, int* iterations_max, const xpic_trace_region* region, int64_t* exit_step, int64_t* alive,
  int64_t* removed, const xpic_trace_collisions* collisions, double* coll_4);

/* ---- background profiles: a spatially resolved background species for the collisional grid traces below.  AN EXTENSION,
 * as the collision operator is.  A profile holds five doubles per local cell, in the cell order of the cell-sorted sorts
 * (x fastest, then y, then z): a density n, a thermal speed per component vth, a drift u[3].  The context owns
 * XPIC_TRACE_BG_MAX slots.  Single z-slab contexts only, as the grid tracers; other contexts are refused.
 * xpic_background_set uploads host arrays n_zyx [nz][ny][nx], vth_zyx [nz][ny][nx] and drift_zyx3 [nz][ny][nx][3] (NULL:
 * no drift).  Refused, the slot left as it was: a slot outside 0 .. XPIC_TRACE_BG_MAX - 1, a NULL n or vth, a negative or
 * non-finite n or vth, a non-finite drift.  xpic_background_get downloads a slot (any output may be NULL; an empty slot
 * is refused), xpic_background_clear empties one.
 * xpic_background_from_sort fills the slot on the device from the records of a sort, cell by cell; N = the cell's records:
 *   n   = (sort.n / sort.Np) N          xpic_collide's n_L: a tracer sees the density the sort's own collisions see
 *   u   = (sum v) / N
 *   vth = sqrt(sum |v - u|^2 / (3 N))   two passes, |d|^2 = (dx dx + dy dy) + dz dz
 * An empty cell gives zeros, a cell of one record vth = 0.  Every sum is taken in a fixed order (lane l of a wave adds the
 * records l, l + 64, ... of the cell in cell order, the 64 partial sums are folded by halves), rounded operation by
 * operation: two calls give the same bits.  The records are not changed: the sort and a following xpic_collide are
 * what they would have been.  (A deferred re-binning of the sort is completed first, as xpic_sort_get_particles and
 * xpic_collide complete it.) */
int xpic_background_set(xpic_ctx* ctx, int slot, const double* n_zyx, const double* vth_zyx, const double* drift_zyx3);
int xpic_background_get(xpic_ctx* ctx, int slot, double* n_zyx, double* vth_zyx, double* drift_zyx3);
int xpic_background_clear(xpic_ctx* ctx, int slot);
int xpic_background_from_sort(xpic_ctx* ctx, int slot, int sort);

/* ---- collisional grid traces: xpic_full_orbit_trace_open and xpic_drift_kinetic_trace_open with the collisions of the
 * collisional traces above, off uniform backgrounds or off the context's background profiles: test particles traced
 * through the fields of a run while they scatter off the plasma of that run.  AN EXTENSION.  The argument lists are the
 * open grid traces' with three more: collisions, profile, coll_4.  Everything xpic_trace_collisions says above holds --
 * when a step collides, every, seed, particle0, the streams and their seven draws, the partner, the guiding centre's
 * gyrophase and basis, the tallies -- and everything else is the open grid traces': samples, counters, exit_step, alive,
 * removed, launches of at most XPIC_FO_LAUNCH_STEPS / XPIC_DK_LAUNCH_STEPS steps, `compact`.  region->geometry may be
 * XPIC_GEOM_NONE as in the model traces: the closed trace; exit_step, alive and removed may then be NULL.
 * profile: NULL, or collisions->nbg entries.  Entry -1 (and NULL): background b is the uniform one of the struct.  Entry
 * s >= 0: background b takes n, vth and drift from slot s at the cell of the particle's pushed position, floor(r / d) per
 * axis folded onto the grid by the true modulus (positions are not folded in the traces); piecewise constant, nothing is
 * interpolated.  The struct's q and m are used, its n, vth and drift ignored.  sigma^2's factor is formed on the device as
 * defined above, ((S (q_a q_a) (q_b q_b) / (m_ab m_ab)) n_L) dt_c, rounded operation by operation.  A cell with n == 0
 * makes no collision for that background: nothing is drawn, the record keeps its bits and neither tally moves.  A position
 * that is not a number, or further than 1e9 cells out, has no cell and meets no profile.
 * Guiding centre: B is what xpic_drift_kinetic_interpolate returns for the segment (r, r) at the pushed position r; with
 * |B| == 0 the skipped tally counts the backgrounds that have somebody to meet there.
 * Refused before anything changes: what the open grid traces and the collisional traces refuse, a profile entry outside
 * -1 .. XPIC_TRACE_BG_MAX - 1, a named slot that is empty, a context that is not a single slab.
 * Guarantees, bit for bit: (a) collisions == NULL, nbg == 0 or strength == 0 is the grid trace, open or (XPIC_GEOM_NONE)
 * closed -- state, samples, counters, exit_step, alive, removed -- and coll_4 is zeros; (b) a call of s1 + s2 steps equals
 * a call of s1 steps followed by one of s2 steps with step0 advanced by s1 and the first call's exit_step; (c) a batch
 * split in two, the second part with particle0 advanced by the first part's size, gives the bits of the whole batch (the
 * float tally coll_4[2] to rounding); (d) the three values of `compact` give the same bits; (e) a profile that holds the
 * struct's n (> 0), vth and drift in every cell gives the bits of profile == NULL; (f) xpic_background_from_sort leaves the
 * sort's records and xpic_collide's results unchanged. */
int xpic_full_orbit_trace_collisional(xpic_ctx* ctx, int64_t n, const xpic_fo_params* params, int64_t steps,
  int64_t sample_every, double* p_6, double* samples, int64_t* iterations_sum, int* iterations_max,
  const xpic_trace_region* region, int64_t* exit_step, int64_t* alive, int64_t* removed,
  const xpic_trace_collisions* collisions, const int32_t* profile, double* coll_4);
int xpic_drift_kinetic_trace_collisional(xpic_ctx* ctx, int64_t n, const xpic_dk_params* params, int gradB_field,
  int64_t steps, int64_t sample_every, double* state_6, double* samples, int64_t* iterations_total, int* iterations_max,
  const xpic_trace_region* region, int64_t* exit_step, int64_t* alive, int64_t* removed,
  const xpic_trace_collisions* collisions, const int32_t* profile, double* coll_4);

/* ---- triplet trace: the whole time loop of the reference's grid tests
 * (tests/drift_kinetic_push/drift_kinetic_grid_boris_ex1..4.cpp, ex1.cpp:79-98) for n triplets, with all seven maxima of
 * ComparisonStats (tests/drift_kinetic_push/drift_kinetic_push.h:253-329) reduced on the device.  Triplet q is three
 * records, all read and overwritten: the Point p_6[6 q ..] (a full orbit on the model, fo: its scheme and tolerances), the
 * PointByField state_model_6[6 q ..] (a guiding centre on the model) and the PointByField state_grid_6[6 q ..] (a guiding
 * centre on the context's XPIC_E / XPIC_B, gradB_field as in xpic_drift_kinetic_trace -- the grid xpic_set_model_field
 * fills, though nothing here requires that).  dk serves both guiding centres.  One step, in the reference's order:
 *   1. DriftKineticPush::process of the analytic centre, the model at rn                 (push_analytical, ex1.cpp:85)
 *   2. DriftKineticPush::process of the grid centre, DriftKineticEsirkepov::interpolate  (push_grid, :86)
 *   3. the orbit's step on the model with fo->scheme: boris_step (drift_kinetic_push.h:280-291) is XPIC_FO_EB2B; all 18
 *      ids are accepted, XPIC_FO_CN with the model at the midpoint as in xpic_model_full_orbit_trace           (:87)
 *   4. Ba, gBa = the model at the analytic centre's new position                                                (:89-90)
 *   5. Bg, gBg = DriftKineticEsirkepov::interpolate(rn = the grid centre after the step, r0 = before it); gBg = 0 with
 *      gradB_field == -1                                                                                        (:92-93)
 *   6. update_comparison_stats (drift_kinetic_push.h:293-329), statement by statement:
 *        err_B      = |Ba - Bg|                 err_gradB = |gBa - gBg|            err_pos = |model.r - grid.r|
 *        err_z      = |grid.z - fo.z|
 *        err_par    = |grid.p_parallel - |fo.p.parallel_to(Ba)||
 *        err_mu     = |grid.mu_p - 0.5 mp |fo.p.transverse_to(Ba)|^2 / |Ba||
 *        err_energy = |0.5 (grid.p_perp^2 + grid.p_parallel^2) - 0.5 fo.p^2|
 * The last four are xpic_paired_trace's with one difference: the orbit's momentum is projected on B_analytical, as the
 * reference does (:314), where xpic_paired_trace, which has no analytical member, projects on B_grid.  Every maximum is
 * m = (m < e) ? e : m: an error that is not a number leaves it alone, an infinite one is kept; |B| = 0 gets no special case.
 * stats_7 [n][XPIC_TRIPLET_NSTATS] (required, in and out): each triplet's running maxima {B, gradB, pos, z, p_parallel, mu,
 * energy}, ComparisonStats' order, read as the maxima so far.  curve_7 [steps / sample_every][7] (or NULL; needs
 * sample_every >= 1): curve_7[k][j] = the maximum over the triplets of error j at step (k + 1) sample_every of this call,
 * 0 where no triplet has an error > 0; written, not accumulated.  dkm_* (required), dkg_* (required with the grid) and
 * fo_* (XPIC_FO_CN: required; otherwise optional and zeroed) are the counters of the three closed traces.
 * with_grid == 0 is the grid-less pair, the analytic centre beside the orbit (drift_kinetic_push_ex9.cpp): there is no
 * grid member; state_grid_6, dkg_* and gradB_field are not read (NULL / -1 will do); statistics 0 .. 2 are neither read
 * nor written, in stats_7 and (left 0) in curve_7; statistics 3 .. 6 have the analytic centre in the grid centre's
 * place; no grid vector is read, so any context is accepted, z-slabs included.  With with_grid != 0: single z-slab contexts
 * only, as for xpic_paired_trace.
 * Checks: those of xpic_paired_trace (dk->maxit within 1 .. XPIC_TRIPLET_DK_MAXIT, fo->dt == dk->dt, fo->qm == dk->qm) and
 * those of the model traces on `model`.  n == 0 succeeds and touches nothing; steps == 0 returns the inputs.  Launches of
 * at most XPIC_TRIPLET_LAUNCH_STEPS steps.  A triplet is never removed: the region rule is not part of this call.
 * Guarantees, all bit for bit: (a) each member is its closed trace over the same steps -- state_model_6 and dkm_* those of
 * xpic_model_drift_kinetic_trace with XPIC_GEOM_NONE, state_grid_6 and dkg_* those of xpic_drift_kinetic_trace, p_6 and
 * fo_* those of xpic_model_full_orbit_trace with XPIC_GEOM_NONE; (b) a call of s1 + s2 steps equals a call of s1 steps
 * followed by one of s2 steps fed the first call's states and stats_7, in all states and in stats_7; (c) curve_7[k][j] is
 * the maximum over q of the error that triplet q alone has at that step; (d) with with_grid == 0, columns 0 .. 2 of stats_7
 * come back exactly as they went in. */
#define XPIC_TRIPLET_NSTATS 7 /* {B, gradB, pos, z, p_parallel, mu, energy}: ComparisonStats' order */
#define XPIC_TRIPLET_LAUNCH_STEPS 64
#define XPIC_TRIPLET_DK_MAXIT 1024
int xpic_triplet_trace(xpic_ctx* ctx, int64_t n, const xpic_fo_params* fo, const xpic_dk_params* dk,
  const xpic_field_model* model, int with_grid, int gradB_field, int64_t steps, int64_t sample_every, double* p_6,
  double* state_model_6, double* state_grid_6, double* stats_7, double* curve_7, int64_t* fo_iterations_sum,
  int* fo_iterations_max, int64_t* dkm_iterations_total, int* dkm_iterations_max, int64_t* dkg_iterations_total,
  int* dkg_iterations_max);

/* ---- z-slab decomposition (DMDA da_processors_z = nranks; src/utils/world.cpp:36-38).  A context created with
 * nranks > 1 owns planes [rank*nz/nranks, (rank+1)*nz/nranks) and must be given a communicator before any
 * call that moves data between slabs (steps, solves, operator applies, re-binning, energy): those calls are
 * collective over the ranks.  Replaces update_cells_mpi (src/interfaces/particles.cpp:118-248), DMGlobalToLocal /
 * DMLocalToGlobal(ADD) and the all-reduces inside VecDot/VecNorm/KSPSolve. */
/* RCCL over xGMI: rank 0 creates the id, every rank (one process per GPU) passes the same 128 bytes */
int xpic_comm_rccl_unique_id(void* id128);
int xpic_comm_init_rccl(xpic_ctx* ctx, const void* id128);
/* host-staged transport supplied by the caller (tests: torch.distributed/gloo).  Ring semantics: send `down` to
 * rank-1 and `up` to rank+1; receive the upper neighbour's `down` message into from_up and the lower neighbour's
 * `up` message into from_down (with 2 ranks both neighbours are the same peer: messages are matched in this order) */
typedef struct xpic_comm_callbacks {
  void* user;
  int (*sendrecv)(void* user, const void* down, size_t ndown, const void* up, size_t nup, void* from_up,
    size_t nfrom_up, void* from_down, size_t nfrom_down);
  int (*allreduce_sum)(void* user, double* buf, int n);
} xpic_comm_callbacks;
int xpic_comm_init_callbacks(xpic_ctx* ctx, const xpic_comm_callbacks* cb);
/* number of ranks of the attached communicator: ncclCommCount for RCCL, the z-slab count for callbacks, 1 without one
 * (MPI_Comm_size on PETSC_COMM_WORLD, src/utils/world.cpp:40-42) */
/* Copy-engine path for the one large message of a step, the matL ghost rows (C11, MatSetValuesCOO's off-process entries,
 * src/impls/ecsim/simulation.cpp:366): every rank publishes a blob describing the buffers its z-neighbours write into
 * (xpic_comm_peer_export: IPC handles, hipIpcGetMemHandle), the caller carries the blobs to the neighbours over its bootstrap
 * channel (as it carries the ncclUniqueId), and each rank maps its lower and its upper neighbour's buffer
 * (xpic_comm_peer_import: hipIpcOpenMemHandle; ranks that are threads of one process, and a self-ring, use the addresses).
 * With bit 2 of xpic_set_overlap the ghost rows then travel as hipMemcpyAsync on a copy stream -- between two GPUs an SDMA
 * engine: no workgroup slot is taken from the assembly's colour launches they run beside -- and the rank's next ring
 * exchange, issued behind the copies, is the neighbour's arrival signal.  RCCL (or the callbacks) keep every other message. */
#define XPIC_PEER_BLOB_BYTES 256
int xpic_comm_peer_export(xpic_ctx* ctx, void* blob /* XPIC_PEER_BLOB_BYTES */);
int xpic_comm_peer_import(xpic_ctx* ctx, const void* lower_blob, const void* upper_blob);
int xpic_comm_size(xpic_ctx* ctx, int* nranks);
/* traffic of this rank since the last reset: out4 = {point-to-point messages sent, bytes sent, all-reduces, their payload
 * bytes} -- what a step puts on the links (the reference's MPI / PetscSF traffic) */
int xpic_comm_stats(xpic_ctx* ctx, int64_t* out4, int reset);

/* ---- measurement: HIP-event timers around kernel families, on the context's own stream */
int xpic_profile_enable(xpic_ctx* ctx, int on);
int xpic_profile_reset(xpic_ctx* ctx);
/* name: "matA_apply","matL_apply","matM_apply","fill_current","move_bin","scatter","second_push",... */
int xpic_profile_get(xpic_ctx* ctx, const char* name, int64_t* launches, double* total_ms);
/* device copy bandwidth probe (bytes moved / s) measured with a float4-style copy kernel */
int xpic_probe_copy_bandwidth(xpic_ctx* ctx, int64_t bytes, int reps, double* bytes_per_s);

#ifdef __cplusplus
}
#endif
/* ---- SetParticles on the device and the builder's particle count: their entry points and their definition */
#include "xpic_set_particles.h"
/* ---- tracer sets that live on the device and ride along with the step, and grad |F| of a grid vector */
#include "xpic_tracers.h"
/* ---- the moments of a tracer set on the grid, once or accumulated into maps on the device */
#include "xpic_tracer_moments.h"
/* ---- field lines of a grid vector or of an analytic model, traced on the device */
#include "xpic_field_lines.h"
/* ---- Gauss's law on the device: its residual and a cleaner (a scalar Poisson CG) */
#include "xpic_gauss.h"
/* ---- the electrostatic scheme XPIC_ES: Boris push, fused charge deposit, Poisson solve */
#include "xpic_es.h"
/* ---- the direct Poisson solve for the cleans and the XPIC_ES step: a separable Hartley transform */
#include "xpic_poisson.h"
/* ---- field spectra on the device: power, axis and shell sums, single modes, a probe that rides with the step */
#include "xpic_spectrum.h"
#endif
