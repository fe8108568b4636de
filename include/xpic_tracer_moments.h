/* xpic_tracer_moments.h -- moments of a tracer set on the grid: the six DistributionMoment moments of the set's live
 * particles, once (xpic_tracers_moment) or accumulated on the device while the set advances or rides (the maps): the
 * residence-time estimate of the density, current and pressure of a test-particle ensemble (an extension: the reference
 * has neither).  Included by xpic_hip.h after xpic_tracers.h; include that header.  (The entry points
 * stand here and in the package's TRACER_MOMENT_PROTOTYPES, as those of xpic_field_lines.h stand in
 * FIELD_LINE_PROTOTYPES; tests/test_abi_tracer_moments.py holds the two to each other.)
 *
 * xpic_tracers_moment: xpic_moment's result for the particles of the set as they stand.  kind: an enum xpic_moment_kind;
 * out[nz][ny][nx][dof] and the cell-centred first-order deposit over 2 x 2 x 2 cells from round(r / d - 1) are
 * xpic_moment's; `weight` stands where n / Np stands for a sort, and q and m are arguments (a set has only qm / mp).
 *   live:    a particle is live iff its exit_step is < 0 when the call is made.  The open traces test a particle at the top
 *            of a step: one whose exit_step will be k has made k steps and still counts after step k, its last; after
 *            step k + 1 it does not.
 *   region:  region6 = {start xyz, size xyz} in cells, NULL: the whole box, checked as xpic_moment's.  The storage cell of
 *            a tracer is floor(r / d) per axis of the position as it is, not folded: the cell the region rule of the
 *            open traces tests.  A live particle counts iff that cell lies in the region; a position outside [0, L)
 *            (a set without a trace region may hold any) or one that is not a number does not count.  A deposit is
 *            wrapped once on the axes the region spans in full and dropped outside the region, as xpic_moment's.
 *   counted: (may be NULL) the particles that counted.
 * Full-orbit sets: v is the record's velocity and the per-particle value is xpic_moment's, cylindrical kinds included.
 * Drift-kinetic sets: b = B(r) / |B(r)| per component, B the second-order staggered gather the field-line tracer takes
 * of XPIC_B (xpic_field_lines.h) at the guiding centre, |B| = sqrt((Bx Bx + By By) + Bz Bz); b = 0 where |B| is 0.  The
 * record's p_parallel and p_perp are velocities, as everywhere in this library.  Values:
 *     density                 1
 *     current                 q p_parallel b_i                    (the guiding-centre drifts are left out)
 *     momentum_flux           m (p_parallel^2 b_i b_j + p_perp^2 / 2 (delta_ij - b_i b_j))   (the gyro-averaged tensor)
 *     momentum_flux_diag      its diagonal
 *     the _cyl kinds          the same with b rotated into (r, phi, z) about (geom_x / 2, geom_y / 2) as xpic_moment
 *                             rotates v; a guiding centre on the axis keeps the Cartesian components
 * The call changes nothing in the set, is legal at any point of its life, and gives zeros for a set with n == 0.  The sums
 * are float64 atomic adds: their last bits depend on the order of arrival.  Uses the scratch vectors xpic_moment uses.
 *
 * Maps.  A map is a float64 accumulator [dof][nz][ny][nx] on the device that its set owns.  Whenever the set's step
 * count since creation reaches a multiple of `every` (>= 1), the moment of the set at that point -- xpic_tracers_moment
 * with the map's kind, q, m, weight and region6 -- is added into it, however the steps were split into xpic_tracers_advance
 * calls and rides.  A map made on a set that has made steps already takes the later due steps only.
 * xpic_tracers_map_get: out in xpic_moment's layout [nz][ny][nx][dof] (may be NULL), so that out / deposits is a time
 * average laid out as a DistributionMoment; info3 (may be NULL) = {deposits made, particle-deposits counted (the sum of
 * the deposits' `counted`), the set's step count}; reset != 0 zeroes the map and its two counters after the copy.
 * Maps are passive: state, exit_step, counters, sample rows and alive of a set with maps are, bit for bit, those of the
 * same set without; a context whose sets have no maps launches what it launched before maps existed.
 * Limits: at most XPIC_TRACERS_MAX_MAPS maps per set, map ids are not reused within a set; xpic_tracers_destroy and
 * xpic_destroy free the maps that are left.  Contexts of several z-slabs (or self_ring) are refused, as by the sets; a
 * set or map id that does not exist and a kind outside the enum are errors with a message in every call.
 * Not offered: a deposit fused into the trace kernels; velocity distributions of a set; the drift currents; any deposit
 * that the run reads (charge, current, mass matrix). */
#ifndef XPIC_TRACER_MOMENTS_H
#define XPIC_TRACER_MOMENTS_H
#ifdef __cplusplus
extern "C" {
#endif
#define XPIC_TRACERS_MAX_MAPS 4
/* xpic_debug_set(ctx, XPIC_DEBUG_TRACER_MOMENT_LDS, v): the deposit's workgroup-private copy of the region is used when
 * region cells x dof <= v doubles (0: never, every deposit goes straight to memory; the default is the kernel's budget,
 * which is also the largest value).  The results agree up to the order of the sums; only the code path changes. */
#define XPIC_DEBUG_TRACER_MOMENT_LDS 3
int xpic_tracers_moment(xpic_ctx* ctx, int set, int kind, double q, double m, double weight, const int region6[6], double* out,
  int64_t* counted);
int xpic_tracers_map_create(xpic_ctx* ctx, int set, int kind, double q, double m, double weight, const int region6[6],
  int64_t every, int* map);
int xpic_tracers_map_get(xpic_ctx* ctx, int set, int map, double* out, int64_t info3[3], int reset);
int xpic_tracers_map_destroy(xpic_ctx* ctx, int set, int map);
#ifdef __cplusplus
}
#endif
#endif
