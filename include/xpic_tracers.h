/* xpic_tracers.h -- tracer sets: batches of test particles that the context owns, that stay on the device and that can
 * ride along with xpic_step; and grad |F| of a grid vector, which the guiding-centre sets need of an evolving B.  Included
 * by xpic_hip.h, which defines xpic_fo_params, xpic_dk_params and xpic_trace_region; include that header.  (The entry
 * points stand here and in the package's TRACER_PROTOTYPES, not in xpic_hip.h and PROTOTYPES: tests/test_abi.py holds those
 * two to a fixed list of calls on a null context, and tests/test_abi_tracers.py holds these to the same rules.)
 *
 * xpic_grad_abs_field: for every node and every axis c
 *     dst[node][c] = (|F|(node + e_c) - |F|(node - e_c)) / (2 d_c),   |F| = sqrt((Fx Fx + Fy Fy) + Fz Fz)
 * of the three components of src stored at the node -- the collocated view the gathers of the traces take -- in float64,
 * operation by operation as written (no contraction), neighbour indices wrapped periodically.  At an extent of 2 (or 1)
 * the two neighbours are one node and the component is exactly 0.  src and dst: any two different xpic_field ids; src is
 * only read.  Single z-slab contexts only, like the traces that read the result.
 *
 * A tracer set is a batch of n Point records {r, v} (XPIC_TRACERS_FULL_ORBIT, params: an xpic_fo_params) or PointByField
 * records {r, p_parallel, p_perp, mu_p} (XPIC_TRACERS_DRIFT_KINETIC, params: an xpic_dk_params) with, per particle,
 * exit_step and the sum and maximum of its iteration counts; with a step counter, the list of its live particles and a
 * sample buffer of sample_capacity rows.  All of it lives on the device from xpic_tracers_create to xpic_tracers_destroy.
 * A set is advanced by the kernels of xpic_full_orbit_trace_open / xpic_drift_kinetic_trace_open, on the context's E and
 * B as they stand when it is advanced:
 *  (1) equality: state, exit_step, counters, sample rows, alive and the removed count of a set that has made s steps are,
 *      bit for bit, what the open trace returns for the same batch (every exit_step -1), params, region (step0 and compact
 *      included), sample_every, steps = s and the same fields, for every scheme and every compact policy;
 *  (2) composition: xpic_tracers_advance(a) then (b) equals (a + b), sample rows included: a row is taken after every step
 *      whose count since the set was created is a multiple of sample_every, however the steps were split into calls;
 *  (3) riding: while a set is attached, every successful xpic_step advances it by one step after the step's last field
 *      update, on the XPIC_E and XPIC_B the step leaves behind; attached sets advance in the order they were created.  A
 *      context without an attached set runs xpic_step as it always did: the same launches, the same bits.  Tracers are
 *      passive: an advance writes the set's own buffers (and, for XPIC_GRADB_AUTO, a vector of the set layer's own) and
 *      nothing a sort, a field or the solver reads.
 * region: an xpic_trace_region, or NULL: no region, every finite position stays and nothing is read back between the
 * launches (step0 = 0; a position that is not a number has no cell and is retired, as in the open traces).  region->step0
 * seeds the step counter that exit_step is counted in.  xpic_tracers_create takes no exit_step: every particle enters
 * alive, and one whose cell fails the region when the set is first advanced gets exit_step = step0 and is returned
 * untouched.
 * gradB_field (drift kinetic only; ignored for full orbits): an xpic_field id whose vector the caller fills, -1 for
 * grad B = 0, as in the drift-kinetic calls; or XPIC_GRADB_AUTO: before every advance (and every ride) the set layer calls
 * the kernel of xpic_grad_abs_field on XPIC_B, into a vector it allocates for itself on first use, which no field id names.
 * sample_every 0: no samples.  When sample_capacity rows are held, further rows are counted as dropped and not stored;
 * no call fails because the buffer is full.  xpic_tracers_samples copies the held rows out, samples[(k * n + q) * 6 ..] for
 * row k as in the traces (a removed particle's state repeated in every later row) and alive[k] (either may be NULL; *count
 * rows are held, so pass room for sample_capacity rows), and empties the buffer.
 * xpic_tracers_get: any pointer may be NULL; info5 = {steps done since creation, particles removed, particles alive, sample
 * rows held, sample rows dropped since creation}.  Iteration counters of a full-orbit set with a Chin scheme are zeros.
 * Limits: at most XPIC_TRACERS_MAX_SETS sets per context; n == 0 is a set; contexts of several z-slabs (or self_ring) are
 * refused; a set id that was never given out or has been destroyed is an error with a message in every call; xpic_destroy
 * frees the sets that are left.  Ids are not reused within a context.
 * Not offered as sets: the paired, triplet, model, timed and collisional traces; contexts of several z-slabs; tracers that
 * deposit charge or current which the run reads.  The moments of a set, which nothing in the run reads, and their
 * accumulation into maps while the set advances are xpic_tracer_moments.h's. */
#ifndef XPIC_TRACERS_H
#define XPIC_TRACERS_H
#ifdef __cplusplus
extern "C" {
#endif
#define XPIC_TRACERS_MAX_SETS 8
#define XPIC_TRACERS_FULL_ORBIT 0
#define XPIC_TRACERS_DRIFT_KINETIC 1
#define XPIC_GRADB_AUTO (-2)
int xpic_grad_abs_field(xpic_ctx* ctx, int src_field, int dst_field);
int xpic_tracers_create(xpic_ctx* ctx, int kind, int64_t n, const void* params, const double* state_6,
  const xpic_trace_region* region, int gradB_field, int64_t sample_every, int64_t sample_capacity, int* set);
int xpic_tracers_advance(xpic_ctx* ctx, int set, int64_t steps);
int xpic_tracers_attach(xpic_ctx* ctx, int set, int on);
int xpic_tracers_get(xpic_ctx* ctx, int set, double* state_6, int64_t* exit_step, int64_t* iterations_sum,
  int* iterations_max, int64_t info5[5]);
int xpic_tracers_samples(xpic_ctx* ctx, int set, double* samples, int64_t* alive, int64_t* count);
int xpic_tracers_destroy(xpic_ctx* ctx, int set);
#ifdef __cplusplus
}
#endif
#endif
