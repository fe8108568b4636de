/* xpic_field_lines.h -- field lines of a grid vector or of an analytic model, traced on the device (an extension: the
 * reference has no field-line tracer).  Included by xpic_hip.h, which defines xpic_trace_region and
 * xpic_field_model; include that header.  (The entry points stand here and in the package's FIELD_LINE_PROTOTYPES, as
 * those of xpic_tracers.h stand in TRACER_PROTOTYPES; tests/test_abi_field_lines.py holds the two to each other.)
 *
 * One lane follows one line from one seed in one direction s = +1 or -1: dr/dl = s F(r) / |F(r)|, classical RK4 at the
 * fixed arc-length step h, in float64, operation by operation as written below (no contraction outside the gather):
 *     |F| = sqrt((Fx Fx + Fy Fy) + Fz Fz),   t(r) = s (F(r) / |F(r)|)   per component
 *     t1 = t(r), t2 = t(r + (h / 2) t1), t3 = t(r + (h / 2) t2), t4 = t(r + h t3)
 *     r' = r + (h / 6) (((t1 + 2 t2) + 2 t3) + t4)
 *     length' = length + h,   volume' = volume + (h / 2) (1 / f0 + 1 / f1),   f0 = |F|(r), f1 = |F|(r')
 * F(r') is the next step's F(r): a step costs four evaluations.  fmin, fmax and smin (the length at which fmin was first
 * seen) run over the seed and every point a step reached.  With no step taken they are |F| at the seed (+inf, 0, 0 when that
 * is not a number).
 * Grid form: F is the second-order staggered gather the full-orbit tracers take of XPIC_B (stagger XPIC_STAGGER_B: for B,
 * B0 and any vector filled like B) or of XPIC_E (XPIC_STAGGER_E), node indices wrapped; positions are not folded.
 * Model form: F is B (component XPIC_STAGGER_B) or E (XPIC_STAGGER_E) of the model at r.
 * A lane stops with a code and keeps the state it had at the start of the step it did not take:
 *     XPIC_LINE_MAXSTEPS  max_steps steps are taken (this test comes first: the point after the last step is not tested);
 *     XPIC_LINE_LEFT      the cell of the point the step would start from fails the region (the open traces' rule:
 *                         the corner floor(r / d) d of the unfolded position; region NULL: only a position that is
 *                         not a number fails);
 *     XPIC_LINE_NULL      |F| at the seed, at a stage or at the point the step would reach is below f_floor, is 0 or is
 *                         not finite;
 *     XPIC_LINE_CLOSED    only with close_tol > 0: after 2 or more steps the point reached lies within close_tol (<=) of
 *                         the seed; the closing step, which passes the seed, is then taken and counted (it can end in
 *                         one of the codes above instead).  With close_tol = h a circle of circumference C closes
 *                         after ceil(C / h) steps.
 * directions: 1 follows +F, 2 follows -F, 3 both.  Every output is [2][n], direction major (row 0: +, row 1: -); the
 * row of a direction that was not asked for is neither read nor written.  end3 [2][n][3], length, volume, fmin, smin,
 * fmax, steps (int64), code (int32): all required.  samples (with sample_every >= 1; NULL and 0: none):
 * [2][n][nsamp][3], nsamp = max_steps / sample_every, row k the point after step (k + 1) sample_every; the rows behind a
 * lane's last step repeat its last point.
 * The lanes stay on the device and advance in launches of at most launch_steps steps (0: XPIC_LINES_LAUNCH_STEPS) until
 * every lane has a code; 8 bytes come back after each launch.  No output depends on launch_steps.
 * Checks, each refused with a message: null pointers, n < 0, h <= 0 or not finite, max_steps outside 1 .. 2^24, f_floor or
 * close_tol negative or not a number, stagger / component, directions, launch_steps < 0, sample_every < 0 or without
 * samples, an unknown or unallocated field id, a bad model, a bad region (region->compact and step0 are not read beyond
 * the open traces' checks).  n == 0 succeeds and touches nothing.  The grid form takes single z-slab contexts only, the
 * model form any context.  The calls write nothing but their outputs. */
#ifndef XPIC_FIELD_LINES_H
#define XPIC_FIELD_LINES_H
#ifdef __cplusplus
extern "C" {
#endif
#define XPIC_LINES_LAUNCH_STEPS 256
#define XPIC_LINES_MAX_STEPS 16777216
#define XPIC_STAGGER_B 0
#define XPIC_STAGGER_E 1
#define XPIC_LINE_RUNNING (-1)
#define XPIC_LINE_MAXSTEPS 0
#define XPIC_LINE_LEFT 1
#define XPIC_LINE_NULL 2
#define XPIC_LINE_CLOSED 3
typedef struct xpic_line_params {
  double h;
  int64_t max_steps;
  double f_floor;
  double close_tol;
  int32_t stagger;
  int32_t directions;   /* 1: +, 2: -, 3: both */
  int32_t launch_steps;
  int32_t component;    /* model form: B or E */
} xpic_line_params;
int xpic_field_lines(xpic_ctx* ctx, int field, int64_t n, const double* seeds3, const xpic_line_params* params,
  const xpic_trace_region* region, int64_t sample_every, double* end3, double* length, double* volume, double* fmin,
  double* smin, double* fmax, int64_t* steps, int32_t* code, double* samples);
int xpic_model_field_lines(xpic_ctx* ctx, const xpic_field_model* model, int64_t n, const double* seeds3,
  const xpic_line_params* params, const xpic_trace_region* region, int64_t sample_every, double* end3, double* length,
  double* volume, double* fmin, double* smin, double* fmax, int64_t* steps, int32_t* code, double* samples);
#ifdef __cplusplus
}
#endif
#endif
