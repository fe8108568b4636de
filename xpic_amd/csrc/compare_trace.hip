// compare_trace.hip -- the comparison traces: a full orbit and one or two guiding centres of the
// same particle advanced in lock-step in one lane, and the reference's comparison of them kept on the device:
//   tests/drift_kinetic_push/drift_kinetic_grid_boris_ex1..4.cpp (ex1.cpp:79-98: push_analytical.process, push_grid.process,
//   boris_step, get_analytical_fields, esirkepov.interpolate, update_comparison_stats)
//   ComparisonStats / update_comparison_stats   tests/drift_kinetic_push/drift_kinetic_push.h:253-329
// The members are a guiding centre on an analytic field model (MODEL), a guiding centre on the context's grid (GRID), and
// the full orbit, which runs on the model where there is one and on the grid otherwise:
//   xpic_paired_trace                   GRID alone: the grid / Boris half of the comparison, the four errors {z, p_parallel,
//                                       mu, energy} projected on B_grid (there is no analytical member)
//   xpic_triplet_trace                  MODEL and GRID: all seven errors {B, gradB, pos, z, p_parallel, mu, energy}, the
//                                       last four of the grid centre and the orbit with B = B_analytical
//                                       (drift_kinetic_push.h:314)
//   xpic_triplet_trace, with_grid = 0   MODEL alone, the grid-less pair (drift_kinetic_push_ex9.cpp's comparison of
//                                       DriftKineticPush with a full orbit on the Gaussian mirror): no grid vector is read,
//                                       statistics 0 .. 2 are neither read nor written, and the analytic centre stands in
//                                       the grid centre's place in statistics 3 .. 6
// One lane per pair or triplet, fp64.  The steps are dk_process on ModelSource as in k_model_dk_trace, dk_process on DKGrid
// as in k_dk_trace, and fo_step / fo_cn_process on ModelSource as in k_model_fo_trace or on the grid as in k_fo_trace: the
// states and all iteration counters are those of the closed traces, bit for bit.  After every step the errors are formed;
// their maxima over the steps stay in registers for the launch (stats[(j - J0) * n + q], read on entry so that calls
// compose), and at a sampled step the maximum over the lanes goes through a wave maximum, one LDS slot per row, statistic and wave, one barrier
// that every thread reaches, and one global atomicMax per row and statistic on the value's bit pattern: curve[row][j].
// Maxima do not depend on the order, so the curve does not depend on timing.  Every running maximum is m = (m < e) ? e : m,
// the reference's std::max(m, e): an error that is not a number leaves it alone, an infinite one is kept.
// The staging, the checks and the launch are one path for both entry points; the kernels are two texts, k_pair_trace and
// k_triplet_trace, because every shape of one text that was built moved their instructions.
// Every loop is bounded by a constant or by an argument the entry point has range-checked: at most 4 nodes per axis,
// fo maxit <= XPIC_FO_MAXIT, 1 <= dk maxit <= XPIC_PAIR_DK_MAXIT = XPIC_TRIPLET_DK_MAXIT, at most XPIC_PAIR_LAUNCH_STEPS =
// XPIC_TRIPLET_LAUNCH_STEPS steps and kOpenRows rows per launch.  Every global index is formed under q < n or row < nsamp.
// With the grid: single z-slab contexts only (G == 0: every index wraps).  The staging is batch.h's batch_compare_trace.
#include <algorithm>
#include <cmath>

#include "batch.h"
#include "common.h"
#include "device_common.h"
#include "ie_shape.h"
#include "trace_open.h"

// as in full_orbit.hip and drift_kinetic.hip: contracted per source expression only, so the step functions round here as
// they do in the closed traces
#pragma clang fp contract(on)

#include "full_orbit_step.h"
#include "drift_kinetic_step.h"
#include "model_source.h"
#include "pair_compare.h"

namespace xpic {

namespace {

constexpr int kBlock = kLaneBlock; // batch.h: lane_grid launches workgroups of this size
constexpr int kLaunchSteps = XPIC_PAIR_LAUNCH_STEPS;
constexpr int kStats = XPIC_TRIPLET_NSTATS;
constexpr int kDkMaxit = XPIC_PAIR_DK_MAXIT;
static_assert(XPIC_TRIPLET_LAUNCH_STEPS == kLaunchSteps && XPIC_TRIPLET_DK_MAXIT == kDkMaxit, "one frame for both traces");
static_assert(kLaunchSteps <= kOpenRows, "the curve holds one LDS row per step of a launch");
static_assert(4 * kOpenRows <= kBlock, "one thread per row and statistic finishes the pair's curve");

// fo_one: full_orbit.hip's (a shared helper moves both files' instructions)
template <bool CN>
__device__ inline int fo_one(const GridDev& g, const double* __restrict__ E, const double* __restrict__ B,
  const xpic_fo_params& P, FOPoint& pn)
{
  if (CN) {
    const FOPoint p0 = pn;
    return fo_cn_process(g, E, B, P.qm, P.dt, P.atol, P.rtol, P.maxit, pn, p0);
  }
  fo_step(P.scheme, g, E, B, P.qm, P.dt, pn);
  return 0;
}

// The pair on the grid: steps first + 1 .. first + nsteps of a paired trace, in place; nsteps <= kLaunchSteps.  Step k
// (counted from 1 over the call) is a sample when sample_every divides it: row k / sample_every - 1 of curve[nsamp][4]
// (null: no curve), which the host has zeroed.  The fo counters are read and written by the CN instance only.  Every thread
// reaches the barrier.
template <bool GRAD, bool CN>
__global__ void __launch_bounds__(kBlock) k_pair_trace(GridDev g, const double* __restrict__ E, const double* __restrict__ B,
  const double* __restrict__ gB, xpic_fo_params F, xpic_dk_params D, long n, double* __restrict__ fo_s,
  double* __restrict__ dk_s, double* __restrict__ stats, long first, int nsteps, long sample_every, long nsamp,
  unsigned long long* curve, long long* __restrict__ fo_sum, int* __restrict__ fo_max, long long* __restrict__ dk_sum,
  int* __restrict__ dk_max)
{
  __shared__ double sm[kOpenRows][4][kBlock / 64];
  const long q = (long)blockIdx.x * kBlock + threadIdx.x;
  const bool live = q < n;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ns = nsteps < kLaunchSteps ? nsteps : kLaunchSteps;
  int nrows = 0;
  long r0 = 0;
  if (curve) {
    r0 = first / sample_every;                 // the first row whose step lies behind `first`
    long r1 = (first + ns) / sample_every;     // one past the last row whose step the launch reaches
    r1 = r1 < nsamp ? r1 : nsamp;
    nrows = r1 > r0 ? (int)(r1 - r0) : 0;
    nrows = nrows < kOpenRows ? nrows : kOpenRows;
  }
  FOPoint fo;
  DKPoint p0, pn;
  double m[4] = {0.0, 0.0, 0.0, 0.0};
  long long fo_total = 0, dk_total = 0;
  int fo_most = 0, dk_most = 0;
  if (live) {
    fo_load(fo_s, n, q, fo);
    dk_load(dk_s, n, q, pn);
#pragma unroll
    for (int j = 0; j < 4; ++j) m[j] = stats[j * n + q];
    if (CN) { fo_total = fo_sum[q]; fo_most = fo_max[q]; }
    dk_total = dk_sum[q];
    dk_most = dk_max[q];
  }
  for (int k = 1; k <= ns; ++k) {
    double e[4] = {0.0, 0.0, 0.0, 0.0};
    if (live) {
      p0 = pn;
      const int dk_it = dk_process<GRAD>(g, E, B, gB, D, p0, pn);
      dk_total += dk_it;
      dk_most = dk_it > dk_most ? dk_it : dk_most;
      const int fo_it = fo_one<CN>(g, E, B, F, fo);
      fo_total += fo_it;
      fo_most = fo_it > fo_most ? fo_it : fo_most;
      // esirkepov.interpolate(E_grid, B_grid, gradB_grid, point_grid.r, point_grid_old.r), ex1.cpp:92-93
      double Eg[3], Bg[3], gBg[3];
      dk_fields<GRAD>(g, E, B, gB, pn.r, p0.r, Eg, Bg, gBg);
      pair_errors(pn, fo, Bg, D.mp, e);
#pragma unroll
      for (int j = 0; j < 4; ++j) m[j] = (m[j] < e[j]) ? e[j] : m[j];
    }
    const long step = first + k;
    if (curve && step % sample_every == 0) {
      const long row = step / sample_every - 1 - r0;
      if (row >= 0 && row < nrows) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const double v = wave_max((0.0 < e[j]) ? e[j] : 0.0); // a NaN, and a lane without a pair, count as 0
          if (lane == 0) sm[row][j][wave] = v;
        }
      }
    }
  }
  if (live) {
    fo_store(fo_s, n, q, fo);
    dk_store(dk_s, n, q, pn);
#pragma unroll
    for (int j = 0; j < 4; ++j) stats[j * n + q] = m[j];
    if (CN) { fo_sum[q] = fo_total; fo_max[q] = fo_most; }
    dk_sum[q] = dk_total;
    dk_max[q] = dk_most;
  }
  __syncthreads();
  if ((int)threadIdx.x < 4 * nrows) {
    const int t = (int)threadIdx.x >> 2, j = (int)threadIdx.x & 3;
    double v = sm[t][j][0];
#pragma unroll
    for (int w = 1; w < kBlock / 64; ++w) v = (v < sm[t][j][w]) ? sm[t][j][w] : v;
    if (v > 0.0) atomicMax(curve + (r0 + t) * 4 + j, (unsigned long long)__double_as_longlong(v));
  }
}

// (a - b).length()
__device__ inline double dist3(const double* a, const double* b)
{
  const double d[3] = {a[0] - b[0], a[1] - b[1], a[2] - b[2]};
  return len3(d);
}

// The triplet and its grid-less pair: steps first + 1 .. first + nsteps of a triplet trace, in place; nsteps <=
// kLaunchSteps.  Step k (counted from 1 over the call) is a sample when sample_every divides it: row k / sample_every - 1
// of curve[nsamp][7] (null: no curve), which the host has zeroed.  stats holds the columns J0 .. 6 as [7 - J0][n], J0 = 0
// with the grid and 3 without.  The fo counters are read and written by the CN instance only, dg_s and the dg counters by
// the GRID instances only.  Every thread reaches the barrier.
template <bool GRID, bool GRAD, bool CN>
__global__ void __launch_bounds__(kBlock) k_triplet_trace(GridDev g, const double* __restrict__ E,
  const double* __restrict__ B, const double* __restrict__ gB, xpic_field_model M, xpic_fo_params F, xpic_dk_params D, long n,
  double* __restrict__ fo_s, double* __restrict__ dm_s, double* __restrict__ dg_s, double* __restrict__ stats, long first,
  int nsteps, long sample_every, long nsamp, unsigned long long* curve, long long* __restrict__ fo_sum,
  int* __restrict__ fo_max, long long* __restrict__ dm_sum, int* __restrict__ dm_max, long long* __restrict__ dg_sum,
  int* __restrict__ dg_max)
{
  constexpr int J0 = GRID ? 0 : 3;
  __shared__ double sm[kOpenRows][kStats][kBlock / 64];
  const long q = (long)blockIdx.x * kBlock + threadIdx.x;
  const bool live = q < n;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ns = nsteps < kLaunchSteps ? nsteps : kLaunchSteps;
  const ModelSource src{M};
  int nrows = 0;
  long r0 = 0;
  if (curve) {
    r0 = first / sample_every;                 // the first row whose step lies behind `first`
    long r1 = (first + ns) / sample_every;     // one past the last row whose step the launch reaches
    r1 = r1 < nsamp ? r1 : nsamp;
    nrows = r1 > r0 ? (int)(r1 - r0) : 0;
    nrows = nrows < kOpenRows ? nrows : kOpenRows;
  }
  FOPoint fo;
  DKPoint m0, mn, g0, gn;
  double m[kStats] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  long long fo_total = 0, dm_total = 0, dg_total = 0;
  int fo_most = 0, dm_most = 0, dg_most = 0;
  if (live) {
    fo_load(fo_s, n, q, fo);
    dk_load(dm_s, n, q, mn);
    if (GRID) dk_load(dg_s, n, q, gn);
#pragma unroll
    for (int j = J0; j < kStats; ++j) m[j] = stats[(j - J0) * n + q];
    if (CN) { fo_total = fo_sum[q]; fo_most = fo_max[q]; }
    dm_total = dm_sum[q];
    dm_most = dm_max[q];
    if (GRID) { dg_total = dg_sum[q]; dg_most = dg_max[q]; }
  }
  for (int k = 1; k <= ns; ++k) {
    double e[kStats] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (live) {
      m0 = mn;
      const int dm_it = dk_process(src, D, m0, mn);                 // push_analytical.process, ex1.cpp:85
      dm_total += dm_it;
      dm_most = dm_it > dm_most ? dm_it : dm_most;
      if (GRID) {
        g0 = gn;
        const int dg_it = dk_process<GRAD>(g, E, B, gB, D, g0, gn); // push_grid.process, :86
        dg_total += dg_it;
        dg_most = dg_it > dg_most ? dg_it : dg_most;
      }
      int fo_it = 0;                                                // boris_step, :87
      if (CN) {
        const FOPoint p0 = fo;
        fo_it = fo_cn_process(src, F.qm, F.dt, F.atol, F.rtol, F.maxit, fo, p0);
      }
      else fo_step(F.scheme, src, F.qm, F.dt, fo);
      fo_total += fo_it;
      fo_most = fo_it > fo_most ? fo_it : fo_most;
      // get_analytical_fields(point_analytical_old.r, point_analytical.r, ...), :89-90: only rn is read
      double Ea[3], Ba[3], gBa[3];
      src.dk(mn.r, m0.r, Ea, Ba, gBa);
      if (GRID) {
        // esirkepov.interpolate(E_grid, B_grid, gradB_grid, point_grid.r, point_grid_old.r), :92-93
        double Eg[3], Bg[3], gBg[3];
        dk_fields<GRAD>(g, E, B, gB, gn.r, g0.r, Eg, Bg, gBg);
        e[0] = dist3(Ba, Bg);                                       // drift_kinetic_push.h:302
        e[1] = dist3(gBa, gBg);                                     // :305
        e[2] = dist3(mn.r, gn.r);                                   // :308
        pair_errors(gn, fo, Ba, D.mp, e + 3);                       // :311-328 with B = B_analytical (:314)
      }
      else pair_errors(mn, fo, Ba, D.mp, e + 3);
#pragma unroll
      for (int j = J0; j < kStats; ++j) m[j] = (m[j] < e[j]) ? e[j] : m[j];
    }
    const long step = first + k;
    if (curve && step % sample_every == 0) {
      const long row = step / sample_every - 1 - r0;
      if (row >= 0 && row < nrows) {
#pragma unroll
        for (int j = J0; j < kStats; ++j) {
          const double v = wave_max((0.0 < e[j]) ? e[j] : 0.0); // a NaN, and a lane without a triplet, count as 0
          if (lane == 0) sm[row][j][wave] = v;
        }
      }
    }
  }
  if (live) {
    fo_store(fo_s, n, q, fo);
    dk_store(dm_s, n, q, mn);
    if (GRID) dk_store(dg_s, n, q, gn);
#pragma unroll
    for (int j = J0; j < kStats; ++j) stats[(j - J0) * n + q] = m[j];
    if (CN) { fo_sum[q] = fo_total; fo_max[q] = fo_most; }
    dm_sum[q] = dm_total;
    dm_max[q] = dm_most;
    if (GRID) { dg_sum[q] = dg_total; dg_max[q] = dg_most; }
  }
  __syncthreads();
  // 7 kOpenRows (row, statistic) slots exceed the workgroup: the finishing pass strides over them
  for (int i = (int)threadIdx.x; i < kStats * nrows; i += kBlock) {
    const int t = i / kStats, j = i % kStats;
    if (j < J0) continue; // no slot of a grid statistic was written
    double v = sm[t][j][0];
#pragma unroll
    for (int w = 1; w < kBlock / 64; ++w) v = (v < sm[t][j][w]) ? sm[t][j][w] : v;
    if (v > 0.0) atomicMax(curve + (r0 + t) * kStats + j, (unsigned long long)__double_as_longlong(v));
  }
}

// the launch of one instance: <false, true, *, *> is the pair on the grid, <true, *, *, *> the triplet and its grid-less pair
template <bool MODEL, bool GRID, bool GRAD, bool CN>
void compare_launch(xpic_ctx* ctx, const double* gradB, const xpic_field_model& M, const xpic_fo_params& F,
  const xpic_dk_params& D, int64_t n, const CompareDev& d, long first, int ns, int64_t sample_every, int64_t nsamp)
{
  if constexpr (MODEL)
    hipLaunchKernelGGL((k_triplet_trace<GRID, GRAD, CN>), lane_grid(n), dim3(kBlock), 0, ctx->stream, ctx->g,
      GRID ? ctx->field[XPIC_E] : nullptr, GRID ? ctx->field[XPIC_B] : nullptr, gradB, M, F, D, (long)n, d.s[0], d.s[1], d.s[2],
      d.stats, first, ns, (long)sample_every, (long)nsamp, d.curve, d.it_sum[0], d.it_max[0], d.it_sum[1], d.it_max[1],
      d.it_sum[2], d.it_max[2]);
  else
    hipLaunchKernelGGL((k_pair_trace<GRAD, CN>), lane_grid(n), dim3(kBlock), 0, ctx->stream, ctx->g, ctx->field[XPIC_E],
      ctx->field[XPIC_B], gradB, F, D, (long)n, d.s[0], d.s[2], d.stats, first, ns, (long)sample_every, (long)nsamp, d.curve,
      d.it_sum[0], d.it_max[0], d.it_sum[2], d.it_max[2]);
}

// The checks of fo_check (full_orbit.hip), of dk_check (drift_kinetic.hip) and of fo_check_params / dk_check_params
// (trace_call.h), in this file's own wording, and what the comparison adds; with a model member those of the model traces (model_trace.hip); the grid's only with the grid member.  `who`
// ("paired_trace", "triplet_trace") heads every message.
int compare_check(xpic_ctx* ctx, const char* who, int64_t n, const xpic_fo_params* F, const xpic_dk_params* D,
  bool with_model, const xpic_field_model* model, bool with_grid, int gradB_field, const double** gradB)
{
  const std::string w = std::string(who) + ": ", unit = with_model ? "triplet" : "pair";
  XPIC_CHECK(ctx != nullptr, "null context");
  XPIC_CHECK(n >= 0, w + "n is negative");
  XPIC_CHECK(n <= ((int64_t)1 << 36), w + "n is larger than 2^36");
  const bool one_slab = ctx->geom.nranks == 1 && ctx->g.G == 0;
  const std::string slabs = w + (with_model ? "with the grid member " : "") +
    "a context of several z-slabs (or a self_ring one) is not supported: the gathers wrap z in the kernel";
  if (!with_model) XPIC_CHECK(one_slab, slabs); // the pair names its context before its arguments
  XPIC_CHECK(F, w + "fo (the full orbit's params) is null");
  XPIC_CHECK(D, w + "dk (the guiding " + (with_model ? "centres'" : "centre's") + " params) is null");
  XPIC_CHECK(F->scheme >= 0 && F->scheme < XPIC_FO_NSCHEMES, w + "unknown scheme id");
  if (F->scheme == XPIC_FO_CN)
    XPIC_CHECK(F->maxit >= 1 && F->maxit <= XPIC_FO_MAXIT, w + "fo maxit must be within 1 .. 64");
  XPIC_CHECK(D->maxit >= 1 && D->maxit <= kDkMaxit, w + "dk maxit must be within 1 .. 1024");
  XPIC_CHECK(D->mp != 0.0, w + "mp must not be 0");
  XPIC_CHECK(F->dt == D->dt, w + "fo->dt and dk->dt differ: the " + unit + " advances in lock-step");
  XPIC_CHECK(F->qm == D->qm, w + "fo->qm and dk->qm differ: the " + unit + " is one particle");
  if (with_model) {
    const char* bad = model_check(model);
    XPIC_CHECK(!bad, w + (bad ? bad : ""));
  }
  *gradB = nullptr;
  if (!with_grid) return 0;
  XPIC_CHECK(one_slab, slabs);
  XPIC_CHECK(ctx->field[XPIC_E] && ctx->field[XPIC_B], w + "the context has no E or B");
  XPIC_CHECK(gradB_field == -1 || (gradB_field >= 0 && gradB_field < XPIC_NFIELDS && ctx->field[gradB_field]),
    w + "gradB_field is neither -1 nor an allocated field id");
  if (gradB_field != -1) *gradB = ctx->field[gradB_field];
  return 0;
}

// a member's arrays as the entry point received them, and their names in its messages
struct NamedMember {
  double* state_6;
  int64_t* it_sum;
  int* it_max;
  const char *state_name, *sum_name, *max_name;
};

// Both entry points: the time loop of drift_kinetic_grid_boris_ex1.cpp:79-98 for n lanes.  member: the orbit, the model
// centre, the grid centre; a null model selects the pair on the grid, whose statistics are four.
int compare_trace(xpic_ctx* ctx, const char* who, const char* label, int64_t n, const xpic_fo_params* fo,
  const xpic_dk_params* dk, bool with_model, const xpic_field_model* model, bool with_grid, int gradB_field, int64_t steps,
  int64_t sample_every, const NamedMember (&member)[kCompareMembers], double* stats, double* curve)
{
  const double* gradB;
  XPIC_CALL(compare_check(ctx, who, n, fo, dk, with_model, model, with_grid, gradB_field, &gradB));
  const bool cn = fo->scheme == XPIC_FO_CN;
  const bool present[kCompareMembers] = {true, with_model, with_grid}, counted[kCompareMembers] = {cn, with_model, with_grid};
  const int width = with_model ? XPIC_TRIPLET_NSTATS : 4, j0 = with_grid ? 0 : 3;
  const std::string w = std::string(who) + ": ", suffix = std::to_string(width);
  XPIC_CHECK(steps >= 0, w + "steps is negative");
  XPIC_CHECK(!curve || sample_every >= 1, w + "sample_every must be >= 1 when curve_" + suffix + " is asked for");
  for (int m = 0; m < kCompareMembers; ++m)
    XPIC_CHECK(member[m].state_6 || !present[m], w + member[m].state_name + " is null");
  XPIC_CHECK(stats, w + "stats_" + suffix + " is null");
  for (int m = 0; m < kCompareMembers; ++m) {
    XPIC_CHECK(member[m].it_sum || !counted[m], w + member[m].sum_name + " is null");
    XPIC_CHECK(member[m].it_max || !counted[m], w + member[m].max_name + " is null");
  }
  const int64_t nsamp = curve ? steps / sample_every : 0;
  XPIC_CHECK(nsamp <= ((int64_t)1 << 40),
    w + "the curve (" + std::to_string(8 * width) + " steps / sample_every bytes) is too large");
  if (n == 0) return 0;
  CompareMember staged[kCompareMembers];
  for (int m = 0; m < kCompareMembers; ++m)
    staged[m] = {present[m] ? member[m].state_6 : nullptr, member[m].it_sum, member[m].it_max, counted[m]};
  const bool grad = gradB != nullptr;
  const xpic_field_model M = with_model ? *model : xpic_field_model{};
  auto launch = !with_grid ? (cn ? compare_launch<true, false, false, true> : compare_launch<true, false, false, false>)
    : with_model ? (grad ? (cn ? compare_launch<true, true, true, true> : compare_launch<true, true, true, false>)
                         : (cn ? compare_launch<true, true, false, true> : compare_launch<true, true, false, false>))
                 : (grad ? (cn ? compare_launch<false, true, true, true> : compare_launch<false, true, true, false>)
                         : (cn ? compare_launch<false, true, false, true> : compare_launch<false, true, false, false>));
  XPIC_CALL(batch_compare_trace(ctx, label, kLaunchSteps, n, steps, nsamp, staged, stats, width, j0, width - j0, curve, width,
    [&](const CompareDev& d, long first, int ns) { launch(ctx, gradB, M, *fo, *dk, n, d, first, ns, sample_every, nsamp); }));
  // a Chin id has no iterations: its launches get null counters, and the caller's are zeroed here
  if (!cn) {
    if (member[0].it_sum) std::fill(member[0].it_sum, member[0].it_sum + n, (int64_t)0);
    if (member[0].it_max) std::fill(member[0].it_max, member[0].it_max + n, 0);
  }
  return 0;
}

}  // namespace

}  // namespace xpic

using namespace xpic;

extern "C" {

int xpic_paired_trace(xpic_ctx* ctx, int64_t n, const xpic_fo_params* fo, const xpic_dk_params* dk, int gradB_field,
  int64_t steps, int64_t sample_every, double* p_6, double* state_6, double* stats_4, double* curve_4,
  int64_t* fo_iterations_sum, int* fo_iterations_max, int64_t* dk_iterations_total, int* dk_iterations_max)
{
  return compare_trace(ctx, "paired_trace", "pair_trace", n, fo, dk, false, nullptr, true, gradB_field, steps, sample_every,
    {{p_6, fo_iterations_sum, fo_iterations_max, "p_6", "fo_iterations_sum", "fo_iterations_max"},
      {nullptr, nullptr, nullptr, "", "", ""},
      {state_6, dk_iterations_total, dk_iterations_max, "state_6", "dk_iterations_total", "dk_iterations_max"}},
    stats_4, curve_4);
}

int xpic_triplet_trace(xpic_ctx* ctx, int64_t n, const xpic_fo_params* fo, const xpic_dk_params* dk,
  const xpic_field_model* model, int with_grid, int gradB_field, int64_t steps, int64_t sample_every, double* p_6,
  double* state_model_6, double* state_grid_6, double* stats_7, double* curve_7, int64_t* fo_iterations_sum,
  int* fo_iterations_max, int64_t* dkm_iterations_total, int* dkm_iterations_max, int64_t* dkg_iterations_total,
  int* dkg_iterations_max)
{
  return compare_trace(ctx, "triplet_trace", "triplet_trace", n, fo, dk, true, model, with_grid != 0, gradB_field, steps,
    sample_every,
    {{p_6, fo_iterations_sum, fo_iterations_max, "p_6", "fo_iterations_sum", "fo_iterations_max"},
      {state_model_6, dkm_iterations_total, dkm_iterations_max, "state_model_6", "dkm_iterations_total", "dkm_iterations_max"},
      {state_grid_6, dkg_iterations_total, dkg_iterations_max, "state_grid_6", "dkg_iterations_total", "dkg_iterations_max"}},
    stats_7, curve_7);
}

}  // extern "C"
