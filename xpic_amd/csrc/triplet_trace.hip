// triplet_trace.hip -- the time loop of the reference's grid tests for a batch: a guiding centre on an
// analytic field model, a guiding centre on the grid filled from that model, and a full orbit on the model, advanced in
// lock-step in one lane, and the reference's comparison of the three kept on the device:
//   tests/drift_kinetic_push/drift_kinetic_grid_boris_ex1..4.cpp (ex1.cpp:79-98: push_analytical.process, push_grid.process,
//   boris_step, get_analytical_fields, esirkepov.interpolate, update_comparison_stats)
//   ComparisonStats / update_comparison_stats   tests/drift_kinetic_push/drift_kinetic_push.h:253-329, all seven maxima
// One lane per triplet, fp64.  The three steps are dk_process on ModelSource as in k_model_dk_trace, dk_process on DKGrid
// as in k_dk_trace, and fo_step / fo_cn_process on ModelSource as in k_model_fo_trace: the three states and all six
// iteration counters are those of the closed traces, bit for bit.  After every step the seven errors {B, gradB, pos, z,
// p_parallel, mu, energy} are formed.  The last four are pair_compare.h's pair_errors of the grid centre and the orbit,
// but with B = B_analytical (drift_kinetic_push.h:314) where xpic_paired_trace, which has no analytical member, projects
// on B_grid.  Maxima, curve and their rule (m = (m < e) ? e : m) are k_pair_trace's: stats[j * n + q] read on entry so that
// calls compose; at a sampled step a wave maximum per statistic, one LDS slot per row, statistic and wave, one barrier that
// every thread reaches, and one global atomicMax per row and statistic on the value's bit pattern.
// GRID = false is the grid-less pair (drift_kinetic_push_ex9.cpp's comparison of DriftKineticPush with a full orbit on the
// Gaussian mirror): no grid member, no grid vector read, statistics 0 .. 2 neither read nor written, and the analytic
// centre in the grid centre's place in statistics 3 .. 6.
// Every loop is bounded by a constant or by an argument the entry point has range-checked: at most 4 nodes per axis,
// fo maxit <= XPIC_FO_MAXIT, 1 <= dk maxit <= XPIC_TRIPLET_DK_MAXIT, at most XPIC_TRIPLET_LAUNCH_STEPS steps and
// kOpenRows rows per launch.  Every global index is formed under q < n or row < nsamp.  With the grid: single z-slab
// contexts only (G == 0: every index wraps).  The staging is batch.h's batch_triplet_trace.
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
constexpr int kLaunchSteps = XPIC_TRIPLET_LAUNCH_STEPS;
constexpr int kStats = XPIC_TRIPLET_NSTATS;
static_assert(kLaunchSteps <= kOpenRows, "the curve holds one LDS row per step of a launch");

// (a - b).length()
__device__ inline double dist3(const double* a, const double* b)
{
  const double d[3] = {a[0] - b[0], a[1] - b[1], a[2] - b[2]};
  return len3(d);
}

// steps first + 1 .. first + nsteps of a triplet trace, in place; nsteps <= kLaunchSteps.  Step k (counted from 1 over the
// call) is a sample when sample_every divides it: row k / sample_every - 1 of curve[nsamp][7] (null: no curve), which the
// host has zeroed.  stats holds the columns J0 .. 6 as [7 - J0][n], J0 = 0 with the grid and 3 without.  The fo counters are
// read and written by the CN instance only, dg_s and the dg counters by the GRID instances only.  Every thread reaches the
// barrier.
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

// the checks of pair_check (paired_trace.hip) and of the model traces (model_trace.hip); the grid's only with the grid
int triplet_check(xpic_ctx* ctx, int64_t n, const xpic_fo_params* F, const xpic_dk_params* D, const xpic_field_model* model,
  bool with_grid, int gradB_field, const double** gradB)
{
  XPIC_CHECK(ctx != nullptr, "null context");
  XPIC_CHECK(n >= 0, "triplet_trace: n is negative");
  XPIC_CHECK(n <= ((int64_t)1 << 36), "triplet_trace: n is larger than 2^36");
  XPIC_CHECK(F, "triplet_trace: fo (the full orbit's params) is null");
  XPIC_CHECK(D, "triplet_trace: dk (the guiding centres' params) is null");
  XPIC_CHECK(F->scheme >= 0 && F->scheme < XPIC_FO_NSCHEMES, "triplet_trace: unknown scheme id");
  if (F->scheme == XPIC_FO_CN)
    XPIC_CHECK(F->maxit >= 1 && F->maxit <= XPIC_FO_MAXIT, "triplet_trace: fo maxit must be within 1 .. 64");
  XPIC_CHECK(D->maxit >= 1 && D->maxit <= XPIC_TRIPLET_DK_MAXIT, "triplet_trace: dk maxit must be within 1 .. 1024");
  XPIC_CHECK(D->mp != 0.0, "triplet_trace: mp must not be 0");
  XPIC_CHECK(F->dt == D->dt, "triplet_trace: fo->dt and dk->dt differ: the triplet advances in lock-step");
  XPIC_CHECK(F->qm == D->qm, "triplet_trace: fo->qm and dk->qm differ: the triplet is one particle");
  const char* bad = model_check(model);
  XPIC_CHECK(!bad, std::string("triplet_trace: ") + (bad ? bad : ""));
  *gradB = nullptr;
  if (!with_grid) return 0;
  XPIC_CHECK(ctx->geom.nranks == 1 && ctx->g.G == 0,
    "triplet_trace: with the grid member a context of several z-slabs (or a self_ring one) is not supported: the gathers "
    "wrap z in the kernel");
  XPIC_CHECK(ctx->field[XPIC_E] && ctx->field[XPIC_B], "triplet_trace: the context has no E or B");
  XPIC_CHECK(gradB_field == -1 || (gradB_field >= 0 && gradB_field < XPIC_NFIELDS && ctx->field[gradB_field]),
    "triplet_trace: gradB_field is neither -1 nor an allocated field id");
  if (gradB_field != -1) *gradB = ctx->field[gradB_field];
  return 0;
}

template <bool GRID, bool GRAD, bool CN>
void triplet_launch(xpic_ctx* ctx, const double* gradB, const xpic_field_model& M, const xpic_fo_params& F,
  const xpic_dk_params& D, int64_t n, double* fo_s, double* dm_s, double* dg_s, double* st, long first, int ns,
  int64_t sample_every, int64_t nsamp, unsigned long long* cv, long long* fo_sum, int* fo_max, long long* dm_sum, int* dm_max,
  long long* dg_sum, int* dg_max)
{
  hipLaunchKernelGGL((k_triplet_trace<GRID, GRAD, CN>), lane_grid(n), dim3(kBlock), 0, ctx->stream, ctx->g,
    GRID ? ctx->field[XPIC_E] : nullptr, GRID ? ctx->field[XPIC_B] : nullptr, gradB, M, F, D, (long)n, fo_s, dm_s, dg_s, st,
    first, ns, (long)sample_every, (long)nsamp, cv, fo_sum, fo_max, dm_sum, dm_max, dg_sum, dg_max);
}

}  // namespace

}  // namespace xpic

using namespace xpic;

extern "C" {

int xpic_triplet_trace(xpic_ctx* ctx, int64_t n, const xpic_fo_params* fo, const xpic_dk_params* dk,
  const xpic_field_model* model, int with_grid, int gradB_field, int64_t steps, int64_t sample_every, double* p_6,
  double* state_model_6, double* state_grid_6, double* stats_7, double* curve_7, int64_t* fo_iterations_sum,
  int* fo_iterations_max, int64_t* dkm_iterations_total, int* dkm_iterations_max, int64_t* dkg_iterations_total,
  int* dkg_iterations_max)
{ // the time loop of drift_kinetic_grid_boris_ex1.cpp:79-98 for n triplets
  const bool grid = with_grid != 0;
  const double* gradB;
  XPIC_CALL(triplet_check(ctx, n, fo, dk, model, grid, gradB_field, &gradB));
  const bool cn = fo->scheme == XPIC_FO_CN;
  XPIC_CHECK(steps >= 0, "triplet_trace: steps is negative");
  XPIC_CHECK(!curve_7 || sample_every >= 1, "triplet_trace: sample_every must be >= 1 when curve_7 is asked for");
  XPIC_CHECK(p_6, "triplet_trace: p_6 is null");
  XPIC_CHECK(state_model_6, "triplet_trace: state_model_6 is null");
  XPIC_CHECK(state_grid_6 || !grid, "triplet_trace: state_grid_6 is null");
  XPIC_CHECK(stats_7, "triplet_trace: stats_7 is null");
  XPIC_CHECK(fo_iterations_sum || !cn, "triplet_trace: fo_iterations_sum is null");
  XPIC_CHECK(fo_iterations_max || !cn, "triplet_trace: fo_iterations_max is null");
  XPIC_CHECK(dkm_iterations_total, "triplet_trace: dkm_iterations_total is null");
  XPIC_CHECK(dkm_iterations_max, "triplet_trace: dkm_iterations_max is null");
  XPIC_CHECK(dkg_iterations_total || !grid, "triplet_trace: dkg_iterations_total is null");
  XPIC_CHECK(dkg_iterations_max || !grid, "triplet_trace: dkg_iterations_max is null");
  const int64_t nsamp = curve_7 ? steps / sample_every : 0;
  XPIC_CHECK(nsamp <= ((int64_t)1 << 40), "triplet_trace: the curve (56 steps / sample_every bytes) is too large");
  if (n == 0) return 0;
  const bool grad = gradB != nullptr;
  XPIC_CALL(batch_triplet_trace(ctx, "triplet_trace", kLaunchSteps, n, steps, nsamp, cn, grid, p_6, state_model_6,
    state_grid_6, stats_7, curve_7, fo_iterations_sum, fo_iterations_max, dkm_iterations_total, dkm_iterations_max,
    dkg_iterations_total, dkg_iterations_max,
    [&](double* fo_s, double* dm_s, double* dg_s, double* st, long first, int ns, unsigned long long* cv, long long* fo_sum,
      int* fo_max, long long* dm_sum, int* dm_max, long long* dg_sum, int* dg_max) {
      auto launch = !grid ? (cn ? triplet_launch<false, false, true> : triplet_launch<false, false, false>)
                    : grad ? (cn ? triplet_launch<true, true, true> : triplet_launch<true, true, false>)
                           : (cn ? triplet_launch<true, false, true> : triplet_launch<true, false, false>);
      launch(ctx, gradB, *model, *fo, *dk, n, fo_s, dm_s, dg_s, st, first, ns, sample_every, nsamp, cv, fo_sum, fo_max,
        dm_sum, dm_max, dg_sum, dg_max);
    }));
  // a Chin id has no iterations: its launches get null counters, and the caller's are zeroed here
  if (!cn) {
    if (fo_iterations_sum) std::fill(fo_iterations_sum, fo_iterations_sum + n, (int64_t)0);
    if (fo_iterations_max) std::fill(fo_iterations_max, fo_iterations_max + n, 0);
  }
  return 0;
}

}  // extern "C"
