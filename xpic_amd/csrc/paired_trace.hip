// paired_trace.hip -- a guiding centre beside the full orbit of the same particle, advanced in lock-step in one lane, and
// the reference's comparison of the two kept on the device:
//   the loop of tests/drift_kinetic_push/drift_kinetic_grid_boris_ex1.cpp:79-98 (process, boris_step, interpolate,
//   update_comparison_stats)
//   ComparisonStats / update_comparison_stats   tests/drift_kinetic_push/drift_kinetic_push.h:253-329 (the grid / Boris
//   half: there is no analytical member here)
// One lane per pair, fp64.  The guiding centre's step is dk_process as in k_dk_trace (drift_kinetic_step.h), the orbit's is
// fo_step / fo_cn_process as in k_fo_trace (full_orbit_step.h): the two states and all four iteration counters are those
// of the closed traces, bit for bit.  After every step the four errors {z, p_parallel, mu, energy} are formed; their maxima
// over the steps stay in registers for the launch (stats[j * n + q], read on entry so that calls compose), and at a sampled
// step the maximum over the pairs goes through a wave maximum, one LDS slot per row, statistic and wave, and one global
// atomicMax per row and statistic on the value's bit pattern (a non-negative double orders as its bits): curve[row][j].
// Maxima do not depend on the order, so the curve does not depend on timing.  Every running maximum is m = (m < e) ? e : m,
// the reference's std::max(m, e): an error that is not a number leaves it alone, an infinite one is kept.
// Every loop is bounded by a constant or by an argument the entry point has range-checked: at most 4 nodes per axis,
// fo maxit <= XPIC_FO_MAXIT, 1 <= dk maxit <= XPIC_PAIR_DK_MAXIT, at most XPIC_PAIR_LAUNCH_STEPS steps and kOpenRows
// rows per launch.  Single z-slab contexts only (G == 0: every index wraps).  The staging is batch.h's batch_pair_trace.
#include <algorithm>
#include <cmath>

#include "batch.h"
#include "common.h"
#include "device_common.h"
#include "ie_shape.h"
#include "trace_open.h"

// as in full_orbit.hip and drift_kinetic.hip: contracted per source expression only, so the step functions round here as
// they do in k_fo_trace and k_dk_trace
#pragma clang fp contract(on)

#include "full_orbit_step.h"
#include "drift_kinetic_step.h"
#include "pair_compare.h"

namespace xpic {

namespace {

constexpr int kBlock = kLaneBlock; // batch.h: lane_grid launches workgroups of this size
constexpr int kLaunchSteps = XPIC_PAIR_LAUNCH_STEPS;
static_assert(kLaunchSteps <= kOpenRows, "the curve holds one LDS row per step of a launch");
static_assert(4 * kOpenRows <= kBlock, "one thread per row and statistic finishes the curve");

// fo_one: full_orbit.hip's
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

// (pair_errors, the four errors of a pair, and wave_max are pair_compare.h's)

// steps first + 1 .. first + nsteps of a paired trace, in place; nsteps <= kLaunchSteps.  Step k (counted from 1 over the
// call) is a sample when sample_every divides it: row k / sample_every - 1 of curve[nsamp][4] (null: no curve), which the
// host has zeroed.  The fo counters are read and written by the CN instance only.  Every thread reaches the barrier.
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

// the checks of fo_check (full_orbit.hip) and of dk_check / dk_check_params (drift_kinetic.hip), and what the pair adds
int pair_check(xpic_ctx* ctx, int64_t n, const xpic_fo_params* F, const xpic_dk_params* D, int gradB_field,
  const double** gradB)
{
  XPIC_CHECK(ctx != nullptr, "null context");
  XPIC_CHECK(n >= 0, "paired_trace: n is negative");
  XPIC_CHECK(n <= ((int64_t)1 << 36), "paired_trace: n is larger than 2^36");
  XPIC_CHECK(ctx->geom.nranks == 1 && ctx->g.G == 0,
    "paired_trace: a context of several z-slabs (or a self_ring one) is not supported: the gathers wrap z in the kernel");
  XPIC_CHECK(F, "paired_trace: fo (the full orbit's params) is null");
  XPIC_CHECK(D, "paired_trace: dk (the guiding centre's params) is null");
  XPIC_CHECK(F->scheme >= 0 && F->scheme < XPIC_FO_NSCHEMES, "paired_trace: unknown scheme id");
  if (F->scheme == XPIC_FO_CN)
    XPIC_CHECK(F->maxit >= 1 && F->maxit <= XPIC_FO_MAXIT, "paired_trace: fo maxit must be within 1 .. 64");
  XPIC_CHECK(D->maxit >= 1 && D->maxit <= XPIC_PAIR_DK_MAXIT, "paired_trace: dk maxit must be within 1 .. 1024");
  XPIC_CHECK(D->mp != 0.0, "paired_trace: mp must not be 0");
  XPIC_CHECK(F->dt == D->dt, "paired_trace: fo->dt and dk->dt differ: the pair advances in lock-step");
  XPIC_CHECK(F->qm == D->qm, "paired_trace: fo->qm and dk->qm differ: the pair is one particle");
  XPIC_CHECK(ctx->field[XPIC_E] && ctx->field[XPIC_B], "paired_trace: the context has no E or B");
  XPIC_CHECK(gradB_field == -1 || (gradB_field >= 0 && gradB_field < XPIC_NFIELDS && ctx->field[gradB_field]),
    "paired_trace: gradB_field is neither -1 nor an allocated field id");
  *gradB = gradB_field == -1 ? nullptr : ctx->field[gradB_field];
  return 0;
}

template <bool GRAD, bool CN>
void pair_launch(xpic_ctx* ctx, const double* gradB, const xpic_fo_params& F, const xpic_dk_params& D, int64_t n,
  double* fo_s, double* dk_s, double* st, long first, int ns, int64_t sample_every, int64_t nsamp, unsigned long long* cv,
  long long* fo_sum, int* fo_max, long long* dk_sum, int* dk_max)
{
  hipLaunchKernelGGL((k_pair_trace<GRAD, CN>), lane_grid(n), dim3(kBlock), 0, ctx->stream, ctx->g, ctx->field[XPIC_E],
    ctx->field[XPIC_B], gradB, F, D, (long)n, fo_s, dk_s, st, first, ns, (long)sample_every, (long)nsamp, cv, fo_sum, fo_max,
    dk_sum, dk_max);
}

}  // namespace

}  // namespace xpic

using namespace xpic;

extern "C" {

int xpic_paired_trace(xpic_ctx* ctx, int64_t n, const xpic_fo_params* fo, const xpic_dk_params* dk, int gradB_field,
  int64_t steps, int64_t sample_every, double* p_6, double* state_6, double* stats_4, double* curve_4,
  int64_t* fo_iterations_sum, int* fo_iterations_max, int64_t* dk_iterations_total, int* dk_iterations_max)
{ // the time loop of drift_kinetic_grid_boris_ex1.cpp:79-98 for n pairs
  const double* gradB;
  XPIC_CALL(pair_check(ctx, n, fo, dk, gradB_field, &gradB));
  const bool cn = fo->scheme == XPIC_FO_CN;
  XPIC_CHECK(steps >= 0, "paired_trace: steps is negative");
  XPIC_CHECK(!curve_4 || sample_every >= 1, "paired_trace: sample_every must be >= 1 when curve_4 is asked for");
  XPIC_CHECK(p_6, "paired_trace: p_6 is null");
  XPIC_CHECK(state_6, "paired_trace: state_6 is null");
  XPIC_CHECK(stats_4, "paired_trace: stats_4 is null");
  XPIC_CHECK(fo_iterations_sum || !cn, "paired_trace: fo_iterations_sum is null");
  XPIC_CHECK(fo_iterations_max || !cn, "paired_trace: fo_iterations_max is null");
  XPIC_CHECK(dk_iterations_total, "paired_trace: dk_iterations_total is null");
  XPIC_CHECK(dk_iterations_max, "paired_trace: dk_iterations_max is null");
  const int64_t nsamp = curve_4 ? steps / sample_every : 0;
  XPIC_CHECK(nsamp <= ((int64_t)1 << 40), "paired_trace: the curve (32 steps / sample_every bytes) is too large");
  if (n == 0) return 0;
  const bool grad = gradB != nullptr;
  XPIC_CALL(batch_pair_trace(ctx, "pair_trace", kLaunchSteps, n, steps, nsamp, cn, p_6, state_6, stats_4, curve_4,
    fo_iterations_sum, fo_iterations_max, dk_iterations_total, dk_iterations_max,
    [&](double* fo_s, double* dk_s, double* st, long first, int ns, unsigned long long* cv, long long* fo_sum, int* fo_max,
      long long* dk_sum, int* dk_max) {
      auto launch = grad ? (cn ? pair_launch<true, true> : pair_launch<true, false>)
                         : (cn ? pair_launch<false, true> : pair_launch<false, false>);
      launch(ctx, gradB, *fo, *dk, n, fo_s, dk_s, st, first, ns, sample_every, nsamp, cv, fo_sum, fo_max, dk_sum, dk_max);
    }));
  // a Chin id has no iterations: its launches get null counters, and the caller's are zeroed here
  if (!cn) {
    if (fo_iterations_sum) std::fill(fo_iterations_sum, fo_iterations_sum + n, (int64_t)0);
    if (fo_iterations_max) std::fill(fo_iterations_max, fo_iterations_max + n, 0);
  }
  return 0;
}

}  // extern "C"
