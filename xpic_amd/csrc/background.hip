// background.hip -- the background profiles of the collisional grid traces (include/xpic_hip.h:
// xpic_background_set): a spatially resolved background species, five fp64 values per local cell in the cell order of
// cell_start -- density n, thermal speed per component vth, drift u[3] -- held by the context in XPIC_TRACE_BG_MAX slots
// as one device array [5][ncell] each ({n, vth, ux, uy, uz}).  AN EXTENSION, as the collision operator is: the reference
// has none.  tests/collisional_grid_trace_ref.py states the moments a second time in numpy float64.
//
// k_background_from_sort turns a cell-sorted sort into a profile, as k_collide (collide.hip) reads one: one wave per
// cell, kWaves cells per workgroup, grid-stride over the cells, cell_start gives the segment.  Lane l sums the records
// l, l + 64, ... of its cell in that order (a cell of more than 64 records loops), the 64 partial sums are folded
// 32, 16, .. 1 across the wave, every lane receiving the same bits; two passes, the second about the mean of the first.
// fp64, no atomics, no LDS, nothing is written but the slot: two calls give the same bits and the records stay as they are.
// Compiled without floating-point contraction: rounded operation by operation, as numpy rounds it.
#include <cmath>
#include <string>
#include <vector>

#include "common.h"
#include "device_common.h"

#pragma clang fp contract(off)

namespace xpic {

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kRows = 5; // n, vth, ux, uy, uz

// the sum over the wave in a fixed order, in every lane (v + its partner's v commutes: both lanes round alike)
__device__ inline double wave_sum_all(double v)
{
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// out [5][ncell]; w: the sort's weight n / Np
__global__ void __launch_bounds__(kBlock) k_background_from_sort(SortDev A, long ncell, double w, double* __restrict__ out)
{
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long nw = (long)gridDim.x * kWaves;
  for (long c = (long)blockIdx.x * kWaves + wave; c < ncell; c += nw) {
    const int b0 = A.cell_start[c], N = A.cell_start[c + 1] - b0;
    double s[3] = {0.0, 0.0, 0.0};
    for (int i = lane; i < N; i += 64) {
      s[0] += A.v[0][b0 + i];
      s[1] += A.v[1][b0 + i];
      s[2] += A.v[2][b0 + i];
    }
    const double dn = (double)N;
    double u[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double sum = wave_sum_all(s[k]);
      u[k] = N > 0 ? sum / dn : 0.0;
    }
    double d2 = 0.0;
    for (int i = lane; i < N; i += 64) {
      const double x = A.v[0][b0 + i] - u[0], y = A.v[1][b0 + i] - u[1], z = A.v[2][b0 + i] - u[2];
      d2 += x * x + y * y + z * z;
    }
    d2 = wave_sum_all(d2);
    if (lane == 0) {
      out[c] = w * dn;
      out[ncell + c] = N > 0 ? sqrt(d2 / (3.0 * dn)) : 0.0;
      out[2 * ncell + c] = u[0];
      out[3 * ncell + c] = u[1];
      out[4 * ncell + c] = u[2];
    }
  }
}

// the checks every entry point shares; slots exist on a single z-slab only, as the grid tracers do
int background_check(xpic_ctx* ctx, const std::string& who, int slot)
{
  XPIC_CHECK(ctx != nullptr, "null context");
  XPIC_CHECK(ctx->geom.nranks == 1 && ctx->g.G == 0,
    who + ": a context of several z-slabs (or a self_ring one) is not supported: a profile covers the whole box");
  XPIC_CHECK(slot >= 0 && slot < XPIC_TRACE_BG_MAX, who + ": the slot must be within 0 .. XPIC_TRACE_BG_MAX - 1");
  return 0;
}

int background_alloc(xpic_ctx* ctx, int slot)
{
  if (!ctx->bg_profile[slot]) XPIC_HIP(hipMalloc(&ctx->bg_profile[slot], sizeof(double) * kRows * ctx->ncell));
  return 0;
}

}  // namespace

void background_free(xpic_ctx* ctx)
{
  for (int s = 0; s < XPIC_TRACE_BG_MAX; ++s) {
    if (ctx->bg_profile[s]) (void)hipFree(ctx->bg_profile[s]);
    ctx->bg_profile[s] = nullptr;
  }
}

}  // namespace xpic

using namespace xpic;

extern "C" {

int xpic_background_set(xpic_ctx* ctx, int slot, const double* n_zyx, const double* vth_zyx, const double* drift_zyx3)
{
  const std::string who = "background_set";
  XPIC_CALL(background_check(ctx, who, slot));
  XPIC_CHECK(n_zyx, who + ": n is null");
  XPIC_CHECK(vth_zyx, who + ": vth is null");
  const long nc = ctx->ncell;
  std::vector<double> h((size_t)kRows * nc, 0.0);
  for (long c = 0; c < nc; ++c) {
    XPIC_CHECK(std::isfinite(n_zyx[c]) && n_zyx[c] >= 0.0, who + ": a density is negative or not finite");
    XPIC_CHECK(std::isfinite(vth_zyx[c]) && vth_zyx[c] >= 0.0, who + ": a thermal speed is negative or not finite");
    h[c] = n_zyx[c];
    h[nc + c] = vth_zyx[c];
    if (!drift_zyx3) continue;
    for (int k = 0; k < 3; ++k) {
      XPIC_CHECK(std::isfinite(drift_zyx3[3 * c + k]), who + ": a drift is not finite");
      h[(2 + k) * nc + c] = drift_zyx3[3 * c + k];
    }
  }
  XPIC_CALL(background_alloc(ctx, slot));
  XPIC_HIP(hipMemcpyAsync(ctx->bg_profile[slot], h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice, ctx->stream));
  XPIC_HIP(hipStreamSynchronize(ctx->stream));
  return 0;
}

int xpic_background_get(xpic_ctx* ctx, int slot, double* n_zyx, double* vth_zyx, double* drift_zyx3)
{
  const std::string who = "background_get";
  XPIC_CALL(background_check(ctx, who, slot));
  XPIC_CHECK(ctx->bg_profile[slot], who + ": the slot is empty");
  const long nc = ctx->ncell;
  std::vector<double> h((size_t)kRows * nc);
  XPIC_HIP(hipMemcpyAsync(h.data(), ctx->bg_profile[slot], sizeof(double) * h.size(), hipMemcpyDeviceToHost, ctx->stream));
  XPIC_HIP(hipStreamSynchronize(ctx->stream));
  for (long c = 0; c < nc; ++c) {
    if (n_zyx) n_zyx[c] = h[c];
    if (vth_zyx) vth_zyx[c] = h[nc + c];
    if (drift_zyx3)
      for (int k = 0; k < 3; ++k) drift_zyx3[3 * c + k] = h[(2 + k) * nc + c];
  }
  return 0;
}

int xpic_background_clear(xpic_ctx* ctx, int slot)
{
  XPIC_CALL(background_check(ctx, "background_clear", slot));
  XPIC_HIP(hipStreamSynchronize(ctx->stream));
  if (ctx->bg_profile[slot]) XPIC_HIP(hipFree(ctx->bg_profile[slot]));
  ctx->bg_profile[slot] = nullptr;
  return 0;
}

int xpic_background_from_sort(xpic_ctx* ctx, int slot, int sort)
{
  const std::string who = "background_from_sort";
  XPIC_CALL(background_check(ctx, who, slot));
  XPIC_CHECK(sort >= 0 && sort < (int)ctx->sorts.size(), who + ": unknown sort id");
  Sort& a = ctx->sorts[sort];
  XPIC_CHECK(a.par.Np > 0, who + ": a sort without Np");
  const double w = a.par.n / a.par.Np; // (xpic_collide's weight: n_L = w N_cell)
  XPIC_CHECK(std::isfinite(w) && w >= 0.0, who + ": the sort's weight n / Np must be finite and not negative");
  XPIC_CALL(sort_materialize(ctx, a)); // (a deferred re-binning whose assembly has not run)
  XPIC_CALL(background_alloc(ctx, slot));
  Timed t(ctx, "background_from_sort");
  if (a.n == 0) { // (no segment to read: every cell is empty)
    XPIC_HIP(hipMemsetAsync(ctx->bg_profile[slot], 0, sizeof(double) * kRows * ctx->ncell, ctx->stream));
    return 0;
  }
  long nb = (ctx->ncell + kWaves - 1) / kWaves;
  if (nb > kRedBlocks) nb = kRedBlocks;
  hipLaunchKernelGGL(k_background_from_sort, dim3((unsigned)nb), dim3(kBlock), 0, ctx->stream, a.d, (long)ctx->ncell, w,
    ctx->bg_profile[slot]);
  XPIC_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
