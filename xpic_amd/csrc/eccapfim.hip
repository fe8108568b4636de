// eccapfim.hip -- the inner kernels of the reference's `eccapfim` scheme, as batch operations
// over path segments r0 -> rn:
//   cell_traversal                     src/impls/eccapfim/cell_traversal.cpp:3-77
//   ImplicitEsirkepov::Shape::setup    src/algorithms/implicit_esirkepov.cpp:11-57
//   ImplicitEsirkepov::interpolate     :60-90   (E with the segment shape, B with Shape(midpoint) + SimpleInterpolation)
//   ImplicitEsirkepov::decompose       :92-117
// One lane per segment, the host arrays staged through batch.h.  The scheme's outer loops (Crank-Nicolson sub-stepping,
// SNES) are not part of this build.  The three entry points are single-slab calls: with G == 0 ie_node folds every index
// on all three axes; on a z-slab of several it does not fold z and nothing checks a position against the ghost planes.
// Held to tests/eccapfim_ref.py by tests/test_gpu_eccapfim.py.
#include <cfloat>

#include "batch.h"
#include "common.h"
#include "device_common.h"
#include "ie_shape.h"
#include "shape2.h"

namespace xpic {

namespace {

constexpr int kBlock = kLaneBlock; // batch.h: lane_grid launches workgroups of this size

__global__ void __launch_bounds__(kBlock) k_ie_interpolate(GridDev g, const double* __restrict__ E,
  const double* __restrict__ B, long n, const double* rn3, const double* r03, double* Ep3, double* Bp3)
{
  const long q = (long)blockIdx.x * kBlock + threadIdx.x;
  if (q >= n) return;
  const double rn[3] = {rn3[3 * q], rn3[3 * q + 1], rn3[3 * q + 2]}, r0[3] = {r03[3 * q], r03[3 * q + 1], r03[3 * q + 2]};
  // B: Shape::setup(midpoint, 1.5, spline_of_2nd_order) + SimpleInterpolation (magnetic products, shape.h:65-72)
  const double rm[3] = {0.5 * (rn[0] + r0[0]), 0.5 * (rn[1] + r0[1]), 0.5 * (rn[2] + r0[2])};
  double Ep[3], Bp[3] = {0, 0, 0};
  Shape2 mid;
  mid.setup(g, rm);
  mid.nodes([&](int gx, int gy, int gz, double Noz, double Shz, double Noy, double Shy, double Nox, double Shx) {
    const long o = ie_node(g, gx, gy, gz);
    Bp[0] += B[o] * (Shz * Shy * Nox);
    Bp[1] += B[g.cstride + o] * (Shz * Noy * Shx);
    Bp[2] += B[2 * g.cstride + o] * (Noz * Shy * Shx);
  });
  IEShape sh;
  sh.setup(g, rn, r0);
  segment_gather_E(g, E, sh, Ep);
#pragma unroll
  for (int c = 0; c < 3; ++c) { Ep3[3 * q + c] = Ep[c]; Bp3[3 * q + c] = Bp[c]; }
}

__global__ void __launch_bounds__(kBlock) k_ie_decompose(GridDev g, double* J, long n, const double* alpha,
  const double* v3, const double* rn3, const double* r03)
{
  const long q = (long)blockIdx.x * kBlock + threadIdx.x;
  if (q >= n) return;
  const double rn[3] = {rn3[3 * q], rn3[3 * q + 1], rn3[3 * q + 2]}, r0[3] = {r03[3 * q], r03[3 * q + 1], r03[3 * q + 2]};
  IEShape sh;
  sh.setup(g, rn, r0);
  const double av[3] = {alpha[q] * v3[3 * q], alpha[q] * v3[3 * q + 1], alpha[q] * v3[3 * q + 2]};
  segment_nodes(g, sh, [&](int cx, long o, double c) {
    const double w = av[cx] * c;
    if (w != 0.0) unsafeAtomicAdd(&J[cx * g.cstride + o], w);
  });
}

__global__ void __launch_bounds__(kBlock) k_cell_traversal(GridDev g, long n, const double* end3, const double* start3,
  int max_pts, double* pts, int* counts)
{
  // Compiled without contraction, as device_common.h's within(): a fused (curr + sg / 2) * d - st moves a crossing
  // parameter by ulp(face) / 2 / dir[c], which the other axes see magnified by dir[c'] / dir[c] in start + dir * t, and
  // it may order two near crossings differently from the reference's ladder.  Rounded step by step the points are the
  // reference's bit for bit.
#pragma clang fp contract(off)
  const long q = (long)blockIdx.x * kBlock + threadIdx.x;
  if (q >= n) return;
  const double d[3] = {g.dx, g.dy, g.dz};
  double st[3], en[3], dir[3], tt[3], dtt[3];
  int curr[3], last[3], sg[3];
  bool same = true;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    st[c] = start3[3 * q + c];
    en[c] = end3[3 * q + c];
    curr[c] = (int)round(st[c] / d[c]);
    last[c] = (int)round(en[c] / d[c]);
    same = same && curr[c] == last[c];
  }
  double* out = pts + 3L * max_pts * q;
  int np = 0;
  auto push = [&](double x, double y, double z) {
    if (np < max_pts) { out[3 * np] = x; out[3 * np + 1] = y; out[3 * np + 2] = z; }
    ++np;
  };
  push(st[0], st[1], st[2]);
  if (!same) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      dir[c] = en[c] - st[c];
      sg[c] = dir[c] > 0 ? 1 : -1;
      const double nxt = (curr[c] + sg[c] * 0.5) * d[c];
      tt[c] = (dir[c] != 0) ? (nxt - st[c]) / dir[c] : DBL_MAX;
      dtt[c] = (dir[c] != 0) ? d[c] / dir[c] * sg[c] : 0.0;
    }
    while (!(curr[0] == last[0] && curr[1] == last[1] && curr[2] == last[2]) && np <= 64) {
      double t;
      if (tt[0] < tt[1]) {
        if (tt[0] < tt[2]) { t = tt[0]; curr[0] += sg[0]; tt[0] += dtt[0]; }
        else { t = tt[2]; curr[2] += sg[2]; tt[2] += dtt[2]; }
      }
      else {
        if (tt[1] < tt[2]) { t = tt[1]; curr[1] += sg[1]; tt[1] += dtt[1]; }
        else { t = tt[2]; curr[2] += sg[2]; tt[2] += dtt[2]; }
      }
      push(st[0] + dir[0] * t, st[1] + dir[1] * t, st[2] + dir[2] * t);
    }
  }
  push(en[0], en[1], en[2]);
  counts[q] = np;
}

}  // namespace

}  // namespace xpic

using namespace xpic;

extern "C" {

int xpic_cell_traversal(xpic_ctx* ctx, int64_t n, const double* end3, const double* start3, int max_pts, double* pts,
  int* counts)
{
  XPIC_CHECK(ctx && end3 && start3 && pts && counts && n >= 0 && max_pts >= 2, "bad argument");
  if (n == 0) return 0;
  DevScratch<double> e, s, p;
  DevScratch<int> k;
  const size_t npts = (size_t)3 * n * max_pts; // doubles
  XPIC_CALL(e.alloc(3 * n)); XPIC_CALL(s.alloc(3 * n));
  XPIC_CALL(p.alloc(npts)); XPIC_CALL(k.alloc(n));
  XPIC_CALL(upload(e, end3, 3 * n, ctx->stream));
  XPIC_CALL(upload(s, start3, 3 * n, ctx->stream));
  XPIC_CALL(zero(p, npts, ctx->stream));
  hipLaunchKernelGGL(k_cell_traversal, lane_grid(n), dim3(kBlock), 0, ctx->stream, ctx->g, (long)n, (const double*)e.p,
    (const double*)s.p, max_pts, p.p, k.p);
  XPIC_HIP(hipGetLastError());
  XPIC_CALL(download(pts, p, npts, ctx->stream));
  XPIC_CALL(download(counts, k, n, ctx->stream));
  XPIC_HIP(hipStreamSynchronize(ctx->stream));
  return 0;
}

int xpic_implicit_esirkepov_interpolate(xpic_ctx* ctx, int64_t n, const double* rn3, const double* r03, double* Ep3,
  double* Bp3)
{
  XPIC_CHECK(ctx && rn3 && r03 && Ep3 && Bp3 && n >= 0, "bad argument");
  if (n == 0) return 0;
  XPIC_CALL(halo_fill(ctx, ctx->field[XPIC_E]));
  XPIC_CALL(halo_fill(ctx, ctx->field[XPIC_B]));
  DevScratch<double> a, b, e, m;
  XPIC_CALL(a.alloc(3 * n)); XPIC_CALL(b.alloc(3 * n));
  XPIC_CALL(e.alloc(3 * n)); XPIC_CALL(m.alloc(3 * n));
  XPIC_CALL(upload(a, rn3, 3 * n, ctx->stream));
  XPIC_CALL(upload(b, r03, 3 * n, ctx->stream));
  hipLaunchKernelGGL(k_ie_interpolate, lane_grid(n), dim3(kBlock), 0, ctx->stream, ctx->g, ctx->field[XPIC_E],
    ctx->field[XPIC_B], (long)n, (const double*)a.p, (const double*)b.p, e.p, m.p);
  XPIC_HIP(hipGetLastError());
  XPIC_CALL(download(Ep3, e, 3 * n, ctx->stream));
  XPIC_CALL(download(Bp3, m, 3 * n, ctx->stream));
  XPIC_HIP(hipStreamSynchronize(ctx->stream));
  return 0;
}

int xpic_implicit_esirkepov_decompose(xpic_ctx* ctx, int64_t n, const double* alpha, const double* v3, const double* rn3,
  const double* r03, int field)
{
  XPIC_CHECK(ctx && alpha && v3 && rn3 && r03 && n >= 0, "bad argument");
  XPIC_CHECK(field >= 0 && field < XPIC_NFIELDS && ctx->field[field], "no such field vector");
  if (n == 0) return 0;
  DevScratch<double> al, v, a, b;
  XPIC_CALL(al.alloc(n)); XPIC_CALL(v.alloc(3 * n));
  XPIC_CALL(a.alloc(3 * n)); XPIC_CALL(b.alloc(3 * n));
  XPIC_CALL(upload(al, alpha, n, ctx->stream));
  XPIC_CALL(upload(v, v3, 3 * n, ctx->stream));
  XPIC_CALL(upload(a, rn3, 3 * n, ctx->stream));
  XPIC_CALL(upload(b, r03, 3 * n, ctx->stream));
  // deposit into a zeroed scratch vector (ghost planes included), fold the ghosts, then add: DMLocalToGlobal(ADD)
  double* tmp = ctx->field[XPIC_W2];
  XPIC_CHECK(tmp != ctx->field[field], "XPIC_W2 is the scratch vector of this call");
  XPIC_HIP(hipMemsetAsync(tmp, 0, sizeof(double) * ctx->nvec, ctx->stream));
  hipLaunchKernelGGL(k_ie_decompose, lane_grid(n), dim3(kBlock), 0, ctx->stream, ctx->g, tmp, (long)n,
    (const double*)al.p, (const double*)v.p, (const double*)a.p, (const double*)b.p);
  XPIC_HIP(hipGetLastError());
  XPIC_CALL(halo_add(ctx, tmp, 3));
  XPIC_CALL(vec_axpy(ctx, ctx->field[field], 1.0, tmp));
  XPIC_HIP(hipStreamSynchronize(ctx->stream));
  return 0;
}

}  // extern "C"
