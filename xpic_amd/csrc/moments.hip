// moments.hip -- the reference's particle diagnostics on the device: DistributionMoment with all six moments and its region
// rule (src/diagnostics/distribution_moment.cpp:59-316), VelocityDistribution, the 2-D histogram of f(v)
// (src/diagnostics/velocity_distribution.cpp:47-200).  Off the step; no state of the context changes.
#include <algorithm>
#include <cmath>

#include "common.h"
#include "device_common.h"
#include "moment_deposit.h"

namespace xpic {

namespace {

// ---- DistributionMoment::collect (distribution_moment.cpp:157-210) -----------------------------------------------
// One workgroup per block of storage cells: kMomCX cells of an x-pencil, kMomCY rows, kMomCZ planes.  Its particles are
// the block's 16 contiguous runs of cell_start (one per row); they deposit into an LDS tile of the block's cells and their
// one-cell halo, (CX + 2) (CY + 2) (CZ + 2) cells x dof, with fp64 LDS atomics, and the tile is then added to memory with
// one global atomic per cell and component: 2.3 atomics per cell and component at 256^3 instead of 8 per particle and
// component (512 at 64 per cell).  (Storing the tile's inner cells, which no other block reaches, would save a tenth of
// them, and would race with the direct deposits of records that sit away from their storage cell.)
constexpr int kMomCX = 64, kMomCY = 4, kMomCZ = 4;
constexpr int kMomWaves = 8;
constexpr int kMomThreads = 64 * kMomWaves;
constexpr int kMomTile = (kMomCX + 2) * (kMomCY + 2) * (kMomCZ + 2); // cells of the largest tile

struct MomParticles { // the records and cell_start of a sort: what the deposit reads of SortDev
  const double* r[3];
  const double* v[3];
  const int* cs;
};

// STRAY = false: the deposit into the tile and the tile's flush; a record whose 2 x 2 x 2 cells leave the tile (it sits away
// from its storage cell: positions moved, cells not yet re-binned -- the phase entry points allow that state) only raises
// *stray.  STRAY = true, launched only then: those records alone, straight to memory.
template <int K, bool STRAY>
__global__ void __launch_bounds__(kMomThreads) k_moment(GridDev g, MomParticles s, MomRegion R, double q, double m, double n_Np,
  MomOut out, int* stray)
{
  constexpr int D = MomDof<K>::v;
  extern __shared__ double tile[]; // [D][TZ][TY][TX]
  const int ib = blockIdx.x % R.nbx, jb = (blockIdx.x / R.nbx) % R.nby, kb = blockIdx.x / (R.nbx * R.nby);
  const int x0 = R.bx[0] + ib * kMomCX, x1 = min(x0 + kMomCX, R.bx[1]);
  const int y0 = R.by[0] + jb * kMomCY, y1 = min(y0 + kMomCY, R.by[1]);
  const int z0 = R.bz[0] + kb * kMomCZ, z1 = min(z0 + kMomCZ, R.bz[1]); // local planes
  const int TX = x1 - x0 + 2, TY = y1 - y0 + 2, TZ = z1 - z0 + 2, TS = TX * TY * TZ;
  if (!STRAY) {
    for (int i = threadIdx.x; i < D * TS; i += kMomThreads) tile[i] = 0.0;
    __syncthreads();
  }

  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int grp = lane >> 3, u = lane & 7;
  const int rows = (y1 - y0) * (z1 - z0);
  bool strays = false;
  for (int row = wave; row < rows; row += kMomWaves) {
    const int yy = y0 + row % (y1 - y0), zz = z0 + row / (y1 - y0);
    const long c0 = ((long)zz * g.ny + yy) * g.nx;
    const int b = s.cs[c0 + x0], e = s.cs[c0 + x1];
    // 8 lanes read 8 consecutive records (a 64-byte run), the 8 groups lie an eighth of the row apart: the lanes of a
    // wave sit in different cells and the rotation below spreads the 8 lanes of a group over the 8 corners
    const int seg = ((e - b + 7) / 8 + 7) & ~7;
    const int gb = b + grp * seg, ge = min(gb + seg, e);
    for (int it = 0; it < seg; it += 8) {
      const int p = gb + it + u;
      if (p >= ge) continue;
      const double r[3] = {s.r[0][p], s.r[1][p], s.r[2][p]};
      const double v[3] = {s.v[0][p], s.v[1][p], s.v[2][p]};
      int st[3];
      double w[3][2];
      mom_shape(g, r, st, w); // DistributionMoment::Shape::setup (:137-151)
      const int tx = st[0] - (x0 - 1), ty = st[1] - (y0 - 1), tz = st[2] - g.z0 - (z0 - 1);
      const bool in_tile = tx >= 0 && tx + 1 < TX && ty >= 0 && ty + 1 < TY && tz >= 0 && tz + 1 < TZ;
      if (in_tile == STRAY) {
        strays = true;
        continue;
      }
      double mv[D];
      moment_of<K>(g, q, m, r[0], r[1], v, mv);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int kk = (k + u) & 7;
        const int ix = kk & 1, iy = (kk >> 1) & 1, iz = kk >> 2;
        const double si = mom_weight(w, kk) * n_Np; // (:196)
        if (si == 0.0) continue;
        if (!STRAY) {
          const int t = ((tz + iz) * TY + (ty + iy)) * TX + (tx + ix);
#pragma unroll
          for (int j = 0; j < D; ++j) atomicAdd(&tile[j * TS + t], mv[j] * si);
        } else {
          const long node = mom_target(g, R, st[0] + ix, st[1] + iy, st[2] + iz);
          if (node >= 0)
#pragma unroll
            for (int j = 0; j < D; ++j) unsafeAtomicAdd(&out.c[j][node], mv[j] * si);
        }
      }
    }
  }
  if (STRAY) return;
  if (strays) *stray = 1;
  __syncthreads();

  for (int t = threadIdx.x; t < TS; t += kMomThreads) {
    const int tx = t % TX, ty = (t / TX) % TY, tz = t / (TX * TY);
    const long node = mom_target(g, R, x0 - 1 + tx, y0 - 1 + ty, g.z0 + z0 - 1 + tz);
    if (node < 0) continue;
#pragma unroll
    for (int j = 0; j < D; ++j) {
      const double val = tile[j * TS + t];
      if (val != 0.0) unsafeAtomicAdd(&out.c[j][node], val);
    }
  }
}

// ---- VelocityDistribution::collect (velocity_distribution.cpp:112-163) ---------------------------------------------
// Workgroups take the rows (y, z) of the AABB in turn.  The cells of a row whose centre passes the tester are one run of x
// (box and cylinder are convex), so the row's particles are ONE contiguous run of cell_start, read coalesced.  Each
// workgroup accumulates into a private LDS histogram when it has at most kVdLdsBins bins and adds it to memory at the end;
// a larger histogram takes one global atomic per particle.
constexpr int kVdThreads = 256;
constexpr int kVdLdsBins = 8192; // 64 KiB of fp64

struct VdParams {
  int proj, geom;
  double gp[7];       // box: min xyz, max xyz; cylinder: center xyz, radius, height
  int a0[3], a1[3];   // AABB in global cells, [a0, a1)
  int y0, y1, z0, z1; // its rows on this slab (z local)
  double dvx, dvy;
  int vs, vn;         // vstart, vsize of BOTH axes (set_regions :57-68 computes them from vx_min, vx_max, dvx)
  double n_Np;
};

template <bool LDS>
__global__ void __launch_bounds__(kVdThreads) k_vdist(GridDev g, SortDev s, VdParams P, double* hist)
{
  __shared__ double lh[LDS ? kVdLdsBins : 1];
  __shared__ int xr[2];
  const int nb = P.vn * P.vn;
  if (LDS) {
    for (int i = threadIdx.x; i < nb; i += kVdThreads) lh[i] = 0.0;
  }
  const int ny = P.y1 - P.y0, rows = ny * (P.z1 - P.z0);
  const int xa = max(P.a0[0], 0), xb = min(P.a1[0], g.nx);
  for (int row = blockIdx.x; row < rows; row += gridDim.x) {
    const int yy = P.y0 + row % ny, zz = P.z0 + row / ny;
    if (threadIdx.x == 0) { xr[0] = g.nx; xr[1] = -1; }
    __syncthreads();
    const double cy = (yy + 0.5) * g.dy, cz = (zz + g.z0 + 0.5) * g.dz;
    for (int x = xa + threadIdx.x; x < xb; x += kVdThreads)
      if (within(P.geom, P.gp, (x + 0.5) * g.dx, cy, cz)) {
        atomicMin(&xr[0], x);
        atomicMax(&xr[1], x);
      }
    __syncthreads();
    const int lo = xr[0], hi = xr[1];
    __syncthreads(); // (xr is reset by the next row)
    if (hi < lo) continue;
    const long c0 = ((long)zz * g.ny + yy) * g.nx;
    const int b = s.cell_start[c0 + lo], e = s.cell_start[c0 + hi + 1];
    for (int p = b + threadIdx.x; p < e; p += kVdThreads) {
      const double vx = s.v[0][p], vy = s.v[1][p], vz = s.v[2][p];
      double a, c;
      if (P.proj == XPIC_PROJ_VX_VY) { a = vx; c = vy; }                            // get_vx_vy (:166-169)
      else if (P.proj == XPIC_PROJ_VZ_VXY) { a = vz; c = sqrt(vx * vx + vy * vy + 0.0 * 0.0); } // get_vz_vxy (:171-175)
      else {                                                                       // get_vr_vphi (:177-193)
        const double v[3] = {vx, vy, vz};
        double o[3];
        v_cyl(s.r[0][p], s.r[1][p], g.Lx, g.Ly, v, o);
        a = o[0]; c = o[1];
      }
      // ROUND_STEP: std::round, half away from zero; compared before the cast so that no value overflows an int
      const double bx = round(a / P.dvx), by = round(c / P.dvy);
      if (!(bx >= P.vs && bx < P.vs + P.vn && by >= P.vs && by < P.vs + P.vn)) continue;
      const int i = ((int)by - P.vs) * P.vn + ((int)bx - P.vs);
      if (LDS) atomicAdd(&lh[i], P.n_Np);
      else unsafeAtomicAdd(&hist[i], P.n_Np);
    }
  }
  if (LDS) {
    __syncthreads();
    for (int i = threadIdx.x; i < nb; i += kVdThreads)
      if (lh[i] != 0.0) unsafeAtomicAdd(&hist[i], lh[i]);
  }
}

template <int K>
int launch_moment(xpic_ctx* c, Sort& s, const MomRegion& R, unsigned nblocks, const MomOut& o)
{
  const size_t lds = sizeof(double) * MomDof<K>::v * kMomTile;
  // the tile of a 6-component moment is more than the default 64 KiB of dynamic LDS; set on every launch (a host-side
  // attribute write: no shared flag between the threads of a process that drive slabs, and right on any device)
  XPIC_HIP(hipFuncSetAttribute((const void*)k_moment<K, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const MomParticles mp{{s.d.r[0], s.d.r[1], s.d.r[2]}, {s.d.v[0], s.d.v[1], s.d.v[2]}, s.d.cell_start};
  int* stray = (int*)c->red_partial; // (reduction scratch: free between reductions)
  XPIC_HIP(hipMemsetAsync(stray, 0, sizeof(int), c->stream));
  {
    Timed t(c, "moment");
    hipLaunchKernelGGL((k_moment<K, false>), dim3(nblocks), dim3(kMomThreads), lds, c->stream, c->g, mp, R, s.par.q, s.par.m,
      s.par.n / s.par.Np, o, stray);
    XPIC_HIP(hipGetLastError());
  }
  int h = 0;
  XPIC_HIP(hipMemcpyAsync(&h, stray, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  XPIC_HIP(hipStreamSynchronize(c->stream));
  if (h) {
    Timed t(c, "moment_stray");
    hipLaunchKernelGGL((k_moment<K, true>), dim3(nblocks), dim3(kMomThreads), 0, c->stream, c->g, mp, R, s.par.q, s.par.m,
      s.par.n / s.par.Np, o, stray);
    XPIC_HIP(hipGetLastError());
  }
  return 0;
}

}  // namespace

int moment_dof(int kind)
{
  static const int dof[6] = {1, 3, 6, 3, 6, 3};
  return kind >= 0 && kind < 6 ? dof[kind] : 0;
}

int moment_region(xpic_ctx* c, Sort& s, int kind, const int* region6, double* const* comp)
{
  const GridDev& g = c->g;
  MomRegion R{};
  XPIC_CHECK(mom_region_of(g, region6, &R), "moment region: start >= 0, size > 0, start + size <= n");
  R.bx[0] = R.s[0]; R.bx[1] = R.e[0];
  R.by[0] = R.s[1]; R.by[1] = R.e[1];
  R.bz[0] = std::max(R.s[2], g.z0) - g.z0;
  R.bz[1] = std::min(R.e[2], g.z0 + g.nzl) - g.z0;
  const int D = moment_dof(kind);
  XPIC_CHECK(D > 0, "unknown moment kind");
  XPIC_CALL(sort_materialize(c, s)); // (a deferred re-binning whose assembly has not run)
  // the output vectors are zeroed whole: ghost planes included (halo_add reads them)
  for (int v = 0; v < (D + 2) / 3; ++v) XPIC_HIP(hipMemsetAsync(comp[3 * v], 0, sizeof(double) * c->nvec, c->stream));
  if (s.n > 0 && R.bz[1] > R.bz[0]) {
    R.nbx = (R.bx[1] - R.bx[0] + kMomCX - 1) / kMomCX;
    R.nby = (R.by[1] - R.by[0] + kMomCY - 1) / kMomCY;
    const int nbz = (R.bz[1] - R.bz[0] + kMomCZ - 1) / kMomCZ;
    const unsigned nblocks = (unsigned)((long)R.nbx * R.nby * nbz);
    MomOut o{};
    for (int j = 0; j < D; ++j) o.c[j] = comp[j];
    switch (kind) {
      case XPIC_MOMENT_DENSITY: XPIC_CALL(launch_moment<XPIC_MOMENT_DENSITY>(c, s, R, nblocks, o)); break;
      case XPIC_MOMENT_CURRENT: XPIC_CALL(launch_moment<XPIC_MOMENT_CURRENT>(c, s, R, nblocks, o)); break;
      case XPIC_MOMENT_MOMENTUM_FLUX: XPIC_CALL(launch_moment<XPIC_MOMENT_MOMENTUM_FLUX>(c, s, R, nblocks, o)); break;
      case XPIC_MOMENT_MOMENTUM_FLUX_DIAG: XPIC_CALL(launch_moment<XPIC_MOMENT_MOMENTUM_FLUX_DIAG>(c, s, R, nblocks, o)); break;
      case XPIC_MOMENT_MOMENTUM_FLUX_CYL: XPIC_CALL(launch_moment<XPIC_MOMENT_MOMENTUM_FLUX_CYL>(c, s, R, nblocks, o)); break;
      default: XPIC_CALL(launch_moment<XPIC_MOMENT_MOMENTUM_FLUX_DIAG_CYL>(c, s, R, nblocks, o)); break;
    }
  }
  // DMLocalToGlobal(ADD): what a slab deposited into its ghost planes goes to their owner (collective: every rank calls it)
  for (int v = 0; v < (D + 2) / 3; ++v) XPIC_CALL(halo_add(c, comp[3 * v], 1));
  return 0;
}

// VelocityDistributionBuilder (builders/velocity_distribution_builder.cpp:32-77) + set_regions (:47-68)
int vdist_sizes(const GridDev& g, int geometry, const double* geom, const double* vreg, int* aabb6, int* vs, int* vn)
{
  const double d[3] = {g.dx, g.dy, g.dz};
  XPIC_CHECK(geometry == XPIC_GEOM_BOX || geometry == XPIC_GEOM_CYLINDER, "unknown geometry");
  XPIC_CHECK(vreg[4] > 0 && vreg[5] > 0, "velocity distribution: dv must be positive");
  for (int a = 0; a < 3; ++a) {
    double lo, hi;
    if (geometry == XPIC_GEOM_BOX) { lo = geom[a]; hi = geom[3 + a]; }
    else {
      const double ext = a < 2 ? geom[3] : 0.5 * geom[4];
      lo = geom[a] - ext;
      hi = geom[a] + ext;
    }
    aabb6[a] = (int)std::floor(lo / d[a]);                // FLOOR_STEP
    aabb6[3 + a] = (int)std::floor(hi / d[a]) - aabb6[a]; // size
  }
  // as written in the reference: the y axis takes vx_min, vx_max and dvx as well; ROUND_STEP = std::round, half away from
  // zero.  Checked in double before the casts: at most 2^15 bins per axis (2^30 in all)
  const double vs_d = std::round(vreg[0] / vreg[4]), vn_d = std::round((vreg[2] - vreg[0]) / vreg[4]);
  XPIC_CHECK(std::fabs(vs_d) < 1e9 && vn_d <= 32768.0, "velocity distribution: more than 2^15 bins per axis");
  *vs = (int)vs_d;
  *vn = (int)std::max(vn_d, 0.0);
  return 0;
}

int velocity_distribution(xpic_ctx* c, Sort& s, int projector, int geometry, const double* geom, const double* vreg, double* hist)
{
  const GridDev& g = c->g;
  XPIC_CHECK(projector >= XPIC_PROJ_VX_VY && projector <= XPIC_PROJ_VR_VPHI, "unknown projector");
  VdParams P{};
  int aabb[6];
  XPIC_CALL(vdist_sizes(g, geometry, geom, vreg, aabb, &P.vs, &P.vn));
  XPIC_CHECK(P.vn > 0, "velocity distribution: empty histogram (vmax <= vmin)");
  const long nb = (long)P.vn * P.vn;
  P.proj = projector;
  P.geom = geometry;
  for (int i = 0; i < 7; ++i) P.gp[i] = geom[i];
  for (int a = 0; a < 3; ++a) { P.a0[a] = aabb[a]; P.a1[a] = aabb[a] + aabb[3 + a]; }
  P.y0 = std::max(P.a0[1], 0);
  P.y1 = std::min(P.a1[1], g.ny);
  P.z0 = std::max(P.a0[2], g.z0) - g.z0;
  P.z1 = std::min(P.a1[2], g.z0 + g.nzl) - g.z0;
  P.dvx = vreg[4];
  P.dvy = vreg[5];
  P.n_Np = s.par.n / s.par.Np;
  XPIC_CALL(sort_materialize(c, s)); // (a deferred re-binning whose assembly has not run)
  XPIC_HIP(hipMemsetAsync(hist, 0, sizeof(double) * nb, c->stream));
  const long rows = (long)std::max(P.y1 - P.y0, 0) * std::max(P.z1 - P.z0, 0);
  const int xa = std::max(P.a0[0], 0), xb = std::min(P.a1[0], g.nx);
  if (s.n > 0 && rows > 0 && xb > xa) {
    Timed t(c, "velocity_distribution");
    const unsigned grid = (unsigned)std::min<long>(rows, 2L * c->num_cus);
    if (nb <= kVdLdsBins) hipLaunchKernelGGL(k_vdist<true>, dim3(grid), dim3(kVdThreads), 0, c->stream, g, s.d, P, hist);
    else hipLaunchKernelGGL(k_vdist<false>, dim3(grid), dim3(kVdThreads), 0, c->stream, g, s.d, P, hist);
    XPIC_HIP(hipGetLastError());
  }
  return comm_allreduce_sum(c, hist, (int)nb); // the VecScatter ADD (:159-160), the whole histogram on every rank
}

}  // namespace xpic
