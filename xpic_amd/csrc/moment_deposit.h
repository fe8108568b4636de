// moment_deposit.h -- what the two moment deposits share on the device: moments.hip (DistributionMoment of a cell-sorted
// sort, one workgroup per block of storage cells) and tracer_moments.hip (the moments of a tracer set, whose records are
// not sorted and may be dead, one lane per record).  The region and its rule for a deposit, the component counts, the six
// per-particle values, and the cell-centred first-order shape.  Included after common.h and device_common.h.
//   DistributionMoment::collect, Shape::setup      src/diagnostics/distribution_moment.cpp:137-210
//   get_density ... get_momentum_flux_diag_cyl     src/diagnostics/distribution_moment.cpp:212-298
#pragma once

namespace xpic {

// global cells [s, e) per axis; full: the region spans the axis, its deposits wrap periodically (l_bound = bound, :104)
struct MomRegion {
  int s[3], e[3], full[3];
  int bx[2], by[2], bz[2]; // local storage cells of the region on this slab (z relative to the first owned plane)
  int nbx, nby;            // blocks along x, y
};

struct MomOut {
  double* c[6];
};

// s, e and full of region6 = {start xyz, size xyz} in global cells (null: the whole box); false: it does not lie in the box
inline bool mom_region_of(const GridDev& g, const int* region6, MomRegion* R)
{
  const int n[3] = {g.nx, g.ny, g.nzg};
  for (int a = 0; a < 3; ++a) {
    R->s[a] = region6 ? region6[a] : 0;
    R->e[a] = region6 ? region6[a] + region6[3 + a] : n[a];
    if (!(R->s[a] >= 0 && R->e[a] > R->s[a] && R->e[a] <= n[a])) return false;
    R->full[a] = R->s[a] == 0 && R->e[a] == n[a];
  }
  return true;
}

template <int K> struct MomDof;
template <> struct MomDof<XPIC_MOMENT_DENSITY> { static constexpr int v = 1; };
template <> struct MomDof<XPIC_MOMENT_CURRENT> { static constexpr int v = 3; };
template <> struct MomDof<XPIC_MOMENT_MOMENTUM_FLUX> { static constexpr int v = 6; };
template <> struct MomDof<XPIC_MOMENT_MOMENTUM_FLUX_DIAG> { static constexpr int v = 3; };
template <> struct MomDof<XPIC_MOMENT_MOMENTUM_FLUX_CYL> { static constexpr int v = 6; };
template <> struct MomDof<XPIC_MOMENT_MOMENTUM_FLUX_DIAG_CYL> { static constexpr int v = 3; };

// _get_v_cyl (:260-277): about the axis (geom_x / 2, geom_y / 2); a point ON the axis keeps its Cartesian components
__device__ inline void v_cyl(double x, double y, double Lx, double Ly, const double* v, double* o)
{
  const double px = x - 0.5 * Lx, py = y - 0.5 * Ly;
  const double r = hypot(px, py);
  if (isinf(1.0 / r)) {
    o[0] = v[0]; o[1] = v[1]; o[2] = v[2];
    return;
  }
  o[0] = (+px * v[0] + py * v[1]) / r;
  o[1] = (-py * v[0] + px * v[1]) / r;
  o[2] = v[2];
}

// get_density ... get_momentum_flux_diag_cyl (:212-298), components in the reference's order
template <int K>
__device__ inline void moment_of(const GridDev& g, double q, double m, double x, double y, const double* v, double* o)
{
  if (K == XPIC_MOMENT_DENSITY) o[0] = 1.0;
  if (K == XPIC_MOMENT_CURRENT) { o[0] = q * v[0]; o[1] = q * v[1]; o[2] = q * v[2]; }
  if (K == XPIC_MOMENT_MOMENTUM_FLUX) {
    o[0] = m * v[0] * v[0]; o[1] = m * v[0] * v[1]; o[2] = m * v[0] * v[2];
    o[3] = m * v[1] * v[1]; o[4] = m * v[1] * v[2]; o[5] = m * v[2] * v[2];
  }
  if (K == XPIC_MOMENT_MOMENTUM_FLUX_DIAG) { o[0] = m * v[0] * v[0]; o[1] = m * v[1] * v[1]; o[2] = m * v[2] * v[2]; }
  if (K == XPIC_MOMENT_MOMENTUM_FLUX_CYL || K == XPIC_MOMENT_MOMENTUM_FLUX_DIAG_CYL) {
    double c[3];
    v_cyl(x, y, g.Lx, g.Ly, v, c);
    if (K == XPIC_MOMENT_MOMENTUM_FLUX_CYL) {
      o[0] = m * c[0] * c[0]; o[1] = m * c[0] * c[1]; o[2] = m * c[0] * c[2];
      o[3] = m * c[1] * c[1]; o[4] = m * c[1] * c[2]; o[5] = m * c[2] * c[2];
    } else {
      o[0] = m * c[0] * c[0]; o[1] = m * c[1] * c[1]; o[2] = m * c[2] * c[2];
    }
  }
}

// DistributionMoment::Shape::setup (:137-151): start = round(r / d - 1), spline_of_1st_order about the cell centres
__device__ inline void mom_shape(const GridDev& g, const double* r, int* st, double (*w)[2])
{
  const double pr[3] = {r[0] / g.dx, r[1] / g.dy, r[2] / g.dz};
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    st[a] = (int)round(pr[a] - 1.0);
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const double d = fabs(pr[a] - ((double)(st[a] + t) + 0.5));
      w[a][t] = d <= 1.0 ? 1.0 - d : 0.0;
    }
  }
}

// the weight of corner kk (bit 0: x, bit 1: y, bit 2: z) of that shape
__device__ inline double mom_weight(const double (*w)[2], int kk)
{
  const int ix = kk & 1, iy = (kk >> 1) & 1, iz = kk >> 2;
  return ((ix ? w[0][1] : w[0][0]) * (iy ? w[1][1] : w[1][0])) * (iz ? w[2][1] : w[2][0]);
}

// A deposit at the (unwrapped) global cell (x, y, zg) -> stored node of this slab, or -1 when the region rule drops it:
// wrapped on the axes the region spans in full, then kept iff it lies in the region (DMLocalToGlobal of a
// DM_BOUNDARY_GHOSTED axis discards the ghosts).  Deposits into the planes just outside the slab land in its ghost planes.
__device__ inline long mom_target(const GridDev& g, const MomRegion& R, int x, int y, int zg)
{
  int p[3] = {x, y, zg};
  const int n[3] = {g.nx, g.ny, g.nzg};
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    if (R.full[a]) p[a] = p[a] < 0 ? p[a] + n[a] : (p[a] >= n[a] ? p[a] - n[a] : p[a]);
    if (p[a] < R.s[a] || p[a] >= R.e[a]) return -1;
  }
  int zl = p[2] - g.z0;
  if (g.G > 0) { // a deposit that wrapped across the periodic z boundary belongs to the ghost plane on the other side
    if (zl < -1) zl += g.nzg;
    else if (zl > g.nzl) zl -= g.nzg;
  }
  if (zl < -g.G || zl >= g.nzl + g.G) return -1; // (a record far from its storage cell: nothing the reference could add)
  return g.node(p[0], p[1], g.wz(zl));
}

}  // namespace xpic
