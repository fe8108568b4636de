// commands.hip -- the per-step commands of an open system on the device (the reference's src/commands/): RemoveParticles,
// InjectParticles, FieldsDamping, and the SetCoilsField and SetApproximateMirrorField setters of SetMagneticField
// (DESIGN.md 5g, 5j).
//
// Removal and injection change a sort's storage through ONE cell-wise rebuild: the new cell counts (the old ones, minus the
// emptied cells, plus the binned new records) are scanned into a new cell_start, every surviving record is moved once to
// new_start[c] + its rank in c, and the new records of a cell follow its old ones -- the reference's order inside a cell
// (the old list, then push_back).  Nothing is re-binned.  Both clear the step's carried state first (Sort::prebinned: the
// next re-binning must not reuse keys of records that are gone).
//
// The file is compiled without floating-point contraction: the geometry tests, the damping factors and the coil quadrature
// are the reference's expressions rounded step by step, so a restatement of them (tests/commands_ref.py) decides the same
// cells and damps by the same factors.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "batch.h"
#include "common.h"
#include "device_common.h"

#pragma clang fp contract(off)

namespace xpic {

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
// workgroup size of the reductions' second stage (reduce_to_host) in this file: one wave, lane l sums the partials l,
// l + 64, ...  The other files run it with 256 threads; that is a different order, and 64 is these results' order.
constexpr int kSumThreads = 64;
constexpr double kMec2 = 511.0;        // src/constants.h:30 (keV)
constexpr int kCoilN = 2000;           // SetCoilsField::N (set_magnetic_field.h:42)
constexpr double kCoilTol = 1e-10;     // SetCoilsField::denominator_tolerance (:40)

inline unsigned cgrid(int64_t n)
{
  int64_t b = (n + kBlock - 1) / kBlock;
  return (unsigned)(b < 1 ? 1 : b);
}

// grid-stride launches that leave one partial sum per workgroup (summed in a fixed order: the results do not depend on
// timing)
inline unsigned rgrid(int64_t n)
{
  int64_t b = (n + kBlock - 1) / kBlock;
  if (b > kRedBlocks) b = kRedBlocks;
  return (unsigned)(b < 1 ? 1 : b);
}

struct CmdGeom {
  int kind; // XPIC_GEOM_BOX, XPIC_GEOM_CYLINDER; -1: none (every cell passes)
  double a[7];
};

__device__ inline void cell_xyz(const GridDev& g, long c, int* x, int* y, int* zl)
{
  *x = (int)(c % g.nx);
  *y = (int)((c / g.nx) % g.ny);
  *zl = (int)(c / g.plane);
}

// RemoveParticles keeps a cell iff its corner (start + g) d passes the test (remove_particles.cpp:25-32)
__device__ inline bool keep_cell(const GridDev& g, const CmdGeom& G, long c)
{
  if (G.kind < 0) return true;
  int x, y, zl;
  cell_xyz(g, c, &x, &y, &zl);
  return within(G.kind, G.a, x * g.dx, y * g.dy, (g.z0 + zl) * g.dz);
}

// new counts: the old ones of the cells that are kept (cell_start differences: cell_count may already hold a pre-binning
// for the next step) plus the injected records; partial = records of the cells that are emptied
__global__ void __launch_bounds__(kBlock) k_cmd_count(GridDev g, const int* __restrict__ cs, CmdGeom G, const int* __restrict__ add,
  int* count, long ncell, double* partial)
{
  double gone[1] = {0.0};
  for (long c = (long)blockIdx.x * kBlock + threadIdx.x; c < ncell; c += (long)gridDim.x * kBlock) {
    const int oc = cs[c + 1] - cs[c];
    const bool keep = oc == 0 || keep_cell(g, G, c);
    count[c] = (keep ? oc : 0) + (add ? add[c] : 0);
    if (!keep) gone[0] += oc;
  }
  block_reduce_store<1, kBlock>(gone, partial, 0, blockIdx.x);
}

// One wave per cell (grid-stride over the cells): a kept cell's records are copied, coalesced, from cell_start[c] to
// ns[c]; an emptied cell's records add 0.5 (m v^2) n/Np (Energy::get_kinetic) to the wave's sum.
__global__ void __launch_bounds__(kBlock) k_cmd_move(GridDev g, SortDev s, const int* __restrict__ ns, CmdGeom G, double m,
  double mpw, long ncell, double* partial)
{
  const int lane = threadIdx.x & 63;
  const long nw = (long)gridDim.x * kWaves;
  double e[1] = {0.0};
  for (long c = (long)blockIdx.x * kWaves + (threadIdx.x >> 6); c < ncell; c += nw) {
    const int b = s.cell_start[c], cnt = s.cell_start[c + 1] - b;
    if (cnt == 0) continue;
    if (keep_cell(g, G, c)) {
      const int d = ns[c];
      for (int j = lane; j < cnt; j += 64) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          s.r2[a][d + j] = s.r[a][b + j];
          s.v2[a][d + j] = s.v[a][b + j];
        }
      }
    }
    else {
      for (int j = lane; j < cnt; j += 64) {
        const double vx = s.v[0][b + j], vy = s.v[1][b + j], vz = s.v[2][b + j];
        e[0] += 0.5 * (m * (vx * vx + vy * vy + vz * vz)) * mpw;
      }
    }
  }
  block_reduce_store<1, kBlock>(e, partial, 0, blockIdx.x);
}

// ---- InjectParticles ------------------------------------------------------------------------------------------------
struct InjDev {
  int coord;
  double geom[7];
  int mkind[2], tov[2];
  double value[2][3], T[2][3], m[2];
  uint64_t key; // stream of pair p: key + p * (odd constant), then splitmix
};

// the key of a call's streams: the seed's splitmix state, xor the step times a constant, splitmix
inline uint64_t stream_key(uint64_t seed, int64_t step)
{
  uint64_t key = seed;
  (void)splitmix(key);
  key ^= (uint64_t)step * 0xD1342543DE82EF95ull;
  return splitmix(key);
}

__device__ inline uint64_t pair_stream(const InjDev& P, int64_t p) { return P.key + (uint64_t)p * 0x2545F4914F6CDD1Dull; }

// PreciseCoordinate / CoordinateInBox / CoordinateInCylinder (particles_load.cpp:6-30), draws in the reference's order
__device__ inline void inj_coordinate(const InjDev& P, uint64_t& st, double* r)
{
  if (P.coord == XPIC_COORD_IN_BOX) {
    r[0] = P.geom[0] + u01(st) * (P.geom[3] - P.geom[0]);
    r[1] = P.geom[1] + u01(st) * (P.geom[4] - P.geom[1]);
    r[2] = P.geom[2] + u01(st) * (P.geom[5] - P.geom[2]);
  }
  else if (P.coord == XPIC_COORD_IN_CYLINDER) {
    const double rr = P.geom[3] * sqrt(u01(st));
    const double phi = 2.0 * M_PI * u01(st);
    r[0] = P.geom[0] + rr * cos(phi);
    r[1] = P.geom[1] + rr * sin(phi);
    r[2] = P.geom[2] + P.geom[4] * (u01(st) - 0.5);
  }
  else { r[0] = P.geom[0]; r[1] = P.geom[1]; r[2] = P.geom[2]; }
}

// PreciseMomentum / MaxwellianMomentum (:46-76): per axis the phase draw, then the amplitude draw
__device__ inline void inj_momentum(const InjDev& P, int k, uint64_t& st, double* p)
{
  if (P.mkind[k] == XPIC_MOMENTUM_MAXWELLIAN) {
    for (int a = 0; a < 3; ++a) {
      const double ph = sin(2.0 * M_PI * u01(st));
      const double amp = sqrt(-2.0 * (P.T[k][a] * P.m[k] / kMec2) * log(u01(st)));
      p[a] = P.value[k][a] + ph * amp;
    }
    if (P.tov[k]) {
      const double den = sqrt(P.m[k] * P.m[k] + (p[0] * p[0] + p[1] * p[1] + p[2] * p[2]));
      p[0] /= den; p[1] /= den; p[2] /= den;
    }
  }
  else { p[0] = P.value[k][0]; p[1] = P.value[k][1]; p[2] = P.value[k][2]; }
}

// the pair's coordinate -> local cell (add_particle's FLOOR_STEP test), its arrival rank among the cell's new records
__global__ void __launch_bounds__(kBlock) k_inj_bin(GridDev g, InjDev P, int64_t pairs, int* add, int* prank, int* nadded)
{
  const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  int c = -1;
  if (p < pairs) {
    uint64_t st = pair_stream(P, p);
    double r[3];
    inj_coordinate(P, st, r);
    c = cell_of(g, r[0], r[1], r[2]);
    prank[p] = c >= 0 ? atomicAdd(&add[c], 1) : -1;
  }
  const unsigned long long in = __ballot(c >= 0);
  if ((threadIdx.x & 63) == 0 && in) atomicAdd(nadded, __popcll(in));
}

// the added pairs' records of sort k, after the cell's old ones: ns[c] + (count[c] - add[c]) + rank; partial rows: energy
template <int K>
__global__ void __launch_bounds__(kBlock) k_inj_write(GridDev g, SortDev s, InjDev P, int64_t pairs, const int* __restrict__ ns,
  const int* __restrict__ count, const int* __restrict__ add, const int* __restrict__ prank, double mpw, double* partial)
{
  double e[1] = {0.0};
  for (int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x; p < pairs; p += (int64_t)gridDim.x * kBlock) {
    const int rk = prank[p];
    if (rk < 0) continue;
    uint64_t st = pair_stream(P, p);
    double r[3], pm[2][3];
    inj_coordinate(P, st, r);
    inj_momentum(P, 0, st, pm[0]);
    inj_momentum(P, 1, st, pm[1]);
    const int c = cell_of(g, r[0], r[1], r[2]);
    const long d = (long)ns[c] + (count[c] - add[c]) + rk;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      s.r2[a][d] = r[a];
      s.v2[a][d] = pm[K][a];
    }
    const double* v = pm[K];
    e[0] += 0.5 * (P.m[K] * (v[0] * v[0] + v[1] * v[1] + v[2] * v[2])) * mpw;
  }
  block_reduce_store<1, kBlock>(e, partial, 0, blockIdx.x);
}

// ---- SetParticles (include/xpic_set_particles.h) ---------------------------------------------------------------------
// particle p draws from pair p's stream: its coordinate, then its momentum.  I: the part InjectParticles' generators read
// (sort 0 of it); the rest belongs to CoordinateOnAnnulus, MaxwellCosinePerturbation and AngularMomentum.
struct SetDev {
  InjDev I;
  int coord, mom;
  double amp[3], wn[3], L[3], center[2];
};

// CoordinateOnAnnulus (particles_load.cpp:32-44); the other three are inj_coordinate
__device__ inline void set_coordinate(const SetDev& P, uint64_t& st, double* r)
{
  if (P.coord != XPIC_COORD_ON_ANNULUS) return inj_coordinate(P.I, st, r);
  const double* g = P.I.geom;
  const double rr = sqrt(g[3] * g[3] + (g[4] * g[4] - g[3] * g[3]) * u01(st));
  const double phi = 2.0 * M_PI * u01(st);
  r[0] = g[0] + rr * cos(phi);
  r[1] = g[1] + rr * sin(phi);
  r[2] = g[2] + g[5] * (u01(st) - 0.5);
}

// temperature_momentum (:52-55)
__device__ inline double set_thermal(const SetDev& P, int a, uint64_t& st)
{
  return sqrt(-2.0 * (P.I.T[0][a] * P.I.m[0] / kMec2) * log(u01(st)));
}

// MaxwellCosinePerturbation (:78-103, L of this call's box) and AngularMomentum (:105-125) as written; the other two are
// inj_momentum
__device__ inline void set_momentum(const SetDev& P, uint64_t& st, const double* r, double* p)
{
  if (P.mom == XPIC_MOMENTUM_COSINE_PERTURBATION) {
    const double m = P.I.m[0];
    for (int a = 0; a < 3; ++a) {
      const double ph = sin(2.0 * M_PI * u01(st));
      p[a] = ph * set_thermal(P, a, st);
    }
    const double den = sqrt(m * m + (p[0] * p[0] + p[1] * p[1] + p[2] * p[2]));
    for (int a = 0; a < 3; ++a) {
      p[a] /= den;
      const double v0 = P.amp[a] * sqrt(P.I.T[0][a] / (m * kMec2));
      p[a] += v0 * cos(2.0 * M_PI * P.wn[a] * r[a] / P.L[a]);
    }
  }
  else if (P.mom == XPIC_MOMENTUM_ANGULAR) {
    const double x = r[0] - P.center[0], y = r[1] - P.center[1];
    const double rr = hypot(x, y);
    const double t[3] = {set_thermal(P, 0, st), set_thermal(P, 1, st), set_thermal(P, 2, st)};
    const double* v = P.I.value[0];
    if (isinf(1.0 / rr)) { p[0] = 0.0 + t[0]; p[1] = 0.0 + t[1]; }
    else { p[0] = -v[0] * (y / rr) + t[0]; p[1] = +v[1] * (x / rr) + t[1]; }
    p[2] = v[2] + t[2];
  }
  else inj_momentum(P.I, 0, st, p);
}

// first pass over the particles p0 + [0, n) (grid-stride): the new records of every local cell, and their number (summed
// over the wave, one atomic per wave and launch: a single counter taken once per 64 particles serialises the pass)
__global__ void __launch_bounds__(kBlock) k_set_count(GridDev g, SetDev P, int64_t p0, int64_t n, int* add,
  unsigned long long* nadded)
{
  int mine = 0;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
    uint64_t st = pair_stream(P.I, p0 + i);
    double r[3];
    set_coordinate(P, st, r);
    const int c = cell_of(g, r[0], r[1], r[2]);
    if (c >= 0) {
      atomicAdd(&add[c], 1);
      ++mine;
    }
  }
  for (int o = 32; o > 0; o >>= 1) mine += __shfl_down(mine, o, 64);
  if ((threadIdx.x & 63) == 0 && mine) atomicAdd(nadded, (unsigned long long)mine);
}

// second pass: the particle's record behind its cell's old records (cs: the old cell_start, ns: the new one), in the
// slot the cell's cursor hands out; partial: the energy of the records written
__global__ void __launch_bounds__(kBlock) k_set_write(GridDev g, SortDev s, SetDev P, int64_t p0, int64_t n,
  const int* __restrict__ ns, int* cursor, double mpw, double* partial)
{
  double e[1] = {0.0};
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
    uint64_t st = pair_stream(P.I, p0 + i);
    double r[3], pm[3];
    set_coordinate(P, st, r);
    const int c = cell_of(g, r[0], r[1], r[2]);
    if (c < 0) continue;
    set_momentum(P, st, r, pm);
    const long d = (long)ns[c] + (s.cell_start[c + 1] - s.cell_start[c]) + atomicAdd(&cursor[c], 1);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      s.r2[a][d] = r[a];
      s.v2[a][d] = pm[a];
    }
    e[0] += 0.5 * (P.I.m[0] * (pm[0] * pm[0] + pm[1] * pm[1] + pm[2] * pm[2])) * mpw;
  }
  block_reduce_store<1, kBlock>(e, partial, 0, blockIdx.x);
}

// ---- FieldsDamping ---------------------------------------------------------------------------------------------------
// DampForBox / DampForCylinder (fields_damping.cpp:71-111) as written
__device__ inline double damp_factor(const GridDev& g, const CmdGeom& G, double coef, const double* r)
{
  if (G.kind == XPIC_GEOM_BOX) {
    const double L[3] = {g.Lx, g.Ly, g.Lz};
    double damping = 1.0;
    for (int i = 0; i < 3; ++i) {
      double width = 0.0, delta = 0.0;
      if (r[i] > G.a[3 + i]) { width = L[i] - G.a[3 + i]; delta = r[i] - G.a[3 + i]; }
      else if (r[i] < G.a[i]) { width = G.a[i] - 0; delta = r[i] - 0; }
      else continue;
      const double q = delta / width - 1.0;
      damping *= 1.0 - coef * (q * q);
    }
    return damping;
  }
  const double rr = hypot(r[0] - G.a[0], r[1] - G.a[1]);
  if (rr < G.a[3]) return 1.0;
  const double width = G.a[0] - G.a[3];
  const double delta = rr - G.a[3];
  const double delta0 = width * (1.0 + 1.0 / sqrt(coef));
  double damping = 0.0;
  if (delta < delta0) {
    const double q = delta / width - 1.0;
    damping = 1.0 - coef * (q * q);
  }
  return damping;
}

// E and B - B0 at every owned node; B = (B - B0) (damped) + B0 everywhere, as the two VecAXPY around the damping leave it
__global__ void __launch_bounds__(kBlock) k_damp(GridDev g, double* E, double* B, const double* __restrict__ B0, CmdGeom G,
  double coef, double* partial)
{
  double e[1] = {0.0};
  for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < g.nown; i += (long)gridDim.x * kBlock) {
    int x, y, zl;
    cell_xyz(g, i, &x, &y, &zl);
    const long nd = g.node(x, y, g.wz(zl));
    const double r[3] = {(x + 0.5) * g.dx, (y + 0.5) * g.dy, (g.z0 + zl + 0.5) * g.dz};
    double fe[3], fb[3], b0[3];
    for (int a = 0; a < 3; ++a) {
      fe[a] = E[a * g.cstride + nd];
      b0[a] = B0[a * g.cstride + nd];
      fb[a] = B[a * g.cstride + nd] + (-1.0 * b0[a]);
    }
    if (!within(G.kind, G.a, r[0], r[1], r[2])) {
      const double d = damp_factor(g, G, coef, r);
      const double k = 1.0 - d * d;
      e[0] += (0.5 * (fe[0] * fe[0] + fe[1] * fe[1] + fe[2] * fe[2])) * k;
      e[0] += (0.5 * (fb[0] * fb[0] + fb[1] * fb[1] + fb[2] * fb[2])) * k;
      for (int a = 0; a < 3; ++a) {
        fe[a] *= d;
        fb[a] *= d;
        E[a * g.cstride + nd] = fe[a];
      }
    }
    for (int a = 0; a < 3; ++a) B[a * g.cstride + nd] = fb[a] + 1.0 * b0[a];
  }
  block_reduce_store<1, kBlock>(e, partial, 0, blockIdx.x);
}

// ---- SetCoilsField ---------------------------------------------------------------------------------------------------
// get_integ_r / get_integ_z (set_magnetic_field.cpp:118-150) of one coil, summed in the reference's order
template <bool RADIAL>
__device__ inline double coil_integral(const double* __restrict__ cs, double z, double r, double R)
{
  double integral = 0.0;
  for (int i = 0; i < kCoilN; ++i) {
    double den = z * z + R * R + r * r - 2.0 * R * r * cs[i];
    if (fabs(den) < kCoilTol) den = kCoilTol;
    integral += (RADIAL ? cs[i] : (R - r * cs[i])) / (den * sqrt(den));
  }
  return (2 * M_PI / kCoilN) * integral;
}

__device__ inline double coils_Br(const double* cs, const double* coils, int nc, double z, double r)
{
  double Br = 0.0;
  for (int k = 0; k < nc; ++k) {
    const double zc = z - coils[3 * k], R = coils[3 * k + 1], I = coils[3 * k + 2];
    Br += I * R * zc * coil_integral<true>(cs, zc, r, R);
  }
  return Br;
}

__device__ inline double coils_Bz(const double* cs, const double* coils, int nc, double z, double r)
{
  double Bz = 0.0;
  for (int k = 0; k < nc; ++k) {
    const double zc = z - coils[3 * k], R = coils[3 * k + 1], I = coils[3 * k + 2];
    Bz += I * R * coil_integral<false>(cs, zc, r, R);
  }
  return Bz;
}

// SetCoilsField::operator() (:38-102): one thread per owned node, F += the three components at their staggered positions
__global__ void __launch_bounds__(kBlock) k_coils(GridDev g, double* F, const double* __restrict__ cs, const double* __restrict__ coils,
  int nc, long i0, long i1)
{
  const long i = i0 + (long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= i1) return;
  int x, y, zl;
  cell_xyz(g, i, &x, &y, &zl);
  const int z = g.z0 + zl;
  const long nd = g.node(x, y, g.wz(zl));
  const double cx = 0.5 * g.Lx, cy = 0.5 * g.Ly;
  double sx, sy, sz, r;

  sx = x * g.dx - cx;
  sy = (y + 0.5) * g.dy - cy;
  sz = (z + 0.5) * g.dz;
  r = hypot(sx, sy);
  F[nd] += coils_Br(cs, coils, nc, sz, r) * sx / r;

  sy = y * g.dy - cy;
  sx = (x + 0.5) * g.dx - cx;
  sz = (z + 0.5) * g.dz;
  r = hypot(sx, sy);
  F[g.cstride + nd] += coils_Br(cs, coils, nc, sz, r) * sy / r;

  sz = z * g.dz;
  sx = (x + 0.5) * g.dx - cx;
  sy = (y + 0.5) * g.dy - cy;
  r = hypot(sx, sy);
  F[2 * g.cstride + nd] += coils_Bz(cs, coils, nc, sz, r);
}

// ---- SetApproximateMirrorField ---------------------------------------------------------------------------------------
// get_B0 / get_B1 (set_magnetic_field.cpp:183-191); sign is a PetscReal there
__device__ inline double mirror_B0(double z, double sign, double D, double R, double I)
{
  const double zc = z + 0.5 * sign * D;
  return 0.5 * I * (R * R) / pow(R * R + zc * zc, 1.5);
}
__device__ inline double mirror_B1(double z, double sign, double D, double R)
{
  const double zc = z + 0.5 * sign * D;
  return zc / (R * R + zc * zc);
}

// SetApproximateMirrorField::operator() (:142-181) as written, one thread per owned node: both transverse terms go to
// the X component, at (z + 1/2) dz; Bz at z dz; the Y component is left alone
__global__ void __launch_bounds__(kBlock) k_mirror(GridDev g, double* F, double D, double R, double I)
{
  const long i = (long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= g.nown) return;
  int x, y, zl;
  cell_xyz(g, i, &x, &y, &zl);
  const int z = g.z0 + zl;
  const long nd = g.node(x, y, g.wz(zl));
  double sz, sm;
  double fx = F[nd], fz = F[2 * g.cstride + nd];

  sz = (z + 0.5) * g.dz;
  sm = 1.5 * (x * g.dx - 0.5 * g.Lx);
  fx += mirror_B0(sz, +1.0, D, R, I) * sm * mirror_B1(sz, +1.0, D, R);
  fx += mirror_B0(sz, -1.0, D, R, I) * sm * mirror_B1(sz, -1.0, D, R);

  sz = (z + 0.5) * g.dz;
  sm = 1.5 * (y * g.dy - 0.5 * g.Ly);
  fx += mirror_B0(sz, +1.0, D, R, I) * sm * mirror_B1(sz, +1.0, D, R);
  fx += mirror_B0(sz, -1.0, D, R, I) * sm * mirror_B1(sz, -1.0, D, R);

  sz = z * g.dz;
  fz += mirror_B0(sz, +1.0, D, R, I);
  fz += mirror_B0(sz, -1.0, D, R, I);
  F[nd] = fx;
  F[2 * g.cstride + nd] = fz;
}

int cmd_geom(int geometry, const double* geom, CmdGeom* G)
{
  XPIC_CHECK(geom, "null geometry");
  XPIC_CHECK(geometry == XPIC_GEOM_BOX || geometry == XPIC_GEOM_CYLINDER, "unknown geometry kind");
  G->kind = geometry;
  for (int i = 0; i < 7; ++i) G->a[i] = geom[i];
  return 0;
}

int cmd_scratch(xpic_ctx* c)
{
  if (!c->cmd_start) {
    XPIC_HIP(hipMalloc(&c->cmd_start, sizeof(int) * (c->ncell + 1 + kCellStartPad)));
    XPIC_HIP(hipMemsetAsync(c->cmd_start, 0, sizeof(int) * (c->ncell + 1 + kCellStartPad), c->stream));
  }
  if (!c->cmd_add) XPIC_HIP(hipMalloc(&c->cmd_add, sizeof(int) * (c->ncell + 1)));
  return 0;
}

// the new order of a sort whose new counts are in cell_count: scan, move the kept records (energy of the others into
// partial[0 .. nblocks)), then `extra` writes the new records into r2 / v2 before the buffers are swapped
template <class Extra>
int cmd_rebuild(xpic_ctx* c, Sort& s, const CmdGeom& G, int* total, Extra extra)
{
  XPIC_CALL(exclusive_scan(c, s.d.cell_count, c->ncell, c->cmd_start, total));
  XPIC_CHECK(*total <= s.cap, "sort capacity exceeded in a command"); // (checked by the callers before anything changed)
  hipLaunchKernelGGL(k_cmd_move, dim3(kRedBlocks), dim3(kBlock), 0, c->stream, c->g, s.d, c->cmd_start, G, s.par.m,
    s.par.n / s.par.Np, (long)c->ncell, c->red_partial);
  XPIC_HIP(hipGetLastError());
  XPIC_CALL(extra());
  for (int a = 0; a < 3; ++a) {
    std::swap(s.d.r[a], s.d.r2[a]);
    std::swap(s.d.v[a], s.d.v2[a]);
  }
  std::swap(s.d.cell_start, c->cmd_start); // (both ncell + 1 + kCellStartPad)
  s.n = *total;
  return 0;
}

}  // namespace

int remove_particles(xpic_ctx* c, Sort& s, int geometry, const double* geom, int64_t* removed, double* energy)
{
  CmdGeom G;
  XPIC_CALL(cmd_geom(geometry, geom, &G));
  XPIC_CALL(sort_materialize(c, s)); // (a deferred re-binning whose assembly has not run)
  s.prebinned = false;               // (the keys of a pre-binning describe records this call may remove)
  XPIC_CALL(cmd_scratch(c));
  Timed t(c, "cmd_remove");
  double res[2] = {0.0, 0.0}; // records removed, energy
  if (s.n > 0) {
    const unsigned nb = rgrid(c->ncell);
    // (cell_count is rewritten even when nothing is removed: then with the old counts.  That is safe because the
    // pre-binning that may have held other counts there was dropped above.)
    hipLaunchKernelGGL(k_cmd_count, dim3(nb), dim3(kBlock), 0, c->stream, c->g, s.d.cell_start, G, (const int*)nullptr,
      s.d.cell_count, (long)c->ncell, c->red_partial);
    XPIC_HIP(hipGetLastError());
    XPIC_CALL(reduce_to_host(c, 1, nb, 1, false, res, kSumThreads));
    if (res[0] > 0) { // (otherwise no record is touched)
      int total = 0;
      XPIC_CALL(cmd_rebuild(c, s, G, &total, [] { return 0; }));
      XPIC_CALL(reduce_to_host(c, 1, kRedBlocks, 1, false, res + 1, kSumThreads));
    }
  }
  XPIC_CALL(comm_allreduce_sum_host(c, res, 2)); // (log_statistics, remove_particles.cpp:47-48)
  if (removed) *removed = (int64_t)res[0];
  if (energy) *energy = res[1];
  return 0;
}

int inject_particles(xpic_ctx* c, Sort& si, Sort& se, const xpic_inject_params& p, int64_t pairs, int64_t step,
  int64_t* added, double* energy2)
{
  XPIC_CHECK(&si != &se, "inject_particles: the ionized and the ejected sort must differ");
  XPIC_CHECK(pairs >= 0 && pairs < (int64_t)2147483000, "inject_particles: pairs must be in [0, 2^31)");
  XPIC_CHECK(p.coordinate >= XPIC_COORD_PRECISE && p.coordinate <= XPIC_COORD_IN_CYLINDER, "unknown coordinate generator");
  InjDev P{};
  P.coord = p.coordinate;
  for (int i = 0; i < 7; ++i) P.geom[i] = p.geom[i];
  Sort* sorts[2] = {&si, &se};
  for (int k = 0; k < 2; ++k) {
    const xpic_momentum_params& m = p.momentum[k];
    XPIC_CHECK(m.kind == XPIC_MOMENTUM_PRECISE || m.kind == XPIC_MOMENTUM_MAXWELLIAN, "unknown momentum generator");
    P.mkind[k] = m.kind;
    P.tov[k] = m.tov;
    for (int a = 0; a < 3; ++a) { P.value[k][a] = m.value[a]; P.T[k][a] = m.T[a]; }
    P.m[k] = sorts[k]->par.m;
  }
  P.key = stream_key(p.seed, step);
  for (Sort* s : sorts) {
    XPIC_CALL(sort_materialize(c, *s)); // (a deferred re-binning whose assembly has not run)
    s->prebinned = false;               // (a pre-binning's keys would be taken for the new records' next step)
  }
  XPIC_CALL(cmd_scratch(c));
  if (c->cmd_rank_n < pairs) {
    if (c->cmd_rank) XPIC_HIP(hipFree(c->cmd_rank));
    c->cmd_rank = nullptr;
    XPIC_HIP(hipMalloc(&c->cmd_rank, sizeof(int) * pairs));
    c->cmd_rank_n = pairs;
  }
  Timed t(c, "cmd_inject");
  int* nadd = (int*)(c->red_out + 64);
  XPIC_HIP(hipMemsetAsync(c->cmd_add, 0, sizeof(int) * (c->ncell + 1), c->stream));
  XPIC_HIP(hipMemsetAsync(nadd, 0, sizeof(int), c->stream));
  if (pairs > 0) {
    hipLaunchKernelGGL(k_inj_bin, dim3(cgrid(pairs)), dim3(kBlock), 0, c->stream, c->g, P, pairs, c->cmd_add, c->cmd_rank, nadd);
    XPIC_HIP(hipGetLastError());
  }
  int hn = 0;
  XPIC_HIP(hipMemcpyAsync(&hn, nadd, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  XPIC_HIP(hipStreamSynchronize(c->stream));
  // capacity, agreed on by all slabs before any sort changes (a slab that returned alone would hang the others)
  double over[1] = {(si.n + hn > si.cap || se.n + hn > se.cap) ? 1.0 : 0.0};
  XPIC_CALL(comm_allreduce_sum_host(c, over, 1));
  XPIC_CHECK(over[0] == 0.0, "sort capacity exceeded in inject_particles");
  double res[3] = {(double)hn, 0.0, 0.0}; // pairs added, energy ionized, energy ejected
  if (hn > 0) {
    const CmdGeom none{-1, {0, 0, 0, 0, 0, 0, 0}};
    for (int k = 0; k < 2; ++k) {
      Sort& s = *sorts[k];
      const unsigned nb = rgrid(c->ncell);
      hipLaunchKernelGGL(k_cmd_count, dim3(nb), dim3(kBlock), 0, c->stream, c->g, s.d.cell_start, none, (const int*)c->cmd_add,
        s.d.cell_count, (long)c->ncell, c->red_partial);
      XPIC_HIP(hipGetLastError());
      int total = 0;
      const unsigned nw = rgrid(pairs);
      XPIC_CALL(cmd_rebuild(c, s, none, &total, [&]() -> int {
        SortDev sd = s.d;
        const double mpw = s.par.n / s.par.Np;
        if (k == 0)
          hipLaunchKernelGGL(k_inj_write<0>, dim3(nw), dim3(kBlock), 0, c->stream, c->g, sd, P, pairs, c->cmd_start,
            s.d.cell_count, c->cmd_add, c->cmd_rank, mpw, c->red_partial);
        else
          hipLaunchKernelGGL(k_inj_write<1>, dim3(nw), dim3(kBlock), 0, c->stream, c->g, sd, P, pairs, c->cmd_start,
            s.d.cell_count, c->cmd_add, c->cmd_rank, mpw, c->red_partial);
        XPIC_HIP(hipGetLastError());
        return 0;
      }));
      XPIC_CALL(reduce_to_host(c, 1, nw, 1, false, res + 1 + k, kSumThreads));
    }
  }
  XPIC_CALL(comm_allreduce_sum_host(c, res, 3)); // (log_statistics, inject_particles.cpp:70-84)
  if (added) *added = (int64_t)res[0];
  if (energy2) { energy2[0] = res[1]; energy2[1] = res[2]; }
  return 0;
}

namespace {

const char* const kSetWho = "xpic_set_particles: ";

bool all_finite(const double* v, int n)
{
  for (int i = 0; i < n; ++i)
    if (!std::isfinite(v[i])) return false;
  return true;
}

// the argument checks of set_particles; nothing has been touched when one of them fails
int set_particles_params(const Sort& s, const xpic_set_particles_params& p, int64_t n, int64_t particle0, SetDev* P)
{
  const std::string who = kSetWho;
  XPIC_CHECK(n >= 0 && particle0 >= 0 && p.chunk >= 0, who + "n, particle0 and chunk must not be negative");
  XPIC_CHECK(particle0 <= INT64_MAX - n, who + "particle0 + n overflows");
  XPIC_CHECK(p.coordinate >= XPIC_COORD_PRECISE && p.coordinate <= XPIC_COORD_ON_ANNULUS, who + "unknown coordinate generator");
  XPIC_CHECK(p.momentum >= XPIC_MOMENTUM_PRECISE && p.momentum <= XPIC_MOMENTUM_ANGULAR, who + "unknown momentum generator");
  XPIC_CHECK(std::isfinite(s.par.m) && s.par.m != 0.0 && s.par.Np > 0 && std::isfinite(s.par.n),
    who + "the sort has no mass or no Np");
  const int ngeom[4] = {3, 6, 5, 6};
  XPIC_CHECK(all_finite(p.geom, ngeom[p.coordinate]), who + "non-finite geometry");
  if (p.coordinate == XPIC_COORD_IN_CYLINDER) XPIC_CHECK(p.geom[3] >= 0.0, who + "negative radius");
  if (p.coordinate == XPIC_COORD_ON_ANNULUS)
    XPIC_CHECK(p.geom[3] >= 0.0 && p.geom[4] >= p.geom[3], who + "the annulus needs 0 <= inner_r <= outer_r");
  *P = SetDev{};
  P->coord = P->I.coord = p.coordinate;
  P->mom = P->I.mkind[0] = p.momentum;
  P->I.tov[0] = p.tov;
  P->I.m[0] = s.par.m;
  for (int i = 0; i < 7; ++i) P->I.geom[i] = p.geom[i];
  if (p.momentum != XPIC_MOMENTUM_COSINE_PERTURBATION) {
    XPIC_CHECK(all_finite(p.value, 3), who + "non-finite momentum");
    for (int a = 0; a < 3; ++a) P->I.value[0][a] = p.value[a];
  }
  if (p.momentum != XPIC_MOMENTUM_PRECISE) {
    XPIC_CHECK(all_finite(p.T, 3) && p.T[0] >= 0.0 && p.T[1] >= 0.0 && p.T[2] >= 0.0, who + "T must be finite and not negative");
    for (int a = 0; a < 3; ++a) P->I.T[0][a] = p.T[a];
  }
  if (p.momentum == XPIC_MOMENTUM_COSINE_PERTURBATION) {
    XPIC_CHECK(all_finite(p.amplitude, 3) && all_finite(p.wave_number, 3) && all_finite(p.box6, 6),
      who + "non-finite perturbation");
    for (int a = 0; a < 3; ++a) {
      P->amp[a] = p.amplitude[a];
      P->wn[a] = p.wave_number[a];
      P->L[a] = p.box6[3 + a] - p.box6[a];
      XPIC_CHECK(P->L[a] != 0.0, who + "the perturbation's box has no extent");
    }
  }
  if (p.momentum == XPIC_MOMENTUM_ANGULAR) {
    XPIC_CHECK(all_finite(p.center, 2), who + "non-finite center");
    P->center[0] = p.center[0];
    P->center[1] = p.center[1];
  }
  return 0;
}

}  // namespace

int set_particles(xpic_ctx* c, Sort& s, const xpic_set_particles_params& p, int64_t n, int64_t particle0, int64_t step,
  int64_t* added, double* energy)
{
  SetDev P;
  XPIC_CALL(set_particles_params(s, p, n, particle0, &P));
  P.I.key = stream_key(p.seed, step);
  if (added) *added = 0;
  if (energy) *energy = 0.0;
  if (n == 0) return 0;
  const int64_t chunk = p.chunk > 0 ? p.chunk : (int64_t)XPIC_SET_PARTICLES_CHUNK;
  XPIC_CALL(sort_materialize(c, s)); // (a deferred re-binning whose assembly has not run)
  XPIC_CALL(cmd_scratch(c));
  Timed t(c, "cmd_set_particles");
  // pass 1, every chunk: the new records per cell and their number
  unsigned long long* nadd = (unsigned long long*)(c->red_out + 64);
  XPIC_HIP(hipMemsetAsync(c->cmd_add, 0, sizeof(int) * (c->ncell + 1), c->stream));
  XPIC_HIP(hipMemsetAsync(nadd, 0, sizeof(unsigned long long), c->stream));
  for (int64_t i0 = 0; i0 < n; i0 += chunk) {
    Timed tc(c, "cmd_set_count");
    const int64_t ni = std::min(chunk, n - i0);
    hipLaunchKernelGGL(k_set_count, dim3(rgrid(ni)), dim3(kBlock), 0, c->stream, c->g, P, particle0 + i0, ni, c->cmd_add, nadd);
    XPIC_HIP(hipGetLastError());
  }
  unsigned long long hn = 0;
  XPIC_HIP(hipMemcpyAsync(&hn, nadd, sizeof(hn), hipMemcpyDeviceToHost, c->stream));
  XPIC_HIP(hipStreamSynchronize(c->stream));
  // capacity (and the range of the cells' int counts and offsets: a cell's count that wrapped has hn beyond it), agreed on
  // by all slabs before the sort changes (a slab that returned alone would hang the others)
  const unsigned long long total_n = (unsigned long long)s.n + hn;
  double over[1] = {(total_n > (unsigned long long)s.cap || total_n > 2147483000ull) ? 1.0 : 0.0};
  XPIC_CALL(comm_allreduce_sum_host(c, over, 1));
  XPIC_CHECK(over[0] == 0.0, std::string(kSetWho) + "sort capacity exceeded");
  double res[2] = {(double)hn, 0.0}; // particles added, their energy
  if (hn > 0) {
    s.prebinned = false; // (a pre-binning's keys would be taken for the new records' next step)
    const CmdGeom none{-1, {0, 0, 0, 0, 0, 0, 0}};
    const unsigned nb = rgrid(c->ncell);
    hipLaunchKernelGGL(k_cmd_count, dim3(nb), dim3(kBlock), 0, c->stream, c->g, s.d.cell_start, none, (const int*)c->cmd_add,
      s.d.cell_count, (long)c->ncell, c->red_partial);
    XPIC_HIP(hipGetLastError());
    int total = 0;
    XPIC_CALL(cmd_rebuild(c, s, none, &total, [&]() -> int {
      // pass 2, every chunk: cmd_add becomes the cells' cursors; one energy per chunk, summed in the chunks' order
      XPIC_HIP(hipMemsetAsync(c->cmd_add, 0, sizeof(int) * (c->ncell + 1), c->stream));
      for (int64_t i0 = 0; i0 < n; i0 += chunk) {
        Timed tw(c, "cmd_set_write");
        const int64_t ni = std::min(chunk, n - i0);
        const unsigned nw = rgrid(ni);
        hipLaunchKernelGGL(k_set_write, dim3(nw), dim3(kBlock), 0, c->stream, c->g, s.d, P, particle0 + i0, ni, c->cmd_start,
          c->cmd_add, s.par.n / s.par.Np, c->red_partial);
        XPIC_HIP(hipGetLastError());
        double e = 0.0;
        XPIC_CALL(reduce_to_host(c, 1, nw, 1, false, &e, kSumThreads));
        res[1] += e;
      }
      return 0;
    }));
  }
  XPIC_CALL(comm_allreduce_sum_host(c, res, 2)); // (log_statistics, set_particles.cpp:49-51)
  if (added) *added = (int64_t)res[0];
  if (energy) *energy = res[1];
  return 0;
}

int particles_number(xpic_ctx* c, const Sort& s, int coordinate, const double* geom, int64_t* out)
{
  const std::string who = "xpic_particles_number: ";
  XPIC_CHECK(geom && out, who + "null argument");
  XPIC_CHECK(coordinate >= XPIC_COORD_PRECISE && coordinate <= XPIC_COORD_ON_ANNULUS, who + "unknown coordinate generator");
  const int Np = s.par.Np;
  const double frac = Np / (c->g.dx * c->g.dy * c->g.dz); // particles_builder.cpp:17
  double v;
  if (coordinate == XPIC_COORD_PRECISE) v = Np;
  else if (coordinate == XPIC_COORD_IN_BOX) v = (geom[3] - geom[0]) * (geom[4] - geom[1]) * (geom[5] - geom[2]) * frac;
  else if (coordinate == XPIC_COORD_IN_CYLINDER) v = M_PI * (geom[3] * geom[3]) * geom[4] * frac;
  else v = M_PI * (geom[4] * geom[4] - geom[3] * geom[3]) * geom[5] * frac;
  XPIC_CHECK(std::isfinite(v) && std::fabs(v) < 9.0e18, who + "the count is not a 64-bit integer");
  *out = (int64_t)v; // (the conversion to PetscInt truncates)
  return 0;
}

int fields_damping(xpic_ctx* c, double* E, double* B, const double* B0, int geometry, const double* geom, double coefficient,
  double* energy)
{
  CmdGeom G;
  XPIC_CALL(cmd_geom(geometry, geom, &G));
  Timed t(c, "cmd_damp");
  const unsigned nb = rgrid(c->g.nown);
  hipLaunchKernelGGL(k_damp, dim3(nb), dim3(kBlock), 0, c->stream, c->g, E, B, B0, G, coefficient, c->red_partial);
  XPIC_HIP(hipGetLastError());
  double e[1];
  XPIC_CALL(reduce_to_host(c, 1, nb, 1, false, e, kSumThreads));
  XPIC_CALL(comm_allreduce_sum_host(c, e, 1)); // (execute, fields_damping.cpp:29)
  if (energy) *energy = e[0];
  return 0;
}

int set_coils_field(xpic_ctx* c, double* F, int ncoils, const double* coils3)
{
  XPIC_CHECK(ncoils >= 0 && (ncoils == 0 || coils3), "set_coils_field: null coils");
  if (ncoils == 0) return 0;
  // the cosine table of the SetCoilsField constructor (:31-32), taken from the host's std::cos as there
  std::vector<double> h(kCoilN + 3 * (size_t)ncoils);
  for (int i = 0; i < kCoilN; ++i) h[i] = std::cos(i * (2 * M_PI / kCoilN));
  for (int i = 0; i < 3 * ncoils; ++i) h[kCoilN + i] = coils3[i];
  DevScratch<double> d;
  XPIC_CALL(d.alloc(h.size()));
  Timed t(c, "cmd_coils");
  XPIC_CALL(upload(d, h.data(), h.size(), c->stream));
  // 6000 fp64 divisions and square roots per node and coil: ~0.23 s for two coils at 256^3, linear in nodes x coils.
  // The launch is split into groups of whole planes of at most ~2^21 nodes x coils (~14 ms each at 256^3), so no single
  // kernel runs for seconds on a larger grid or with more coils.
  const long plane = c->g.plane;
  const long per = std::max(1L, (1L << 21) / (plane * ncoils)) * plane;
  for (long i0 = 0; i0 < c->g.nown; i0 += per) {
    const long i1 = std::min(c->g.nown, i0 + per);
    hipLaunchKernelGGL(k_coils, dim3(cgrid(i1 - i0)), dim3(kBlock), 0, c->stream, c->g, F, d.p, d.p + kCoilN, ncoils, i0, i1);
    XPIC_HIP(hipGetLastError());
  }
  XPIC_HIP(hipStreamSynchronize(c->stream));
  return 0;
}

int set_mirror_field(xpic_ctx* c, double* F, double D, double R, double I)
{
  Timed t(c, "cmd_mirror");
  hipLaunchKernelGGL(k_mirror, dim3(cgrid(c->g.nown)), dim3(kBlock), 0, c->stream, c->g, F, D, R, I);
  XPIC_HIP(hipGetLastError());
  XPIC_HIP(hipStreamSynchronize(c->stream));
  return 0;
}

}  // namespace xpic
