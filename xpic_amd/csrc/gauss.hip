// gauss.hip -- Gauss's law on the device (include/xpic_gauss.h; an extension: the reference has no Gauss-law cleaner):
// the residual res = D F - (rho - mean rho) of a field, and the cleaner F <- F - G phi with D G phi = res solved by
// conjugate gradients on the scalar 7-point Laplacian.  D is k_div_neg_add's divergence (fields.hip), G the forward
// difference on the Yee edges, so that D G is symmetric and rot(+) G = 0.  All kernels are streaming kernels over one
// component's planes: a scalar lives as one component of a stored vector (planes p, r, Ap of one, phi, rho, res of a
// second), and no kernel here reads more than the planes it names.  One CG iteration moves 11 scalar vectors, as
// krylov.hip's CG on matM moves 11 3-vectors: k_lap_dot (2), k_gauss_update (6), k_gauss_dir (3), two small reductions.
// poisson_direct is the other solve (include/xpic_poisson.h): poisson.hip's transform solve with iterative refinement, on
// the planes p and Ap as its work planes; the entry points of that header stand at the end of this file.
#include <cmath>

#include "common.h"
#include "device_common.h"

namespace xpic {

namespace {

constexpr int kBlock = 256;

// planes of the two work vectors
enum { kP = 0, kR = 1, kAp = 2, kPhi = 3, kRho = 4, kRes = 5 };

inline double* plane_of(xpic_ctx* c, int which) { return c->gauss_ws + (long)(which / 3) * c->nvec + (long)(which % 3) * c->g.cstride; }
inline double* vector_of(xpic_ctx* c, int which) { return c->gauss_ws + (long)(which / 3) * c->nvec; }

inline unsigned red_blocks(const GridDev& g, int per_thread)
{
  long blocks = (g.nown + (long)kBlock * per_thread - 1) / ((long)kBlock * per_thread);
  if (blocks > kRedBlocks) blocks = kRedBlocks;
  if (blocks < 1) blocks = 1;
  return (unsigned)blocks;
}

// dst = 0 (MODE 0), dst = src (1), dst += src (2) on the owned nodes of one component; src, dst: stored planes
template <int MODE>
__global__ void __launch_bounds__(kBlock) k_gauss_acc(GridDev g, const double* __restrict__ src, double* __restrict__ dst)
{
  const long off = (long)g.G * g.plane;
  const long stride = (long)gridDim.x * kBlock;
  for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < g.nown; i += stride) {
    if (MODE == 0) dst[off + i] = 0.0;
    else if (MODE == 1) dst[off + i] = src[off + i];
    else dst[off + i] += src[off + i];
  }
}

// dst = src - shift on the owned nodes of one component
__global__ void __launch_bounds__(kBlock) k_gauss_shift(GridDev g, const double* __restrict__ src, double shift, double* __restrict__ dst)
{
  const long off = (long)g.G * g.plane;
  const long stride = (long)gridDim.x * kBlock;
  for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < g.nown; i += stride) dst[off + i] = src[off + i] - shift;
}

// partial[blk] = sum (rho - shift)   (shift = 0: the plain sum, bit for bit)
__global__ void __launch_bounds__(kBlock) k_gauss_sum(GridDev g, const double* __restrict__ rho, double shift, double* partial)
{
  double acc[1] = {0.0};
  const long off = (long)g.G * g.plane;
  const long stride = (long)gridDim.x * kBlock;
  for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < g.nown; i += stride) acc[0] += rho[off + i] - shift;
  block_reduce_store<1, kBlock>(acc, partial, gridDim.x, blockIdx.x);
}

// res = D F - (rho - mean); partial rows: sum |res|, sum res^2, sum (rho - mean)^2   (F's lower ghost plane must be filled)
__global__ void __launch_bounds__(kBlock) k_gauss_residual(GridDev g, const double* __restrict__ F, const double* __restrict__ rho,
  double mean, double* __restrict__ res, double* partial)
{
  const double ix = g.inv[0], iy = g.inv[1], iz = g.inv[2];
  const double* __restrict__ Fx = F;
  const double* __restrict__ Fy = F + g.cstride;
  const double* __restrict__ Fz = F + 2 * g.cstride;
  double acc[3] = {0.0, 0.0, 0.0};
  const long stride = (long)gridDim.x * kBlock;
  for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < g.nown; i += stride) {
    const int x = (int)(i % g.nx), y = (int)((i / g.nx) % g.ny), z = (int)(i / g.plane);
    const long c0 = g.node(x, y, g.wz(z));
    const double dv = +ix * Fx[c0] - ix * Fx[g.nodew(x - 1, y, z)] + iy * Fy[c0] - iy * Fy[g.nodew(x, y - 1, z)] + iz * Fz[c0] -
      iz * Fz[g.nodew(x, y, z - 1)];
    const double rt = rho[c0] - mean;
    const double r = dv - rt;
    res[c0] = r;
    acc[0] += fabs(r);
    acc[1] += r * r;
    acc[2] += rt * rt;
  }
  block_reduce_store<3, kBlock>(acc, partial, gridDim.x, blockIdx.x);
}

// (D G p) at a node: the 7-point Laplacian as the composition of the two differences.  The wrapped neighbours x - 1 and
// x + 1 of an extent of 2 are one node: both terms reach it, the off-diagonal weight is 2 / d^2.
__device__ inline double lap_at(const GridDev& g, const double* __restrict__ p, int x, int y, int z, long c0, double p0)
{
  const double ix = g.inv[0], iy = g.inv[1], iz = g.inv[2];
  const double lx = (p[g.nodew(x + 1, y, z)] - p0) - (p0 - p[g.nodew(x - 1, y, z)]);
  const double ly = (p[g.nodew(x, y + 1, z)] - p0) - (p0 - p[g.nodew(x, y - 1, z)]);
  const double lz = (p[g.nodew(x, y, z + 1)] - p0) - (p0 - p[g.nodew(x, y, z - 1)]);
  return (ix * ix) * lx + (iy * iy) * ly + (iz * iz) * lz;
}

// Ap = D G p and partial[blk] = sum p . Ap   (p's ghost planes must be filled)
__global__ void __launch_bounds__(kBlock) k_lap_dot(GridDev g, const double* __restrict__ p, double* __restrict__ Ap, double* partial)
{
  double acc[1] = {0.0};
  const long stride = (long)gridDim.x * kBlock;
  for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < g.nown; i += stride) {
    const int x = (int)(i % g.nx), y = (int)((i / g.nx) % g.ny), z = (int)(i / g.plane);
    const long c0 = g.node(x, y, g.wz(z));
    const double p0 = p[c0];
    const double a = lap_at(g, p, x, y, z, c0, p0);
    Ap[c0] = a;
    acc[0] += p0 * a;
  }
  block_reduce_store<1, kBlock>(acc, partial, gridDim.x, blockIdx.x);
}

// r = res - D G phi and partial[blk] = sum r . r: the residual of the solve formed explicitly (phi's ghost planes filled)
__global__ void __launch_bounds__(kBlock) k_lap_residual(GridDev g, const double* __restrict__ phi, const double* __restrict__ res,
  double* __restrict__ r, double* partial)
{
  double acc[1] = {0.0};
  const long stride = (long)gridDim.x * kBlock;
  for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < g.nown; i += stride) {
    const int x = (int)(i % g.nx), y = (int)((i / g.nx) % g.ny), z = (int)(i / g.plane);
    const long c0 = g.node(x, y, g.wz(z));
    const double rv = res[c0] - lap_at(g, phi, x, y, z, c0, phi[c0]);
    r[c0] = rv;
    acc[0] += rv * rv;
  }
  block_reduce_store<1, kBlock>(acc, partial, gridDim.x, blockIdx.x);
}

// x += alpha p ; r -= alpha Ap ; partial[blk] = sum r . r (after the update): k_cg_update on one component
__global__ void __launch_bounds__(kBlock) k_gauss_update(GridDev g, double alpha, const double* __restrict__ p,
  const double* __restrict__ Ap, double* __restrict__ x, double* __restrict__ r, double* partial)
{
  double acc[1] = {0.0};
  const long off = (long)g.G * g.plane;
  const long stride = (long)gridDim.x * kBlock;
  for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < g.nown; i += stride) {
    x[off + i] += alpha * p[off + i];
    const double rv = r[off + i] - alpha * Ap[off + i];
    r[off + i] = rv;
    acc[0] += rv * rv;
  }
  block_reduce_store<1, kBlock>(acc, partial, gridDim.x, blockIdx.x);
}

// p = r + beta p
__global__ void __launch_bounds__(kBlock) k_gauss_dir(GridDev g, double beta, const double* __restrict__ r, double* __restrict__ p)
{
  const long off = (long)g.G * g.plane;
  const long stride = (long)gridDim.x * kBlock;
  for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < g.nown; i += stride) p[off + i] = r[off + i] + beta * p[off + i];
}

// F -= G phi ; partial[blk] = sum |G phi|^2   (phi's upper ghost plane must be filled)
__global__ void __launch_bounds__(kBlock) k_gauss_correct(GridDev g, const double* __restrict__ phi, double* __restrict__ F, double* partial)
{
  const double ix = g.inv[0], iy = g.inv[1], iz = g.inv[2];
  double acc[1] = {0.0};
  const long stride = (long)gridDim.x * kBlock;
  for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < g.nown; i += stride) {
    const int x = (int)(i % g.nx), y = (int)((i / g.nx) % g.ny), z = (int)(i / g.plane);
    const long c0 = g.node(x, y, g.wz(z));
    const double p0 = phi[c0];
    const double gx = ix * (phi[g.nodew(x + 1, y, z)] - p0);
    const double gy = iy * (phi[g.nodew(x, y + 1, z)] - p0);
    const double gz = iz * (phi[g.nodew(x, y, z + 1)] - p0);
    F[c0] -= gx;
    F[c0 + g.cstride] -= gy;
    F[c0 + 2 * g.cstride] -= gz;
    acc[0] += gx * gx + gy * gy + gz * gz;
  }
  block_reduce_store<1, kBlock>(acc, partial, gridDim.x, blockIdx.x);
}

int gauss_alloc(xpic_ctx* c)
{
  if (c->gauss_ws) return 0;
  XPIC_HIP(hipMalloc(&c->gauss_ws, sizeof(double) * c->nvec * 2));
  XPIC_HIP(hipMemsetAsync(c->gauss_ws, 0, sizeof(double) * c->nvec * 2, c->stream));
  return 0;
}

template <int MODE>
int acc_plane(xpic_ctx* c, const double* src, double* dst)
{
  hipLaunchKernelGGL(k_gauss_acc<MODE>, dim3(red_blocks(c->g, 4)), dim3(kBlock), 0, c->stream, c->g, src, dst);
  XPIC_HIP(hipGetLastError());
  return 0;
}

// *mean = the mean of plane kRho over the whole box.  refine: a second pass sums rho - mean and corrects the mean by it.  The
// plain sum of N values of size |rho| leaves the mean wrong by some eps |rho|, a constant sqrt(N) eps |rho| in the residual
// that no phi removes; the electrostatic step meets loads (a quiet two-stream start) whose rho~ is 1e-4 |rho| and whose
// tolerance lies below that.  The cleans of xpic_gauss.h keep the single pass and their bits.
int charge_mean(xpic_ctx* c, double* mean, bool refine)
{
  const unsigned blocks = red_blocks(c->g, 4);
  const double cells = (double)c->g.nx * c->g.ny * c->g.nzg;
  double shift = 0.0;
  for (int pass = 0; pass < (refine ? 2 : 1); ++pass) {
    hipLaunchKernelGGL(k_gauss_sum, dim3(blocks), dim3(kBlock), 0, c->stream, c->g, plane_of(c, kRho), shift, c->red_partial);
    XPIC_HIP(hipGetLastError());
    double sum;
    XPIC_CALL(reduce_to_host(c, 1, (int)blocks, 1, true, &sum));
    shift = pass == 0 ? sum / cells : shift + sum / cells;
  }
  *mean = shift;
  return 0;
}

// plane kRho = the sorts' charge densities in creation order (+ the background), the mean left in.
// given: the sorts' sum is handed in (component 0 of a stored vector) and nothing is deposited here.
int deposit_charge(xpic_ctx* c, const double* given = nullptr)
{
  double* rho = plane_of(c, kRho);
  double* tmp = c->field[XPIC_W2]; // the deposit's scratch vector, as xpic_charge_density's
  bool first = true;
  if (given) {
    XPIC_CALL(acc_plane<1>(c, given, rho));
    first = false;
  }
  else
    for (auto& s : c->sorts) {
      XPIC_CALL(charge_density(c, s, tmp));
      XPIC_CALL(first ? acc_plane<1>(c, tmp, rho) : acc_plane<2>(c, tmp, rho));
      first = false;
    }
  if (c->gauss_bg) XPIC_CALL(first ? acc_plane<1>(c, c->gauss_bg, rho) : acc_plane<2>(c, c->gauss_bg, rho));
  else if (first) XPIC_CALL(acc_plane<0>(c, nullptr, rho));
  return 0;
}

// deposit_charge, and *mean = the mean of plane kRho over the whole box
int collect_charge(xpic_ctx* c, double* mean, const double* given = nullptr)
{
  XPIC_CALL(deposit_charge(c, given));
  return charge_mean(c, mean, given != nullptr);
}

// plane kRes = D F - (rho - mean) from plane kRho; out3 = { |res|_1, |res|_2^2, |rho~|_2^2 }
int residual_of(xpic_ctx* c, double* F, double mean, double* out3)
{
  XPIC_CALL(halo_fill(c, F, 1));
  const unsigned blocks = red_blocks(c->g, 1);
  {
    Timed t(c, "gauss_residual");
    hipLaunchKernelGGL(k_gauss_residual, dim3(blocks), dim3(kBlock), 0, c->stream, c->g, F, plane_of(c, kRho), mean, plane_of(c, kRes),
      c->red_partial);
    XPIC_HIP(hipGetLastError());
  }
  XPIC_CALL(reduce_to_host(c, 3, (int)blocks, 1, true, out3));
  XPIC_CHECK(std::isfinite(out3[0]) && std::isfinite(out3[1]) && std::isfinite(out3[2]) && std::isfinite(mean),
    "gauss: the field or the charge is not finite");
  return 0;
}

int scalar_to_host(xpic_ctx* c, const double* plane, double* zyx)
{
  XPIC_HIP(hipMemcpyAsync(zyx, plane + (long)c->g.G * c->g.plane, sizeof(double) * c->g.nown, hipMemcpyDeviceToHost, c->stream));
  XPIC_HIP(hipStreamSynchronize(c->stream));
  return 0;
}

// Conjugate gradients on D G (negative semidefinite, its null space the constants; res is mean-free): phi from 0 until
// |r|_2 <= tol.  true: converged, phi's ghost planes are filled.
int poisson_cg(xpic_ctx* c, double rr, double tol, int maxit, int* its_out, bool* converged, double* rnorm)
{
  const GridDev& g = c->g;
  double *p = plane_of(c, kP), *r = plane_of(c, kR), *Ap = plane_of(c, kAp), *phi = plane_of(c, kPhi), *res = plane_of(c, kRes);
  XPIC_CALL(acc_plane<0>(c, nullptr, phi));
  XPIC_CALL(acc_plane<1>(c, res, r));
  XPIC_CALL(acc_plane<1>(c, res, p));
  const unsigned sblocks = red_blocks(g, 1), eblocks = red_blocks(g, 4);
  int its = 0;
  *converged = false;
  while (its < maxit) {
    XPIC_CALL(halo_fill(c, vector_of(c, kP), 1));
    double pAp;
    {
      Timed t(c, "gauss_lap_dot");
      hipLaunchKernelGGL(k_lap_dot, dim3(sblocks), dim3(kBlock), 0, c->stream, g, p, Ap, c->red_partial);
      XPIC_HIP(hipGetLastError());
    }
    XPIC_CALL(reduce_to_host(c, 1, (int)sblocks, 1, true, &pAp));
    if (!(pAp < 0.0)) break; // p in the null space, or not a number: nothing more to gain
    const double alpha = rr / pAp;
    double rr1;
    {
      Timed t(c, "gauss_update");
      hipLaunchKernelGGL(k_gauss_update, dim3(eblocks), dim3(kBlock), 0, c->stream, g, alpha, p, Ap, phi, r, c->red_partial);
      XPIC_HIP(hipGetLastError());
    }
    XPIC_CALL(reduce_to_host(c, 1, (int)eblocks, 1, true, &rr1));
    ++its;
    double beta = rr1 / rr;
    if (std::sqrt(rr1) <= tol) {
      // the recurrence says converged: the residual res - D G phi is formed explicitly, and the iteration restarts from it
      // if it disagrees
      XPIC_CALL(halo_fill(c, vector_of(c, kPhi), 1));
      hipLaunchKernelGGL(k_lap_residual, dim3(sblocks), dim3(kBlock), 0, c->stream, g, phi, res, r, c->red_partial);
      XPIC_HIP(hipGetLastError());
      XPIC_CALL(reduce_to_host(c, 1, (int)sblocks, 1, true, &rr1));
      if (std::sqrt(rr1) <= tol) { rr = rr1; *converged = true; break; }
      beta = 0.0;
    }
    rr = rr1;
    {
      Timed t(c, "gauss_dir");
      hipLaunchKernelGGL(k_gauss_dir, dim3(eblocks), dim3(kBlock), 0, c->stream, g, beta, r, p);
      XPIC_HIP(hipGetLastError());
    }
  }
  *its_out = its;
  *rnorm = std::sqrt(rr);
  return 0;
}

// The direct path (poisson.hip; XPIC_POISSON_DIRECT), poisson_cg's contract: phi from 0 until |r|_2 <= tol, phi's ghost
// planes filled.  One application of the transform solve to r is added to phi and r = res - D G phi is formed explicitly;
// a residual above the tolerance is solved for again (iterative refinement).  its counts the applications.  Not converged:
// maxit applications, or one that did not halve the residual it was given (what rounding leaves is reached, or not a number).
int poisson_direct(xpic_ctx* c, double rr, double tol, int maxit, int* its_out, bool* converged, double* rnorm)
{
  const GridDev& g = c->g;
  double *p = plane_of(c, kP), *r = plane_of(c, kR), *Ap = plane_of(c, kAp), *phi = plane_of(c, kPhi), *res = plane_of(c, kRes);
  XPIC_CALL(acc_plane<1>(c, res, r));
  const unsigned sblocks = red_blocks(g, 1);
  const long off = (long)g.G * g.plane; // (0: the direct path runs on contexts without ghost planes only)
  int its = 0;
  double rn = std::sqrt(rr);
  *converged = false;
  while (its < maxit) {
    XPIC_CALL(poisson_transform_solve(c, r + off, p + off, Ap + off, phi + off, its > 0));
    ++its;
    XPIC_CALL(halo_fill(c, vector_of(c, kPhi), 1));
    double rr1;
    hipLaunchKernelGGL(k_lap_residual, dim3(sblocks), dim3(kBlock), 0, c->stream, g, phi, res, r, c->red_partial);
    XPIC_HIP(hipGetLastError());
    XPIC_CALL(reduce_to_host(c, 1, (int)sblocks, 1, true, &rr1));
    const double rn1 = std::sqrt(rr1);
    const bool halved = rn1 <= 0.5 * rn; // (false for a NaN)
    rn = rn1;
    if (rn1 <= tol) { *converged = true; break; }
    if (!halved) break;
  }
  *its_out = its;
  *rnorm = rn;
  return 0;
}

int gauss_clean(xpic_ctx* c, int field, double rtol, double atol, int maxit, double* phi_zyx, int* iterations, double* out4,
  const double* rho_given = nullptr)
{
  XPIC_CALL(gauss_alloc(c));
  double* F = c->field[field];
  double mean, o3[3];
  XPIC_CALL(collect_charge(c, &mean, rho_given));
  XPIC_CALL(residual_of(c, F, mean, o3));
  const double before = std::sqrt(o3[1]);
  const double tol = std::max(rtol * std::sqrt(o3[2]), atol);
  int its = 0;
  double after = before, gphi = 0.0;
  if (before <= tol) XPIC_CALL(acc_plane<0>(c, nullptr, plane_of(c, kPhi))); // already clean: phi = 0, F is not written
  else {
    bool converged;
    double rn;
    if (c->poisson_kind == XPIC_POISSON_DIRECT) XPIC_CALL(poisson_direct(c, o3[1], tol, maxit, &its, &converged, &rn));
    else XPIC_CALL(poisson_cg(c, o3[1], tol, maxit, &its, &converged, &rn));
    if (!converged) {
      set_error("gauss clean did not converge: " + std::to_string(its) + " iterations, |r| = " + std::to_string(rn) +
        ", tolerance " + std::to_string(tol));
      return 4;
    }
    const unsigned blocks = red_blocks(c->g, 1);
    {
      Timed t(c, "gauss_correct");
      hipLaunchKernelGGL(k_gauss_correct, dim3(blocks), dim3(kBlock), 0, c->stream, c->g, plane_of(c, kPhi), F, c->red_partial);
      XPIC_HIP(hipGetLastError());
    }
    XPIC_CALL(reduce_to_host(c, 1, (int)blocks, 1, true, &gphi));
    gphi = std::sqrt(gphi);
    XPIC_CALL(residual_of(c, F, mean, o3)); // from the corrected field
    after = std::sqrt(o3[1]);
  }
  if (phi_zyx) XPIC_CALL(scalar_to_host(c, plane_of(c, kPhi), phi_zyx));
  *iterations = its;
  out4[0] = before; out4[1] = after; out4[2] = mean; out4[3] = gphi;
  double* info = c->gauss_info;
  info[0] += 1; info[1] += its; info[2] = before; info[3] = after; info[4] = mean; info[5] = its;
  return 0;
}

}  // namespace

int gauss_ride(xpic_ctx* c)
{
  int its;
  double o4[4];
  return gauss_clean(c, XPIC_E, c->gauss_rtol, c->gauss_atol, c->gauss_maxit, nullptr, &its, o4);
}

int gauss_reserve(xpic_ctx* c) { return gauss_alloc(c); }

// spectrum.hip's work planes: r to stage a host scalar in, p and Ap for the passes, as xpic_poisson_apply takes them.  No
// clean and no step carries state in them from one call to the next.
int gauss_lend_planes(xpic_ctx* c, double** stage, double** w0, double** w1)
{
  XPIC_CALL(gauss_alloc(c));
  *stage = plane_of(c, kR); *w0 = plane_of(c, kP); *w1 = plane_of(c, kAp);
  return 0;
}

int gauss_charge_plane(xpic_ctx* c, const double** rho)
{
  XPIC_CALL(gauss_alloc(c));
  XPIC_CALL(deposit_charge(c));
  *rho = plane_of(c, kRho);
  return 0;
}

int gauss_clean_given(xpic_ctx* c, const double* rho_vec, double rtol, double atol, int maxit, int* iterations)
{
  double o4[4];
  return gauss_clean(c, XPIC_E, rtol, atol, maxit, nullptr, iterations, o4, rho_vec);
}

void gauss_free(xpic_ctx* c)
{
  (void)hipFree(c->gauss_ws);
  (void)hipFree(c->gauss_bg);
  c->gauss_ws = c->gauss_bg = nullptr;
}

}  // namespace xpic

using namespace xpic;

#define GAUSS_FIELD_CHECK(f)                                                                                         \
  XPIC_CHECK((f) >= 0 && (f) < XPIC_NFIELDS && ctx->field[f], "gauss: unknown or unallocated field id");             \
  XPIC_CHECK((f) != XPIC_W2, "gauss: XPIC_W2 is the charge deposit's scratch and cannot be the field")
#define GAUSS_TOL_CHECK(rtol, atol, maxit)                                                                           \
  XPIC_CHECK((rtol) >= 0.0 && (atol) >= 0.0 && std::isfinite(rtol) && std::isfinite(atol), "gauss: rtol and atol must be finite and >= 0"); \
  XPIC_CHECK((maxit) >= 1, "gauss: maxit must be >= 1")

extern "C" {

int xpic_gauss_background(xpic_ctx* ctx, const double* rho_zyx)
{
  XPIC_CHECK(ctx != nullptr, "null context");
  XPIC_HIP(hipStreamSynchronize(ctx->stream));
  if (!rho_zyx) {
    if (ctx->gauss_bg) XPIC_HIP(hipFree(ctx->gauss_bg));
    ctx->gauss_bg = nullptr;
    return 0;
  }
  const GridDev& g = ctx->g;
  if (!ctx->gauss_bg) {
    XPIC_HIP(hipMalloc(&ctx->gauss_bg, sizeof(double) * g.cstride));
    XPIC_HIP(hipMemsetAsync(ctx->gauss_bg, 0, sizeof(double) * g.cstride, ctx->stream));
  }
  XPIC_HIP(hipMemcpyAsync(ctx->gauss_bg + (long)g.G * g.plane, rho_zyx, sizeof(double) * g.nown, hipMemcpyHostToDevice, ctx->stream));
  XPIC_HIP(hipStreamSynchronize(ctx->stream));
  return 0;
}

int xpic_gauss_residual(xpic_ctx* ctx, int field, double* res_zyx, double* out4)
{
  XPIC_CHECK(ctx != nullptr, "null context");
  XPIC_CHECK(out4, "null argument");
  GAUSS_FIELD_CHECK(field);
  XPIC_CALL(gauss_alloc(ctx));
  double mean, o3[3];
  XPIC_CALL(collect_charge(ctx, &mean));
  XPIC_CALL(residual_of(ctx, ctx->field[field], mean, o3));
  if (res_zyx) XPIC_CALL(scalar_to_host(ctx, plane_of(ctx, kRes), res_zyx));
  out4[0] = o3[0]; out4[1] = std::sqrt(o3[1]); out4[2] = mean; out4[3] = std::sqrt(o3[2]);
  return 0;
}

int xpic_gauss_clean(xpic_ctx* ctx, int field, double rtol, double atol, int maxit, double* phi_zyx, int* iterations,
  double* out4)
{
  XPIC_CHECK(ctx != nullptr, "null context");
  XPIC_CHECK(iterations && out4, "null argument");
  GAUSS_FIELD_CHECK(field);
  GAUSS_TOL_CHECK(rtol, atol, maxit);
  return gauss_clean(ctx, field, rtol, atol, maxit, phi_zyx, iterations, out4);
}

int xpic_set_gauss_clean(xpic_ctx* ctx, int every, double rtol, double atol, int maxit)
{
  XPIC_CHECK(ctx != nullptr, "null context");
  XPIC_CHECK(every >= 0, "gauss: every must be >= 0");
  XPIC_CHECK(ctx->scheme != XPIC_ES, "gauss: the electrostatic step solves Gauss's law itself; a clean cannot ride with it");
  if (every > 0) {
    GAUSS_TOL_CHECK(rtol, atol, maxit);
    XPIC_CALL(gauss_alloc(ctx)); // sized here, not in the middle of a step
  }
  ctx->gauss_every = every; ctx->gauss_rtol = rtol; ctx->gauss_atol = atol; ctx->gauss_maxit = maxit;
  return 0;
}

int xpic_gauss_info(xpic_ctx* ctx, double* out6)
{
  XPIC_CHECK(ctx != nullptr, "null context");
  XPIC_CHECK(out6, "null argument");
  for (int i = 0; i < 6; ++i) out6[i] = ctx->gauss_info[i];
  return 0;
}

// ---- include/xpic_poisson.h
int xpic_set_poisson_solver(xpic_ctx* ctx, int kind)
{
  XPIC_CHECK(ctx != nullptr, "null context");
  XPIC_CHECK(kind == XPIC_POISSON_CG || kind == XPIC_POISSON_DIRECT, "poisson: unknown solver kind");
  if (kind == XPIC_POISSON_DIRECT) XPIC_CALL(poisson_check(ctx));
  ctx->poisson_kind = kind;
  return 0;
}

int xpic_get_poisson_solver(xpic_ctx* ctx, int* kind)
{
  XPIC_CHECK(ctx != nullptr, "null context");
  XPIC_CHECK(kind, "null argument");
  *kind = ctx->poisson_kind;
  return 0;
}

// plane `to` = rhs_zyx - its mean, `stage` the plane the host's values land in (to for none).  The mean in two passes
// (charge_mean's refinement), taken out before the transform sees the data.
static int poisson_stage(xpic_ctx* ctx, const double* rhs_zyx, double* stage, double* to)
{
  const GridDev& g = ctx->g;
  XPIC_HIP(hipMemcpyAsync(stage, rhs_zyx, sizeof(double) * g.nown, hipMemcpyHostToDevice, ctx->stream));
  const unsigned blocks = red_blocks(g, 4);
  double mean = 0.0;
  for (int pass = 0; pass < 2; ++pass) {
    hipLaunchKernelGGL(k_gauss_sum, dim3(blocks), dim3(kBlock), 0, ctx->stream, g, stage, mean, ctx->red_partial);
    XPIC_HIP(hipGetLastError());
    double sum;
    XPIC_CALL(reduce_to_host(ctx, 1, (int)blocks, 1, true, &sum));
    XPIC_CHECK(std::isfinite(sum), "poisson: the right-hand side is not finite");
    mean += sum / (double)g.nown;
  }
  hipLaunchKernelGGL(k_gauss_shift, dim3(blocks), dim3(kBlock), 0, ctx->stream, g, stage, mean, to);
  XPIC_HIP(hipGetLastError());
  return 0;
}

int xpic_poisson_apply(xpic_ctx* ctx, const double* rhs_zyx, double* phi_zyx)
{
  XPIC_CHECK(ctx != nullptr, "null context");
  XPIC_CHECK(rhs_zyx && phi_zyx, "null argument");
  XPIC_CALL(poisson_check(ctx));
  XPIC_CALL(gauss_alloc(ctx));
  double* r = plane_of(ctx, kR);
  XPIC_CALL(poisson_stage(ctx, rhs_zyx, plane_of(ctx, kRes), r));
  XPIC_CALL(poisson_transform_solve(ctx, r, plane_of(ctx, kP), plane_of(ctx, kAp), plane_of(ctx, kPhi), false));
  return scalar_to_host(ctx, plane_of(ctx, kPhi), phi_zyx);
}

int xpic_poisson_solve(xpic_ctx* ctx, const double* rhs_zyx, double tol, int maxit, double* phi_zyx, int* applications,
  double* rnorm)
{
  XPIC_CHECK(ctx != nullptr, "null context");
  XPIC_CHECK(rhs_zyx && phi_zyx && applications && rnorm, "null argument");
  XPIC_CHECK(tol >= 0.0 && std::isfinite(tol), "poisson: tol must be finite and >= 0");
  XPIC_CHECK(maxit >= 1, "poisson: maxit must be >= 1");
  XPIC_CALL(poisson_check(ctx));
  XPIC_CALL(gauss_alloc(ctx));
  const GridDev& g = ctx->g;
  double *res = plane_of(ctx, kRes), *phi = plane_of(ctx, kPhi);
  XPIC_CALL(poisson_stage(ctx, rhs_zyx, plane_of(ctx, kRho), res));
  // |res|_2^2, which the clean has from its residual kernel: the explicit residual of phi = 0
  XPIC_CALL(acc_plane<0>(ctx, nullptr, phi));
  XPIC_CALL(halo_fill(ctx, vector_of(ctx, kPhi), 1));
  const unsigned sblocks = red_blocks(g, 1);
  double rr;
  hipLaunchKernelGGL(k_lap_residual, dim3(sblocks), dim3(kBlock), 0, ctx->stream, g, phi, res, plane_of(ctx, kR), ctx->red_partial);
  XPIC_HIP(hipGetLastError());
  XPIC_CALL(reduce_to_host(ctx, 1, (int)sblocks, 1, true, &rr));
  bool converged; // (not an error here: the caller asked for a count)
  XPIC_CALL(poisson_direct(ctx, rr, tol, maxit, applications, &converged, rnorm));
  return scalar_to_host(ctx, phi, phi_zyx);
}

}  // extern "C"
