// spectrum.hip -- field spectra on the device (include/xpic_spectrum.h; an extension: the reference has no spectral
// diagnostic).  poisson.hip's three forward passes give the separable transform T of a scalar; here T becomes the DFT:
//     H(k) = 1/2 [ T(r_x k) + T(r_y k) + T(r_z k) - T(r_xyz k) ],   r_a: k_a -> (n_a - k_a) mod n_a,   H(-k) = H(r_xyz k),
//     Re F^ = (H(k) + H(-k)) / 2,   Im F^ = -(H(k) - H(-k)) / 2,   P(k) = (H(k)^2 + H(-k)^2) / 2.
// k_spectrum_combine<false> stores P; k_spectrum_combine<true> reduces it instead: a workgroup owns kRows rows (y) of one
// z plane, a wave a row at a time with the lane on x, so that T's rows -- the reflected ones are the same rows read
// backwards, x -> nx - x on consecutive lanes, the same cache lines -- are read coalesced.  It leaves one partial sum per
// (workgroup, x), one sum per (z, y) row and one shell histogram per workgroup; k_spectrum_colsum and k_spectrum_rowsum add
// those in a fixed order.  Only the shell histogram uses atomics, on LDS, inside a workgroup.
// The whole file is compiled without contraction: H(k) at -k and H(-k) at k are the same expression and must round alike.
#pragma clang fp contract(off)
#include <cmath>

#include <vector>

#include "common.h"
#include "device_common.h"

namespace xpic {

struct SpectrumProbe {
  int id = 0, source = 0, comp = 0, nmodes = 0, every = 1;
  int64_t capacity = 0, recorded = 0, dropped = 0;
  int* modes = nullptr;   // [nmodes][3] on the device
  double* rows = nullptr; // [capacity][1 + 2 nmodes] on the device: step, (Re, Im) per mode
};

struct SpectrumState {
  double* ws = nullptr; // tables, edges, partial sums and results of xpic_spectrum (grown on demand)
  size_t ws_n = 0;
  int* modes = nullptr; // xpic_spectrum_modes' list and result (grown on demand)
  double* modes_out = nullptr;
  int modes_n = 0;
  std::vector<SpectrumProbe> probes; // the live probes in creation order; ids are never given twice
  int next_id = 0;
};

namespace {

constexpr int kThreads = 256; // four waves
constexpr int kRows = 16;     // rows of a workgroup: wave w takes rows w, w + 4, w + 8, w + 12
constexpr int kParts = 8, kCols = 32; // k_spectrum_colsum: 8 interleaved partial sums of 32 columns

// H(k) and H(-k) at k = (x, y, z) from the separable transform T; (rx, ry, rz) = -k.  The four terms in the header's order.
__device__ inline void hartley_pair(const double* __restrict__ T, int nx, long plane, int x, int y, int z, int rx, int ry, int rz,
  double* hk, double* hm)
{
  const double* r00 = T + z * plane + (long)y * nx;
  const double* r10 = T + z * plane + (long)ry * nx;
  const double* r01 = T + rz * plane + (long)y * nx;
  const double* r11 = T + rz * plane + (long)ry * nx;
  *hk = 0.5 * (((r00[rx] + r10[x]) + r01[x]) - r11[rx]); // r_x k, r_y k, r_z k, r_xyz k
  *hm = 0.5 * (((r11[x] + r01[rx]) + r10[rx]) - r00[x]); // the same of -k: (x, ry, rz), (rx, y, rz), (rx, ry, z), k
}

__device__ inline int reflect(int k, int n) { return k == 0 ? 0 : n - k; }

// FUSED false: P[z][y][x] stored.  FUSED true: colpart[blk][x] = the sum of P over the workgroup's rows, rowsum[z][y] = the
// sum over x, shellpart[blk][2 (nshell + 1)] = the workgroup's shell powers (the last: outside every shell) and counts.
// grid (ceil(ny / kRows), nz); dynamic LDS: (nshell + 1) (edges, powers: double; counts: int) when nshell > 0.
template <bool FUSED>
__global__ void __launch_bounds__(kThreads) k_spectrum_combine(int nx, int ny, int nz, const double* __restrict__ T,
  double* __restrict__ P, double* __restrict__ colpart, double* __restrict__ rowsum, int nshell, const double* __restrict__ edges2,
  const double* __restrict__ kx2, const double* __restrict__ ky2, const double* __restrict__ kz2, double* __restrict__ shellpart)
{
  extern __shared__ double dyn[];
  __shared__ double colw[kThreads / 64][64];
  const int t = threadIdx.x, w = t >> 6, l = t & 63;
  const int z = blockIdx.y, y0 = blockIdx.x * kRows;
  const int rz = reflect(z, nz);
  const long plane = (long)nx * ny;
  const long blk = (long)blockIdx.y * gridDim.x + blockIdx.x;
  double* se = dyn;                // edges
  double* sp = dyn + (nshell + 1); // powers; sp[nshell]: outside
  int* sc = (int*)(dyn + 2 * (nshell + 1));
  if (FUSED && nshell > 0) {
    for (int j = t; j <= nshell; j += kThreads) { se[j] = edges2[j]; sp[j] = 0.0; sc[j] = 0; }
    __syncthreads();
  }
  double rowacc[kRows / 4];
#pragma unroll
  for (int r = 0; r < kRows / 4; ++r) rowacc[r] = 0.0;
  for (int xt = 0; xt < nx; xt += 64) {
    const int x = xt + l;
    const bool in = x < nx;
    const int rx = in ? reflect(x, nx) : 0;
    double col = 0.0;
#pragma unroll
    for (int r = 0; r < kRows / 4; ++r) {
      const int y = y0 + w + 4 * r;
      if (!in || y >= ny) continue;
      double hk, hm;
      hartley_pair(T, nx, plane, x, y, z, rx, reflect(y, ny), rz, &hk, &hm);
      const double p = 0.5 * (hk * hk + hm * hm);
      if (!FUSED) { P[z * plane + (long)y * nx + x] = p; continue; }
      col += p;
      rowacc[r] += p;
      if (nshell > 0) {
        const double s = (kx2[x] + ky2[y]) + kz2[z];
        int j = nshell;
        if (s >= se[0] && s < se[nshell]) {
          int lo = 0, hi = nshell; // se[lo] <= s < se[hi]
          while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (s >= se[mid]) lo = mid; else hi = mid;
          }
          j = lo;
        }
        atomicAdd(&sp[j], p);
        atomicAdd(&sc[j], 1);
      }
    }
    if (FUSED) {
      colw[w][l] = col;
      __syncthreads();
      if (w == 0 && in) colpart[blk * nx + x] = ((colw[0][l] + colw[1][l]) + colw[2][l]) + colw[3][l];
      __syncthreads();
    }
  }
  if (!FUSED) return;
#pragma unroll
  for (int r = 0; r < kRows / 4; ++r) {
    const int y = y0 + w + 4 * r;
    const double v = wave_sum(rowacc[r]);
    if (l == 0 && y < ny) rowsum[(long)z * ny + y] = v;
  }
  if (nshell > 0) {
    __syncthreads();
    double* out = shellpart + blk * 2 * (nshell + 1);
    for (int j = t; j <= nshell; j += kThreads) { out[j] = sp[j]; out[nshell + 1 + j] = (double)sc[j]; }
  }
}

// out[i] = sum_b part[b * stride + i], b < nb, i < n: kParts interleaved partial sums per column, added in the order 0, 1, ..
__global__ void __launch_bounds__(kThreads) k_spectrum_colsum(const double* __restrict__ part, long nb, int n, long stride,
  double* __restrict__ out)
{
  __shared__ double sm[kParts][kCols];
  const int i = blockIdx.x * kCols + (threadIdx.x % kCols), p = threadIdx.x / kCols;
  double a = 0.0;
  if (i < n)
    for (long b = p; b < nb; b += kParts) a += part[b * stride + i];
  sm[p][threadIdx.x % kCols] = a;
  __syncthreads();
  if (p == 0 && i < n) {
    double v = sm[0][threadIdx.x];
    for (int q = 1; q < kParts; ++q) v += sm[q][threadIdx.x];
    out[i] = v;
  }
}

// out[r] = sum_i in[r * n + i], i = 0, 1, ..
__global__ void __launch_bounds__(kThreads) k_spectrum_rowsum(const double* __restrict__ in, int rows, int n, double* __restrict__ out)
{
  const int r = blockIdx.x * kThreads + threadIdx.x;
  if (r >= rows) return;
  double v = 0.0;
  for (int i = 0; i < n; ++i) v += in[(long)r * n + i];
  out[r] = v;
}

// out[m] = (Re, Im) F^ of the signed mode numbers modes[m][3]; *step_out = step where it is given (a probe's row)
__global__ void __launch_bounds__(kThreads) k_spectrum_modes(int nx, int ny, int nz, const double* __restrict__ T, int nmodes,
  const int* __restrict__ modes, double* __restrict__ out, double* __restrict__ step_out, double step)
{
  const int m = blockIdx.x * kThreads + threadIdx.x;
  if (m == 0 && step_out) *step_out = step;
  if (m >= nmodes) return;
  const int x = GridDev::wrap(modes[3 * m], nx), y = GridDev::wrap(modes[3 * m + 1], ny), z = GridDev::wrap(modes[3 * m + 2], nz);
  double hk, hm;
  hartley_pair(T, nx, (long)nx * ny, x, y, z, reflect(x, nx), reflect(y, ny), reflect(z, nz), &hk, &hm);
  out[2 * m] = 0.5 * (hk + hm);
  out[2 * m + 1] = -(0.5 * (hk - hm));
}

int spectrum_check(const xpic_ctx* c, int source, int comp, bool host_allowed)
{
  XPIC_CHECK(c->g.G == 0, "spectrum: spectra are for single-slab contexts (a transform along z needs every plane); "
    "this context has ghost planes");
  XPIC_CHECK(c->g.nx <= XPIC_POISSON_MAX_EXTENT && c->g.ny <= XPIC_POISSON_MAX_EXTENT && c->g.nzl <= XPIC_POISSON_MAX_EXTENT,
    "spectrum: the transform holds a dense n x n table per extent and takes extents up to " + std::to_string(XPIC_POISSON_MAX_EXTENT));
  if (source == XPIC_SPECTRUM_HOST) {
    XPIC_CHECK(host_allowed, "spectrum: XPIC_SPECTRUM_HOST is not a probe source");
    return 0;
  }
  if (source == XPIC_SPECTRUM_RHO) return 0;
  XPIC_CHECK(source >= 0 && source < XPIC_NFIELDS && c->field[source], "spectrum: unknown source or unallocated field id");
  XPIC_CHECK(source != XPIC_W2, "spectrum: XPIC_W2 is the charge deposit's scratch and cannot be the source");
  XPIC_CHECK(comp >= 0 && comp < 3, "spectrum: comp must be 0, 1 or 2");
  return 0;
}

SpectrumState* state_of(xpic_ctx* c)
{
  if (!c->spectrum) c->spectrum = new SpectrumState;
  return c->spectrum;
}

// *T = the separable transform of the source (in plane w0 of the Gauss vectors)
int transform_source(xpic_ctx* c, int source, int comp, const double* scalar_zyx, const double** T)
{
  double *stage, *w0, *w1;
  XPIC_CALL(gauss_lend_planes(c, &stage, &w0, &w1));
  const double* in;
  if (source == XPIC_SPECTRUM_HOST) {
    XPIC_HIP(hipMemcpyAsync(stage, scalar_zyx, sizeof(double) * c->g.nown, hipMemcpyHostToDevice, c->stream));
    in = stage;
  }
  else if (source == XPIC_SPECTRUM_RHO) XPIC_CALL(gauss_charge_plane(c, &in));
  else in = c->field[source] + (long)comp * c->g.cstride;
  XPIC_CALL(poisson_forward(c, in, w0, w1));
  *T = w0;
  return 0;
}

int host_scalar_check(const xpic_ctx* c, int source, const double* scalar_zyx)
{
  if (source != XPIC_SPECTRUM_HOST) return 0;
  XPIC_CHECK(scalar_zyx, "spectrum: XPIC_SPECTRUM_HOST needs the scalar");
  for (long i = 0; i < c->g.nown; ++i) XPIC_CHECK(std::isfinite(scalar_zyx[i]), "spectrum: the scalar is not finite");
  return 0;
}

int launch_modes(xpic_ctx* c, const double* T, int nmodes, const int* modes, double* out, double* step_out, double step)
{
  Timed t(c, "spectrum_modes");
  hipLaunchKernelGGL(k_spectrum_modes, dim3((unsigned)((nmodes + kThreads - 1) / kThreads)), dim3(kThreads), 0, c->stream, c->g.nx,
    c->g.ny, c->g.nzl, T, nmodes, modes, out, step_out, step);
  XPIC_HIP(hipGetLastError());
  return 0;
}

// k^2 of index i of an axis: k = 2 pi m / (n d), m = i folded to (-n/2, n/2]
void k2_table(int n, double d, double* out)
{
  for (int i = 0; i < n; ++i) {
    const int m = i <= n / 2 ? i : i - n;
    const double k = 2.0 * 3.14159265358979323846 * (double)m / ((double)n * d);
    out[i] = k * k;
  }
}

}  // namespace

int spectrum_ride(xpic_ctx* c)
{
  int done_source = -1, done_comp = -1; // the transform the planes hold: probes of one source share it
  const double* T = nullptr;
  for (auto& p : c->spectrum->probes) {
    if (c->steps_done % p.every != 0) continue;
    if (p.recorded == p.capacity) { p.dropped += 1; continue; }
    if (p.source != done_source || p.comp != done_comp) XPIC_CALL(transform_source(c, p.source, p.comp, nullptr, &T));
    done_source = p.source; done_comp = p.comp;
    double* row = p.rows + p.recorded * (1 + 2 * (long)p.nmodes);
    XPIC_CALL(launch_modes(c, T, p.nmodes, p.modes, row + 1, row, (double)c->steps_done));
    p.recorded += 1;
  }
  return 0;
}

void spectrum_free(xpic_ctx* c)
{
  if (!c->spectrum) return;
  for (auto& p : c->spectrum->probes) { (void)hipFree(p.modes); (void)hipFree(p.rows); }
  (void)hipFree(c->spectrum->ws); (void)hipFree(c->spectrum->modes); (void)hipFree(c->spectrum->modes_out);
  delete c->spectrum;
  c->spectrum = nullptr;
}

}  // namespace xpic

using namespace xpic;

extern "C" {

int xpic_spectrum_power(xpic_ctx* ctx, int source, int comp, const double* scalar_zyx, double* power_zyx)
{
  XPIC_CHECK(ctx != nullptr, "null context");
  XPIC_CHECK(power_zyx, "null argument");
  XPIC_CALL(spectrum_check(ctx, source, comp, true));
  XPIC_CALL(host_scalar_check(ctx, source, scalar_zyx));
  const GridDev& g = ctx->g;
  const double* T;
  XPIC_CALL(transform_source(ctx, source, comp, scalar_zyx, &T));
  double *stage, *w0, *w1;
  XPIC_CALL(gauss_lend_planes(ctx, &stage, &w0, &w1));
  {
    Timed t(ctx, "spectrum_combine");
    hipLaunchKernelGGL(k_spectrum_combine<false>, dim3((unsigned)((g.ny + kRows - 1) / kRows), (unsigned)g.nzl), dim3(kThreads), 0,
      ctx->stream, g.nx, g.ny, g.nzl, T, w1, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr);
    XPIC_HIP(hipGetLastError());
  }
  XPIC_HIP(hipMemcpyAsync(power_zyx, w1, sizeof(double) * g.nown, hipMemcpyDeviceToHost, ctx->stream));
  XPIC_HIP(hipStreamSynchronize(ctx->stream));
  return 0;
}

int xpic_spectrum(xpic_ctx* ctx, int source, int comp, const double* scalar_zyx, double* axis_x, double* axis_y, double* axis_z,
  int nshell, const double* edges2, double* shell, int64_t* shell_count, double* outside2, double* total)
{
  XPIC_CHECK(ctx != nullptr, "null context");
  XPIC_CALL(spectrum_check(ctx, source, comp, true));
  XPIC_CHECK(nshell >= 0 && nshell <= XPIC_SPECTRUM_MAX_SHELLS, "spectrum: nshell must be 0 .. " + std::to_string(XPIC_SPECTRUM_MAX_SHELLS));
  if (nshell > 0) {
    XPIC_CHECK(edges2 && shell, "spectrum: nshell > 0 needs edges2 and shell");
    for (int j = 0; j <= nshell; ++j) XPIC_CHECK(std::isfinite(edges2[j]), "spectrum: edges2 is not finite");
    for (int j = 0; j < nshell; ++j) XPIC_CHECK(edges2[j] < edges2[j + 1], "spectrum: edges2 must be strictly ascending");
  }
  XPIC_CALL(host_scalar_check(ctx, source, scalar_zyx));
  const GridDev& g = ctx->g;
  const int nx = g.nx, ny = g.ny, nz = g.nzl, ns1 = nshell > 0 ? nshell + 1 : 0;
  const long nblk = (long)nz * ((ny + kRows - 1) / kRows);
  // the workspace: tables | edges | colpart | rowsum | shellpart | results (axis_x, axis_y, axis_z, shells, counts)
  const size_t o_edges = (size_t)nx + ny + nz, o_col = o_edges + ns1, o_row = o_col + (size_t)nblk * nx,
    o_shell = o_row + (size_t)nz * ny, o_res = o_shell + (size_t)nblk * 2 * ns1, n_res = (size_t)nx + ny + nz + 2 * ns1,
    need = o_res + n_res;
  SpectrumState* st = state_of(ctx);
  if (st->ws_n < need) {
    XPIC_HIP(hipStreamSynchronize(ctx->stream));
    if (st->ws) XPIC_HIP(hipFree(st->ws));
    st->ws = nullptr; st->ws_n = 0;
    XPIC_HIP(hipMalloc(&st->ws, sizeof(double) * need));
    st->ws_n = need;
  }
  std::vector<double> host(o_col);
  k2_table(nx, g.dx, host.data());
  k2_table(ny, g.dy, host.data() + nx);
  k2_table(nz, g.dz, host.data() + nx + ny);
  for (int j = 0; j < ns1; ++j) host[o_edges + j] = edges2[j];
  XPIC_HIP(hipMemcpyAsync(st->ws, host.data(), sizeof(double) * o_col, hipMemcpyHostToDevice, ctx->stream));
  const double* T;
  XPIC_CALL(transform_source(ctx, source, comp, scalar_zyx, &T));
  double* ws = st->ws;
  {
    Timed t(ctx, "spectrum_combine");
    hipLaunchKernelGGL(k_spectrum_combine<true>, dim3((unsigned)((ny + kRows - 1) / kRows), (unsigned)nz), dim3(kThreads),
      sizeof(double) * 2 * ns1 + sizeof(int) * ns1, ctx->stream, nx, ny, nz, T, nullptr, ws + o_col, ws + o_row, nshell, ws + o_edges, ws,
      ws + nx, ws + nx + ny, ws + o_shell);
    XPIC_HIP(hipGetLastError());
  }
  double* res = ws + o_res;
  {
    Timed t(ctx, "spectrum_reduce");
    auto colsum = [&](const double* part, long nb, int n, long stride, double* out) {
      hipLaunchKernelGGL(k_spectrum_colsum, dim3((unsigned)((n + kCols - 1) / kCols)), dim3(kThreads), 0, ctx->stream, part, nb, n, stride, out);
    };
    colsum(ws + o_col, nblk, nx, nx, res);
    colsum(ws + o_row, nz, ny, ny, res + nx);
    hipLaunchKernelGGL(k_spectrum_rowsum, dim3((unsigned)((nz + kThreads - 1) / kThreads)), dim3(kThreads), 0, ctx->stream, ws + o_row, nz,
      ny, res + nx + ny);
    if (ns1) colsum(ws + o_shell, nblk, 2 * ns1, 2 * ns1, res + nx + ny + nz);
    XPIC_HIP(hipGetLastError());
  }
  std::vector<double> out(n_res);
  XPIC_HIP(hipMemcpyAsync(out.data(), res, sizeof(double) * n_res, hipMemcpyDeviceToHost, ctx->stream));
  XPIC_HIP(hipStreamSynchronize(ctx->stream));
  double sum = 0.0;
  for (int z = 0; z < nz; ++z) sum += out[nx + ny + z];
  for (int i = 0; i < nx && axis_x; ++i) axis_x[i] = out[i];
  for (int i = 0; i < ny && axis_y; ++i) axis_y[i] = out[nx + i];
  for (int i = 0; i < nz && axis_z; ++i) axis_z[i] = out[nx + ny + i];
  const double* sh = out.data() + nx + ny + nz;
  for (int j = 0; j < nshell; ++j) {
    shell[j] = sh[j];
    if (shell_count) shell_count[j] = (int64_t)sh[ns1 + j];
  }
  if (outside2) {
    outside2[0] = nshell > 0 ? sh[nshell] : sum;
    outside2[1] = nshell > 0 ? sh[ns1 + nshell] : (double)g.nown;
  }
  if (total) *total = sum;
  return 0;
}

int xpic_spectrum_modes(xpic_ctx* ctx, int source, int comp, const double* scalar_zyx, int nmodes, const int32_t* modes_xyz,
  double* re_im)
{
  XPIC_CHECK(ctx != nullptr, "null context");
  XPIC_CALL(spectrum_check(ctx, source, comp, true));
  XPIC_CHECK(nmodes >= 1, "spectrum: nmodes must be >= 1");
  XPIC_CHECK(modes_xyz && re_im, "null argument");
  XPIC_CALL(host_scalar_check(ctx, source, scalar_zyx));
  SpectrumState* st = state_of(ctx);
  if (st->modes_n < nmodes) {
    XPIC_HIP(hipStreamSynchronize(ctx->stream));
    (void)hipFree(st->modes); (void)hipFree(st->modes_out);
    st->modes = nullptr; st->modes_out = nullptr; st->modes_n = 0;
    XPIC_HIP(hipMalloc(&st->modes, sizeof(int) * 3 * nmodes));
    XPIC_HIP(hipMalloc(&st->modes_out, sizeof(double) * 2 * nmodes));
    st->modes_n = nmodes;
  }
  XPIC_HIP(hipMemcpyAsync(st->modes, modes_xyz, sizeof(int) * 3 * nmodes, hipMemcpyHostToDevice, ctx->stream));
  const double* T;
  XPIC_CALL(transform_source(ctx, source, comp, scalar_zyx, &T));
  XPIC_CALL(launch_modes(ctx, T, nmodes, st->modes, st->modes_out, nullptr, 0.0));
  XPIC_HIP(hipMemcpyAsync(re_im, st->modes_out, sizeof(double) * 2 * nmodes, hipMemcpyDeviceToHost, ctx->stream));
  XPIC_HIP(hipStreamSynchronize(ctx->stream));
  return 0;
}

int xpic_spectrum_probe_create(xpic_ctx* ctx, int source, int comp, int nmodes, const int32_t* modes_xyz, int every,
  int64_t capacity, int* id)
{
  XPIC_CHECK(ctx != nullptr, "null context");
  XPIC_CALL(spectrum_check(ctx, source, comp, false));
  XPIC_CHECK(nmodes >= 1, "spectrum: nmodes must be >= 1");
  XPIC_CHECK(every >= 1, "spectrum: every must be >= 1");
  XPIC_CHECK(capacity >= 1, "spectrum: capacity must be >= 1");
  XPIC_CHECK(modes_xyz && id, "null argument");
  XPIC_CHECK(!ctx->spectrum || (int)ctx->spectrum->probes.size() < XPIC_SPECTRUM_MAX_PROBES, "spectrum: a context takes at most " + std::to_string(XPIC_SPECTRUM_MAX_PROBES) + " live probes");
  // everything a probed step needs is made now, not in the middle of a step
  double *stage, *w0, *w1;
  XPIC_CALL(gauss_lend_planes(ctx, &stage, &w0, &w1));
  XPIC_CALL(poisson_tables(ctx));
  SpectrumProbe p;
  p.source = source; p.comp = source == XPIC_SPECTRUM_RHO ? 0 : comp; p.nmodes = nmodes; p.every = every; p.capacity = capacity;
  XPIC_HIP(hipMalloc(&p.modes, sizeof(int) * 3 * nmodes));
  if (hipMalloc(&p.rows, sizeof(double) * (size_t)capacity * (1 + 2 * (size_t)nmodes)) != hipSuccess) {
    (void)hipGetLastError();
    (void)hipFree(p.modes);
    XPIC_CHECK(false, "spectrum: no device memory for the probe's rows");
  }
  if (hipMemcpyAsync(p.modes, modes_xyz, sizeof(int) * 3 * nmodes, hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
      hipStreamSynchronize(ctx->stream) != hipSuccess) {
    (void)hipGetLastError();
    (void)hipFree(p.modes); (void)hipFree(p.rows);
    XPIC_CHECK(false, "spectrum: the probe's modes could not be uploaded");
  }
  SpectrumState* st = state_of(ctx);
  p.id = st->next_id++;
  st->probes.push_back(p);
  *id = p.id;
  return 0;
}

// the slot of a live probe, or -1
static int probe_slot(const xpic_ctx* ctx, int id)
{
  if (!ctx->spectrum) return -1;
  for (size_t i = 0; i < ctx->spectrum->probes.size(); ++i)
    if (ctx->spectrum->probes[i].id == id) return (int)i;
  return -1;
}

int xpic_spectrum_probe_get(xpic_ctx* ctx, int id, int64_t rows, int64_t* step, double* re_im, int64_t* recorded, int64_t* dropped,
  int reset)
{
  XPIC_CHECK(ctx != nullptr, "null context");
  const int slot = probe_slot(ctx, id);
  XPIC_CHECK(slot >= 0, "spectrum: unknown or destroyed probe id");
  XPIC_CHECK(rows >= 0, "spectrum: rows must be >= 0");
  SpectrumProbe& p = ctx->spectrum->probes[slot];
  const int64_t n = rows < p.recorded ? rows : p.recorded;
  const size_t w = 1 + 2 * (size_t)p.nmodes;
  if (n > 0 && (step || re_im)) {
    std::vector<double> host((size_t)n * w);
    XPIC_HIP(hipMemcpyAsync(host.data(), p.rows, sizeof(double) * host.size(), hipMemcpyDeviceToHost, ctx->stream));
    XPIC_HIP(hipStreamSynchronize(ctx->stream));
    for (int64_t r = 0; r < n; ++r) {
      if (step) step[r] = (int64_t)host[r * w];
      for (size_t j = 0; j + 1 < w && re_im; ++j) re_im[r * (w - 1) + j] = host[r * w + 1 + j];
    }
  }
  if (recorded) *recorded = p.recorded;
  if (dropped) *dropped = p.dropped;
  if (reset) p.recorded = p.dropped = 0;
  return 0;
}

int xpic_spectrum_probe_destroy(xpic_ctx* ctx, int id)
{
  XPIC_CHECK(ctx != nullptr, "null context");
  const int slot = probe_slot(ctx, id);
  XPIC_CHECK(slot >= 0, "spectrum: unknown or destroyed probe id");
  SpectrumProbe& p = ctx->spectrum->probes[slot];
  XPIC_HIP(hipStreamSynchronize(ctx->stream));
  (void)hipFree(p.modes); (void)hipFree(p.rows);
  ctx->spectrum->probes.erase(ctx->spectrum->probes.begin() + slot);
  return 0;
}

}  // extern "C"
