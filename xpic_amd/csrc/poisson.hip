// poisson.hip -- the direct solve of the periodic 7-point Poisson problem D G phi = res (include/xpic_poisson.h; an
// extension: the reference has no such solver).  D G is a sum of three Kronecker terms, each a symmetric circulant along one
// axis, and the discrete Hartley matrix H_n[k][j] = (cos(2 pi k j / n) + sin(2 pi k j / n)) / sqrt(n) -- real, symmetric,
// its own inverse -- diagonalises every symmetric circulant of extent n.  So
//     phi = Hx Hy Hz [ (Hx Hy Hz res) / (lam_x[kx] + lam_y[ky] + lam_z[kz]) ],   lam_a[k] = -4 sin^2(pi k / n_a) / d_a^2,
// the (0, 0, 0) mode set to 0: six dense passes C = H . X along one axis each, all float64, no complex numbers, any extent.
// One kernel does every pass as a row-major product D[m][c] = sum_k A[m][k] B[k][c] on v_mfma_f64_16x16x4_f64:
//     along x:       A = the scalar as [ny nz][nx], B = Hx                      (H symmetric: X . H = the transform of every row)
//     along y and z: A = H, B = the scalar as [n][inner], one product per outer index (nz of them along y, one along z)
// so that the column of a tile, which the instruction keeps on the lane, is always the index that is contiguous in memory.
// Tiles of both operands are staged in LDS, zero-padded there where an extent is no multiple of the tile; nothing is padded
// in memory.  The k order of the sum is the tile order, then the instruction's: two calls on the same data return the same bits.
#include <cmath>

#include <vector>

#include "common.h"
#include "device_common.h"

namespace xpic {

namespace {

constexpr int kThreads = 256;          // four waves: wave w owns rows 16 w .. 16 w + 15 of the tile and all of its columns
constexpr int kTM = 64, kTC = 64, kTK = 16;
constexpr int kAPitch = kTK + 2;       // doubles per row of the A tile in LDS (the fragment read m * pitch + k meets no bank twice)
constexpr int kBPitch = kTC + 16;      // the same for the B tile (k * pitch + c)

typedef double f64x4 __attribute__((ext_vector_type(4)));

enum { kStore = 0, kDivide = 1, kAdd = 2 };

// D[b][m][c] (= / += ) sum_k A[b][m][k] B[b][k][c], all row-major with no padding (lda = K, ldb = ldc = C); b = blockIdx.z with
// the strides sA, sB, sD (0: the operand is shared).  m_fast: blockIdx.x counts the tiles in m, else those in c -- the
// workgroups that share a tile of the streamed operand are launched side by side.
// EPI kDivide: the element at linear index e of D (= the node (z ny + y) nx + x of the scalar) is divided by
// lam_x[x] + lam_y[y] + lam_z[z], and e = 0, the constant mode, whose divisor is 0, is set to 0.
template <int EPI>
__global__ void __launch_bounds__(kThreads) k_hartley_pass(int M, int C, int K, const double* __restrict__ A, long sA,
  const double* __restrict__ B, long sB, double* __restrict__ D, long sD, int m_fast, int nx, int ny,
  const double* __restrict__ lam_x, const double* __restrict__ lam_y, const double* __restrict__ lam_z)
{
  __shared__ double As[kTM * kAPitch];
  __shared__ double Bs[kTK * kBPitch];
  const int t = threadIdx.x, w = t >> 6, l = t & 63;
  const int m0 = (m_fast ? blockIdx.x : blockIdx.y) * kTM;
  const int c0 = (m_fast ? blockIdx.y : blockIdx.x) * kTC;
  A += (long)blockIdx.z * sA;
  B += (long)blockIdx.z * sB;
  D += (long)blockIdx.z * sD;

  double ra[4], rb[4];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int idx = t + kThreads * e;
      const int am = m0 + (idx >> 4), ak = k0 + (idx & 15);
      ra[e] = (am < M && ak < K) ? A[(long)am * K + ak] : 0.0;
      const int bk = k0 + (idx >> 6), bc = c0 + (idx & 63);
      rb[e] = (bk < K && bc < C) ? B[(long)bk * C + bc] : 0.0;
    }
  };

  f64x4 acc[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) acc[s] = f64x4{0.0, 0.0, 0.0, 0.0};

  fetch(0);
  for (int k0 = 0; k0 < K; k0 += kTK) {
    __syncthreads(); // the tile before this one has been read
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int idx = t + kThreads * e;
      As[(idx >> 4) * kAPitch + (idx & 15)] = ra[e];
      Bs[(idx >> 6) * kBPitch + (idx & 63)] = rb[e];
    }
    __syncthreads();
    if (k0 + kTK < K) fetch(k0 + kTK);
    // lane l holds A[row l & 15][k = l >> 4] and B[k = l >> 4][column l & 15] of a 16 x 16 x 4 product
#pragma unroll
    for (int kk = 0; kk < kTK / 4; ++kk) {
      const int k = kk * 4 + (l >> 4);
      const double a = As[(w * 16 + (l & 15)) * kAPitch + k];
#pragma unroll
      for (int s = 0; s < 4; ++s) acc[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, Bs[k * kBPitch + s * 16 + (l & 15)], acc[s], 0, 0, 0);
    }
  }

  // result register i of lane l: row (l >> 4) + 4 i, column l & 15
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int col = c0 + s * 16 + (l & 15);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = m0 + w * 16 + (l >> 4) + 4 * i;
      if (row >= M || col >= C) continue;
      const long e = (long)row * C + col;
      double v = acc[s][i];
      if (EPI == kDivide) {
        const long q = (long)blockIdx.z * sD + e;
        const int x = (int)(q % nx), y = (int)((q / nx) % ny), z = (int)(q / ((long)nx * ny));
        v = q == 0 ? 0.0 : v / (lam_x[x] + lam_y[y] + lam_z[z]);
      }
      if (EPI == kAdd) D[e] += v;
      else D[e] = v;
    }
  }
}

template <int EPI>
int pass(xpic_ctx* c, int axis, const double* in, double* out)
{
  const GridDev& g = c->g;
  const double* H = c->poisson_H[axis];
  int M, C, K, batch, m_fast;
  const double *A, *B;
  long sB = 0;
  if (axis == 0) { M = g.ny * g.nzl; C = K = g.nx; A = in; B = H; batch = 1; m_fast = 0; }
  else if (axis == 1) { M = K = g.ny; C = g.nx; A = H; B = in; batch = g.nzl; sB = g.plane; m_fast = 1; }
  else { M = K = g.nzl; C = (int)g.plane; A = H; B = in; batch = 1; m_fast = 1; }
  const unsigned tm = (unsigned)((M + kTM - 1) / kTM), tc = (unsigned)((C + kTC - 1) / kTC);
  XPIC_CHECK((m_fast ? tc : tm) <= 65535u, "poisson: the grid is too large for the transform's launch");
  Timed t(c, axis == 0 ? "poisson_pass_x" : (axis == 1 ? "poisson_pass_y" : "poisson_pass_z"));
  hipLaunchKernelGGL(k_hartley_pass<EPI>, m_fast ? dim3(tm, tc, (unsigned)batch) : dim3(tc, tm, (unsigned)batch), dim3(kThreads), 0,
    c->stream, M, C, K, A, 0L, B, sB, out, sB, m_fast, g.nx, g.ny, c->poisson_lam[0], c->poisson_lam[1], c->poisson_lam[2]);
  XPIC_HIP(hipGetLastError());
  return 0;
}

// H_n and lam of one axis in long double, k j reduced modulo n in integers before the angle is formed, rounded to double
void hartley_host(int n, double d, std::vector<double>& H, std::vector<double>& lam)
{
  const long double pi = 3.14159265358979323846264338327950288L;
  const long double scale = 1.0L / sqrtl((long double)n);
  H.resize((size_t)n * n);
  lam.resize(n);
  for (int k = 0; k < n; ++k) {
    for (int j = 0; j < n; ++j) {
      const long double a = 2.0L * pi * (long double)(((long)k * j) % n) / (long double)n;
      H[(size_t)k * n + j] = (double)((cosl(a) + sinl(a)) * scale);
    }
    const long double s = sinl(pi * (long double)k / (long double)n);
    lam[k] = (double)(-4.0L * s * s / ((long double)d * (long double)d));
  }
}

}  // namespace

int poisson_check(const xpic_ctx* c)
{
  XPIC_CHECK(c->g.G == 0, "poisson: the direct solve is for single-slab contexts (a transform along z needs every plane); "
    "this context has ghost planes");
  XPIC_CHECK(c->g.nx <= XPIC_POISSON_MAX_EXTENT && c->g.ny <= XPIC_POISSON_MAX_EXTENT && c->g.nzl <= XPIC_POISSON_MAX_EXTENT,
    "poisson: the direct solve holds a dense n x n table per extent and takes extents up to " +
      std::to_string(XPIC_POISSON_MAX_EXTENT));
  return 0;
}

// the tables of this context's grid, made by the first call: one H per distinct extent, one lam per axis
int poisson_tables(xpic_ctx* c)
{
  if (c->poisson_lam[2]) return 0;
  XPIC_CALL(poisson_check(c));
  const int n[3] = {c->g.nx, c->g.ny, c->g.nzl};
  const double d[3] = {c->g.dx, c->g.dy, c->g.dz};
  std::vector<double> H, lam;
  for (int a = 0; a < 3; ++a) {
    hartley_host(n[a], d[a], H, lam);
    for (int b = 0; b < a; ++b)
      if (n[b] == n[a]) c->poisson_H[a] = c->poisson_H[b];
    if (!c->poisson_H[a]) {
      XPIC_HIP(hipMalloc(&c->poisson_H[a], sizeof(double) * H.size()));
      XPIC_HIP(hipMemcpy(c->poisson_H[a], H.data(), sizeof(double) * H.size(), hipMemcpyHostToDevice));
    }
    XPIC_HIP(hipMalloc(&c->poisson_lam[a], sizeof(double) * lam.size()));
    XPIC_HIP(hipMemcpy(c->poisson_lam[a], lam.data(), sizeof(double) * lam.size(), hipMemcpyHostToDevice));
  }
  return 0;
}

// out (= / +=) the mean-free phi with D G phi = rhs, one application: three passes forward, the division folded into the third,
// three passes back.  rhs, w0, w1, out: the owned nodes of four distinct scalar planes [nz][ny][nx]; w0 and w1 are overwritten.
int poisson_transform_solve(xpic_ctx* c, const double* rhs, double* w0, double* w1, double* out, bool add)
{
  XPIC_CALL(poisson_tables(c));
  XPIC_CALL(pass<kStore>(c, 0, rhs, w0));
  XPIC_CALL(pass<kStore>(c, 1, w0, w1));
  XPIC_CALL(pass<kDivide>(c, 2, w1, w0));
  XPIC_CALL(pass<kStore>(c, 2, w0, w1));
  XPIC_CALL(pass<kStore>(c, 1, w1, w0));
  return add ? pass<kAdd>(c, 0, w0, out) : pass<kStore>(c, 0, w0, out);
}

// the three forward passes alone, x, y, z as the solve makes them: w0 = Hz Hy Hx in (include/xpic_spectrum.h).  in, w0, w1:
// the owned nodes of three distinct scalar planes; in is only read, w1 is overwritten.
int poisson_forward(xpic_ctx* c, const double* in, double* w0, double* w1)
{
  XPIC_CALL(poisson_tables(c));
  XPIC_CALL(pass<kStore>(c, 0, in, w0));
  XPIC_CALL(pass<kStore>(c, 1, w0, w1));
  return pass<kStore>(c, 2, w1, w0);
}

void poisson_free(xpic_ctx* c)
{
  for (int a = 0; a < 3; ++a) {
    bool shared = false;
    for (int b = 0; b < a; ++b) shared = shared || c->poisson_H[b] == c->poisson_H[a];
    if (!shared) (void)hipFree(c->poisson_H[a]);
    (void)hipFree(c->poisson_lam[a]);
  }
  for (int a = 0; a < 3; ++a) c->poisson_H[a] = c->poisson_lam[a] = nullptr;
}

}  // namespace xpic
