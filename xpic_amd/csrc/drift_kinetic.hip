// drift_kinetic.hip -- the reference's drift-kinetic (guiding-centre) pusher with its grid interpolation:
//   DriftKineticEsirkepov::interpolate   src/algorithms/drift_kinetic_implicit.cpp:11-31
//   DriftKineticPush::process            src/algorithms/drift_kinetic_push.cpp:48-160
//   PointByField                         src/interfaces/point.h:37-58
// One lane per particle, fp64, no cross-lane operation: the lanes of a wave leave the Picard loop independently.  The
// state {x, y, z, p_parallel, p_perp, mu_p} lives in structure-of-arrays device buffers (s[k * n + q]).  Positions are
// not folded into the box: the gathers wrap their node indices (ie_node), folding is the caller's business as
// correct_coordinates is in the reference.  Single z-slab contexts only (G == 0: every index wraps, so no position,
// however far out, reads outside a field vector).
#include <algorithm>
#include <vector>

#include "common.h"
#include "device_common.h"
#include "ie_shape.h"

// The pusher's own expressions are contracted per source expression only (not across statements), so k_dk_push and
// k_dk_trace, which inline the same dk_process, round identically whatever surrounds the call.  (The segment shape in
// ie_shape.h keeps the build's default, as in eccapfim.hip: the E gather here returns k_ie_interpolate's bits.)
#pragma clang fp contract(on)

namespace xpic {

namespace {

constexpr int kBlock = 256;
constexpr int kLaunchSteps = XPIC_DK_LAUNCH_STEPS;

struct DKPoint {
  double r[3], ppar, pperp, mu;
};

// Vector3::length (src/utils/vector3.h:160-164) is std::hypot of three arguments
__device__ inline double len3(const double* a) { return norm3d(a[0], a[1], a[2]); }
__device__ inline double dot3(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
// Vector3::cross (:212-219)
__device__ inline void cross3(const double* a, const double* b, double* o)
{
  o[0] = +(a[1] * b[2] - a[2] * b[1]);
  o[1] = -(a[0] * b[2] - a[2] * b[0]);
  o[2] = +(a[0] * b[1] - a[1] * b[0]);
}
// Vector3::normalized (:150-158)
__device__ inline void normalized3(const double* a, double* o)
{
  const double l = len3(a);
  if (l > 0) { o[0] = a[0] / l; o[1] = a[1] / l; o[2] = a[2] / l; }
  else { o[0] = o[1] = o[2] = 0.0; }
}

// DriftKineticEsirkepov::interpolate(E_p, B_p, gradB_p, rn, r0): E_p with the segment shape of (rn, r0)
// (ImplicitEsirkepov::interpolate, implicit_esirkepov.cpp:71-90), B_p and gradB_p with Shape::setup(rn, 1.5,
// spline_of_2nd_order) (src/utils/shape.cpp:31-41) and SimpleInterpolation's magnetic products (shape.h:65-72): one set
// of weights, one pass over the nodes.  GRAD = false is the reference's gradB_g == nullptr: gradB_p = 0.
template <bool GRAD>
__device__ inline void dk_fields(const GridDev& g, const double* __restrict__ E, const double* __restrict__ B,
  const double* __restrict__ gB, const double* rn, const double* r0, double* Ep, double* Bp, double* gBp)
{
  const double d[3] = {g.dx, g.dy, g.dz};
  // a position that is not a number, or further out than an int counts cells, has no node: its fields are NaN and no
  // index is formed from it
  bool ok = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) ok = ok && fabs(rn[a]) <= 1e9 * d[a] && fabs(r0[a]) <= 1e9 * d[a];
  if (!ok) {
    const double nan = __builtin_nan("");
#pragma unroll
    for (int a = 0; a < 3; ++a) { Ep[a] = nan; Bp[a] = nan; gBp[a] = GRAD ? nan : 0.0; }
    return;
  }
  {
    IEShape sh;
    sh.setup(g, rn, r0);
    Ep[0] = Ep[1] = Ep[2] = 0.0;
#pragma unroll
    for (int cx = 0; cx < 3; cx++) {
      const int cy = (cx + 1) % 3, cz = (cx + 2) % 3;
#pragma unroll
      for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 3; j++)
#pragma unroll
          for (int k = 0; k < 3; k++) { // i[cx], i[cy], i[cz] of the reference's loop nest, m = its running index
            int o[3];
            o[cx] = i; o[cy] = j; o[cz] = k;
            const int m = ((cx * 2 + i) * 3 + j) * 3 + k;
            Ep[cx] += E[cx * g.cstride + ie_node(g, sh.start[0] + o[0], sh.start[1] + o[1], sh.start[2] + o[2])] * sh.cache[m];
          }
    }
  }
  Bp[0] = Bp[1] = Bp[2] = 0.0;
  gBp[0] = gBp[1] = gBp[2] = 0.0;
  // x and y weights in registers, the z pair formed plane by plane: the plane loop stays rolled, which keeps the 96 loads
  // of a plane in flight without holding all 384 of the footprint in registers
  int st[3], sz[3];
  double No[2][4], Sh[2][4], prz = 0.0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double pr = rn[a] / d[a];
    st[a] = (int)round(pr - 1.5);
    sz[a] = (int)floor(pr + 1.5) + 1 - st[a]; // 3 or 4
    if (a == 2) { prz = pr; break; }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const double gx = (double)(st[a] + t);
      No[a][t] = spline2_ref(pr - gx);
      Sh[a][t] = spline2_ref(pr - (gx + 0.5));
    }
  }
#pragma unroll 1
  for (int kz = 0; kz < sz[2]; ++kz) {
    const double gz = (double)(st[2] + kz);
    const double Noz = spline2_ref(prz - gz), Shz = spline2_ref(prz - (gz + 0.5));
#pragma unroll
    for (int jy = 0; jy < 4; ++jy) {
      if (jy < sz[1]) {
#pragma unroll
        for (int ix = 0; ix < 4; ++ix) {
          if (ix < sz[0]) {
            const long o = ie_node(g, st[0] + ix, st[1] + jy, st[2] + kz);
            const double wx = Shz * Sh[1][jy] * No[0][ix];
            const double wy = Shz * No[1][jy] * Sh[0][ix];
            const double wz = Noz * Sh[1][jy] * Sh[0][ix];
            Bp[0] += B[o] * wx;
            Bp[1] += B[g.cstride + o] * wy;
            Bp[2] += B[2 * g.cstride + o] * wz;
            if (GRAD) {
              gBp[0] += gB[o] * wx;
              gBp[1] += gB[g.cstride + o] * wy;
              gBp[2] += gB[2 * g.cstride + o] * wz;
            }
          }
        }
      }
    }
  }
}

// DriftKineticPush::get_Vd (drift_kinetic_push.cpp:111-119)
__device__ inline void dk_get_Vd(const xpic_dk_params& P, const DKPoint& p0, const double* h, double Vh, double Bh,
  const double* gradBh, const double* Eh, double* Vd)
{
  if (Bh < 1e-12) { Vd[0] = Vd[1] = Vd[2] = 0.0; return; }
  double Exh[3], gb[3], hxg[3];
  cross3(Eh, h, Exh);
#pragma unroll
  for (int c = 0; c < 3; ++c) gb[c] = gradBh[c] / Bh;
  cross3(h, gb, hxg);
  const double f = 1.0 / P.qm * (Vh * Vh / Bh + p0.mu / P.mp);
#pragma unroll
  for (int c = 0; c < 3; ++c) Vd[c] = Exh[c] / Bh + f * hxg[c];
}

// the right-hand side that update_v_parallel (:133-142) assigns and get_residue_v (:150-160) compares with:
// dt qm (Eh . h + term) - mu_term
__device__ inline void dk_v_terms(const xpic_dk_params& P, const DKPoint& p0, double Vh, const double* h, const double* Vd,
  double lenBp, double lenB0, const double* Eh, double* drive, double* mu_term)
{
  const bool small = fabs(Vh) < 1e-12;
  const double term = small ? 0.0 : (dot3(Eh, Vd) / Vh);
  const double dB = lenBp - lenB0;
  *mu_term = small ? 0.0 : (p0.mu / P.mp) * (dB / Vh);
  *drive = P.dt * P.qm * (dot3(Eh, h) + term);
}

// DriftKineticPush::process(dt, pn, p0) (:48-108), statement by statement; pn enters as the initial guess.  Returns the
// reference's `it`: the number of updates made, maxit for a lane that did not meet the tolerances (the reference's
// trailing PetscCheckAbort is the caller's to make).
template <bool GRAD>
__device__ inline int dk_process(const GridDev& g, const double* __restrict__ E, const double* __restrict__ B,
  const double* __restrict__ gB, const xpic_dk_params& P, const DKPoint& p0, DKPoint& pn)
{
  double Eh[3], Bp[3], gradBp[3];
  dk_fields<GRAD>(g, E, B, gB, pn.r, p0.r, Eh, Bp, gradBp); // set_fields(p0.r, pn.r, Eh, Bp, gradBp)
  double Vd[3], Vhh[3], B0[3], Bh[3], gradB0[3], gradBh[3], b0[3], bp[3], h[3];
  double Vh = 0.0, R1 = 0.0, R2 = 0.0;
#pragma unroll
  for (int c = 0; c < 3; ++c) { B0[c] = Bh[c] = Bp[c]; gradB0[c] = gradBh[c] = gradBp[c]; }
  normalized3(Bp, b0);
#pragma unroll
  for (int c = 0; c < 3; ++c) bp[c] = h[c] = b0[c];
  const double lenB0 = len3(B0);
  double lenBp = lenB0;
  int it;
  for (it = 0; it < P.maxit; ++it) {
    Vh = 0.5 * (pn.ppar + p0.ppar);
    dk_get_Vd(P, p0, h, Vh, len3(Bh), gradBh, Eh, Vd);
    double res[3], drive, mu_term;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      Vhh[c] = Vh * h[c];
      res[c] = pn.r[c] - p0.r[c] - P.dt * (Vhh[c] + Vd[c]);
    }
    R1 = len3(res);                                                         // get_residue_r :144-148
    dk_v_terms(P, p0, Vh, h, Vd, lenBp, lenB0, Eh, &drive, &mu_term);
    R2 = fabs((pn.ppar - p0.ppar) - drive + mu_term);                       // get_residue_v :150-160
    if ((R1 < P.eps) && (R2 < P.delta) && it) break;
#pragma unroll
    for (int c = 0; c < 3; ++c) pn.r[c] = p0.r[c] + P.dt * (Vhh[c] + Vd[c]); // update_r :121-125
    dk_fields<GRAD>(g, E, B, gB, pn.r, p0.r, Eh, Bp, gradBp);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      Bh[c] = 0.5 * (Bp[c] + B0[c]);
      gradBh[c] = 0.5 * (gradBp[c] + gradB0[c]);
    }
    normalized3(Bp, bp);
#pragma unroll
    for (int c = 0; c < 3; ++c) h[c] = 0.5 * (bp[c] + b0[c]);
    lenBp = len3(Bp);
    pn.pperp = p0.pperp * sqrt(lenBp / lenB0);                              // update_v_perp :127-131
    dk_v_terms(P, p0, Vh, h, Vd, lenBp, lenB0, Eh, &drive, &mu_term);
    pn.ppar = p0.ppar + drive - mu_term;                                    // update_v_parallel :133-142
  }
  return it;
}

__device__ inline void dk_load(const double* __restrict__ s, long n, long q, DKPoint& p)
{
  p.r[0] = s[q]; p.r[1] = s[n + q]; p.r[2] = s[2 * n + q];
  p.ppar = s[3 * n + q]; p.pperp = s[4 * n + q]; p.mu = s[5 * n + q];
}
__device__ inline void dk_store(double* __restrict__ s, long n, long q, const DKPoint& p)
{
  s[q] = p.r[0]; s[n + q] = p.r[1]; s[2 * n + q] = p.r[2];
  s[3 * n + q] = p.ppar; s[4 * n + q] = p.pperp; s[5 * n + q] = p.mu;
}

template <bool GRAD>
__global__ void __launch_bounds__(kBlock) k_dk_interpolate(GridDev g, const double* __restrict__ E,
  const double* __restrict__ B, const double* __restrict__ gB, long n, const double* rn3, const double* r03, double* Ep3,
  double* Bp3, double* gBp3)
{
  const long q = (long)blockIdx.x * kBlock + threadIdx.x;
  if (q >= n) return;
  const double rn[3] = {rn3[3 * q], rn3[3 * q + 1], rn3[3 * q + 2]}, r0[3] = {r03[3 * q], r03[3 * q + 1], r03[3 * q + 2]};
  double Ep[3], Bp[3], gBp[3];
  dk_fields<GRAD>(g, E, B, gB, rn, r0, Ep, Bp, gBp);
#pragma unroll
  for (int c = 0; c < 3; ++c) { Ep3[3 * q + c] = Ep[c]; Bp3[3 * q + c] = Bp[c]; gBp3[3 * q + c] = gBp[c]; }
}

template <bool GRAD>
__global__ void __launch_bounds__(kBlock) k_dk_push(GridDev g, const double* __restrict__ E, const double* __restrict__ B,
  const double* __restrict__ gB, xpic_dk_params P, long n, const double* __restrict__ s0, double* __restrict__ sn,
  int* __restrict__ iterations)
{
  const long q = (long)blockIdx.x * kBlock + threadIdx.x;
  if (q >= n) return;
  DKPoint p0, pn;
  dk_load(s0, n, q, p0);
  pn = p0;
  iterations[q] = dk_process<GRAD>(g, E, B, gB, P, p0, pn);
  dk_store(sn, n, q, pn);
}

// steps first + 1 .. first + nsteps of a trace, in place.  Step k (counted from 1) is sampled when sample_every divides
// it: sample k / sample_every - 1 of samples[sample][6][n].
template <bool GRAD>
__global__ void __launch_bounds__(kBlock) k_dk_trace(GridDev g, const double* __restrict__ E, const double* __restrict__ B,
  const double* __restrict__ gB, xpic_dk_params P, long n, double* __restrict__ s, long first, int nsteps, long sample_every,
  double* __restrict__ samples, long long* __restrict__ it_total, int* __restrict__ it_max)
{
  const long q = (long)blockIdx.x * kBlock + threadIdx.x;
  if (q >= n) return;
  DKPoint p0, pn;
  dk_load(s, n, q, pn);
  long long total = it_total[q];
  int most = it_max[q];
  for (int k = 1; k <= nsteps; ++k) {
    p0 = pn;
    const int it = dk_process<GRAD>(g, E, B, gB, P, p0, pn);
    total += it;
    most = it > most ? it : most;
    const long step = first + k;
    if (samples && step % sample_every == 0) dk_store(samples + (step / sample_every - 1) * 6 * n, n, q, pn);
  }
  dk_store(s, n, q, pn);
  it_total[q] = total;
  it_max[q] = most;
}

struct DevBuf { // device scratch of one call, freed on scope exit
  void* p = nullptr;
  ~DevBuf() { if (p) (void)hipFree(p); }
};

inline dim3 dk_grid(int64_t n) { return dim3((unsigned)((n + kBlock - 1) / kBlock)); }

// [n][6] host records -> [6][n], and back
void to_soa(const double* aos, int64_t n, std::vector<double>& soa)
{
  soa.resize((size_t)6 * n);
  for (int64_t q = 0; q < n; ++q)
    for (int k = 0; k < 6; ++k) soa[(size_t)k * n + q] = aos[6 * q + k];
}
void to_aos(const double* soa, int64_t n, double* aos)
{
  for (int64_t q = 0; q < n; ++q)
    for (int k = 0; k < 6; ++k) aos[6 * q + k] = soa[(size_t)k * n + q];
}

}  // namespace

int dk_interpolate(xpic_ctx* c, int64_t n, const double* rn3, const double* r03, const double* gradB, double* Ep3,
  double* Bp3, double* gradBp3)
{
  DevBuf a, b, o;
  XPIC_HIP(hipMalloc(&a.p, 24 * n)); XPIC_HIP(hipMalloc(&b.p, 24 * n)); XPIC_HIP(hipMalloc(&o.p, 72 * n));
  XPIC_HIP(hipMemcpyAsync(a.p, rn3, 24 * n, hipMemcpyHostToDevice, c->stream));
  XPIC_HIP(hipMemcpyAsync(b.p, r03, 24 * n, hipMemcpyHostToDevice, c->stream));
  double* out = (double*)o.p;
  {
    Timed t(c, "dk_interpolate");
    if (gradB)
      hipLaunchKernelGGL(k_dk_interpolate<true>, dk_grid(n), dim3(kBlock), 0, c->stream, c->g, c->field[XPIC_E], c->field[XPIC_B],
        gradB, (long)n, (const double*)a.p, (const double*)b.p, out, out + 3 * n, out + 6 * n);
    else
      hipLaunchKernelGGL(k_dk_interpolate<false>, dk_grid(n), dim3(kBlock), 0, c->stream, c->g, c->field[XPIC_E], c->field[XPIC_B],
        gradB, (long)n, (const double*)a.p, (const double*)b.p, out, out + 3 * n, out + 6 * n);
    XPIC_HIP(hipGetLastError());
  }
  XPIC_HIP(hipMemcpyAsync(Ep3, out, 24 * n, hipMemcpyDeviceToHost, c->stream));
  XPIC_HIP(hipMemcpyAsync(Bp3, out + 3 * n, 24 * n, hipMemcpyDeviceToHost, c->stream));
  XPIC_HIP(hipMemcpyAsync(gradBp3, out + 6 * n, 24 * n, hipMemcpyDeviceToHost, c->stream));
  XPIC_HIP(hipStreamSynchronize(c->stream));
  return 0;
}

int dk_push(xpic_ctx* c, int64_t n, const xpic_dk_params& P, const double* gradB, const double* p0_6, double* pn_6,
  int* iterations)
{
  std::vector<double> h;
  to_soa(p0_6, n, h);
  DevBuf s0, sn, it;
  XPIC_HIP(hipMalloc(&s0.p, 48 * n)); XPIC_HIP(hipMalloc(&sn.p, 48 * n)); XPIC_HIP(hipMalloc(&it.p, 4 * n));
  XPIC_HIP(hipMemcpyAsync(s0.p, h.data(), 48 * n, hipMemcpyHostToDevice, c->stream));
  {
    Timed t(c, "dk_push");
    if (gradB)
      hipLaunchKernelGGL(k_dk_push<true>, dk_grid(n), dim3(kBlock), 0, c->stream, c->g, c->field[XPIC_E], c->field[XPIC_B], gradB,
        P, (long)n, (const double*)s0.p, (double*)sn.p, (int*)it.p);
    else
      hipLaunchKernelGGL(k_dk_push<false>, dk_grid(n), dim3(kBlock), 0, c->stream, c->g, c->field[XPIC_E], c->field[XPIC_B], gradB,
        P, (long)n, (const double*)s0.p, (double*)sn.p, (int*)it.p);
    XPIC_HIP(hipGetLastError());
  }
  XPIC_HIP(hipMemcpyAsync(h.data(), sn.p, 48 * n, hipMemcpyDeviceToHost, c->stream));
  XPIC_HIP(hipMemcpyAsync(iterations, it.p, 4 * n, hipMemcpyDeviceToHost, c->stream));
  XPIC_HIP(hipStreamSynchronize(c->stream));
  to_aos(h.data(), n, pn_6);
  return 0;
}

int dk_trace(xpic_ctx* c, int64_t n, const xpic_dk_params& P, const double* gradB, int64_t steps, int64_t sample_every,
  double* state_6, double* samples, int64_t* iterations_total, int* iterations_max)
{
  const int64_t nsamp = samples ? steps / sample_every : 0;
  std::vector<double> h;
  to_soa(state_6, n, h);
  DevBuf s, sm, tot, mx;
  XPIC_HIP(hipMalloc(&s.p, 48 * n)); XPIC_HIP(hipMalloc(&tot.p, 8 * n)); XPIC_HIP(hipMalloc(&mx.p, 4 * n));
  if (nsamp > 0) XPIC_HIP(hipMalloc(&sm.p, 48 * n * nsamp));
  XPIC_HIP(hipMemcpyAsync(s.p, h.data(), 48 * n, hipMemcpyHostToDevice, c->stream));
  XPIC_HIP(hipMemsetAsync(tot.p, 0, 8 * n, c->stream));
  XPIC_HIP(hipMemsetAsync(mx.p, 0, 4 * n, c->stream));
  // one launch covers at most kLaunchSteps steps, so no launch runs for seconds however long the trace
  for (int64_t first = 0; first < steps; first += kLaunchSteps) {
    const int ns = (int)std::min<int64_t>(kLaunchSteps, steps - first);
    Timed t(c, "dk_trace");
    if (gradB)
      hipLaunchKernelGGL(k_dk_trace<true>, dk_grid(n), dim3(kBlock), 0, c->stream, c->g, c->field[XPIC_E], c->field[XPIC_B], gradB,
        P, (long)n, (double*)s.p, (long)first, ns, (long)sample_every, (double*)sm.p, (long long*)tot.p, (int*)mx.p);
    else
      hipLaunchKernelGGL(k_dk_trace<false>, dk_grid(n), dim3(kBlock), 0, c->stream, c->g, c->field[XPIC_E], c->field[XPIC_B], gradB,
        P, (long)n, (double*)s.p, (long)first, ns, (long)sample_every, (double*)sm.p, (long long*)tot.p, (int*)mx.p);
    XPIC_HIP(hipGetLastError());
  }
  XPIC_HIP(hipMemcpyAsync(h.data(), s.p, 48 * n, hipMemcpyDeviceToHost, c->stream));
  XPIC_HIP(hipMemcpyAsync(iterations_total, tot.p, 8 * n, hipMemcpyDeviceToHost, c->stream));
  XPIC_HIP(hipMemcpyAsync(iterations_max, mx.p, 4 * n, hipMemcpyDeviceToHost, c->stream));
  std::vector<double> hs;
  if (nsamp > 0) {
    hs.resize((size_t)6 * n * nsamp);
    XPIC_HIP(hipMemcpyAsync(hs.data(), sm.p, 48 * n * nsamp, hipMemcpyDeviceToHost, c->stream)); // the samples, once
  }
  XPIC_HIP(hipStreamSynchronize(c->stream));
  to_aos(h.data(), n, state_6);
  for (int64_t k = 0; k < nsamp; ++k) to_aos(hs.data() + (size_t)6 * n * k, n, samples + (size_t)6 * n * k);
  return 0;
}

}  // namespace xpic
