// full_orbit_host.cpp -- the device functions of xpic_amd/csrc/full_orbit_step.h compiled for the host, with a main of
// their own: tools/full_orbit_host_check.py runs them against the numpy restatement (tests/full_orbit_ref.py) before
// anything is sent to a GPU.  No HIP call is made and no GPU is needed; host sanitizers apply (the script's --sanitize).
//   hipcc -x hip --offload-host-only -O2 -std=c++17 -DXPIC_FO_HOST tools/full_orbit_host.cpp -o full_orbit_host
//   full_orbit_host <in> <out>
// <in>:  int32 {nx, ny, nz, n, mode, maxit, steps, 0}, double {dx, dy, dz, qm, dt, atol, rtol}, E and B as
//        [3][nz][ny][nx] (the stored layout of a single-slab context), records [n][6]
//        mode 0 .. 17: `steps` steps of that xpic_fo_scheme; -1: the gather at r (records {r, -});
//        -2: the segment gather (records {rn, r0})
// <out>: double [n][7]: the six results ({E_p, B_p} for the gathers) and the last step's iteration count
#include <cmath>
#include <cstdio>
#include <vector>

#include "../xpic_amd/csrc/common.h"
// every `__device__ inline` function of the headers below becomes a host function too
#undef __device__
#define __device__ __attribute__((host)) __attribute__((device))
#include "../xpic_amd/csrc/device_common.h"
#include "../xpic_amd/csrc/ie_shape.h"

#pragma clang fp contract(on)

#include "../xpic_amd/csrc/full_orbit_step.h"

using namespace xpic;

template <class T>
static bool read_n(FILE* f, std::vector<T>& v, size_t n)
{
  v.resize(n);
  return fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char** argv)
{
  if (argc != 3) { fprintf(stderr, "usage: %s <in> <out>\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  std::vector<int32_t> hi;
  std::vector<double> hd, E, B, pts;
  bool ok = read_n(f, hi, 8) && read_n(f, hd, 7);
  if (!ok || hi[0] < 1 || hi[1] < 1 || hi[2] < 1 || hi[3] < 0 || hi[5] > XPIC_FO_MAXIT || hi[6] < 0) {
    fprintf(stderr, "bad header\n");
    return 2;
  }
  const int nx = hi[0], ny = hi[1], nz = hi[2], mode = hi[4], maxit = hi[5], steps = hi[6];
  const size_t n = (size_t)hi[3], nvec = (size_t)3 * nx * ny * nz;
  ok = read_n(f, E, nvec) && read_n(f, B, nvec) && read_n(f, pts, 6 * n);
  fclose(f);
  if (!ok) { fprintf(stderr, "short input\n"); return 2; }

  GridDev g{};
  g.nx = nx; g.ny = ny; g.nzl = nz; g.nzg = nz; g.z0 = 0; g.G = 0; g.nzs = nz;
  g.dx = hd[0]; g.dy = hd[1]; g.dz = hd[2];
  g.plane = (long)nx * ny; g.cstride = (long)nz * g.plane; g.nown = g.cstride;
  const double qm = hd[3], dt = hd[4], atol = hd[5], rtol = hd[6];

  std::vector<double> out(7 * n, 0.0);
  for (size_t q = 0; q < n; ++q) {
    const double* p = &pts[6 * q];
    double* o = &out[7 * q];
    if (mode == -1) fo_gather<true>(g, E.data(), B.data(), p, o, o + 3);
    else if (mode == -2) fo_gather_segment(g, E.data(), B.data(), p, p + 3, o, o + 3);
    else {
      FOPoint pn;
      for (int c = 0; c < 3; ++c) { pn.r[c] = p[c]; pn.p[c] = p[3 + c]; }
      int it = 0;
      for (int k = 0; k < steps; ++k) {
        if (mode == XPIC_FO_CN) {
          const FOPoint p0 = pn;
          it = fo_cn_process(g, E.data(), B.data(), qm, dt, atol, rtol, maxit, pn, p0);
        }
        else fo_step(mode, g, E.data(), B.data(), qm, dt, pn);
      }
      for (int c = 0; c < 3; ++c) { o[c] = pn.r[c]; o[3 + c] = pn.p[c]; }
      o[6] = it;
    }
  }
  f = fopen(argv[2], "wb");
  if (!f) { perror(argv[2]); return 2; }
  ok = fwrite(out.data(), sizeof(double), out.size(), f) == out.size();
  fclose(f);
  return ok ? 0 : 2;
}
