// shape2.h -- the second-order shape of the particle kernels, written once: Shape::setup(r, 1.5, spline_of_2nd_order)
// with the node pass of SimpleInterpolation, the walk over the 54 weights of the segment shape, the deposit weights of
// ParticlesChargeDensity and the small vector helpers of the tracers.  (The LDS-tile gather of the two hot pushes is
// not here: k_esirkepov_push<0> and k_es_push each carry their own text, see their file headers; k_es_push also keeps
// its own copy of deposit_weights3's expressions.  DESIGN.md 5i has the measurements.)
//   Shape::setup(r, 1.5, spline_of_2nd_order)        src/utils/shape.cpp:31-41
//   SimpleInterpolation, Shape::electric / magnetic  src/utils/shape.h:54-72
//   ImplicitEsirkepov::interpolate / decompose       src/algorithms/implicit_esirkepov.cpp:60-117
//   ParticlesChargeDensity::collect                  src/diagnostics/charge_conservation.cpp:34-97
// Rounding contract: this file sets no `#pragma clang fp contract` of its own; its text rounds as the pragma in force
// where it is FIRST included says.  The tracer units include it (through their step headers) after their
// `#pragma clang fp contract(on)`: contraction per source expression only.  eccapfim.hip and particles.hip include it
// at the top, under the compiler's default.  Every expression stands as its callers had it:
// the order of the sums over nodes is the reference's, the products are (z * y) * x with the field value multiplied
// afterwards, and the lattice and golden tests hold the bits.
// Everything is `__device__ inline`: tools/full_orbit_host.cpp compiles this text for the host.
// (esirkepov.hip's branch-free spline2 is a different expression, used only there; it stays there.)
#pragma once

#include "common.h"
#include "device_common.h"
#include "ie_shape.h"

namespace xpic {

// ---- Vector3 (src/utils/vector3.h) on double[3]
// Vector3::length (:160-164) is std::hypot of three arguments
__device__ inline double len3(const double* a)
{
#ifdef XPIC_FO_HOST
  return std::hypot(a[0], a[1], a[2]);
#else
  return norm3d(a[0], a[1], a[2]);
#endif
}
__device__ inline double dot3(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
// Vector3::cross (:212-219)
__device__ inline void cross3(const double* a, const double* b, double* o)
{
  o[0] = +(a[1] * b[2] - a[2] * b[1]);
  o[1] = -(a[0] * b[2] - a[2] * b[0]);
  o[2] = +(a[0] * b[1] - a[1] * b[0]);
}

// ---- Shape::setup(r) from global memory: the box [st, st + sz) of 3 or 4 nodes per axis.  The x and y weights of the
// node-centred ("No") and half-shifted ("Sh") kinds stay in registers; the z pair is formed plane by plane and the
// plane loop stays rolled (at most 4 trips, 16 nodes each), which keeps the loads of one plane in flight without
// holding the whole footprint in registers.
struct Shape2 {
  int st[3], sz[3];
  double No[2][4], Sh[2][4], prz;

  __device__ inline void setup(const GridDev& g, const double* r)
  {
    const double d[3] = {g.dx, g.dy, g.dz};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double pr = r[a] / d[a];
      st[a] = (int)round(pr - 1.5);             // Shape::make_start
      sz[a] = (int)floor(pr + 1.5) + 1 - st[a]; // Shape::make_end: 3 or 4
      if (a == 2) prz = pr; // its weights: nodes(), plane by plane
      else {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const double gx = (double)(st[a] + t);
          No[a][t] = spline2_ref(pr - gx);
          Sh[a][t] = spline2_ref(pr - (gx + 0.5));
        }
      }
    }
  }

  // f(gx, gy, gz, Noz, Shz, Noy, Shy, Nox, Shx) for every node of the box in the reference's order (x fastest, then y,
  // z); gx, gy, gz in global numbering.  The index of the node and the sums are the caller's.
  template <class F>
  __device__ inline void nodes(F&& f) const
  {
    const int nz = sz[2] < 4 ? sz[2] : 4; // 3 or 4 by construction; the bound does not depend on that
#pragma unroll 1
    for (int kz = 0; kz < nz; ++kz) {
      const double gz = (double)(st[2] + kz);
      const double Noz = spline2_ref(prz - gz), Shz = spline2_ref(prz - (gz + 0.5));
#pragma unroll
      for (int jy = 0; jy < 4; ++jy) {
        if (jy < sz[1]) {
#pragma unroll
          for (int ix = 0; ix < 4; ++ix) {
            if (ix < sz[0]) f(st[0] + ix, st[1] + jy, st[2] + kz, Noz, Shz, No[1][jy], Sh[1][jy], No[0][ix], Sh[0][ix]);
          }
        }
      }
    }
  }
};

// ---- the 54 weights of the segment shape (ie_shape.h) in the reference's running index m: f(cx, node, weight), cx the
// component, node its element in a field vector's component
template <class F>
__device__ inline void segment_nodes(const GridDev& g, const IEShape& sh, F&& f)
{
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
          f(cx, ie_node(g, sh.start[0] + o[0], sh.start[1] + o[1], sh.start[2] + o[2]), sh.cache[m]);
        }
  }
}

// E_p of ImplicitEsirkepov::interpolate (:71-90)
__device__ inline void segment_gather_E(const GridDev& g, const double* __restrict__ E, const IEShape& sh, double* Ep)
{
  Ep[0] = Ep[1] = Ep[2] = 0.0;
  segment_nodes(g, sh, [&](int cx, long o, double w) { Ep[cx] += E[cx * g.cstride + o] * w; });
}

// ---- ParticlesChargeDensity::collect (:34-97): three nodes per axis from st = ceil(pr - 1.5), pr the scaled position
__device__ inline void deposit_weights3(const double* pr, int* st, double (*w)[3])
{
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    st[a] = (int)ceil(pr[a] - 1.5);
#pragma unroll
    for (int t = 0; t < 3; ++t) w[a][t] = spline2_ref(pr[a] - (double)(st[a] + t));
  }
}

}  // namespace xpic
