// ie_shape.h -- the segment shape of ImplicitEsirkepov (src/algorithms/implicit_esirkepov.cpp:11-57) and the node
// numbering of its gathers, shared by eccapfim.hip and the tracers.  shape2.h walks its 54 weights (segment_nodes,
// segment_gather_E).
#pragma once

#include "common.h"

namespace xpic {

__device__ inline double ie_sfunc_1(double s) { return 1.0 - fabs(s); }
__device__ inline double ie_sfunc_2(int j, double s)
{
  s = fabs(s);
  return j == 1 ? (0.75 - s * s) : 0.5 * (1.5 - s) * (1.5 - s);
}
struct IEShape {
  int start[3];
  double cache[54];
  __device__ void setup(const GridDev& g, const double* rn, const double* r0)
  {
    const double d[3] = {g.dx, g.dy, g.dz};
    double prn[3], pr0[3], prh[3], gc[3], gv[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      prn[c] = rn[c] / d[c];
      pr0[c] = r0[c] / d[c];
      prh[c] = 0.5 * (prn[c] + pr0[c]);
      gc[c] = round(prh[c]);
      start[c] = (int)gc[c] - 1;
      gv[c] = gc[c] + 0.5;
    }
    int m = 0;
    const double sixth = 1.0 / 6.0;
#pragma unroll
    for (int cx = 0; cx < 3; cx++) {
      const int cy = (cx + 1) % 3, cz = (cx + 2) % 3;
#pragma unroll
      for (int i = 0; i < 2; i++) {
        const double shx = sixth * ie_sfunc_1(gv[cx] + (i - 1) - prh[cx]);
#pragma unroll
        for (int j = 0; j < 3; j++) {
          const double sny = ie_sfunc_2(j, gc[cy] + (j - 1) - prn[cy]);
          const double s0y = ie_sfunc_2(j, gc[cy] + (j - 1) - pr0[cy]);
#pragma unroll
          for (int k = 0; k < 3; k++) {
            const double snz = ie_sfunc_2(k, gc[cz] + (k - 1) - prn[cz]);
            const double s0z = ie_sfunc_2(k, gc[cz] + (k - 1) - pr0[cz]);
            cache[m++] = shx * (sny * (2 * snz + s0z) + s0y * (2 * s0z + snz));
          }
        }
      }
    }
  }
};

// node (gx, gy, gz) in global numbering -> element of component c of a field vector
__device__ inline long ie_node(const GridDev& g, int gx, int gy, int gz)
{
  const int x = g.wrap(gx, g.nx), y = g.wrap(gy, g.ny);
  const int zl = g.G == 0 ? g.wrap(gz, g.nzl) : gz - g.z0;
  return g.node(x, y, g.wz(zl));
}

}  // namespace xpic
