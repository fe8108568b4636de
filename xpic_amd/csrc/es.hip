// es.hip -- the particle phase of the electrostatic scheme (include/xpic_es.h; an extension: the reference has no
// electrostatic scheme): gather E^n and B at r^n, Boris kick v^{n-1/2} -> v^{n+1/2}, full move r^n -> r^{n+1},
// and the second-order charge deposit of r^{n+1} -- xpic_charge_density's rule (particles.hip: k_charge_density), fused
// into the push.
//
// The layout is esirkepov.hip's (its header comment), cut down to what a scalar deposit needs:
//   * a workgroup (4 waves) owns one x-pencil of cells and marches along it in ROUNDS.  A round takes the particles of as
//     many consecutive cells (up to 16) as fit into its 256 lanes, one particle per lane whatever the occupancy of the
//     cells; a cell with more particles than that continues in the next round.  The rounds depend on cell_start alone
//     and are composed by every wave alike from scalar loads, one round ahead; the particles of round r + 1 are
//     requested while round r works.
//   * the gather reads E and B from an LDS tile of the 21 x 6 x 6 nodes the round's particles can reach (nodes c-2 .. c+3
//     of each axis): k_esirkepov_push<0>'s node ranges, weight types per component and summation order, at the stored
//     position instead of the half-moved one.  (That text is copied, not shared: the issue of this
//     scheme left k_esirkepov_push untouched.  A change to either gather belongs in both; esirkepov.hip's header says so too.)
//   * the deposit: a particle that ends within one cell of its home cell has its three nodes per axis inside c-2 .. c+3:
//     its 27 values are added into a circular LDS window of 32 x 6 x 6 nodes along x with LDS fp64 adds -- no global
//     atomic.  The window nodes the march has passed leave with one global fp64 atomic each (zeros stay).  A particle
//     that ends further away -- any number of cells, across the periodic wrap -- adds its 27 values to the global
//     accumulator with atomics (slow path): the same weights, the same products, indices folded by a true modulo.
// LDS: tile 6 x 756 doubles (36 288 B) + window 1 152 doubles (9 216 B) = 45.5 KB; 254 VGPRs: two workgroups per CU (__launch_bounds__(256, 2)),
// registers the limit.
// The matrix-core form of the deposit (a rank-K product per cell, a third of esirkepov.hip's phase 2) is not built:
// DESIGN.md 5zb.
#include <cstring>

#include "common.h"
#include "device_common.h"

namespace xpic {

namespace {

constexpr int kThreadsE = 256;
constexpr int kSegE = 16;                        // cells per round
constexpr int kTE = 6;                           // tile and window per transverse axis: nodes c-2 .. c+3
constexpr int kTXE = kSegE + kTE - 1;            // tile along x
constexpr int kTileE = kTXE * kTE * kTE;         // nodes of one component's tile
constexpr int kFtE = (6 * kTileE + kThreadsE - 1) / kThreadsE;
constexpr int kWinX = 32;                        // circular window along x (a power of two >= kTXE)
constexpr int kWinN = kWinX * kTE * kTE;
static_assert(kSegE <= kCellStartPad && kTXE <= kWinX && (kWinX & (kWinX - 1)) == 0, "round geometry");

using UniformIntsE = const __attribute__((address_space(4))) int*; // wave-uniform reads of cell_start: scalar loads

// drains LDS traffic only: the particle stores, the atomics and the next round's requests stay in flight across it
__device__ inline void lds_barrier_e()
{
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

struct EsRound {
  int base;            // first cell of the round (>= nx: the pencil is done)
  int p0, pend;        // its particles: consecutive in the sort, lane t takes p0 + t
  int ncell;           // cells it covers
  int next, next_off;  // where the next round starts: cell, particles of that cell already handed out
  int cv[kSegE + 1];   // cell_start of the cells base .. base + kSegE
};

struct EsAhead {
  int p, crel;
  double r[3], v[3];
};

template <bool P2>
__global__ void __launch_bounds__(kThreadsE, 2) k_es_push(GridDev g, SortDev s, const double* __restrict__ E,
  const double* __restrict__ B, double* __restrict__ rho, double qm, double qn, int* bad_count)
{
  __shared__ double ftile[6 * kTileE]; // Ex, Ey, Ez, Bx, By, Bz
  __shared__ double win[kWinN];        // rho on the nodes [flushed, flushed + 32) x (cy-2 .. cy+3) x (cz-2 .. cz+3)

  const int cy = blockIdx.x % g.ny;
  const int cz = blockIdx.x / g.ny;
  const long pencil0 = ((long)cz * g.ny + cy) * g.nx;
  UniformIntsE cs = (UniformIntsE)(s.cell_start + pencil0);
  for (int t = threadIdx.x; t < kWinN; t += kThreadsE) win[t] = 0.0;

  auto compose = [&](int cur, int cur_off) {
    EsRound R;
    R.base = cur; R.p0 = 0; R.pend = 0; R.ncell = 0; R.next = cur; R.next_off = 0;
#pragma unroll
    for (int i = 0; i <= kSegE; ++i) R.cv[i] = 0;
    if (cur >= g.nx) return R;
#pragma unroll
    for (int i = 0; i <= kSegE; ++i) R.cv[i] = cs[min(cur + i, g.nx)];
    const int p0 = R.cv[0] + cur_off;
    int ncell = 0, pend = p0;
    bool open = true;
#pragma unroll
    for (int i = 0; i < kSegE; ++i) {
      if (open && cur + i < g.nx) {
        if (R.cv[i + 1] - p0 <= kThreadsE) { ncell = i + 1; pend = R.cv[i + 1]; }
        else open = false;
      }
    }
    R.p0 = p0;
    if (ncell == 0) { // what is left of the first cell is more than a round holds: a full round of it
      R.pend = p0 + kThreadsE; R.ncell = 1; R.next = cur; R.next_off = cur_off + kThreadsE;
    }
    else { R.pend = pend; R.ncell = ncell; R.next = cur + ncell; R.next_off = 0; }
    return R;
  };
  auto request = [&](const EsRound& R) {
    EsAhead pf;
    pf.p = -1; pf.crel = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) { pf.r[a] = 0.0; pf.v[a] = 0.0; }
    const int p = R.p0 + (int)threadIdx.x;
    if (R.base < g.nx && p < R.pend) {
      int crel = 0;
#pragma unroll
      for (int i = 1; i < kSegE; ++i) crel += (i < R.ncell && p >= R.cv[i]) ? 1 : 0;
      pf.p = p; pf.crel = crel;
#pragma unroll
      for (int a = 0; a < 3; ++a) { pf.r[a] = s.r[a][p]; pf.v[a] = s.v[a][p]; }
    }
    return pf;
  };
  // the window's nodes [from, upto) along x leave: one global atomic per node that holds something
  auto flush = [&](int from, int upto) {
    const int cnt = upto - from;
    for (int e = threadIdx.x; e < cnt * kTE * kTE; e += kThreadsE) {
      const int xi = e % cnt, yz = e / cnt;
      const int x = from + xi;
      const int w = yz * kWinX + ((x + 2) & (kWinX - 1));
      const double val = win[w];
      if (val != 0.0) {
        win[w] = 0.0;
        unsafeAtomicAdd(&rho[g.nodew(x, cy - 2 + yz % kTE, cz - 2 + yz / kTE)], val);
      }
    }
  };

  const double dt = g.dt;
  int bad = 0;
  int flushed = -2; // the window starts at node -2 = base - 2 of the first round

  EsRound R = compose(0, 0);
  __syncthreads();
  EsAhead pf = request(R);
  while (R.base < g.nx) {
    const int base = R.base;
    const bool any = R.pend > R.p0;
    // ---- this round's tile: DMGlobalToLocal(E), (B) for the nodes its particles gather from
    double ft[kFtE];
    if (any) {
#pragma unroll
      for (int k = 0; k < kFtE; ++k) {
        const int t = threadIdx.x + k * kThreadsE;
        ft[k] = 0.0;
        if (t < 6 * kTileE) {
          const int f = t / kTileE, n = t % kTileE;
          const int tx = n % kTXE, ty = (n / kTXE) % kTE, tz = n / (kTXE * kTE);
          const double* F = (f < 3 ? E : B) + (f % 3) * g.cstride;
          // (a particle of the pencil's last cell reaches node nx + 2 at most, and nodew folds an index once)
          if (base - 2 + tx <= g.nx + 2) ft[k] = F[g.nodew(base - 2 + tx, cy - 2 + ty, cz - 2 + tz)];
        }
      }
    }
    const EsRound Rn = compose(R.next, R.next_off);
    if (any) {
#pragma unroll
      for (int k = 0; k < kFtE; ++k) {
        const int t = threadIdx.x + k * kThreadsE;
        if (t < 6 * kTileE) ftile[t] = ft[k];
      }
    }
    lds_barrier_e();
    const EsAhead me = pf;
    pf = request(Rn);

    if (me.p >= 0) {
      const int p = me.p, crel = me.crel;
      double r[3] = {me.r[0], me.r[1], me.r[2]}, v[3] = {me.v[0], me.v[1], me.v[2]};
      const int cc[3] = {base + crel, cy, cz + g.z0};
      double Ep[3] = {0, 0, 0}, Bp[3] = {0, 0, 0};
      // shape.setup(point.r) ; interpolation.process: k_esirkepov_push<0>'s gather (esirkepov.hip), its expressions and order
      int off[3], nN[3];
      double No[3][3], Sh[3][3];
      bool inside = true;
      double prs[3];
      scaled_position<P2>(g, r[0], r[1], r[2], prs);
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const double pr = prs[a];
        inside = inside && fabs(pr) < 1.0e9; // (not a number, or beyond what an int holds: no index is formed from it)
        const int gst = inside ? (int)round(pr - 1.5) : 0;
        const int gsz = inside ? (int)floor(pr + 1.5) + 1 - gst : 0;
        inside = inside && gst >= cc[a] - 2 && gst + gsz <= cc[a] + 4;
        nN[a] = (pr - (double)gst) < 1.5 ? 0 : 1;
        off[a] = gst - (cc[a] - 2);
        const double sN = pr - (double)(gst + nN[a]), sS = pr - ((double)gst + 0.5);
        const double tNl = 1.5 - sN, tNr = 1.5 + (sN - 2.0), tSl = 1.5 - sS, tSr = 1.5 + (sS - 2.0);
        No[a][0] = 0.5 * tNl * tNl; No[a][1] = 0.75 - (sN - 1.0) * (sN - 1.0); No[a][2] = 0.5 * tNr * tNr;
        Sh[a][0] = 0.5 * tSl * tSl; Sh[a][1] = 0.75 - (sS - 1.0) * (sS - 1.0); Sh[a][2] = 0.5 * tSr * tSr;
      }
      if (inside) {
        off[0] += crel; // the tile's x origin is base - 2, the cell's own is cx - 2
        const int bN[3] = {off[0] + nN[0], off[1] + nN[1], off[2] + nN[2]};
#pragma nounroll
        for (int kz = 0; kz < 3; ++kz) {
          const double nz = No[2][kz], sz = Sh[2][kz];
          const int zN = (bN[2] + kz) * kTE, zS = (off[2] + kz) * kTE;
#pragma unroll
          for (int jy = 0; jy < 3; ++jy) {
            const int yN = bN[1] + jy, yS = off[1] + jy;
            const double nn = nz * No[1][jy], ns = nz * Sh[1][jy], sn = sz * No[1][jy], ss = sz * Sh[1][jy];
            double f[6][3];
#pragma unroll
            for (int ix = 0; ix < 3; ++ix) {
              const int xN = bN[0] + ix, xS = off[0] + ix;
              f[0][ix] = ftile[0 * kTileE + (zN + yN) * kTXE + xS];
              f[1][ix] = ftile[1 * kTileE + (zN + yS) * kTXE + xN];
              f[2][ix] = ftile[2 * kTileE + (zS + yN) * kTXE + xN];
              f[3][ix] = ftile[3 * kTileE + (zS + yS) * kTXE + xN];
              f[4][ix] = ftile[4 * kTileE + (zS + yN) * kTXE + xS];
              f[5][ix] = ftile[5 * kTileE + (zN + yS) * kTXE + xS];
            }
            double tx[6];
#pragma unroll
            for (int q = 0; q < 6; ++q) {
              const double (&wx)[3] = (q == 0 || q >= 4) ? Sh[0] : No[0];
              tx[q] = f[q][0] * wx[0] + f[q][1] * wx[1] + f[q][2] * wx[2];
            }
            Ep[0] += nn * tx[0];
            Ep[1] += ns * tx[1];
            Ep[2] += sn * tx[2];
            Bp[0] += ss * tx[3];
            Bp[1] += sn * tx[4];
            Bp[2] += ns * tx[5];
          }
        }
        update_vEB(dt, qm, Ep, Bp, v);            // push.update_vEB(dt)
#pragma unroll
        for (int a = 0; a < 3; ++a) r[a] += v[a] * dt; // push.update_r(dt): the full leapfrog move
      }
      // ---- the deposit at the new position: k_charge_density's expressions
      const double pn[3] = {r[0] / g.dx, r[1] / g.dy, r[2] / g.dz};
      bool ok = inside && fabs(pn[0]) < 1.0e9 && fabs(pn[1]) < 1.0e9 && fabs(pn[2]) < 1.0e9;
      if (!ok) ++bad; // a stale cell, or a position or velocity that is not finite: nothing is stored or deposited
      else {
#pragma unroll
        for (int a = 0; a < 3; ++a) { s.r[a][p] = r[a]; s.v[a][p] = v[a]; }
        int st[3];
        double w[3][3];
        bool fast = true;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          st[a] = (int)ceil(pn[a] - 1.5);
#pragma unroll
          for (int t = 0; t < 3; ++t) w[a][t] = spline2_ref(pn[a] - (double)(st[a] + t));
          fast = fast && st[a] >= cc[a] - 2 && st[a] + 2 <= cc[a] + 3;
        }
        if (fast) {
          const int ox = st[0] + 2, oy = st[1] - (cc[1] - 2), oz = st[2] - (cc[2] - 2);
#pragma unroll
          for (int k = 0; k < 3; ++k)
#pragma unroll
            for (int j = 0; j < 3; ++j)
#pragma unroll
              for (int i = 0; i < 3; ++i) {
                const double val = w[0][i] * w[1][j] * w[2][k];
                if (val != 0.0) unsafeAtomicAdd(&win[((oz + k) * kTE + (oy + j)) * kWinX + ((ox + i) & (kWinX - 1))], qn * val);
              }
        }
        else {
          for (int k = 0; k < 3; ++k) {
            // the plane: folded over the whole box; on a slab it must then lie in the stored planes
            int zl = st[2] + k - g.z0, zs;
            if (g.G == 0) zs = GridDev::wrap(zl, g.nzl);
            else {
              if (zl < -g.G || zl >= g.nzl + g.G) {
                zl = GridDev::wrap(zl, g.nzg);
                if (zl >= g.nzl + g.G) zl -= g.nzg;
              }
              if (zl < -g.G || zl >= g.nzl + g.G) { ++bad; continue; } // beyond the neighbour slabs' ghost planes
              zs = zl + g.G;
            }
            for (int j = 0; j < 3; ++j)
              for (int i = 0; i < 3; ++i) {
                const int x = GridDev::wrap(st[0] + i, g.nx), y = GridDev::wrap(st[1] + j, g.ny);
                const double val = w[0][i] * w[1][j] * w[2][k];
                if (val != 0.0) unsafeAtomicAdd(&rho[g.node(x, y, zs)], qn * val);
              }
          }
        }
      }
    }
    lds_barrier_e();
    // nodes below the next round's base - 2 are complete
    const int upto = min(Rn.base, g.nx) - 2;
    if (upto > flushed) { flush(flushed, upto); flushed = upto; }
    R = Rn;
  }
  __syncthreads();
  flush(flushed, flushed + kWinX); // what is left: every column once (columns that hold nothing form no index)
  if (bad) atomicAdd(bad_count, bad);
}

}  // namespace

int es_push(xpic_ctx* c, Sort& s, const double* E, const double* B, double* rho)
{
  XPIC_CALL(sort_materialize(c, s));
  s.prebinned = false;
  const GridDev& g = c->g;
  XPIC_CHECK(g.nx >= 6 && g.ny >= 6 && g.nzl >= 6, "the electrostatic push needs every grid extent >= 6");
  const long nblocks = (long)g.ny * g.nzl; // one workgroup per x-pencil
  XPIC_CHECK(nblocks < 2147483647L, "too many pencils for one launch");
  double red[1] = {0.0};
  if (s.n > 0) {
    int* flag = (int*)c->red_out;
    XPIC_HIP(hipMemsetAsync(flag, 0, sizeof(double), c->stream));
    const double qm = s.par.q / s.par.m;
    const double qn = s.par.q * (s.par.n / s.par.Np); // charge_density's value
    {
      Timed t(c, "es_push");
      hipLaunchKernelGGL(g.pow2 ? k_es_push<true> : k_es_push<false>, dim3((unsigned)nblocks), dim3(kThreadsE), 0, c->stream, g, s.d, E, B,
        rho, qm, qn, flag);
      XPIC_HIP(hipGetLastError());
    }
    XPIC_HIP(hipMemcpyAsync(c->red_host, flag, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    XPIC_HIP(hipStreamSynchronize(c->stream));
    int bad;
    memcpy(&bad, c->red_host, sizeof(int));
    red[0] = (double)bad;
  }
  // every z-slab leaves with the same return code (an empty slab takes part too)
  XPIC_CALL(comm_allreduce_sum_host(c, red, 1));
  if (red[0] != 0.0) {
    set_error(std::to_string((long)red[0]) + " particle(s) of an electrostatic push are not finite, lie outside their cell, or left "
      "the neighbouring z-slabs' ghost planes");
    return 6;
  }
  return 0;
}

}  // namespace xpic
