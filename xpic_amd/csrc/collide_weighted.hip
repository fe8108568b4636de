// collide_weighted.hip -- binary Coulomb collisions between two sorts of unequal weight n / Np (Nanbu and Yonemura,
// J. Comput. Phys. 145, 639, 1998; the density factor for repeated meetings after Higginson et al., J. Comput. Phys. 413,
// 109450, 2020), DESIGN.md 5t.  AN EXTENSION, as collide.hip is: include/xpic_hip.h (xpic_collide_weighted) is the
// definition, tests/collisions_weighted_ref.py states it a second time in numpy float64.
//
// The mapping is k_collide<true>'s (collide.hip): one wave per cell, kWaves cells per workgroup, the keys and slots of a
// cell in LDS (cells above XPIC_COLLIDE_LDS_CELL: the second path through rank[]), one lane owning a short-side record
// through its meetings, no atomic on a velocity.  The pairing, the streams and the pair collision are xpic_collide's
// (collide_perm.h, collide_pair.h).  What is new: the density factor w_max N_short, a fourth draw u4 from the pair's
// stream, and the selection -- the lighter-weighted record always takes its new velocity, the heavier-weighted one iff
// u4 < r = w_min / w_max.  collide_pair runs on register copies; a rejected long-side record is not stored at all, a
// rejected short-side record keeps the value its lane holds.
//
// Compiled without floating-point contraction, as collide.hip is.
#include <cmath>

#include "common.h"
#include "device_common.h"
#include "collide_pair.h"
#include "collide_perm.h"

#pragma clang fp contract(off)

namespace xpic {

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kSumThreads = 64; // second stage of the reduction: one wave (as collide.hip)
constexpr int kLds = XPIC_COLLIDE_LDS_CELL;
constexpr int kTally = 7; // out6 and the cells that took the second path (xpic_collide_info)

struct ColWDev {
  uint64_t key;  // stream of (seed, step, sort_a, sort_b): xpic_collide's
  double c0;     // S q_a^2 q_b^2 / m_ab^2
  double wmax;   // the larger of the two weights n / Np
  double r;      // w_min / w_max, formed on the host
  double dt;
  double fa, fb; // m_ab / m_a, m_ab / m_b
  int a_heavy;   // the heavier-weighted sort is the call's a (equal weights: b, and r == 1 updates both)
};

constexpr int kTagPermA = 0, kTagPermB = 1, kTagPairs = 2; // the sub-streams of a cell (collide_pair.h: sub_key)

__device__ inline void load_v(const SortDev& s, int i, double* v) { v[0] = s.v[0][i]; v[1] = s.v[1][i]; v[2] = s.v[2][i]; }
__device__ inline void store_v(const SortDev& s, int i, const double* v) { s.v[0][i] = v[0]; s.v[1][i] = v[1]; s.v[2][i] = v[2]; }

// u4 of pair p: the draw after collide_pair's u1 u2 u3 from the same stream state
__device__ inline double fourth_draw(uint64_t st)
{
  (void)splitmix(st);
  (void)splitmix(st);
  (void)splitmix(st);
  return u01(st);
}

// the pairs of one cell; ba, bb: first record of the cell in A, B; sa, sb: the permutations
__device__ inline void cell_pairs(const ColWDev& P, const SortDev& A, const SortDev& B, uint64_t ck, int ba, int na, int bb,
  int nb, const int* sa, const int* sb, int lane, double* t)
{
  const uint64_t pairs = sub_key(ck, kTagPairs);
  const bool swap = na < nb; // the short side is the call's a
  const int ns = swap ? na : nb, nl = swap ? nb : na;
  const bool heavy_short = swap == (P.a_heavy != 0);
  const double cd = P.c0 * (P.wmax * (double)ns) * P.dt;
  for (int l = lane; l < ns; l += 64) {
    const int is = swap ? ba + sa[l] : bb + sb[l];
    double vs[3], vl[3];
    load_v(swap ? A : B, is, vs);
    for (int j = l; j < nl; j += ns) {
      const int il = swap ? bb + sb[j] : ba + sa[j];
      load_v(swap ? B : A, il, vl);
      double xs[3] = {vs[0], vs[1], vs[2]}, xl[3] = {vl[0], vl[1], vl[2]};
      const uint64_t st = item_state(pairs, j);
      const double made = t[0];
      if (swap) collide_pair(P.fa, P.fb, cd, st, xs, xl, t);
      else collide_pair(P.fa, P.fb, cd, st, xl, xs, t);
      if (t[0] == made) continue; // (|u| == 0: skipped and counted, nothing drawn, nothing stored)
      const bool keep = fourth_draw(st) < P.r;
      t[4] += keep ? 1.0 : 0.0;
      t[5] += keep ? 0.0 : 1.0;
      const bool ks = keep || !heavy_short; // the short-side record takes its new velocity
      vs[0] = ks ? xs[0] : vs[0];
      vs[1] = ks ? xs[1] : vs[1];
      vs[2] = ks ? xs[2] : vs[2];
      if (keep || heavy_short) store_v(swap ? B : A, il, xl); // (a rejected long-side record is not stored)
    }
    store_v(swap ? A : B, is, vs);
  }
}

template <bool LDS>
__device__ inline void cell_body(const ColWDev& P, const SortDev& A, const SortDev& B, uint64_t ck, int ba, int na, int bb, int nb,
  uint64_t* keys, int* sa, int* sb, int lane, double* t)
{
  permute<LDS>(sub_key(ck, kTagPermA), na, keys, sa, lane);
  permute<LDS>(sub_key(ck, kTagPermB), nb, keys, sb, lane);
  cell_pairs(P, A, B, ck, ba, na, bb, nb, sa, sb, lane, t);
}

// partial rows: out6, cells on the second path
__global__ void __launch_bounds__(kBlock) k_collide_weighted(GridDev g, SortDev A, SortDev B, ColWDev P, long ncell, double* partial)
{
  __shared__ uint64_t keys[kWaves][kLds];
  __shared__ int slot[kWaves][2][kLds];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long nw = (long)gridDim.x * kWaves;
  double t[kTally] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (long c = (long)blockIdx.x * kWaves + wave; c < ncell; c += nw) {
    const int ba = A.cell_start[c], na = A.cell_start[c + 1] - ba;
    const int bb = B.cell_start[c], nb = B.cell_start[c + 1] - bb;
    if (na == 0 || nb == 0) continue;
    const int x = (int)(c % g.nx), y = (int)((c / g.nx) % g.ny), zl = (int)(c / g.plane);
    const uint64_t ck = cell_key(P.key, ((long)(g.z0 + zl) * g.ny + y) * g.nx + x);
    if (na <= kLds && nb <= kLds) cell_body<true>(P, A, B, ck, ba, na, bb, nb, keys[wave], slot[wave][0], slot[wave][1], lane, t);
    else {
      cell_body<false>(P, A, B, ck, ba, na, bb, nb, nullptr, A.rank + ba, B.rank + bb, lane, t);
      if (lane == 0) t[6] += 1.0;
    }
  }
  block_reduce_store<kTally, kBlock>(t, partial, gridDim.x, blockIdx.x);
}

}  // namespace

int collide_weighted(xpic_ctx* c, int ia, int ib, const xpic_collision_params& p, int64_t step, double* out6)
{
  Sort& a = c->sorts[ia];
  Sort& b = c->sorts[ib];
  XPIC_CHECK(std::isfinite(p.strength) && p.strength >= 0.0, "collide_weighted: the strength must be finite and not negative");
  XPIC_CHECK(a.par.m > 0.0 && b.par.m > 0.0 && a.par.Np > 0 && b.par.Np > 0, "collide_weighted: a sort without mass or Np");
  const double wa = a.par.n / a.par.Np, wb = b.par.n / b.par.Np;
  XPIC_CHECK(std::isfinite(wa) && std::isfinite(wb) && wa > 0.0 && wb > 0.0,
    "collide_weighted: both sorts need a finite, positive weight n / Np");
  for (int k = 0; k < 6; ++k) out6[k] = 0.0;
  if (ia == ib) { // intra-species: always equal-weight, xpic_collide's path and bits; both records of a pair are updated
    XPIC_CALL(collide(c, ia, ib, p, step, out6));
    out6[4] = out6[0];
    return 0;
  }
  if (p.strength == 0.0) return 0; // (nothing is launched, nothing changes)
  ColWDev P{};
  uint64_t key = p.seed; // xpic_collide's call key
  (void)splitmix(key);
  key ^= (uint64_t)step * 0xD1342543DE82EF95ull;
  key = splitmix(key);
  key ^= (((uint64_t)(uint32_t)ia << 32) | (uint64_t)(uint32_t)ib) * 0x9FB21C651E98DF25ull;
  P.key = splitmix(key);
  const double mab = a.par.m * b.par.m / (a.par.m + b.par.m);
  P.c0 = p.strength * (a.par.q * a.par.q) * (b.par.q * b.par.q) / (mab * mab);
  P.wmax = wa > wb ? wa : wb;
  P.r = (wa > wb ? wb : wa) / P.wmax;
  P.a_heavy = wa > wb ? 1 : 0;
  P.dt = p.dt > 0.0 ? p.dt : c->g.dt;
  P.fa = mab / a.par.m;
  P.fb = mab / b.par.m;
  XPIC_CALL(sort_materialize(c, a)); // (a deferred re-binning whose assembly has not run)
  a.prebinned = false;               // (a pre-binning was made with the old velocities)
  XPIC_CALL(sort_materialize(c, b));
  b.prebinned = false;
  Timed t(c, "cmd_collide_weighted");
  double res[kTally] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (a.n > 0 && b.n > 0) {
    long nb = (c->ncell + kWaves - 1) / kWaves;
    if (nb > kRedBlocks) nb = kRedBlocks;
    hipLaunchKernelGGL(k_collide_weighted, dim3((unsigned)nb), dim3(kBlock), 0, c->stream, c->g, a.d, b.d, P, (long)c->ncell,
      c->red_partial);
    XPIC_HIP(hipGetLastError());
    XPIC_CALL(reduce_to_host(c, kTally, (int)nb, 1, false, res, kSumThreads));
  }
  c->collide_large_cells = (int64_t)res[6]; // (xpic_collide_info; this slab's)
  XPIC_CALL(comm_allreduce_sum_host(c, res, 6));
  for (int k = 0; k < 6; ++k) out6[k] = res[k];
  return 0;
}

}  // namespace xpic
