// collide.hip -- binary Coulomb collisions between the records of one cell (Takizuka and Abe, J. Comput. Phys. 25, 205,
// 1977), non-relativistic.  AN EXTENSION: the reference has no collision operator; include/xpic_hip.h
// (xpic_collide) is the definition, tests/collisions_ref.py states it a second time in numpy float64.
//
// One wave per cell, kWaves cells per workgroup.  The lanes form the 64-bit keys of the cell's records (record i, in cell
// order) into LDS; a record's rank is the number of (key, i) below its own -- a count over the staged keys, quadratic in the
// cell's population, which is tens -- and slot[rank] = i is the permutation.  Each lane then takes pairs: a record is read
// and written by exactly one lane, so there is no atomic on a velocity.  The odd cell's triple and the meetings of one
// record of the short side are serial by definition and stay in one lane.  Cells of more than XPIC_COLLIDE_LDS_CELL records
// of a sort take the same body with the keys recomputed where they are compared and the slots in the sort's rank[] array
// (binning scratch: the callers drop the pre-binning anyway, its keys describe the old velocities).
//
// Compiled without floating-point contraction: the collision is rounded operation by operation, as numpy rounds it.  The
// collision itself and the streams are collide_pair.h's, shared with collide_trace.hip; the permutation and the wave-level
// hand-over are collide_perm.h's, shared with collide_weighted.hip.
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
constexpr int kSumThreads = 64; // second stage of the reduction: one wave (as commands.hip)
constexpr int kLds = XPIC_COLLIDE_LDS_CELL;
constexpr int kTally = 5; // out4 and the cells that took the second path (xpic_collide_info)

struct ColDev {
  uint64_t key;  // stream of (seed, step, sort_a, sort_b)
  double c0;     // S q_a^2 q_b^2 / m_ab^2
  double w;      // n / Np of both sorts
  double dt;
  double fa, fb; // m_ab / m_a, m_ab / m_b
};

constexpr int kTagPermA = 0, kTagPermB = 1, kTagPairs = 2; // the sub-streams of a cell (collide_pair.h: sub_key)

// one collision of pair p of the cell's pair stream (collide_pair.h); cdt = c0 n_L dt of this pair
__device__ inline void collide_pair(const ColDev& P, double cdt, uint64_t pairs, int p, double* va, double* vb, double* t)
{
  collide_pair(P.fa, P.fb, cdt, item_state(pairs, p), va, vb, t);
}

__device__ inline void load_v(const SortDev& s, int i, double* v) { v[0] = s.v[0][i]; v[1] = s.v[1][i]; v[2] = s.v[2][i]; }
__device__ inline void store_v(const SortDev& s, int i, const double* v) { s.v[0][i] = v[0]; s.v[1][i] = v[1]; s.v[2][i] = v[2]; }

// the pairs of one cell; ba, bb: first record of the cell in A, B; sa, sb: the permutations (INTER: of both)
template <bool INTER>
__device__ inline void cell_pairs(const ColDev& P, const SortDev& A, const SortDev& B, uint64_t ck, int ba, int na, int bb,
  int nb, const int* sa, const int* sb, int lane, double* t)
{
  const uint64_t pairs = sub_key(ck, kTagPairs);
  if (!INTER) {
    const double cn = P.c0 * (P.w * (double)na);
    const int first = (na & 1) ? 3 : 0; // an odd cell starts with the triple: its pairs are p = 0, 1, 2
    const int np = (na - first) >> 1;
    if (first && lane == 63) {
      const int i0 = ba + sa[0], i1 = ba + sa[1], i2 = ba + sa[2];
      double v0[3], v1[3], v2[3];
      load_v(A, i0, v0);
      load_v(A, i1, v1);
      load_v(A, i2, v2);
      const double ch = cn * (0.5 * P.dt);
      collide_pair(P, ch, pairs, 0, v0, v1, t);
      collide_pair(P, ch, pairs, 1, v1, v2, t);
      collide_pair(P, ch, pairs, 2, v2, v0, t);
      store_v(A, i0, v0);
      store_v(A, i1, v1);
      store_v(A, i2, v2);
    }
    const double cd = cn * P.dt;
    for (int k = lane; k < np; k += 64) {
      const int i0 = ba + sa[first + 2 * k], i1 = ba + sa[first + 2 * k + 1];
      double v0[3], v1[3];
      load_v(A, i0, v0);
      load_v(A, i1, v1);
      collide_pair(P, cd, pairs, first + k, v0, v1, t);
      store_v(A, i0, v0);
      store_v(A, i1, v1);
    }
  }
  else {
    const bool swap = na < nb; // the short side is the call's a
    const int ns = swap ? na : nb, nl = swap ? nb : na;
    const double cd = P.c0 * (P.w * (double)ns) * P.dt;
    for (int l = lane; l < ns; l += 64) {
      const int is = swap ? ba + sa[l] : bb + sb[l];
      double vs[3], vl[3];
      load_v(swap ? A : B, is, vs);
      for (int j = l; j < nl; j += ns) {
        const int il = swap ? bb + sb[j] : ba + sa[j];
        load_v(swap ? B : A, il, vl);
        if (swap) collide_pair(P, cd, pairs, j, vs, vl, t);
        else collide_pair(P, cd, pairs, j, vl, vs, t);
        store_v(swap ? B : A, il, vl);
      }
      store_v(swap ? A : B, is, vs);
    }
  }
}

template <bool INTER, bool LDS>
__device__ inline void cell_body(const ColDev& P, const SortDev& A, const SortDev& B, uint64_t ck, int ba, int na, int bb, int nb,
  uint64_t* keys, int* sa, int* sb, int lane, double* t)
{
  permute<LDS>(sub_key(ck, kTagPermA), na, keys, sa, lane);
  if (INTER) permute<LDS>(sub_key(ck, kTagPermB), nb, keys, sb, lane);
  cell_pairs<INTER>(P, A, B, ck, ba, na, bb, nb, sa, sb, lane, t);
}

// partial rows: out4, cells on the second path
template <bool INTER>
__global__ void __launch_bounds__(kBlock) k_collide(GridDev g, SortDev A, SortDev B, ColDev P, long ncell, double* partial)
{
  __shared__ uint64_t keys[kWaves][kLds];
  __shared__ int slot[kWaves][2][kLds];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long nw = (long)gridDim.x * kWaves;
  double t[kTally] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (long c = (long)blockIdx.x * kWaves + wave; c < ncell; c += nw) {
    const int ba = A.cell_start[c], na = A.cell_start[c + 1] - ba;
    const int bb = INTER ? B.cell_start[c] : ba, nb = INTER ? B.cell_start[c + 1] - bb : na;
    if (INTER ? (na == 0 || nb == 0) : na < 2) continue;
    const int x = (int)(c % g.nx), y = (int)((c / g.nx) % g.ny), zl = (int)(c / g.plane);
    const uint64_t ck = cell_key(P.key, ((long)(g.z0 + zl) * g.ny + y) * g.nx + x);
    if (na <= kLds && nb <= kLds) cell_body<INTER, true>(P, A, B, ck, ba, na, bb, nb, keys[wave], slot[wave][0], slot[wave][1], lane, t);
    else {
      cell_body<INTER, false>(P, A, B, ck, ba, na, bb, nb, nullptr, A.rank + ba, B.rank + bb, lane, t);
      if (lane == 0) t[4] += 1.0;
    }
  }
  block_reduce_store<kTally, kBlock>(t, partial, gridDim.x, blockIdx.x);
}

}  // namespace

int collide(xpic_ctx* c, int ia, int ib, const xpic_collision_params& p, int64_t step, double* out4)
{
  Sort& a = c->sorts[ia];
  Sort& b = c->sorts[ib];
  const bool inter = ia != ib;
  XPIC_CHECK(std::isfinite(p.strength) && p.strength >= 0.0, "collide: the strength must be finite and not negative");
  XPIC_CHECK(a.par.m > 0.0 && b.par.m > 0.0 && a.par.Np > 0 && b.par.Np > 0, "collide: a sort without mass or Np");
  const double wa = a.par.n / a.par.Np, wb = b.par.n / b.par.Np;
  XPIC_CHECK(wa == wb, "collide: the two sorts must carry the same weight n / Np (Takizuka-Abe pairs equal-weight particles)");
  for (int k = 0; k < 4; ++k) out4[k] = 0.0;
  if (p.strength == 0.0) return 0; // (nothing is launched, nothing changes)
  ColDev P{};
  uint64_t key = p.seed;
  (void)splitmix(key);
  key ^= (uint64_t)step * 0xD1342543DE82EF95ull;
  key = splitmix(key);
  key ^= (((uint64_t)(uint32_t)ia << 32) | (uint64_t)(uint32_t)ib) * 0x9FB21C651E98DF25ull;
  P.key = splitmix(key);
  const double mab = a.par.m * b.par.m / (a.par.m + b.par.m);
  P.c0 = p.strength * (a.par.q * a.par.q) * (b.par.q * b.par.q) / (mab * mab);
  P.w = wa;
  P.dt = p.dt > 0.0 ? p.dt : c->g.dt;
  P.fa = mab / a.par.m;
  P.fb = mab / b.par.m;
  XPIC_CALL(sort_materialize(c, a)); // (a deferred re-binning whose assembly has not run)
  a.prebinned = false;               // (a pre-binning was made with the old velocities)
  if (inter) {
    XPIC_CALL(sort_materialize(c, b));
    b.prebinned = false;
  }
  Timed t(c, "cmd_collide");
  double res[kTally] = {0.0, 0.0, 0.0, 0.0, 0.0};
  if (a.n > 0 && b.n > 0) {
    long nb = (c->ncell + kWaves - 1) / kWaves;
    if (nb > kRedBlocks) nb = kRedBlocks;
    if (inter)
      hipLaunchKernelGGL(k_collide<true>, dim3((unsigned)nb), dim3(kBlock), 0, c->stream, c->g, a.d, b.d, P, (long)c->ncell, c->red_partial);
    else
      hipLaunchKernelGGL(k_collide<false>, dim3((unsigned)nb), dim3(kBlock), 0, c->stream, c->g, a.d, a.d, P, (long)c->ncell, c->red_partial);
    XPIC_HIP(hipGetLastError());
    XPIC_CALL(reduce_to_host(c, kTally, (int)nb, 1, false, res, kSumThreads));
  }
  c->collide_large_cells = (int64_t)res[4]; // (xpic_collide_info; this slab's)
  XPIC_CALL(comm_allreduce_sum_host(c, res, 4));
  for (int k = 0; k < 4; ++k) out4[k] = res[k];
  return 0;
}

}  // namespace xpic
