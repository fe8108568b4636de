// collide.hip -- binary Coulomb collisions between the records of one cell, non-relativistic: Takizuka and Abe (J. Comput.
// Phys. 25, 205, 1977) inside one sort and between two sorts of equal weight n / Np, Nanbu and Yonemura
// (J. Comput. Phys. 145, 639, 1998; the density factor for repeated meetings after Higginson et al., J. Comput. Phys. 413,
// 109450, 2020) between two sorts of unequal weight.  AN EXTENSION: the reference has no collision operator;
// include/xpic_hip.h (xpic_collide, xpic_collide_weighted) is the definition, tests/collisions_ref.py and
// tests/collisions_weighted_ref.py state it a second time in numpy float64.
//
// One wave per cell, kWaves cells per workgroup.  The lanes form the 64-bit keys of the cell's records (record i, in cell
// order) into LDS; a record's rank is the number of (key, i) below its own -- a count over the staged keys, quadratic in the
// cell's population, which is tens -- and slot[rank] = i is the permutation.  Each lane then takes pairs: a record is read
// and written by exactly one lane, so there is no atomic on a velocity.  The odd cell's triple and the meetings of one
// record of the short side are serial by definition and stay in one lane.  Cells of more than XPIC_COLLIDE_LDS_CELL records
// of a sort take the same body with the keys recomputed where they are compared and the slots in the sort's rank[] array
// (binning scratch: the callers drop the pre-binning anyway, its keys describe the old velocities).
//
// The weighted pairing is the inter-species one with the density factor w_max N_short, a fourth draw u4 from the pair's
// stream, and the selection: the lighter-weighted record always takes its new velocity, the heavier-weighted one iff
// u4 < r = w_min / w_max.  There collide_pair runs on register copies; a rejected long-side record is not stored at all, a
// rejected short-side record keeps the value its lane holds.
//
// Compiled without floating-point contraction: the collision is rounded operation by operation, as numpy rounds it.  The
// collision itself and the streams are collide_pair.h's, shared with collide_trace.hip.
#include <cmath>
#include <string>

#include "common.h"
#include "device_common.h"
#include "collide_pair.h"

#pragma clang fp contract(off)

namespace xpic {

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kSumThreads = 64; // second stage of the reduction: one wave (as commands.hip)
constexpr int kLds = XPIC_COLLIDE_LDS_CELL;

enum class Pairing { Intra, Inter, Weighted }; // one sort; two sorts of equal weight; two sorts, the selection by weight

// tally rows: out4 (Weighted: out6), then the cells that took the second path (xpic_collide_info)
constexpr int tally_rows(Pairing M) { return M == Pairing::Weighted ? 7 : 5; }

// The kernel's last argument, behind ncell and partial.  Only Weighted reads r and a_heavy, and they come last: what Intra
// and Inter read (ncell, partial, key ... fb) is then 64 contiguous bytes that one scalar load fetches; with the two
// members in between, or the struct ahead of ncell, that load splits and the scalar registers are allotted worse
// (measured)
struct ColDev {
  uint64_t key;  // stream of (seed, step, sort_a, sort_b)
  double c0;     // S q_a^2 q_b^2 / m_ab^2
  double w;      // n / Np of both sorts; Weighted: the larger of the two
  double dt;
  double fa, fb; // m_ab / m_a, m_ab / m_b
  double r;      // w_min / w_max, formed on the host
  int a_heavy;   // the heavier-weighted sort is the call's a (equal weights: b, and r == 1 updates both)
};

constexpr int kTagPermA = 0, kTagPermB = 1, kTagPairs = 2; // the sub-streams of a cell (collide_pair.h: sub_key)

// what one lane wrote is read by the other lanes of its wave: LDS operations of a wave complete in order, the fence keeps
// the compiler from moving them; the second path's slots go through global memory
template <bool LDS>
__device__ inline void wave_sync()
{
  if (LDS) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
  else __threadfence();
}

// slot[rank of record i] = i for the n records of a cell, ordered by (key, i)
template <bool LDS>
__device__ inline void permute(uint64_t sub, int n, uint64_t* keys, int* slot, int lane)
{
  if (LDS) {
    for (int i = lane; i < n; i += 64) keys[i] = item_key(sub, i);
    wave_sync<LDS>();
  }
  for (int i = lane; i < n; i += 64) {
    const uint64_t ki = LDS ? keys[i] : item_key(sub, i);
    int r = 0;
    for (int j = 0; j < n; ++j) {
      const uint64_t kj = LDS ? keys[j] : item_key(sub, j);
      r += (kj < ki || (kj == ki && j < i)) ? 1 : 0;
    }
    slot[r] = i;
  }
  wave_sync<LDS>(); // (the slots are read, and the keys rewritten, by other lanes)
}

// one collision of pair p of the cell's pair stream (collide_pair.h); cdt = c0 n_L dt of this pair
__device__ inline void collide_pair(const ColDev& P, double cdt, uint64_t pairs, int p, double* va, double* vb, double* t)
{
  collide_pair(P.fa, P.fb, cdt, item_state(pairs, p), va, vb, t);
}

__device__ inline void load_v(const SortDev& s, int i, double* v) { v[0] = s.v[0][i]; v[1] = s.v[1][i]; v[2] = s.v[2][i]; }
__device__ inline void store_v(const SortDev& s, int i, const double* v) { s.v[0][i] = v[0]; s.v[1][i] = v[1]; s.v[2][i] = v[2]; }

// u4 of a pair: the draw after collide_pair's u1 u2 u3 from the same stream state
__device__ inline double fourth_draw(uint64_t st)
{
  (void)splitmix(st);
  (void)splitmix(st);
  (void)splitmix(st);
  return u01(st);
}

// the pairs of one cell; ba, bb: first record of the cell in A, B; sa, sb: the permutations (two sorts: of both)
template <Pairing M>
__device__ inline void cell_pairs(const ColDev& P, const SortDev& A, const SortDev& B, uint64_t ck, int ba, int na, int bb,
  int nb, const int* sa, const int* sb, int lane, double* t)
{
  const uint64_t pairs = sub_key(ck, kTagPairs);
  if constexpr (M == Pairing::Intra) {
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
        if constexpr (M == Pairing::Inter) {
          if (swap) collide_pair(P, cd, pairs, j, vs, vl, t);
          else collide_pair(P, cd, pairs, j, vl, vs, t);
          store_v(swap ? B : A, il, vl);
        }
        else {
          double xs[3] = {vs[0], vs[1], vs[2]}, xl[3] = {vl[0], vl[1], vl[2]};
          const uint64_t st = item_state(pairs, j);
          const double made = t[0];
          if (swap) collide_pair(P.fa, P.fb, cd, st, xs, xl, t);
          else collide_pair(P.fa, P.fb, cd, st, xl, xs, t);
          if (t[0] == made) continue; // (|u| == 0: skipped and counted, nothing drawn, nothing stored)
          const bool heavy_short = swap == (P.a_heavy != 0);
          const bool keep = fourth_draw(st) < P.r;
          t[4] += keep ? 1.0 : 0.0;
          t[5] += keep ? 0.0 : 1.0;
          const bool ks = keep || !heavy_short; // the short-side record takes its new velocity
          vs[0] = ks ? xs[0] : vs[0];
          vs[1] = ks ? xs[1] : vs[1];
          vs[2] = ks ? xs[2] : vs[2];
          if (keep || heavy_short) store_v(swap ? B : A, il, xl); // (a rejected long-side record is not stored)
        }
      }
      store_v(swap ? A : B, is, vs);
    }
  }
}

template <Pairing M, bool LDS>
__device__ inline void cell_body(const ColDev& P, const SortDev& A, const SortDev& B, uint64_t ck, int ba, int na, int bb, int nb,
  uint64_t* keys, int* sa, int* sb, int lane, double* t)
{
  permute<LDS>(sub_key(ck, kTagPermA), na, keys, sa, lane);
  if (M != Pairing::Intra) permute<LDS>(sub_key(ck, kTagPermB), nb, keys, sb, lane);
  cell_pairs<M>(P, A, B, ck, ba, na, bb, nb, sa, sb, lane, t);
}

// partial rows: tally_rows(M)
template <Pairing M>
__global__ void __launch_bounds__(kBlock) k_collide(GridDev g, SortDev A, SortDev B, long ncell, double* partial, ColDev P)
{
  constexpr bool kTwo = M != Pairing::Intra;
  constexpr int kTally = tally_rows(M);
  __shared__ uint64_t keys[kWaves][kLds];
  __shared__ int slot[kWaves][2][kLds];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long nw = (long)gridDim.x * kWaves;
  double t[kTally] = {};
  for (long c = (long)blockIdx.x * kWaves + wave; c < ncell; c += nw) {
    const int ba = A.cell_start[c], na = A.cell_start[c + 1] - ba;
    const int bb = kTwo ? B.cell_start[c] : ba, nb = kTwo ? B.cell_start[c + 1] - bb : na;
    if (kTwo ? (na == 0 || nb == 0) : na < 2) continue;
    const int x = (int)(c % g.nx), y = (int)((c / g.nx) % g.ny), zl = (int)(c / g.plane);
    const uint64_t ck = cell_key(P.key, ((long)(g.z0 + zl) * g.ny + y) * g.nx + x);
    if (na <= kLds && nb <= kLds) cell_body<M, true>(P, A, B, ck, ba, na, bb, nb, keys[wave], slot[wave][0], slot[wave][1], lane, t);
    else {
      cell_body<M, false>(P, A, B, ck, ba, na, bb, nb, nullptr, A.rank + ba, B.rank + bb, lane, t);
      if (lane == 0) t[kTally - 1] += 1.0;
    }
  }
  block_reduce_store<kTally, kBlock>(t, partial, gridDim.x, blockIdx.x);
}

}  // namespace

// xpic_collide (weighted false, out: 4 counters) and xpic_collide_weighted (true, 6 counters)
int collide(xpic_ctx* c, int ia, int ib, const xpic_collision_params& p, int64_t step, bool weighted, double* out)
{
  Sort& a = c->sorts[ia];
  Sort& b = c->sorts[ib];
  const bool inter = ia != ib;
  const auto msg = [weighted](const char* text) { return std::string(weighted ? "collide_weighted: " : "collide: ") + text; };
  XPIC_CHECK(std::isfinite(p.strength) && p.strength >= 0.0, msg("the strength must be finite and not negative"));
  XPIC_CHECK(a.par.m > 0.0 && b.par.m > 0.0 && a.par.Np > 0 && b.par.Np > 0, msg("a sort without mass or Np"));
  const double wa = a.par.n / a.par.Np, wb = b.par.n / b.par.Np;
  if (weighted)
    XPIC_CHECK(std::isfinite(wa) && std::isfinite(wb) && wa > 0.0 && wb > 0.0,
      msg("both sorts need a finite, positive weight n / Np"));
  else
    XPIC_CHECK(wa == wb, msg("the two sorts must carry the same weight n / Np (Takizuka-Abe pairs equal-weight particles)"));
  for (int k = 0; k < (weighted ? 6 : 4); ++k) out[k] = 0.0;
  if (p.strength == 0.0) return 0; // (nothing is launched, nothing changes)
  // the selection runs between two sorts only: one sort has one weight and takes xpic_collide's path, bits and label
  const bool select = weighted && inter;
  const int counters = select ? 6 : 4;
  ColDev P{};
  P.key = call_key(p.seed, step, ia, ib);
  const double mab = a.par.m * b.par.m / (a.par.m + b.par.m);
  P.c0 = p.strength * (a.par.q * a.par.q) * (b.par.q * b.par.q) / (mab * mab);
  P.w = wb > wa ? wb : wa; // (equal weights: wa, the common one)
  P.r = (wb > wa ? wa : wb) / P.w;
  P.a_heavy = wa > wb ? 1 : 0;
  P.dt = p.dt > 0.0 ? p.dt : c->g.dt;
  P.fa = mab / a.par.m;
  P.fb = mab / b.par.m;
  XPIC_CALL(sort_materialize(c, a)); // (a deferred re-binning whose assembly has not run)
  a.prebinned = false;               // (a pre-binning was made with the old velocities)
  if (inter) {
    XPIC_CALL(sort_materialize(c, b));
    b.prebinned = false;
  }
  Timed t(c, select ? "cmd_collide_weighted" : "cmd_collide");
  double res[tally_rows(Pairing::Weighted)] = {};
  if (a.n > 0 && b.n > 0) {
    long nb = (c->ncell + kWaves - 1) / kWaves;
    if (nb > kRedBlocks) nb = kRedBlocks;
    // (equal weights through xpic_collide stay on Inter: the same bits as Weighted at r == 1, and faster)
    const auto kernel = select ? k_collide<Pairing::Weighted> : inter ? k_collide<Pairing::Inter> : k_collide<Pairing::Intra>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)nb), dim3(kBlock), 0, c->stream, c->g, a.d, b.d, (long)c->ncell, c->red_partial, P);
    XPIC_HIP(hipGetLastError());
    XPIC_CALL(reduce_to_host(c, counters + 1, (int)nb, 1, false, res, kSumThreads));
  }
  c->collide_large_cells = (int64_t)res[counters]; // (xpic_collide_info; this slab's)
  XPIC_CALL(comm_allreduce_sum_host(c, res, counters));
  for (int k = 0; k < counters; ++k) out[k] = res[k];
  if (weighted && !inter) out[4] = out[0]; // (both records of every pair are updated)
  return 0;
}

}  // namespace xpic
