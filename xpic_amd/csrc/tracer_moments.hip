// tracer_moments.hip -- the moments of a tracer set (include/xpic_tracer_moments.h; an extension: the
// reference has neither sets nor their moments).  The records of a set are not cell-sorted and some are dead, so k_moment's
// tile per block of storage cells (moments.hip) does not apply: here one lane takes one record, through the set's live
// list where there is one.  What the two kernels share is moment_deposit.h: the per-particle values, the shape, the
// region and mom_target.  Two paths:
//   LDS     the region's cells x dof fit kTracerMomentLds doubles: every workgroup sums into a private copy of the region
//           in LDS (fp64 LDS atomics) and adds its non-zero entries to memory at the end.  A trapped ensemble sits in a
//           few cells; without the copy all its lanes would queue on a handful of addresses in memory.
//   direct  a larger region: unsafeAtomicAdd to memory, 8 x dof per counted particle, the 8 corners rotated over the
//           lanes so that neighbours in a wave start on different corners.
// A guiding-centre set takes b = B / |B| from fo_gather's magnetic half and fl_abs, the functions the field-line tracer
// samples B with (full_orbit_step.h, field_line_step.h).  The same kernel fills the scratch vectors of the one-shot call
// and a map's accumulator.  Every loop is bounded: a grid-stride loop over the m entries, 8 corners, dof <= 6.
#include <algorithm>
#include <string>
#include <vector>

#include "batch.h"
#include "common.h"
#include "device_common.h"
#include "ie_shape.h"
#include "tracer_set.h"

// the per-particle values and the shape without contraction: tests/tracer_moments_ref.py states the same operations, so
// what is left between the two is the order of the sums (moments.hip compiles the same text with the default setting)
#pragma clang fp contract(off)

#include "moment_deposit.h"

// the gather is compiled as in full_orbit.hip and field_lines.hip, contracted per source expression only
#pragma clang fp contract(on)

#include "full_orbit_step.h"

#include "field_line_step.h"

namespace xpic {

namespace {

constexpr int kBlock = kLaneBlock;

struct TMArgs {
  const double* s;       // the state [6][n]
  long n;
  const long long* ex;   // exit_step [n]
  const long long* list; // the entries to visit; null: 0 .. m - 1
  long m;
  const double* B;       // drift kinetic: the context's B
  MomRegion R;
  double q, mass, w;
  MomOut out;
  unsigned long long* counted;
};

// the values of a guiding centre {p_parallel, p_perp} whose field direction is b (the zero vector where |B| is 0): the
// gyro-average of moment_of over the phase.  The cylindrical kinds rotate b as v_cyl rotates v.  No contraction: the
// restatement (tests/tracer_moments_ref.py) writes the same operations.
template <int K>
__device__ inline void dk_moment_of(const GridDev& g, double q, double m, double x, double y, double ppar, double pperp,
  const double* b, double* o)
{
#pragma clang fp contract(off)
  if (K == XPIC_MOMENT_DENSITY) o[0] = 1.0;
  if (K == XPIC_MOMENT_CURRENT) {
    const double qp = q * ppar;
    o[0] = qp * b[0]; o[1] = qp * b[1]; o[2] = qp * b[2];
  }
  if (K >= XPIC_MOMENT_MOMENTUM_FLUX) {
    double c[3] = {b[0], b[1], b[2]};
    if (K == XPIC_MOMENT_MOMENTUM_FLUX_CYL || K == XPIC_MOMENT_MOMENTUM_FLUX_DIAG_CYL) v_cyl(x, y, g.Lx, g.Ly, b, c);
    const double par = m * (ppar * ppar), perp = m * (0.5 * (pperp * pperp));
    if (K == XPIC_MOMENT_MOMENTUM_FLUX || K == XPIC_MOMENT_MOMENTUM_FLUX_CYL) {
      int j = 0;
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int e = a; e < 3; ++e) {
          const double bb = c[a] * c[e];
          o[j++] = par * bb + perp * ((a == e ? 1.0 : 0.0) - bb);
        }
    } else {
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const double bb = c[a] * c[a];
        o[a] = par * bb + perp * (1.0 - bb);
      }
    }
  }
}

// b = B(r) / |B(r)| per component; |B| == 0: the zero vector
__device__ inline void dk_direction(const GridDev& g, const double* __restrict__ B, const double* r, double* b)
{
#pragma clang fp contract(off)
  double Bp[3];
  fo_gather<false>(g, nullptr, B, r, nullptr, Bp);
  const double f = fl_abs(Bp);
#pragma unroll
  for (int a = 0; a < 3; ++a) b[a] = f == 0.0 ? 0.0 : Bp[a] / f;
}

// Single z-slab contexts only (G == 0, z0 == 0): a stored node is (z ny + y) nx + x.  tile: [D][RZ][RY][RX], LDS only.
template <int K, bool DK, bool LDS>
__global__ void __launch_bounds__(kBlock) k_tracer_moment(GridDev g, TMArgs A)
{
  constexpr int D = MomDof<K>::v;
  extern __shared__ double tile[];
  const MomRegion& R = A.R;
  const int RX = R.e[0] - R.s[0], RY = R.e[1] - R.s[1], RZ = R.e[2] - R.s[2], TS = RX * RY * RZ;
  if (LDS) {
    for (int i = threadIdx.x; i < D * TS; i += kBlock) tile[i] = 0.0;
    __syncthreads();
  }
  const int lane = threadIdx.x & 63;
  const long n = A.n;
  int mine = 0;
  for (long j = (long)blockIdx.x * kBlock + threadIdx.x; j < A.m; j += (long)gridDim.x * kBlock) {
    const long p = A.list ? (long)A.list[j] : j;
    if (p < 0 || p >= n || A.ex[p] >= 0) continue;
    const double r[3] = {A.s[p], A.s[n + p], A.s[2 * n + p]};
    const double u[3] = {A.s[3 * n + p], A.s[4 * n + p], A.s[5 * n + p]};
    // the storage cell, open_keep's: floor of the scaled position as it is.  Compared as doubles: a position that is
    // not a number, or too far out for an int, fails
    double pn[3];
    if (g.pow2) scaled_position<true>(g, r[0], r[1], r[2], pn);
    else scaled_position<false>(g, r[0], r[1], r[2], pn);
    bool in = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double c = floor(pn[a]);
      in = in && c >= (double)R.s[a] && c < (double)R.e[a];
    }
    if (!in) continue;
    ++mine;
    double mv[D];
    if (DK) {
      double b[3];
      dk_direction(g, A.B, r, b);
      dk_moment_of<K>(g, A.q, A.mass, r[0], r[1], u[0], u[1], b, mv);
    } else {
      moment_of<K>(g, A.q, A.mass, r[0], r[1], u, mv);
    }
    int st[3];
    double w[3][2];
    mom_shape(g, r, st, w);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int kk = (k + lane) & 7;
      const double si = mom_weight(w, kk) * A.w;
      if (si == 0.0) continue;
      const long node = mom_target(g, R, st[0] + (kk & 1), st[1] + ((kk >> 1) & 1), st[2] + (kk >> 2));
      if (node < 0) continue;
      if (LDS) { // (the host takes this path only when a node index fits 32 bits)
        const unsigned nd = (unsigned)node, z = nd / (unsigned)g.plane, rem = nd - z * (unsigned)g.plane;
        const unsigned y = rem / (unsigned)g.nx, x = rem - y * (unsigned)g.nx;
        const int t = (((int)z - R.s[2]) * RY + ((int)y - R.s[1])) * RX + ((int)x - R.s[0]);
#pragma unroll
        for (int c = 0; c < D; ++c) atomicAdd(&tile[c * TS + t], mv[c] * si);
      } else {
#pragma unroll
        for (int c = 0; c < D; ++c) unsafeAtomicAdd(&A.out.c[c][node], mv[c] * si);
      }
    }
  }
  // one add per wave: every thread of the wave is here
  for (int o = 32; o > 0; o >>= 1) mine += __shfl_down(mine, o, 64);
  if (lane == 0 && mine) atomicAdd(A.counted, (unsigned long long)mine);
  if (!LDS) return;
  __syncthreads();
  for (int t = threadIdx.x; t < TS; t += kBlock) {
    const int x = R.s[0] + t % RX, y = R.s[1] + (t / RX) % RY, z = R.s[2] + t / (RX * RY);
    const long node = g.node(x, y, z);
#pragma unroll
    for (int c = 0; c < D; ++c) {
      const double val = tile[c * TS + t];
      if (val != 0.0) unsafeAtomicAdd(&A.out.c[c][node], val);
    }
  }
}

template <int K, bool DK, bool LDS>
int launch_one(xpic_ctx* c, const TMArgs& A, size_t lds, unsigned blocks)
{
  // more than the default 64 KiB of dynamic LDS for a large region; set on every launch, as moments.hip does
  if (LDS) XPIC_HIP(hipFuncSetAttribute((const void*)k_tracer_moment<K, DK, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  Timed t(c, LDS ? "tracer_moment_lds" : "tracer_moment");
  hipLaunchKernelGGL((k_tracer_moment<K, DK, LDS>), dim3(blocks), dim3(kBlock), LDS ? lds : 0, c->stream, c->g, A);
  XPIC_HIP(hipGetLastError());
  return 0;
}

template <int K>
int launch_kind(xpic_ctx* c, bool dk, bool lds, const TMArgs& A, size_t bytes, unsigned blocks)
{
  if (dk) return lds ? launch_one<K, true, true>(c, A, bytes, blocks) : launch_one<K, true, false>(c, A, bytes, blocks);
  return lds ? launch_one<K, false, true>(c, A, bytes, blocks) : launch_one<K, false, false>(c, A, bytes, blocks);
}

// what a deposit is made with
struct MomentSpec {
  int kind;
  double q, m, weight;
  const int* region6; // or null
};

int check_spec(const GridDev& g, const std::string& who, const MomentSpec& S, MomRegion* R)
{
  XPIC_CHECK(moment_dof(S.kind) > 0, who + ": unknown moment kind");
  XPIC_CHECK(mom_region_of(g, S.region6, R), who + ": region: start >= 0, size > 0, start + size <= n");
  return 0;
}

// the moment S of the set as it stands, ADDED into out (component c: out.c[c][node]) and *counted
int deposit(xpic_ctx* c, TracerSet& T, const MomentSpec& S, const MomOut& out, unsigned long long* counted)
{
  const GridDev& g = c->g;
  TMArgs A{};
  XPIC_CALL(check_spec(g, "tracer moment", S, &A.R));
  A.m = (long)(T.L.list ? T.L.listed : T.n);
  if (T.n == 0 || A.m == 0) return 0;
  A.s = T.s.p; A.n = (long)T.n; A.ex = (const long long*)T.ex.p; A.list = (const long long*)T.L.list;
  A.B = c->field[XPIC_B];
  A.q = S.q; A.mass = S.m; A.w = S.weight;
  A.out = out;
  A.counted = counted;
  const int D = moment_dof(S.kind);
  const long cells = (long)(A.R.e[0] - A.R.s[0]) * (A.R.e[1] - A.R.s[1]) * (A.R.e[2] - A.R.s[2]);
  const bool lds = cells * D <= (long)c->tracer_moment_lds && g.cstride < (1L << 31);
  const size_t bytes = sizeof(double) * D * cells;
  // the LDS path pays a zeroing and a flush of the region per workgroup: two workgroups per CU, each striding over the
  // entries; the direct path has nothing per workgroup to amortise
  const long want = (A.m + kBlock - 1) / kBlock;
  const unsigned blocks = (unsigned)std::min<long>(want, (lds ? 2L : 16L) * c->num_cus);
  const bool dk = T.kind == XPIC_TRACERS_DRIFT_KINETIC;
  switch (S.kind) {
    case XPIC_MOMENT_DENSITY: return launch_kind<XPIC_MOMENT_DENSITY>(c, dk, lds, A, bytes, blocks);
    case XPIC_MOMENT_CURRENT: return launch_kind<XPIC_MOMENT_CURRENT>(c, dk, lds, A, bytes, blocks);
    case XPIC_MOMENT_MOMENTUM_FLUX: return launch_kind<XPIC_MOMENT_MOMENTUM_FLUX>(c, dk, lds, A, bytes, blocks);
    case XPIC_MOMENT_MOMENTUM_FLUX_DIAG: return launch_kind<XPIC_MOMENT_MOMENTUM_FLUX_DIAG>(c, dk, lds, A, bytes, blocks);
    case XPIC_MOMENT_MOMENTUM_FLUX_CYL: return launch_kind<XPIC_MOMENT_MOMENTUM_FLUX_CYL>(c, dk, lds, A, bytes, blocks);
    default: return launch_kind<XPIC_MOMENT_MOMENTUM_FLUX_DIAG_CYL>(c, dk, lds, A, bytes, blocks);
  }
}

// D components of nown doubles each on the device -> out[node][D] on the host (one synchronisation)
int export_dof_last(xpic_ctx* c, const MomOut& o, int D, double* out)
{
  const long nown = c->g.nown;
  std::vector<double> h((size_t)D * nown);
  for (int j = 0; j < D; ++j)
    XPIC_HIP(hipMemcpyAsync(h.data() + (size_t)j * nown, o.c[j], sizeof(double) * nown, hipMemcpyDeviceToHost, c->stream));
  XPIC_HIP(hipStreamSynchronize(c->stream));
  for (long i = 0; i < nown; ++i)
    for (int j = 0; j < D; ++j) out[(size_t)i * D + j] = h[(size_t)j * nown + i];
  return 0;
}

// the checks every entry point makes first
int entry(xpic_ctx* ctx, const std::string& who, int set, TracerSet** T)
{
  XPIC_CHECK(ctx != nullptr, "null context");
  XPIC_CHECK(ctx->geom.nranks == 1 && ctx->g.G == 0,
    who + ": a context of several z-slabs (or a self_ring one) is not supported: the deposit wraps z in the kernel");
  return tracers_find(ctx, who, set, T);
}

int find_map(TracerSet& T, const std::string& who, int map, TracerMap** out)
{
  for (auto& m : T.maps)
    if (m->id == map) { *out = m.get(); return 0; }
  XPIC_CHECK(false, who + ": map " + std::to_string(map) + " of set " + std::to_string(T.id) +
    " does not exist (never created, or destroyed)");
  return 0;
}

MomOut map_out(const xpic_ctx* c, TracerMap& M)
{
  MomOut o{};
  for (int j = 0; j < M.dof; ++j) o.c[j] = M.acc.p + (size_t)j * c->g.nown;
  return o;
}

}  // namespace

int tracer_maps_deposit(xpic_ctx* ctx, TracerSet& T)
{
  for (auto& m : T.maps) {
    if (T.done % m->every != 0) continue;
    const MomentSpec S{m->kind, m->q, m->m, m->weight, m->whole ? nullptr : m->region6};
    XPIC_CALL(deposit(ctx, T, S, map_out(ctx, *m), m->count.p));
    m->deposits += 1;
  }
  return 0;
}

}  // namespace xpic

using namespace xpic;

extern "C" {

int xpic_tracers_moment(xpic_ctx* ctx, int set, int kind, double q, double m, double weight, const int region6[6], double* out,
  int64_t* counted)
{
  const std::string who = "tracers_moment";
  TracerSet* T = nullptr;
  XPIC_CALL(entry(ctx, who, set, &T));
  const MomentSpec S{kind, q, m, weight, region6};
  MomRegion R{};
  XPIC_CALL(check_spec(ctx->g, who, S, &R));
  XPIC_CHECK(out, who + ": out is null");
  const int D = moment_dof(kind);
  // the scratch vectors of xpic_moment: XPIC_W2, and XPIC_W1 as well for six components; zeroed whole
  MomOut o{};
  for (int j = 0; j < D; ++j) o.c[j] = ctx->field[D > 3 ? XPIC_W1 + j / 3 : XPIC_W2] + (long)(j % 3) * ctx->g.cstride;
  for (int v = 0; v < (D + 2) / 3; ++v) XPIC_HIP(hipMemsetAsync(o.c[3 * v], 0, sizeof(double) * ctx->nvec, ctx->stream));
  DevScratch<unsigned long long> cnt;
  XPIC_CALL(cnt.alloc(1));
  XPIC_CALL(zero(cnt, 1, ctx->stream));
  XPIC_CALL(deposit(ctx, *T, S, o, cnt.p));
  unsigned long long h = 0;
  XPIC_CALL(download(&h, cnt, 1, ctx->stream));
  XPIC_CALL(export_dof_last(ctx, o, D, out));
  if (counted) *counted = (int64_t)h;
  return 0;
}

int xpic_tracers_map_create(xpic_ctx* ctx, int set, int kind, double q, double m, double weight, const int region6[6],
  int64_t every, int* map)
{
  const std::string who = "tracers_map_create";
  TracerSet* T = nullptr;
  XPIC_CALL(entry(ctx, who, set, &T));
  const MomentSpec S{kind, q, m, weight, region6};
  MomRegion R{};
  XPIC_CALL(check_spec(ctx->g, who, S, &R));
  XPIC_CHECK(every >= 1, who + ": every must be >= 1");
  XPIC_CHECK(map, who + ": map is null");
  XPIC_CHECK((int)T->maps.size() < XPIC_TRACERS_MAX_MAPS,
    who + ": the set already has " + std::to_string(XPIC_TRACERS_MAX_MAPS) + " maps");
  auto M = std::make_unique<TracerMap>();
  M->kind = kind; M->dof = moment_dof(kind);
  M->q = q; M->m = m; M->weight = weight;
  M->whole = region6 == nullptr;
  if (region6) std::copy(region6, region6 + 6, M->region6);
  M->every = every;
  const size_t len = (size_t)M->dof * ctx->g.nown;
  XPIC_CALL(M->acc.alloc(len)); XPIC_CALL(M->count.alloc(1));
  XPIC_CALL(zero(M->acc, len, ctx->stream)); XPIC_CALL(zero(M->count, 1, ctx->stream));
  *map = M->id = T->next_map++;
  T->maps.push_back(std::move(M));
  return 0;
}

int xpic_tracers_map_get(xpic_ctx* ctx, int set, int map, double* out, int64_t info3[3], int reset)
{
  const std::string who = "tracers_map_get";
  TracerSet* T = nullptr;
  TracerMap* M = nullptr;
  XPIC_CALL(entry(ctx, who, set, &T));
  XPIC_CALL(find_map(*T, who, map, &M));
  unsigned long long h = 0;
  XPIC_CALL(download(&h, M->count, 1, ctx->stream));
  if (out) XPIC_CALL(export_dof_last(ctx, map_out(ctx, *M), M->dof, out));
  else XPIC_HIP(hipStreamSynchronize(ctx->stream));
  if (info3) { info3[0] = M->deposits; info3[1] = (int64_t)h; info3[2] = T->done; }
  if (reset) {
    XPIC_CALL(zero(M->acc, (size_t)M->dof * ctx->g.nown, ctx->stream));
    XPIC_CALL(zero(M->count, 1, ctx->stream));
    M->deposits = 0;
  }
  return 0;
}

int xpic_tracers_map_destroy(xpic_ctx* ctx, int set, int map)
{
  const std::string who = "tracers_map_destroy";
  TracerSet* T = nullptr;
  TracerMap* M = nullptr;
  XPIC_CALL(entry(ctx, who, set, &T));
  XPIC_CALL(find_map(*T, who, map, &M));
  XPIC_HIP(hipStreamSynchronize(ctx->stream));
  T->maps.erase(std::find_if(T->maps.begin(), T->maps.end(), [&](const std::unique_ptr<TracerMap>& m) { return m.get() == M; }));
  return 0;
}

}  // extern "C"
