// field_lines.hip -- field lines of a grid vector or of an analytic model (include/xpic_field_lines.h; an
// extension: the reference has no field-line tracer).  One lane follows one line from one seed in one direction: fp64,
// no LDS, no cross-lane operation but the ballot that counts the lanes a launch finished.  The step, its accumulators and
// its stop rules are field_line_step.h's; the grid source is fo_gather (full_orbit_step.h), the analytic one ModelSource
// (model_source.h), the region rule open_keep (trace_open.h), the staging batch.h's.  The lanes' state lives in
// structure-of-arrays device buffers over 2 n slots (slot = direction * n + seed), so a wave's loads and stores are
// coalesced; a launch covers the lanes of the directions asked for.  Positions are not folded into the box: the gather
// wraps its node indices.  Every loop is bounded: 4 stages of at most 4 x 4 x 4 nodes, at most launch_steps steps per
// launch (checked on the host), at most max_steps / launch_steps (rounded up) launches.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "batch.h"
#include "common.h"
#include "device_common.h"
#include "ie_shape.h"
#include "trace_open.h"

// the gather is compiled as in full_orbit.hip, contracted per source expression only, so that it rounds here as it does
// for the tracers; field_line_step.h switches contraction off inside its own functions
#pragma clang fp contract(on)

#include "full_orbit_step.h"
#include "model_source.h"

#include "field_line_step.h"

namespace xpic {

namespace {

constexpr int kBlock = kLaneBlock;      // batch.h: lane_grid launches workgroups of this size
constexpr int kMaxLaunchSteps = 1 << 16; // the longest launch a caller may ask for
constexpr int kStateRows = 8;           // r[3], length, volume, fmin, smin, fmax

// the grid vector F with the magnetic (ELECTRIC = false) or the electric products of fo_gather
template <bool ELECTRIC>
struct FLGrid {
  GridDev g;
  const double* __restrict__ F;
  __device__ inline void at(const double* r, double* out) const
  {
    if (ELECTRIC) {
      double Bp[3];
      fo_gather<true>(g, F, F, r, out, Bp);
    }
    else {
      fo_gather<false>(g, nullptr, F, r, nullptr, out);
    }
  }
};

// B or E of an analytic model
struct FLModel {
  xpic_field_model m;
  int electric;
  __device__ inline void at(const double* r, double* out) const
  {
    double Ep[3], Bp[3];
    ModelSource{m}.at(r, Ep, Bp);
#pragma unroll
    for (int c = 0; c < 3; ++c) out[c] = electric ? Ep[c] : Bp[c];
  }
};

// what one launch gets beside its source
struct FLLaunch {
  OpenRegion R;
  double h, f_floor, close_tol;
  long long max_steps;
  long n;            // seeds; the state has 2 n slots
  int directions;    // 1, 2 or 3
  int ns;            // steps of this launch
  long every, nsamp; // a sample row after every every-th step; rows of samples
  const double* seeds;          // [3][n]
  double* st;                   // [kStateRows][2 n]
  long long* steps;             // [2 n]
  int* code;                    // [2 n]
  double* samples;              // [nsamp][3][2 n], or null
  unsigned long long* finished; // the lanes that have a code, summed over the launches
};

template <class SRC>
__global__ void __launch_bounds__(kBlock) k_field_lines(GridDev g, SRC src, FLLaunch A)
{
  const long j = (long)blockIdx.x * kBlock + threadIdx.x;
  const long n = A.n, W = 2 * n;
  const long lanes = A.directions == 3 ? W : n;
  bool fin = false;
  if (j < lanes) {
    const long slot = A.directions == 2 ? n + j : j; // direction major: slots n .. 2 n - 1 follow -F
    const long q = slot < n ? slot : slot - n;
    if (A.code[slot] < 0) {
      FLState L;
#pragma unroll
      for (int c = 0; c < 3; ++c) L.r[c] = A.st[c * W + slot];
      L.length = A.st[3 * W + slot]; L.volume = A.st[4 * W + slot];
      L.fmin = A.st[5 * W + slot]; L.smin = A.st[6 * W + slot]; L.fmax = A.st[7 * W + slot];
      L.steps = A.steps[slot];
      const double seed[3] = {A.seeds[q], A.seeds[n + q], A.seeds[2 * n + q]};
      const int code = fl_advance(src,
        [&](const double* r) { return open_keep(g, A.R, r); },
        [&](const FLState& S) {
          if (A.samples && S.steps % A.every == 0) {
            const long row = (long)(S.steps / A.every) - 1;
            if (row < A.nsamp) {
#pragma unroll
              for (int c = 0; c < 3; ++c) A.samples[(row * 3 + c) * W + slot] = S.r[c];
            }
          }
        },
        slot < n ? 1.0 : -1.0, A.h, A.f_floor, A.close_tol, A.max_steps, A.ns, seed, L);
#pragma unroll
      for (int c = 0; c < 3; ++c) A.st[c * W + slot] = L.r[c];
      A.st[3 * W + slot] = L.length; A.st[4 * W + slot] = L.volume;
      A.st[5 * W + slot] = L.fmin; A.st[6 * W + slot] = L.smin; A.st[7 * W + slot] = L.fmax;
      A.steps[slot] = L.steps;
      A.code[slot] = code;
      fin = code >= 0;
    }
  }
  const int cnt = __popcll(__ballot(fin)); // every thread of the wave is here
  if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(A.finished, (unsigned long long)cnt);
}

// what both entry points were given beside their field
struct LineCall {
  std::string who;
  int64_t n;
  const double* seeds3;
  const xpic_line_params* P;
  const xpic_trace_region* region;
  int64_t every;
  double *end3, *length, *volume, *fmin, *smin, *fmax;
  int64_t* steps;
  int32_t* code;
  double* samples;
};

// the checks of a call; *go: there is something to do (n > 0)
int lines_check(const LineCall& c, const char* component_name, int component, OpenRegion* R, bool* go)
{
  const std::string& who = c.who;
  const xpic_line_params* P = c.P;
  *go = false;
  XPIC_CHECK(c.n >= 0 && c.n <= ((int64_t)1 << 35), who + ": n is negative or larger than 2^35");
  XPIC_CHECK(P, who + ": params is null");
  XPIC_CHECK(P->h > 0.0 && std::isfinite(P->h), who + ": h must be positive and finite");
  XPIC_CHECK(P->max_steps >= 1 && P->max_steps <= XPIC_LINES_MAX_STEPS, who + ": max_steps must be within 1 .. 2^24");
  XPIC_CHECK(P->f_floor >= 0.0, who + ": f_floor is negative or not a number");
  XPIC_CHECK(P->close_tol >= 0.0, who + ": close_tol is negative or not a number");
  XPIC_CHECK(component == XPIC_STAGGER_B || component == XPIC_STAGGER_E,
    who + ": " + component_name + " must be XPIC_STAGGER_B (0) or XPIC_STAGGER_E (1)");
  XPIC_CHECK(P->directions >= 1 && P->directions <= 3, who + ": directions must be 1 (+), 2 (-) or 3 (both)");
  XPIC_CHECK(P->launch_steps >= 0 && P->launch_steps <= kMaxLaunchSteps, who + ": launch_steps must be within 0 .. 65536");
  XPIC_CHECK(c.every >= 0, who + ": sample_every is negative");
  XPIC_CHECK((c.samples != nullptr) == (c.every > 0) || c.n == 0, who + ": samples and sample_every go together");
  if (c.region) XPIC_CALL(trace_region(who, c.region, false, true, R));
  else {
    const double inf = std::numeric_limits<double>::infinity(); // a box every finite position passes
    *R = OpenRegion{XPIC_GEOM_BOX, {-inf, -inf, -inf, inf, inf, inf, 0.0}, 0};
  }
  if (c.n == 0) return 0;
  XPIC_CHECK(c.seeds3, who + ": seeds3 is null");
  XPIC_CHECK(c.end3 && c.length && c.volume && c.fmin && c.smin && c.fmax && c.steps && c.code, who + ": a null output array");
  int64_t nsamp;
  XPIC_CHECK(trace_sample_bytes(c.n, P->max_steps, std::max<int64_t>(c.every, 1), c.samples != nullptr, &nsamp) >= 0,
    who + ": the sample buffer (48 n max_steps / sample_every bytes) is too large");
  *go = true;
  return 0;
}

// the lanes of one call: staged, launched until every lane has a code, copied back
template <class SRC>
int lines_run(xpic_ctx* ctx, const LineCall& c, const OpenRegion& R, const SRC& src)
{
  const xpic_line_params& P = *c.P;
  const int64_t n = c.n, W = 2 * n;
  const int first = P.directions == 2 ? 1 : 0, last = P.directions == 1 ? 0 : 1; // the directions asked for
  const int64_t lanes = (last - first + 1) * n;
  const int64_t nsamp = c.samples ? P.max_steps / c.every : 0;
  const int ls = P.launch_steps > 0 ? P.launch_steps : XPIC_LINES_LAUNCH_STEPS;
  std::vector<double> hseed, hst((size_t)kStateRows * W, 0.0), hsm;
  to_soa(c.seeds3, n, hseed, 3);
  for (int dir = 0; dir < 2; ++dir)
    for (int a = 0; a < 3; ++a) std::copy(hseed.begin() + a * n, hseed.begin() + (a + 1) * n, hst.begin() + a * W + dir * n);
  std::fill(hst.begin() + 5 * W, hst.begin() + 6 * W, std::numeric_limits<double>::infinity()); // fmin
  const std::vector<int> running(W, XPIC_LINE_RUNNING);
  DevScratch<double> seeds, st, sm;
  DevScratch<int64_t> steps, fin;
  DevScratch<int> code;
  XPIC_CALL(seeds.alloc(3 * n)); XPIC_CALL(st.alloc(hst.size())); XPIC_CALL(steps.alloc(W)); XPIC_CALL(code.alloc(W));
  XPIC_CALL(fin.alloc(1));
  if (nsamp > 0) XPIC_CALL(sm.alloc((size_t)3 * W * nsamp));
  XPIC_CALL(upload(seeds, hseed.data(), 3 * n, ctx->stream));
  XPIC_CALL(upload(st, hst.data(), hst.size(), ctx->stream));
  XPIC_CALL(upload(code, running.data(), W, ctx->stream));
  XPIC_CALL(zero(steps, W, ctx->stream));
  XPIC_CALL(zero(fin, 1, ctx->stream));
  FLLaunch A{R, P.h, P.f_floor, P.close_tol, (long long)P.max_steps, (long)n, P.directions, ls, (long)std::max<int64_t>(c.every, 1),
    (long)nsamp, seeds.p, st.p, (long long*)steps.p, code.p, sm.p, (unsigned long long*)fin.p};
  const int64_t launches = (P.max_steps + ls - 1) / ls; // after which every lane has taken max_steps steps, if nothing else
  int64_t finished = 0;
  for (int64_t l = 0; l < launches && finished < lanes; ++l) {
    {
      Timed t(ctx, "field_lines");
      hipLaunchKernelGGL(k_field_lines<SRC>, lane_grid(lanes), dim3(kBlock), 0, ctx->stream, ctx->g, src, A);
      XPIC_HIP(hipGetLastError());
    }
    XPIC_CALL(download(&finished, fin, 1, ctx->stream)); // the one read-back between launches
    XPIC_HIP(hipStreamSynchronize(ctx->stream));
  }
  XPIC_CHECK(finished == lanes, c.who + ": internal error: lanes without a code after the last launch");
  std::vector<int64_t> hsteps(W);
  std::vector<int> hcode(W);
  XPIC_CALL(download(hst.data(), st, hst.size(), ctx->stream));
  XPIC_CALL(download(hsteps.data(), steps, W, ctx->stream));
  XPIC_CALL(download(hcode.data(), code, W, ctx->stream));
  if (nsamp > 0) {
    hsm.resize((size_t)3 * W * nsamp);
    XPIC_CALL(download(hsm.data(), sm, hsm.size(), ctx->stream));
  }
  XPIC_HIP(hipStreamSynchronize(ctx->stream));
  double* const rows[5] = {c.length, c.volume, c.fmin, c.smin, c.fmax};
  for (int64_t slot = first * n; slot < (last + 1) * n; ++slot) {
    for (int a = 0; a < 3; ++a) c.end3[3 * slot + a] = hst[a * W + slot];
    for (int k = 0; k < 5; ++k) rows[k][slot] = hst[(3 + k) * W + slot];
    c.steps[slot] = hsteps[slot];
    c.code[slot] = hcode[slot];
    const int64_t held = nsamp > 0 ? std::min(hsteps[slot] / c.every, nsamp) : 0; // the rows the lane wrote
    for (int64_t k = 0; k < nsamp; ++k)
      for (int a = 0; a < 3; ++a)
        c.samples[((size_t)slot * nsamp + k) * 3 + a] = k < held ? hsm[((size_t)k * 3 + a) * W + slot] : hst[a * W + slot];
  }
  return 0;
}

}  // namespace

}  // namespace xpic

using namespace xpic;

extern "C" {

int xpic_field_lines(xpic_ctx* ctx, int field, int64_t n, const double* seeds3, const xpic_line_params* params,
  const xpic_trace_region* region, int64_t sample_every, double* end3, double* length, double* volume, double* fmin,
  double* smin, double* fmax, int64_t* steps, int32_t* code, double* samples)
{
  const LineCall c{"field_lines", n, seeds3, params, region, sample_every, end3, length, volume, fmin, smin, fmax, steps, code,
    samples};
  XPIC_CHECK(ctx != nullptr, "null context");
  XPIC_CHECK(ctx->geom.nranks == 1 && ctx->g.G == 0,
    c.who + ": a context of several z-slabs (or a self_ring one) is not supported: the gathers wrap z in the kernel");
  XPIC_CHECK(field >= 0 && field < XPIC_NFIELDS && ctx->field[field], c.who + ": unknown or unallocated field id");
  OpenRegion R{};
  bool go = false;
  XPIC_CALL(lines_check(c, "stagger", params ? params->stagger : 0, &R, &go));
  if (!go) return 0;
  if (params->stagger == XPIC_STAGGER_E) return lines_run(ctx, c, R, FLGrid<true>{ctx->g, ctx->field[field]});
  return lines_run(ctx, c, R, FLGrid<false>{ctx->g, ctx->field[field]});
}

int xpic_model_field_lines(xpic_ctx* ctx, const xpic_field_model* model, int64_t n, const double* seeds3,
  const xpic_line_params* params, const xpic_trace_region* region, int64_t sample_every, double* end3, double* length,
  double* volume, double* fmin, double* smin, double* fmax, int64_t* steps, int32_t* code, double* samples)
{
  const LineCall c{"model_field_lines", n, seeds3, params, region, sample_every, end3, length, volume, fmin, smin, fmax, steps,
    code, samples};
  XPIC_CHECK(ctx != nullptr, "null context");
  const char* bad = model_check(model);
  XPIC_CHECK(!bad, c.who + ": " + (bad ? bad : ""));
  OpenRegion R{};
  bool go = false;
  XPIC_CALL(lines_check(c, "component", params ? params->component : 0, &R, &go));
  if (!go) return 0;
  return lines_run(ctx, c, R, FLModel{*model, params->component == XPIC_STAGGER_E});
}

}  // extern "C"
