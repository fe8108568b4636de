// trace_call.h -- the one statement of what every trace entry point of one batch checks and does:
// full_orbit.hip and drift_kinetic.hip (closed and open, on the grid), model_trace.hip (on an analytic model, timed or
// not), collide_trace.hip (either, with collisions).  The pusher-parameter checks, the first checks of an entry point on
// a model, the checks of the trace's own arguments under the names the entry point's messages use, the zero-fill of a
// Chin id's counters, and the call of batch.h's batch_trace.  Host code only.
#pragma once

#include <algorithm>
#include <string>
#include <type_traits>

#include "batch.h"
#include "field_model.h"
#include "trace_open.h"

namespace xpic {

// the checks of a pusher's parameters; `who` heads every message ("full_orbit" on the grid, the entry point's name on a
// model)
inline int fo_check_params(const std::string& who, const xpic_fo_params* P)
{
  XPIC_CHECK(P, who + ": params is null");
  XPIC_CHECK(P->scheme >= 0 && P->scheme < XPIC_FO_NSCHEMES, who + ": unknown scheme id");
  if (P->scheme == XPIC_FO_CN)
    XPIC_CHECK(P->maxit >= 1 && P->maxit <= XPIC_FO_MAXIT, who + ": maxit must be within 1 .. 64");
  return 0;
}
// maxit_cap: the largest maxit the kernel's loop is bounded by, 0: none (the grid pusher)
inline int dk_check_params(const std::string& who, const xpic_dk_params* P, int maxit_cap)
{
  XPIC_CHECK(P, who + ": params is null");
  XPIC_CHECK(P->maxit >= 1 && (!maxit_cap || P->maxit <= maxit_cap),
    who + (maxit_cap ? ": maxit must be within 1 .. " + std::to_string(maxit_cap) : ": maxit must be >= 1"));
  XPIC_CHECK(P->mp != 0.0, who + ": mp must not be 0");
  return 0;
}

inline int model_ok(const std::string& who, const xpic_field_model* model)
{
  const char* bad = model_check(model);
  XPIC_CHECK(!bad, who + ": " + (bad ? bad : ""));
  return 0;
}
// the checks an entry point on a model makes first, for either pusher: the context, n, the pusher's parameters, the model
template <class Params>
int model_checks(const std::string& who, xpic_ctx* ctx, int64_t n, const Params* params, const xpic_field_model* model)
{
  XPIC_CHECK(ctx != nullptr, "null context");
  XPIC_CHECK(n >= 0, who + ": n is negative");
  if constexpr (std::is_same_v<Params, xpic_fo_params>) XPIC_CALL(fo_check_params(who, params));
  else XPIC_CALL(dk_check_params(who, params, XPIC_MODEL_DK_MAXIT));
  return model_ok(who, model);
}

// An entry point as its messages name it and its arrays, and the labels its launches and its compactions are timed under.
// closed: the entry point has no region, exit_step, alive or removed in its argument list (xpic_full_orbit_trace,
// xpic_drift_kinetic_trace); it words sample_every's message without `alive`, and a call of zero steps still zeroes its
// counters.
struct TraceEntry {
  const char *who, *state, *it_sum, *it_max;
  bool closed;
  const char *label, *compact_label;
};
// an entry point on a model, or a collisional one on the grid, which words its messages alike (`who` outlives the entry): it
// says "the particle array" and, for both counters, "an iteration counter"; without a compact_label its list is never rebuilt
inline TraceEntry model_entry(const std::string& who, const char* label, const char* compact_label = nullptr)
{
  return {who.c_str(), "the particle array", "an iteration counter", "an iteration counter", false, label,
    compact_label ? compact_label : label};
}

// The checks and the driver every trace shares, after its own checks of the context, the pusher and the region.  R.kind < 0:
// no region, and A.exit_step and A.removed may be null (batch_trace makes the stand-ins).  A trace without A.counters gets
// null counters in its launches, and the caller's, where given, are zeroed here.  A.sums_4 is staged here and reaches the
// launches as TraceDev's extra; without it they get `extra` (device, [4][n], or null).  launch: batch_trace's.
template <class Launch>
int trace_call(xpic_ctx* ctx, const TraceEntry& E, int launch_steps, const TraceArrays& A, const OpenRegion& R, int policy,
  double* extra, Launch launch)
{
  const std::string who = E.who;
  const bool open = R.kind >= 0;
  const int64_t n = A.n;
  XPIC_CHECK(n <= ((int64_t)1 << 36), who + ": n is larger than 2^36");
  XPIC_CHECK(A.steps >= 0, who + ": steps is negative");
  XPIC_CHECK((!A.samples && !A.alive) || A.sample_every >= 1,
    who + ": sample_every must be >= 1 when " + (E.closed ? "samples" : "samples or alive") + " are asked for");
  XPIC_CHECK(A.state_6, who + ": " + E.state + " is null");
  XPIC_CHECK(A.exit_step || !open, who + ": exit_step is null");
  XPIC_CHECK(A.removed || !open, who + ": removed is null");
  XPIC_CHECK(A.it_sum || !A.counters, who + ": " + E.it_sum + " is null");
  XPIC_CHECK(A.it_max || !A.counters, who + ": " + E.it_max + " is null");
  int64_t nsamp;
  XPIC_CHECK(trace_sample_bytes(A, &nsamp) >= 0, who + ": the sample buffer (48 n steps / sample_every bytes) is too large");
  if (A.removed) *A.removed = 0;
  if (n == 0 || (A.steps == 0 && !E.closed)) return 0;
  std::vector<double> hsum;
  DevScratch<double> dsum;
  if (A.sums_4) {
    to_soa(A.sums_4, n, hsum, 4);
    XPIC_CALL(dsum.alloc(4 * n));
    XPIC_CALL(upload(dsum, hsum.data(), 4 * n, ctx->stream));
    extra = dsum.p;
  }
  TraceDev d{};
  d.nsamp = (long)nsamp;
  d.extra = extra;
  XPIC_CALL(batch_trace(ctx, E.label, E.compact_label, launch_steps, A, policy, R.step0, d, launch));
  if (A.sums_4) {
    XPIC_CALL(download(hsum.data(), dsum, 4 * n, ctx->stream));
    XPIC_HIP(hipStreamSynchronize(ctx->stream));
    to_aos(hsum.data(), n, A.sums_4, 4);
  }
  if (!A.counters) {
    if (A.it_sum) std::fill(A.it_sum, A.it_sum + n, (int64_t)0);
    if (A.it_max) std::fill(A.it_max, A.it_max + n, 0);
  }
  return 0;
}

#ifdef __HIPCC__
// One launch of an open grid trace over the entries d names (full_orbit.hip, drift_kinetic.hip): what the open entry
// points start from trace_call's launch, and what a tracer set (tracers.hip) starts on arrays that stay on the device.
// n: the batch; every: sample_every (>= 1); gradB: the grad |B| vector or null
void fo_launch_open(xpic_ctx* ctx, const xpic_fo_params& P, const OpenRegion& R, long n, long every, const TraceDev& d);
void dk_launch_open(xpic_ctx* ctx, const xpic_dk_params& P, const double* gradB, const OpenRegion& R, long n, long every,
  const TraceDev& d);
#endif

}  // namespace xpic
