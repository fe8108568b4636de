// trace_call.h -- the one statement of what every trace entry point of one batch checks and does:
// full_orbit.hip and drift_kinetic.hip (closed and open, on the grid), model_trace.hip (on an analytic model, timed or
// not).  The pusher-parameter checks, the checks of the trace's own arguments under the names the entry point's messages
// use, the zero-fill of a Chin id's counters, and the call of batch.h's batch_trace.  Host code only.
#pragma once

#include <algorithm>
#include <string>

#include "batch.h"
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

// An entry point as its messages name it and its arrays (the model traces say "the particle array" and, for both
// counters, "an iteration counter").  closed: the entry point has no region, exit_step, alive or removed in its argument
// list (xpic_full_orbit_trace, xpic_drift_kinetic_trace); it words sample_every's message without `alive`, and a call of
// zero steps still zeroes its counters.
struct TraceEntry {
  const char *who, *state, *it_sum, *it_max;
  bool closed;
};

// The checks and the driver every trace shares, after its own checks of the context, the pusher and the region.  R.kind < 0:
// no region, and exit_step and removed may be null (batch_trace makes the stand-ins).  A trace without `counters` gets null
// counters in its launches, and the caller's, where given, are zeroed here.  sums_4 (null: none; the timed full orbit's)
// is staged as [4][n] around the launches.  launch: batch_trace's, with nsamp behind nsteps and the device's sums at the end.
template <class Launch>
int trace_call(xpic_ctx* ctx, const TraceEntry& E, const char* label, const char* compact_label, int launch_steps, int64_t n,
  bool counters, int64_t steps, int64_t sample_every, double* state_6, double* samples, int64_t* it_sum, int* it_max,
  const OpenRegion& R, int policy, int64_t* exit_step, int64_t* alive, int64_t* removed, double* sums_4, Launch launch)
{
  const std::string who = E.who;
  const bool open = R.kind >= 0;
  XPIC_CHECK(n <= ((int64_t)1 << 36), who + ": n is larger than 2^36");
  XPIC_CHECK(steps >= 0, who + ": steps is negative");
  XPIC_CHECK((!samples && !alive) || sample_every >= 1,
    who + ": sample_every must be >= 1 when " + (E.closed ? "samples" : "samples or alive") + " are asked for");
  XPIC_CHECK(state_6, who + ": " + E.state + " is null");
  XPIC_CHECK(exit_step || !open, who + ": exit_step is null");
  XPIC_CHECK(removed || !open, who + ": removed is null");
  XPIC_CHECK(it_sum || !counters, who + ": " + E.it_sum + " is null");
  XPIC_CHECK(it_max || !counters, who + ": " + E.it_max + " is null");
  int64_t nsamp;
  XPIC_CHECK(trace_sample_bytes(samples ? n : 0, steps, sample_every, samples || alive, &nsamp) >= 0,
    who + ": the sample buffer (48 n steps / sample_every bytes) is too large");
  if (removed) *removed = 0;
  if (n == 0 || (steps == 0 && !E.closed)) return 0;
  std::vector<double> hsum;
  DevScratch<double> dsum;
  if (sums_4) {
    to_soa(sums_4, n, hsum, 4);
    XPIC_CALL(dsum.alloc(4 * n));
    XPIC_CALL(upload(dsum, hsum.data(), 4 * n, ctx->stream));
  }
  XPIC_CALL(batch_trace(ctx, label, compact_label, launch_steps, n, steps, sample_every, nsamp, counters, policy, R.step0,
    state_6, samples, it_sum, it_max, exit_step, alive, removed,
    [&](double* s, const int64_t* list, long m, long first, int ns, double* sm, long long* sum, int* mx, long long* ex,
      unsigned long long* al, unsigned long long* rm) {
      launch(s, (const long long*)list, m, first, ns, (long)nsamp, sm, sum, mx, ex, al, rm, dsum.p);
    }));
  if (sums_4) {
    XPIC_CALL(download(hsum.data(), dsum, 4 * n, ctx->stream));
    XPIC_HIP(hipStreamSynchronize(ctx->stream));
    to_aos(hsum.data(), n, sums_4, 4);
  }
  if (!counters) {
    if (it_sum) std::fill(it_sum, it_sum + n, (int64_t)0);
    if (it_max) std::fill(it_max, it_max + n, 0);
  }
  return 0;
}

}  // namespace xpic
