// batch.h -- the host side that the batch particle calls share (eccapfim.hip, drift_kinetic.hip, full_orbit.hip,
// model_trace.hip, compare_trace.hip): host arrays of particles are staged on the device, a kernel runs one lane per
// particle, the results are copied back.  batch_trace is the one driver of every trace of one batch, closed or open
// (trace_open.h, trace_open.hip: exit steps, alive counts, and the list of live particles between launches); the entry
// points reach it through trace_call.h.  batch_compare_trace is the driver for two or three batches advanced side by side
// (compare_trace.hip).
// DevScratch also owns every other device buffer that lives for one call (fields.hip, particles.hip, commands.hip,
// api.hip).  Host code only: no kernel or device function is declared here.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace xpic {

// ---- This part uses nothing from HIP: a plain host compiler compiles it (and a sanitizer build runs it) ----------------

// [n][w] host records -> [w][n], and back; w = 6: a particle.  With a stride: the w columns from `first` on of records
// `stride` wide (the statistics of a comparison trace); the records' other columns are neither read nor written.
inline void to_soa(const double* aos, int64_t n, std::vector<double>& soa, int w = 6, int stride = 0, int first = 0)
{
  const int s = stride ? stride : w;
  soa.resize((size_t)w * n);
  for (int64_t q = 0; q < n; ++q)
    for (int k = 0; k < w; ++k) soa[(size_t)k * n + q] = aos[s * q + first + k];
}
inline void to_aos(const double* soa, int64_t n, double* aos, int w = 6, int stride = 0, int first = 0)
{
  const int s = stride ? stride : w;
  for (int64_t q = 0; q < n; ++q)
    for (int k = 0; k < w; ++k) aos[s * q + first + k] = soa[(size_t)k * n + q];
}

// The sample buffer of a trace of n >= 0 particles over steps >= 0 steps: a sample after every sample_every-th step
// (>= 1 when sampled), six doubles per particle and sample.  -> its bytes, formed in 64-bit; -1: the count overflows or
// exceeds 2^46 bytes, and the trace is refused before anything is allocated or launched.
inline int64_t trace_sample_bytes(int64_t n, int64_t steps, int64_t sample_every, bool sampled, int64_t* nsamp)
{
  *nsamp = sampled ? steps / sample_every : 0;
  int64_t row_bytes = 0, bytes = 0;
  const bool fits = !__builtin_mul_overflow((int64_t)(6 * sizeof(double)), n, &row_bytes) &&
    !__builtin_mul_overflow(row_bytes, *nsamp, &bytes) && bytes <= ((int64_t)1 << 46);
  return fits ? bytes : -1;
}

// What a trace call of one batch was given by its caller (trace_call.h, batch_trace): host pointers and counts as the C
// entry points take them.
struct TraceArrays {
  int64_t n;            // particles
  int64_t steps;        // steps of this call
  int64_t sample_every; // a sample row after every sample_every-th step; >= 1 when samples or alive is given
  double* state_6;      // [n][6], in and out
  double* samples;      // [nsamp][n][6], or null
  int64_t* it_sum;      // [n] the sum and
  int* it_max;          // [n] the maximum of each particle's iteration counts; either may be null without `counters`
  int64_t* exit_step;   // [n] in and out as the open entry points document it; null (a closed trace): all enter alive
  int64_t* alive;       // [nsamp], or null
  int64_t* removed;     // one count; null (a closed trace): nothing can leave, nothing is read back between launches
  bool counters;        // the launches count iterations: it_sum and it_max are staged, zeroed, and come back
  double* sums_4;       // [n][4] in and out, staged as [4][n] around the launches (the timed full orbit's), or null
};
// the sample buffer of such a call: its rows hold particles only when samples are asked for
inline int64_t trace_sample_bytes(const TraceArrays& A, int64_t* nsamp)
{
  return trace_sample_bytes(A.samples ? A.n : 0, A.steps, A.sample_every, A.samples || A.alive, nsamp);
}

// An open trace (batch_trace): whether the list of `listed` entries, `live` of them alive, is rebuilt before the next
// launch.  policy: enum xpic_trace_compact (0: when fewer than half are alive, 1: never, 2: whenever one is not).
inline bool trace_compacts(int policy, int64_t live, int64_t listed)
{
  if (policy == 1 || live >= listed) return false;
  return policy == 2 || 2 * live < listed;
}

// An open trace's sample rows [nsamp][n][6] on the host: row k is the state after step (k + 1) sample_every of the call.
// The kernels write a particle's rows only while it steps; here a particle that is not alive at the end (exit_out >= 0)
// gets its final state, which is the state it was removed with, in every row behind its last step: behind step
// exit_out - step0 when this call removed it, in every row when it entered removed (exit_in >= 0).
inline void fill_frozen_samples(int64_t n, int64_t nsamp, int64_t sample_every, int64_t step0, const int64_t* exit_in,
  const int64_t* exit_out, const double* state_6, double* samples)
{
  for (int64_t q = 0; q < n; ++q) {
    if (exit_out[q] < 0) continue;
    const int64_t done = exit_in[q] >= 0 ? 0 : exit_out[q] - step0;
    for (int64_t k = done > 0 ? done / sample_every : 0; k < nsamp; ++k)
      for (int a = 0; a < 6; ++a) samples[((size_t)k * n + q) * 6 + a] = state_6[6 * q + a];
  }
}

}  // namespace xpic

#ifdef __HIPCC__ // ---- from here on: the device runtime ---------------------------------------------------------------

#include <algorithm>

#include "common.h"

namespace xpic {

// device memory of one call, freed on scope exit (so an early return between alloc and the end does not leak it)
template <class T>
struct DevScratch {
  T* p = nullptr;
  DevScratch() = default;
  DevScratch(const DevScratch&) = delete;
  DevScratch& operator=(const DevScratch&) = delete;
  ~DevScratch() { if (p) (void)hipFree(p); }
  int alloc(size_t count) { XPIC_HIP(hipMalloc(&p, sizeof(T) * count)); return 0; }
};

// count elements host -> d, d (from element `first`) -> host, and zero bytes over them; all asynchronous on stream
template <class T>
int upload(DevScratch<T>& d, const T* host, size_t count, hipStream_t stream)
{
  XPIC_HIP(hipMemcpyAsync(d.p, host, sizeof(T) * count, hipMemcpyHostToDevice, stream));
  return 0;
}
template <class T>
int download(T* host, const DevScratch<T>& d, size_t count, hipStream_t stream, size_t first = 0)
{
  XPIC_HIP(hipMemcpyAsync(host, d.p + first, sizeof(T) * count, hipMemcpyDeviceToHost, stream));
  return 0;
}
template <class T>
int zero(DevScratch<T>& d, size_t count, hipStream_t stream)
{
  XPIC_HIP(hipMemsetAsync(d.p, 0, sizeof(T) * count, stream));
  return 0;
}

// one lane per particle, workgroups of kLaneBlock
constexpr int kLaneBlock = 256;
inline dim3 lane_grid(int64_t n) { return dim3((unsigned)((n + kLaneBlock - 1) / kLaneBlock)); }

// One step of n > 0 particles, p0_6 -> pn_6 ([n][6] host records, staged as [6][n]), with one iteration count per
// particle when `counters`.  launch(s0, sn, iterations) starts the kernel (iterations: null without counters) and is
// timed under `label`.
template <class Launch>
int batch_push(xpic_ctx* c, const char* label, int64_t n, bool counters, const double* p0_6, double* pn_6, int* iterations,
  Launch launch)
{
  std::vector<double> h;
  to_soa(p0_6, n, h);
  DevScratch<double> s0, sn;
  DevScratch<int> it;
  XPIC_CALL(s0.alloc(6 * n)); XPIC_CALL(sn.alloc(6 * n));
  if (counters) XPIC_CALL(it.alloc(n));
  XPIC_CALL(upload(s0, h.data(), 6 * n, c->stream));
  {
    Timed t(c, label);
    launch((const double*)s0.p, sn.p, it.p);
    XPIC_HIP(hipGetLastError());
  }
  XPIC_CALL(download(h.data(), sn, 6 * n, c->stream));
  if (counters) XPIC_CALL(download(iterations, it, n, c->stream));
  XPIC_HIP(hipStreamSynchronize(c->stream));
  to_aos(h.data(), n, pn_6);
  return 0;
}

// The trace driver for the members of a comparison trace, advanced side by side in one lane (compare_trace.hip; DESIGN.md 5k,
// 5m, 5p).  A member is a host batch state_6 [n][6], in and out (null: the member is absent and nothing of it is staged),
// with the sum and the maximum of its iteration counts when `counters` (zeroed here).
struct CompareMember {
  double* state_6;
  int64_t* it_sum;
  int* it_max;
  bool counters;
};
constexpr int kCompareMembers = 3;
// what a launch of a comparison trace gets: per member the state [6][n] and the counters (null where the member is absent
// or has none), the travelling statistics [stats_w][n] and the curve (null without one)
struct CompareDev {
  double* s[kCompareMembers];
  long long* it_sum[kCompareMembers];
  int* it_max[kCompareMembers];
  double* stats;
  unsigned long long* curve;
};

// what one launch of a trace of one batch gets (batch_trace), typed as the kernels take it: the launch runs the steps
// first + 1 .. first + ns over the m entries of list
struct TraceDev {
  double* s;                   // the state [6][n]
  const long long* list;       // the particles the launch covers; null: the particles 0 .. m - 1
  long m;                      // its entries
  long first;                  // steps of the call before this launch
  int ns;                      // steps of this launch
  long nsamp;                  // rows of samples and of alive
  double* samples;             // [nsamp][6][n]; null: the call has none
  long long* it_sum;           // [n] and
  int* it_max;                 // [n]; null in a call without counters
  long long* exit_step;        // [n]; a closed trace's is a stand-in, which its kernels do not take
  unsigned long long* alive;   // [nsamp], zeroed before the first launch, the kernel adds to its rows; null: none
  unsigned long long* removed; // one count, zeroed before the first launch, the kernel adds to it
  double* extra;               // [4][n] of the caller: the timed trace's sums, the collisional traces' tallies, or null
};

// `steps` steps of n > 0 lanes in place.  The running maxima stats [n][stats_width] are in and out: the stats_w columns
// from stats_first on travel, staged as [stats_w][n], and the other columns of the caller's array are neither read nor
// written (a pair: 4 / 0 / 4; a triplet: 7 / 0 / 7; its grid-less pair: 7 / 3 / 4).  curve [nsamp][curve_width] (null with
// nsamp == 0) is zeroed on the device and written by the kernel's atomic maxima.  launch(dev, first, nsteps) starts the
// kernel for steps first + 1 .. first + nsteps; each launch is timed under `label`.  Everything comes back once, after the
// last launch.
template <class Launch>
int batch_compare_trace(xpic_ctx* c, const char* label, int launch_steps, int64_t n, int64_t steps, int64_t nsamp,
  const CompareMember (&member)[kCompareMembers], double* stats, int stats_width, int stats_first, int stats_w, double* curve,
  int curve_width, Launch launch)
{
  const size_t row = (size_t)6 * n; // doubles of one state
  std::vector<double> h[kCompareMembers], hst;
  DevScratch<double> s[kCompareMembers], st, cv;
  DevScratch<int64_t> tot[kCompareMembers];
  DevScratch<int> mx[kCompareMembers];
  for (int m = 0; m < kCompareMembers; ++m) {
    if (!member[m].state_6) continue;
    to_soa(member[m].state_6, n, h[m]);
    XPIC_CALL(s[m].alloc(row));
    XPIC_CALL(upload(s[m], h[m].data(), row, c->stream));
    if (!member[m].counters) continue;
    XPIC_CALL(tot[m].alloc(n)); XPIC_CALL(mx[m].alloc(n));
    XPIC_CALL(zero(tot[m], n, c->stream)); XPIC_CALL(zero(mx[m], n, c->stream));
  }
  to_soa(stats, n, hst, stats_w, stats_width, stats_first);
  XPIC_CALL(st.alloc((size_t)stats_w * n));
  XPIC_CALL(upload(st, hst.data(), (size_t)stats_w * n, c->stream));
  if (nsamp > 0) {
    XPIC_CALL(cv.alloc(curve_width * nsamp));
    XPIC_CALL(zero(cv, curve_width * nsamp, c->stream));
  }
  CompareDev dev{};
  for (int m = 0; m < kCompareMembers; ++m) {
    dev.s[m] = s[m].p;
    dev.it_sum[m] = (long long*)tot[m].p;
    dev.it_max[m] = mx[m].p;
  }
  dev.stats = st.p;
  dev.curve = (unsigned long long*)cv.p;
  for (int64_t first = 0; first < steps; first += launch_steps) {
    const int ns = (int)std::min<int64_t>(launch_steps, steps - first);
    Timed t(c, label);
    launch(dev, (long)first, ns);
    XPIC_HIP(hipGetLastError());
  }
  for (int m = 0; m < kCompareMembers; ++m) {
    if (s[m].p) XPIC_CALL(download(h[m].data(), s[m], row, c->stream));
    if (tot[m].p) {
      XPIC_CALL(download(member[m].it_sum, tot[m], n, c->stream));
      XPIC_CALL(download(member[m].it_max, mx[m], n, c->stream));
    }
  }
  XPIC_CALL(download(hst.data(), st, (size_t)stats_w * n, c->stream));
  if (nsamp > 0) XPIC_CALL(download(curve, cv, curve_width * nsamp, c->stream));
  XPIC_HIP(hipStreamSynchronize(c->stream));
  for (int m = 0; m < kCompareMembers; ++m)
    if (s[m].p) to_aos(h[m].data(), n, member[m].state_6);
  to_aos(hst.data(), n, stats, stats_w, stats_width, stats_first);
  return 0;
}

// trace_open.hip: out[0 .. cap) = the entries of list[0 .. m) (null: 0 .. m - 1) whose exit_step is < 0, in their order;
// blk and off: one element per workgroup of kLaneBlock entries.  Timed under `label`.
int live_compact(xpic_ctx* c, const char* label, const int64_t* exit_step, const int64_t* list, int64_t m, int64_t cap,
  int64_t* out, double* blk, int64_t* off);

// The list of live particles of an open trace and what the host knows of it.  batch_trace keeps one for the length of a
// call, a tracer set (tracers.hip) for its life.
struct LiveList {
  DevScratch<double> blk;        // live_compact's count per workgroup and
  DevScratch<int64_t> off;       // its prefix: sized by the first compaction (the list only shrinks)
  DevScratch<int64_t> lst[2];    // the list and the one the next compaction writes, alternating
  const int64_t* list = nullptr; // the entries the next launch covers: null = every particle
  int64_t listed = 0, live = 0;  // its entries, and how many of them are alive
  int64_t gone = 0;              // what the device's `removed` count held when it was last read
  int next = 0;                  // the buffer the next compaction writes
  bool due = false;              // a launch has run since the list was last weighed (trace_compacts)
};

// The launches of steps first + 1 .. first + steps of a trace whose arrays `d` names, in launches of at most launch_steps
// steps, each timed under `label`.  track: after every launch the count removed so far comes back (8 bytes, one
// synchronisation), so the host knows how many entries are alive: when none is, the remaining launches are skipped, and by
// `policy` (trace_compacts) the list is rebuilt in front of the next launch, timed under `compact_label`.  Without it
// nothing is read back and nothing synchronises between the launches.  d.first and d.ns, d.list and d.m are set here.
template <class Launch>
int trace_launches(xpic_ctx* c, const char* label, const char* compact_label, int launch_steps, int64_t first, int64_t steps,
  int policy, bool track, TraceDev& d, LiveList& L, Launch launch)
{
  const int64_t end = first + steps;
  for (; first < end && L.live > 0; first += launch_steps) {
    if (L.due && trace_compacts(policy, L.live, L.listed)) {
      if (!L.blk.p) { // (the list only shrinks: the first compaction's workgroup count bounds the later ones)
        const size_t nb = lane_grid(L.listed).x;
        XPIC_CALL(L.blk.alloc(nb)); XPIC_CALL(L.off.alloc(nb));
      }
      // (so do the live counts: buffer 0 is as long as the first list, buffer 1 as the second, and they alternate)
      if (!L.lst[L.next].p) XPIC_CALL(L.lst[L.next].alloc(L.live));
      XPIC_CALL(live_compact(c, compact_label, (const int64_t*)d.exit_step, L.list, L.listed, L.live, L.lst[L.next].p, L.blk.p,
        L.off.p));
      L.list = L.lst[L.next].p;
      L.listed = L.live;
      L.next ^= 1;
    }
    L.due = false;
    d.list = (const long long*)L.list; d.m = (long)L.listed;
    d.first = (long)first; d.ns = (int)std::min<int64_t>(launch_steps, end - first);
    {
      Timed t(c, label);
      launch(d);
      XPIC_HIP(hipGetLastError());
    }
    if (!track) continue;
    int64_t g = 0;
    XPIC_HIP(hipMemcpyAsync(&g, d.removed, sizeof g, hipMemcpyDeviceToHost, c->stream));
    XPIC_HIP(hipStreamSynchronize(c->stream));
    L.live -= g - L.gone;
    L.gone = g;
    L.due = true;
  }
  return 0;
}

// The steps of A (TraceArrays, A.n > 0) in place in A.state_6, the particles kept on the device, with the region rule of
// an open trace (include/xpic_hip.h: xpic_trace_region) when the kernel applies one.  `d` (TraceDev) comes
// with nsamp (trace_sample_bytes) and extra set by the caller; its other members are filled here, and launch(d) starts
// the kernel (trace_launches, which tracks the live list when A.removed is given).  A.sums_4 is the caller's to stage
// (trace_call.h).  The sample rows behind a removed particle's last step are filled here, on the host, from the final
// state (fill_frozen_samples): a launch no longer covers a particle that compaction has dropped.
template <class Launch>
int batch_trace(xpic_ctx* c, const char* label, const char* compact_label, int launch_steps, const TraceArrays& A, int policy,
  int64_t step0, TraceDev d, Launch launch)
{
  const int64_t n = A.n, steps = A.steps, nsamp = d.nsamp;
  int64_t* exit_step = A.exit_step;
  const size_t row = (size_t)6 * n; // doubles of one state
  std::vector<double> h, hs;
  to_soa(A.state_6, n, h);
  std::vector<int64_t> exit_in(n, -1), exit_own(exit_step ? 0 : n); // the closed trace's stand-ins
  if (exit_step) exit_in.assign(exit_step, exit_step + n);
  else exit_step = exit_own.data();
  int64_t live = 0;
  for (int64_t q = 0; q < n; ++q) live += exit_in[q] < 0;
  DevScratch<double> s, sm;
  DevScratch<int64_t> tot, ex, al, rm;
  DevScratch<int> mx;
  XPIC_CALL(s.alloc(row)); XPIC_CALL(ex.alloc(n)); XPIC_CALL(rm.alloc(1));
  XPIC_CALL(zero(rm, 1, c->stream));
  if (A.counters) {
    XPIC_CALL(tot.alloc(n)); XPIC_CALL(mx.alloc(n));
    XPIC_CALL(zero(tot, n, c->stream)); XPIC_CALL(zero(mx, n, c->stream));
  }
  if (A.samples && nsamp > 0) XPIC_CALL(sm.alloc(row * nsamp));
  if (A.alive && nsamp > 0) {
    XPIC_CALL(al.alloc(nsamp));
    XPIC_CALL(zero(al, nsamp, c->stream));
  }
  XPIC_CALL(upload(s, h.data(), row, c->stream));
  XPIC_CALL(upload(ex, exit_in.data(), n, c->stream));
  d.s = s.p; d.samples = sm.p; d.exit_step = (long long*)ex.p;
  d.it_sum = (long long*)tot.p; d.it_max = mx.p;
  d.alive = (unsigned long long*)al.p; d.removed = (unsigned long long*)rm.p;
  LiveList L;
  L.listed = n; L.live = live;
  XPIC_CALL(trace_launches(c, label, compact_label, launch_steps, 0, steps, policy, A.removed != nullptr, d, L, launch));
  XPIC_CALL(download(h.data(), s, row, c->stream));
  XPIC_CALL(download(exit_step, ex, n, c->stream));
  if (A.counters) {
    XPIC_CALL(download(A.it_sum, tot, n, c->stream));
    XPIC_CALL(download(A.it_max, mx, n, c->stream));
  }
  if (sm.p) {
    hs.resize(row * nsamp);
    XPIC_CALL(download(hs.data(), sm, row * nsamp, c->stream)); // the samples, once
  }
  if (al.p) XPIC_CALL(download(A.alive, al, nsamp, c->stream));
  XPIC_HIP(hipStreamSynchronize(c->stream));
  to_aos(h.data(), n, A.state_6);
  if (sm.p) {
    for (int64_t k = 0; k < nsamp; ++k) to_aos(hs.data() + row * k, n, A.samples + row * k);
    fill_frozen_samples(n, nsamp, A.sample_every, step0, exit_in.data(), exit_step, A.state_6, A.samples);
  }
  if (A.removed) *A.removed = L.gone;
  return 0;
}

}  // namespace xpic

#endif  // __HIPCC__
