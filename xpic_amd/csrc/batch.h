// batch.h -- the host side that the batch particle calls share (eccapfim.hip, drift_kinetic.hip, full_orbit.hip): host
// arrays of particles are staged on the device, a kernel runs one lane per particle, the results are copied back.
// DevScratch also owns every other device buffer that lives for one call (fields.hip, particles.hip, commands.hip,
// api.hip).  Host code only: no kernel or device function is declared here.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace xpic {

// ---- This part uses nothing from HIP: a plain host compiler compiles it (and a sanitizer build runs it) ----------------

// [n][6] host records -> [6][n], and back
inline void to_soa(const double* aos, int64_t n, std::vector<double>& soa)
{
  soa.resize((size_t)6 * n);
  for (int64_t q = 0; q < n; ++q)
    for (int k = 0; k < 6; ++k) soa[(size_t)k * n + q] = aos[6 * q + k];
}
inline void to_aos(const double* soa, int64_t n, double* aos)
{
  for (int64_t q = 0; q < n; ++q)
    for (int k = 0; k < 6; ++k) aos[6 * q + k] = soa[(size_t)k * n + q];
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

// `steps` steps of n > 0 particles in place in state_6, the particles kept on the device; nsamp samples
// (trace_sample_bytes) into samples[nsamp][n][6]; with `counters` the sum and the maximum of each particle's iteration
// counts.  launch(s, first, nsteps, samples, it_sum, it_max) starts the kernel for steps first + 1 .. first + nsteps
// (samples: null without samples; it_sum, it_max: null without counters); each launch is timed under `label`.
template <class Launch>
int batch_trace(xpic_ctx* c, const char* label, int launch_steps, int64_t n, int64_t steps, int64_t nsamp, bool counters,
  double* state_6, double* samples, int64_t* it_sum, int* it_max, Launch launch)
{
  const size_t row = (size_t)6 * n; // doubles of one state
  std::vector<double> h, hs;
  to_soa(state_6, n, h);
  DevScratch<double> s, sm;
  DevScratch<int64_t> tot;
  DevScratch<int> mx;
  XPIC_CALL(s.alloc(row));
  if (counters) {
    XPIC_CALL(tot.alloc(n)); XPIC_CALL(mx.alloc(n));
    XPIC_CALL(zero(tot, n, c->stream)); XPIC_CALL(zero(mx, n, c->stream));
  }
  if (nsamp > 0) XPIC_CALL(sm.alloc(row * nsamp));
  XPIC_CALL(upload(s, h.data(), row, c->stream));
  // one launch covers at most launch_steps steps, so no launch runs for seconds however long the trace
  for (int64_t first = 0; first < steps; first += launch_steps) {
    const int ns = (int)std::min<int64_t>(launch_steps, steps - first);
    Timed t(c, label);
    launch(s.p, (long)first, ns, sm.p, (long long*)tot.p, mx.p);
    XPIC_HIP(hipGetLastError());
  }
  XPIC_CALL(download(h.data(), s, row, c->stream));
  if (counters) {
    XPIC_CALL(download(it_sum, tot, n, c->stream));
    XPIC_CALL(download(it_max, mx, n, c->stream));
  }
  if (nsamp > 0) {
    hs.resize(row * nsamp);
    XPIC_CALL(download(hs.data(), sm, row * nsamp, c->stream)); // the samples, once
  }
  XPIC_HIP(hipStreamSynchronize(c->stream));
  to_aos(h.data(), n, state_6);
  for (int64_t k = 0; k < nsamp; ++k) to_aos(hs.data() + row * k, n, samples + row * k);
  return 0;
}

}  // namespace xpic

#endif  // __HIPCC__
