// trace_open.hip -- the list of live particles of an open trace: between two launches batch_trace
// (batch.h) may replace the list the next launch covers by its live entries, in their order.  A scan and a scatter:
//   k_live_count    one count per workgroup of 256 entries (block_reduce_store, device_common.h)
//   k_live_offsets  their exclusive prefix, one workgroup
//   k_live_scatter  entry j -> out[offset of its workgroup + live entries before it in the workgroup]
// A null list stands for the identity 0 .. m - 1 (no launch has been compacted yet).  Order-preserving, so the list is
// the same whatever the timing; plain vector stores only.
#include <algorithm>

#include "batch.h"
#include "common.h"
#include "device_common.h"

namespace xpic {

namespace {

constexpr int kBlock = kLaneBlock;
constexpr int kWaves = kBlock / 64;

__device__ inline bool live_entry(const long long* __restrict__ exit_step, const long long* __restrict__ list, long m, long j,
  long long* q)
{
  if (j >= m) return false;
  *q = list ? list[j] : j;
  return exit_step[*q] < 0;
}

// The counts travel as doubles because block_reduce_store, the workgroup reduction the kernel files share, sums doubles:
// a count is at most 256 here and at most n <= 2^36 once summed, far inside the 2^53 a double holds exactly, and
// k_live_offsets turns them back into integers.
__global__ void __launch_bounds__(kBlock) k_live_count(const long long* __restrict__ exit_step,
  const long long* __restrict__ list, long m, double* __restrict__ blk, int nblocks)
{
  long long q;
  double acc[1] = {live_entry(exit_step, list, m, (long)blockIdx.x * kBlock + threadIdx.x, &q) ? 1.0 : 0.0};
  block_reduce_store<1, kBlock>(acc, blk, nblocks, blockIdx.x);
}

// thread t sums the counts of its run of ceil(nb / 256) workgroups, the 256 sums are prefixed, and the run is walked again.
// The prefix is each thread's own loop over the sums before it (at most 255 additions from LDS): one small workgroup per
// compaction, not worth a log-step scan.
__global__ void __launch_bounds__(kBlock) k_live_offsets(const double* __restrict__ blk, long nb, long long* __restrict__ off)
{
  __shared__ long long sm[kBlock];
  const long run = (nb + kBlock - 1) / kBlock;
  const long lo = (long)threadIdx.x * run, b0 = lo < nb ? lo : nb, b1 = b0 + run < nb ? b0 + run : nb;
  long long s = 0;
  for (long b = b0; b < b1; ++b) s += (long long)blk[b];
  sm[threadIdx.x] = s;
  __syncthreads();
  long long base = 0;
  for (int t = 0; t < (int)threadIdx.x; ++t) base += sm[t];
  for (long b = b0; b < b1; ++b) {
    off[b] = base;
    base += (long long)blk[b];
  }
}

// cap: entries of out (the live count the host carries; a slot beyond it is never written)
__global__ void __launch_bounds__(kBlock) k_live_scatter(const long long* __restrict__ exit_step,
  const long long* __restrict__ list, long m, const long long* __restrict__ off, long long* __restrict__ out, long cap)
{
  __shared__ int wv[kWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  long long q = 0;
  const bool live = live_entry(exit_step, list, m, (long)blockIdx.x * kBlock + threadIdx.x, &q);
  const unsigned long long b = __ballot(live);
  if (lane == 0) wv[wave] = __popcll(b);
  __syncthreads();
  if (!live) return;
  long long pos = off[blockIdx.x];
  for (int w = 0; w < wave; ++w) pos += wv[w];
  pos += __popcll(b & ((1ull << lane) - 1ull));
  if (pos < cap) out[pos] = q;
}

}  // namespace

int live_compact(xpic_ctx* c, const char* label, const int64_t* exit_step, const int64_t* list, int64_t m, int64_t cap,
  int64_t* out, double* blk, int64_t* off)
{
  XPIC_CHECK(m > 0 && cap > 0 && out != list, "live_compact: nothing to compact, or in place");
  const dim3 grid = lane_grid(m);
  Timed t(c, label);
  hipLaunchKernelGGL(k_live_count, grid, dim3(kBlock), 0, c->stream, (const long long*)exit_step, (const long long*)list,
    (long)m, blk, (int)grid.x);
  XPIC_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_live_offsets, dim3(1), dim3(kBlock), 0, c->stream, (const double*)blk, (long)grid.x, (long long*)off);
  XPIC_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_live_scatter, grid, dim3(kBlock), 0, c->stream, (const long long*)exit_step, (const long long*)list,
    (long)m, (const long long*)off, (long long*)out, (long)cap);
  XPIC_HIP(hipGetLastError());
  return 0;
}

}  // namespace xpic
