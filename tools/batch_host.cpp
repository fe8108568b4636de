// batch_host.cpp -- the host half of xpic_amd/csrc/batch.h (the part above its __HIPCC__ line: transposition,
// trace_sample_bytes, trace_compacts, fill_frozen_samples) in a stand-alone program, so that a plain host compiler and its
// sanitizers can run it without a GPU, on the shapes of tests/test_gpu_open_trace.py: 775 particles, 21 sample rows,
// particles removed before their first step, after the 7th, the 146th and the 149th, and one that entered removed.
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -I xpic_amd/csrc tools/batch_host.cpp \
//     -o /tmp/batch_host && /tmp/batch_host
// prints "batch.h host staging: ok"; tests/test_batch_host.py builds it without the sanitizers and runs it.
#undef NDEBUG
#include <cassert>
#include <cstdio>
#include <vector>
#include "batch.h"
using namespace xpic;
int main()
{
  const int64_t n = 775, steps = 150, every = 7, step0 = 70;
  int64_t nsamp;
  assert(trace_sample_bytes(n, steps, every, true, &nsamp) == 48 * n * 21 && nsamp == 21);
  std::vector<double> state(6 * n), soa, back(6 * n), samples(6 * n * nsamp, -1.0);
  for (size_t i = 0; i < state.size(); ++i) state[i] = (double)i;
  to_soa(state.data(), n, soa);
  to_aos(soa.data(), n, back.data());
  assert(back == state);
  std::vector<int64_t> in(n, -1), out(n, -1);
  in[3] = 5; out[3] = 5;                       // entered removed: every row
  out[4] = step0;                               // removed before its first step: every row
  out[5] = step0 + 7;                           // after 7 steps: rows 1..
  out[6] = step0 + 149;                         // after 149 steps: no row (147 is the last sampled step)
  out[n - 1] = step0 + 146;                     // after 146: row 20 (step 147)
  fill_frozen_samples(n, nsamp, every, step0, in.data(), out.data(), state.data(), samples.data());
  auto filled = [&](int64_t k, int64_t q) { return samples[(k * n + q) * 6] == state[6 * q] && samples[(k * n + q) * 6 + 5] == state[6 * q + 5]; };
  for (int64_t k = 0; k < nsamp; ++k) {
    assert(filled(k, 3) && filled(k, 4));
    assert(filled(k, 5) == (k >= 1));
    assert(!filled(k, 6) && !filled(k, 7));
    assert(filled(k, n - 1) == (k >= 20));
  }
  assert(!trace_compacts(0, 400, 775) && trace_compacts(0, 387, 775) && !trace_compacts(0, 388, 775));
  assert(!trace_compacts(1, 1, 775) && trace_compacts(2, 774, 775) && !trace_compacts(2, 775, 775) && !trace_compacts(0, 775, 775));
  fill_frozen_samples(0, 0, 1, 0, nullptr, nullptr, nullptr, nullptr);
  std::puts("batch.h host staging: ok");
  return 0;
}
