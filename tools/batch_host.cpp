// batch_host.cpp -- the host half of xpic_amd/csrc/batch.h (the part above its __HIPCC__ line: transposition,
// trace_sample_bytes and the record of a call's arrays it reads, trace_compacts, fill_frozen_samples) in a stand-alone
// program, so that a plain host compiler and its sanitizers can run it without a GPU, on the shapes of tests/test_gpu_open_trace.py: 775 particles, 21 sample rows,
// particles removed before their first step, after the 7th, the 146th and the 149th, and one that entered removed; and the
// windowed transposition of a comparison trace's statistics: 775 records of width 7 with the window 3 .. 6 (columns 0 .. 2
// keep their sentinels), width 4 with the full window, and no record at all.
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
  // the record of a call's arrays gives the same rows; only a call with samples counts particles into the bytes
  std::vector<int64_t> rows(21);
  TraceArrays A{n, steps, every, state.data(), samples.data(), nullptr, nullptr, nullptr, nullptr, nullptr, false, nullptr};
  nsamp = -1;
  assert(trace_sample_bytes(A, &nsamp) == 48 * n * 21 && nsamp == 21);
  A.samples = nullptr; // neither samples nor alive: no row, and sample_every is not read
  A.sample_every = 0;
  assert(trace_sample_bytes(A, &nsamp) == 0 && nsamp == 0);
  A.alive = rows.data(); // alive alone: the rows are counted, no particle is
  A.sample_every = every;
  assert(trace_sample_bytes(A, &nsamp) == 0 && nsamp == 21);
  A.samples = samples.data();
  A.n = 0; // zero particles
  assert(trace_sample_bytes(A, &nsamp) == 0 && nsamp == 21);
  A.n = n;
  A.sample_every = steps + 1; // sample_every larger than steps: no row
  assert(trace_sample_bytes(A, &nsamp) == 0 && nsamp == 0);
  A.sample_every = 1; // the refusal above 2^46 bytes: a row of 2^36 particles is 3 * 2^40 bytes
  A.n = (int64_t)1 << 36;
  A.steps = 21; // 63 * 2^40 bytes
  assert(trace_sample_bytes(A, &nsamp) == 48 * A.n * 21 && nsamp == 21);
  A.steps = 22; // 66 * 2^40 bytes: refused
  assert(trace_sample_bytes(A, &nsamp) == -1);
  A.steps = INT64_MAX; // the product overflows: refused
  assert(trace_sample_bytes(A, &nsamp) == -1);
  nsamp = 21;
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
  // the statistics of the grid-less pair: columns 3 .. 6 of [n][7] travel as [4][n], columns 0 .. 2 stay as they are
  std::vector<double> st7(7 * n), w4, out7(7 * n, -7.0);
  for (size_t i = 0; i < st7.size(); ++i) st7[i] = 0.5 + (double)i;
  to_soa(st7.data(), n, w4, 4, 7, 3);
  assert(w4.size() == (size_t)4 * n);
  for (int64_t q = 0; q < n; ++q)
    for (int k = 0; k < 4; ++k) assert(w4[k * n + q] == st7[7 * q + 3 + k]);
  to_aos(w4.data(), n, out7.data(), 4, 7, 3);
  for (int64_t q = 0; q < n; ++q)
    for (int k = 0; k < 7; ++k) assert(out7[7 * q + k] == (k < 3 ? -7.0 : st7[7 * q + k]));
  // a pair's [n][4] with the full window is the plain transposition
  std::vector<double> st4(st7.begin(), st7.begin() + 4 * n), full, plain, back4(4 * n);
  to_soa(st4.data(), n, full, 4, 4, 0);
  to_soa(st4.data(), n, plain, 4);
  assert(full == plain);
  to_aos(full.data(), n, back4.data(), 4, 4, 0);
  assert(back4 == st4);
  to_soa(nullptr, 0, w4, 4, 7, 3);
  assert(w4.empty());
  to_aos(w4.data(), 0, nullptr, 4, 7, 3);
  std::puts("batch.h host staging: ok");
  return 0;
}
