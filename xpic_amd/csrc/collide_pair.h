// collide_pair.h -- one Takizuka-Abe collision (J. Comput. Phys. 25, 205, 1977) as a device function, and the streams its
// draws come from: shared by collide.hip (the records of a cell against each other, include/xpic_hip.h: xpic_collide and
// xpic_collide_weighted) and collide_trace.hip (a test particle against a partner drawn from a Maxwellian background,
// xpic_trace_collisions).  AN EXTENSION: the reference has no collision operator.  tests/collisions_ref.py and
// tests/collisional_trace_ref.py state the same text and the same constants a second time in numpy float64.
//
// The including files differ in their floating-point contraction (collide.hip: off, the tracers: on), so every function
// here that rounds carries `#pragma clang fp contract(off)` in its body: the collision is rounded operation by operation,
// as numpy rounds it, wherever it is included.  Included after device_common.h.  Device code, but for the keys the host
// forms (trace_step_key, call_key).
#pragma once

#include <cmath>

#include "device_common.h"

namespace xpic {

namespace {

// ---- xpic_collide's streams: cell <- (call, global cell); sub-stream <- (cell, tag); item i of a sub-stream: its state
// starts at key + i * (odd constant), as commands.hip's pair_stream
__device__ inline uint64_t cell_key(uint64_t call, long gcell)
{
  uint64_t k = call ^ ((uint64_t)gcell * 0xD6E8FEB86659FD93ull);
  return splitmix(k);
}
__device__ inline uint64_t sub_key(uint64_t cell, int tag)
{
  uint64_t k = cell ^ ((uint64_t)(tag + 1) * 0xA0761D6478BD642Full);
  return splitmix(k);
}
__device__ inline uint64_t item_state(uint64_t sub, int i) { return sub + (uint64_t)i * 0x2545F4914F6CDD1Dull; }
__device__ inline uint64_t item_key(uint64_t sub, int i)
{
  uint64_t st = item_state(sub, i);
  return splitmix(st);
}

// ---- the collisional traces' streams, in the same style: step <- (seed, global step k) as xpic_collide's call key begins
// (the seed's splitmix state, xor k * constant, splitmix); particle <- cell_key(step, global particle index); the stream
// of background b is sub_key(particle, b): its state yields the seven draws a1 a2 a3 a4, a5, u1 u2 u3 in this order
__host__ __device__ inline uint64_t trace_step_key(uint64_t seed, long long k)
{
  uint64_t key = seed;
  (void)splitmix(key);
  key ^= (uint64_t)k * 0xD1342543DE82EF95ull;
  return splitmix(key);
}
// xpic_collide's call key, the stream of (seed, step, sort_a, sort_b): the step key, xor the packed sort pair * constant,
// splitmix
__host__ inline uint64_t call_key(uint64_t seed, int64_t step, int ia, int ib)
{
  uint64_t key = trace_step_key(seed, step);
  key ^= (((uint64_t)(uint32_t)ia << 32) | (uint64_t)(uint32_t)ib) * 0x9FB21C651E98DF25ull;
  return splitmix(key);
}
__device__ inline uint64_t trace_stream(uint64_t step_key, long long particle, int b)
{
  return sub_key(cell_key(step_key, (long)particle), b);
}

// One collision (include/xpic_hip.h: xpic_collide) of v_a with v_b; cdt = S q_a^2 q_b^2 n_L dt / m_ab^2 of this pair,
// fa = m_ab / m_a, fb = m_ab / m_b; st: the stream state the three draws u1 u2 u3 come from (by value).  t: the tallies
// {collided, skipped, sum of sigma^2, sigma^2 > 1}, added to.  A caller that does not keep the partner passes a copy.
__device__ inline void collide_pair(double fa, double fb, double cdt, uint64_t st, double* va, double* vb, double* t)
{
#pragma clang fp contract(off)
  const double ux = va[0] - vb[0], uy = va[1] - vb[1], uz = va[2] - vb[2];
  const double u = sqrt(ux * ux + uy * uy + uz * uz);
  if (u == 0.0) {
    t[1] += 1.0;
    return;
  }
  const double s2 = cdt / (u * u * u);
  const double u1 = u01(st), u2 = u01(st), u3 = u01(st);
  const double delta = sqrt(s2) * sqrt(-2.0 * log(u1)) * cos(2.0 * M_PI * u2);
  const double phi = 2.0 * M_PI * u3;
  const double d2 = delta * delta;
  // sin Theta, 1 - cos Theta; a relative velocity so small that sigma^2 or delta^2 leaves the range of a double (or
  // comes within a factor of it: 2 delta^2 must not overflow) scatters by Theta = pi, the limit of both expressions,
  // which they have reached to the last place long before (inf / inf otherwise)
  const bool back = !(d2 <= 1e300);
  const double sinT = back ? 0.0 : 2.0 * delta / (1.0 + d2), omc = back ? 2.0 : 2.0 * d2 / (1.0 + d2);
  const double cp = cos(phi), sp = sin(phi);
  const double up = sqrt(ux * ux + uy * uy);
  double d[3];
  if (up == 0.0) {
    d[0] = u * sinT * cp;
    d[1] = u * sinT * sp;
    d[2] = -uz * omc;
  }
  else {
    d[0] = (ux / up) * uz * sinT * cp - (uy / up) * u * sinT * sp - ux * omc;
    d[1] = (uy / up) * uz * sinT * cp + (ux / up) * u * sinT * sp - uy * omc;
    d[2] = -up * sinT * cp - uz * omc;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    va[k] += fa * d[k];
    vb[k] -= fb * d[k];
  }
  t[0] += 1.0;
  if (s2 <= 1.79769313486231570815e308) t[2] += s2; // (an overflowed sigma^2 is counted above 1 and left out of the sum)
  if (s2 > 1.0) t[3] += 1.0;
}

}  // namespace

}  // namespace xpic
