// collide_perm.h -- the per-cell permutation of the binary collisions and the wave-level hand-over it needs: shared by
// collide.hip (xpic_collide) and collide_weighted.hip (xpic_collide_weighted), which rank the records of a cell in the
// same way from the same keys.  Included after collide_pair.h (item_key).  Device code only.
#pragma once

#include "device_common.h"
#include "collide_pair.h"

namespace xpic {

namespace {

// what one lane wrote is read by the other lanes of its wave: LDS operations of a wave complete in order, the fence keeps
// the compiler from moving them; the second path's slots go through global memory
template <bool LDS>
__device__ inline void wave_sync()
{
  if (LDS) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
  else __threadfence();
}

// slot[rank of record i] = i for the n records of a cell, ordered by (key, i)
template <bool LDS>
__device__ inline void permute(uint64_t sub, int n, uint64_t* keys, int* slot, int lane)
{
  if (LDS) {
    for (int i = lane; i < n; i += 64) keys[i] = item_key(sub, i);
    wave_sync<LDS>();
  }
  for (int i = lane; i < n; i += 64) {
    const uint64_t ki = LDS ? keys[i] : item_key(sub, i);
    int r = 0;
    for (int j = 0; j < n; ++j) {
      const uint64_t kj = LDS ? keys[j] : item_key(sub, j);
      r += (kj < ki || (kj == ki && j < i)) ? 1 : 0;
    }
    slot[r] = i;
  }
  wave_sync<LDS>(); // (the slots are read, and the keys rewritten, by other lanes)
}

}  // namespace

}  // namespace xpic
