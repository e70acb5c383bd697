// The wave-level fold of integer counts that the units with integer count tables (planes.hip, consistency.hip,
// plane_masks.hip) share.  The fixed float64 fold of the units that sum in a fixed order (depth_cues.hip, plane_masks.hip),
// wave_fold, is in g4s_device.h beside the other wave sums.
#pragma once
#include "../g4s_device.h"

namespace g4s {

// table[key] += the number of active lanes that hold `key`, one atomic per distinct key of the wave.  Every lane of the wave
// must call it (inactive ones with active = false).
__device__ __forceinline__ void wave_count(uint32_t* __restrict__ table, uint32_t key, bool active) {
    unsigned long long todo = __ballot(active);
    while (todo != 0ull) {  // wave-uniform
        const int leader = __builtin_ctzll(todo);
        const uint32_t k = (uint32_t)__shfl((int)key, leader);
        const unsigned long long same = __ballot(active && key == k);
        if (lane_id() == leader) atomicAdd(table + k, (uint32_t)__builtin_popcountll(same));
        todo &= ~same;
    }
}

}  // namespace g4s
