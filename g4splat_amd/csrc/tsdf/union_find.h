// The lock-free union-find that mesh_ops.hip (triangle clusters) and plane_masks.hip (pixel components) share: the larger
// root is always linked under the smaller, so the root of a finished tree is the smallest member of its set whatever the
// interleaving.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace g4s {

__device__ inline uint32_t uf_load(const uint32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Root of x, halving the path on the way.  parent[i] <= i always, and only a root's word is ever the target of a CAS:
// the halving stores hit non-roots and write one of their ancestors, so they never change a tree's membership.
__device__ inline uint32_t uf_find(uint32_t* parent, uint32_t x) {
    for (;;) {
        const uint32_t p = uf_load(parent + x);
        if (p == x) return x;
        const uint32_t g = uf_load(parent + p);
        if (g == p) return p;
        __hip_atomic_store(parent + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        x = g;
    }
}

__device__ inline void uf_unite(uint32_t* parent, uint32_t a, uint32_t b) {
    for (;;) {
        a = uf_find(parent, a);
        b = uf_find(parent, b);
        if (a == b) return;
        if (a < b) {
            const uint32_t t = a;
            a = b;
            b = t;
        }
        if (atomicCAS(parent + a, a, b) == a) return;  // a was still a root: now below the smaller root
    }
}

}  // namespace g4s
