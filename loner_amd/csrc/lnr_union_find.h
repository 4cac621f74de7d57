// The lock-free union-find of the connected components (lnr_mesh_tools.hip: triangles over shared edges; lnr_cloud_segment.hip: core
// points within eps).  The larger root is hooked under the smaller by compare-and-swap; a failed swap means another lane hooked that
// root, and the loop goes on from what it found there: no lane waits for another.  A root is therefore its component's smallest member.
// Integer atomics only, which commute: the roots are a function of the links, not of the order the lanes ran in.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

// parents are read past the per-CU cache: a lane must see the hooks of other CUs, or it would retry on a stale root for ever
__device__ inline uint32_t uf_load(uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root above x.  A parent is smaller than its child (uf_unite), so the walk ends whatever other lanes do meanwhile; on the way each
// node is pointed at its grandparent (atomicMin: an ancestor, and never above a closer one written since)
__device__ inline uint32_t uf_find(uint32_t* parent, uint32_t x) {
    for (;;) {
        const uint32_t p = uf_load(parent + x);
        if (p == x) return x;
        const uint32_t g = uf_load(parent + p);
        if (g != p) atomicMin(parent + x, g);
        x = p;
    }
}

// max(a, b) falls with every failed swap, so the loop ends; it never waits for another lane
__device__ inline void uf_unite(uint32_t* parent, uint32_t a, uint32_t b) {
    for (;;) {
        a = uf_find(parent, a);
        b = uf_find(parent, b);
        if (a == b) return;
        if (a < b) { const uint32_t s = a; a = b; b = s; }
        const uint32_t old = atomicCAS(parent + a, a, b);
        if (old == a) return;
        a = old;                                                        // a was hooked meanwhile, under old < a
    }
}

}  // namespace
