// union_find.h -- the lock-free union-find shared by kernels_objects.hip (on table rows) and kernels_parts.hip (on the
// voxels of one day; kernels_genealogy.hip runs that one through launch_parts_union() of object_rows.h).  parent[x] <= x always, so a tree's root is
// its smallest member under any schedule.  find_root() reads with relaxed agent-scope atomic loads and shortens the path
// behind it (any value ever stored in parent[x] is an ancestor of x).  unite() puts the larger root under the smaller by
// a compare-and-swap that succeeds only while the target is still its own parent; on failure both ends are found again.
// No wave waits for another: a failed compare-and-swap means another lane made progress.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace xmhw {

__device__ __forceinline__ int32_t parent_load(const int32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ int32_t find_root(int32_t* __restrict__ parent, int32_t x) {
    int32_t p = parent_load(parent + x);
    while (p != x) {                                 // parent[x] < x for every non-root: the walk ends
        const int32_t gp = parent_load(parent + p);
        if (gp != p) __hip_atomic_store(parent + x, gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        x = p;
        p = gp;
    }
    return x;
}

__device__ __forceinline__ void unite(int32_t* __restrict__ parent, int32_t a, int32_t b) {
    for (;;) {
        a = find_root(parent, a);
        b = find_root(parent, b);
        if (a == b) return;
        if (a < b) { const int32_t t = a; a = b; b = t; }
        int32_t expected = a;                        // only a root may be linked: a stale root is found again
        if (__hip_atomic_compare_exchange_strong(parent + a, &expected, b, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT))
            return;
    }
}

}  // namespace xmhw
