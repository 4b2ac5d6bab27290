// kernels_parts.hip -- mhw_track_parts(): into how many connected parts every selected object falls on each of its
// days.  The footprint of object i on day t is the set of cells that hold a row of i covering t; two
// footprint cells are adjacent iff one is among the other's K spatial neighbours nbr[c][K]; a part is a connected
// component.  Entry offsets[i] + (t - time_start[i]) of the ragged arrays of mhw_tracks() receives the number of parts,
// the cells of the part with the most cells and the largest sum of wq[c] over one part (two independent maxima).
//
// A voxel is a day of a selected row: voxel (r, t) has the number vox_off[r] + t - start[r], vox_off being the exclusive
// prefix sum of the durations of the selected rows (V voxels in all).  Per voxel: parent int32, cells int32, area int64.
//
//   parts_init     lane = voxel / entry: parent[v] = v, cells[v] = area[v] = 0; the three outputs = 0.
//   parts_link     lane = row.  For every neighbour cell nc < c (each pair is united once, from the larger cell, as in
//                  objects_link) a binary search of nc's rows for the first with end >= start_r, then a walk while
//                  start_j <= end_r.  A row of another slot is passed over (parts never join cells of different
//                  objects, whatever K the objects were built with); for every day of the overlap the two voxels are
//                  united.  The union-find is that of kernels_objects.hip (union_find.h): the smaller root wins by
//                  compare-and-swap, no wave waits for another.  Only voxels of one day are ever united.
//   parts_flatten  lane = voxel: parent[v] = find(v) (no union runs any more: the roots are final).
//   parts_reduce   lane = row, walking its days: cells[root] += 1, area[root] += wq[cell]; integer atomics without a
//                  return value.
//   parts_count    the same walk: a voxel that is its own root adds 1 to n_parts[e] and raises cells_largest[e] and
//                  area_largest_q[e] (an unsigned 64-bit maximum: areas are >= 0) by atomic maxima.
//
// The rows, the fit rule (fit_row<true>: with voxels) and the search of a neighbour cell's rows live in object_rows.h,
// shared with the other stages of the object chain.  parts_link and parts_flatten are also the union-find of
// kernels_genealogy.hip, which reaches them through launch_parts_union().  A selected row that is not fit is left out of
// every kernel and counted in *n_bad by parts_count; nothing outside entries 0..L-1 and voxels 0..V-1 is ever written.
// Everything is an integer sum or maximum: exact, and the same under any schedule.
#include "device_common.h"
#include "kernels.h"
#include "object_rows.h"
#include "union_find.h"

namespace xmhw {

namespace {

using u64 = unsigned long long;

__global__ __launch_bounds__(kRowThreads) void parts_init(int64_t V, int32_t* __restrict__ parent,
                                                           int32_t* __restrict__ cells, int64_t* __restrict__ area,
                                                           int64_t L, int32_t* __restrict__ n_parts,
                                                           int32_t* __restrict__ cells_largest,
                                                           int64_t* __restrict__ area_largest_q) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i < V) {
        parent[i] = static_cast<int32_t>(i);
        cells[i] = 0;
        area[i] = 0;
    }
    if (i < L) {
        n_parts[i] = 0;
        cells_largest[i] = 0;
        area_largest_q[i] = 0;
    }
}

__global__ __launch_bounds__(kRowThreads) void parts_link(ObjectRows a, const int64_t* __restrict__ row_offsets,
                                                          const int32_t* __restrict__ nbr, int32_t K,
                                                          int32_t* __restrict__ parent) {
    const int64_t r = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (r >= a.n) return;
    ObjectRow me;
    if (fit_row<true>(a, r, me) != 1) return;
    for (int32_t k = 0; k < K; ++k) {
        const int32_t nc = nbr[static_cast<int64_t>(me.c) * K + k];
        if (nc < 0 || nc >= me.c) continue;          // the pair is united from the side of the larger cell
        int64_t last = row_offsets[nc + 1];
        const int64_t first = first_row_reaching(a.end, row_offsets[nc], last, a.n, me.s);
        for (int64_t j = first; j < last && a.start[j] <= me.e; ++j) {
            if (a.slot[j] != me.sl) continue;        // another object, or not selected
            ObjectRow other;
            if (fit_row<true>(a, j, other) != 1) continue;
            const int32_t d0 = other.s > me.s ? other.s : me.s, d1 = other.e < me.e ? other.e : me.e;
            for (int32_t t = d0; t <= d1; ++t)       // fit rows: both voxels are within [0, V)
                unite(parent, static_cast<int32_t>(me.vox + (t - me.s)), static_cast<int32_t>(other.vox + (t - other.s)));
        }
    }
}

__global__ __launch_bounds__(kRowThreads) void parts_flatten(int64_t V, int32_t* __restrict__ parent) {
    const int64_t v = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (v >= V) return;
    int32_t x = static_cast<int32_t>(v);
    for (int32_t p = parent_load(parent + x); p != x; p = parent_load(parent + x)) x = p;
    __hip_atomic_store(parent + v, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(kRowThreads) void parts_reduce(ObjectRows a, const int64_t* __restrict__ wq,
                                                             const int32_t* __restrict__ parent,
                                                             int32_t* __restrict__ cells, u64* __restrict__ area) {
    const int64_t r = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (r >= a.n) return;
    ObjectRow me;
    if (fit_row<true>(a, r, me) != 1) return;
    const u64 w = static_cast<u64>(wq[me.c]);
    const int64_t days = static_cast<int64_t>(me.e) - me.s + 1;
    for (int64_t d = 0; d < days; ++d) {
        const int32_t root = parent[me.vox + d];     // a root is a voxel of a fit row of the same day: within [0, V)
        atomicAdd(cells + root, 1);
        if (w) atomicAdd(area + root, w);
    }
}

__global__ __launch_bounds__(kRowThreads) void parts_count(ObjectRows a, const int32_t* __restrict__ parent,
                                                            const int32_t* __restrict__ cells,
                                                            const u64* __restrict__ area, int32_t* __restrict__ n_parts,
                                                            int32_t* __restrict__ cells_largest,
                                                            u64* __restrict__ area_largest_q, int32_t* __restrict__ n_bad) {
    const int64_t r = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (r >= a.n) return;
    ObjectRow me;
    const int fit = fit_row<true>(a, r, me);
    if (fit < 0) atomicAdd(n_bad, 1);
    if (fit != 1) return;
    const int64_t days = static_cast<int64_t>(me.e) - me.s + 1;
    for (int64_t d = 0; d < days; ++d) {
        const int64_t v = me.vox + d;
        if (parent[v] != v) continue;
        const int64_t e = me.entry + d;              // within [offsets[slot], offsets[slot + 1]), itself within [0, L)
        atomicAdd(n_parts + e, 1);
        atomicMax(cells_largest + e, cells[v]);
        atomicMax(area_largest_q + e, area[v]);
    }
}

}  // namespace

void launch_parts_union(const ObjectRows& rows, const int64_t* row_offsets, const int32_t* nbr, int32_t K, int32_t* parent,
                        int64_t V, hipStream_t stream) {
    hipLaunchKernelGGL(parts_link, dim3(blocks_for(rows.n)), dim3(kRowThreads), 0, stream, rows, row_offsets, nbr, K, parent);
    hipLaunchKernelGGL(parts_flatten, dim3(blocks_for(V)), dim3(kRowThreads), 0, stream, V, parent);
}

size_t object_parts_scratch_bytes(int64_t V) { return static_cast<size_t>(kPartsVoxelBytes) * static_cast<size_t>(V > 0 ? V : 1); }

hipError_t launch_object_parts(const int32_t* start, const int32_t* end, const int32_t* slot, const int32_t* cell_of_row,
                               int64_t n, const int64_t* row_offsets, int64_t C, const int32_t* nbr, int32_t K,
                               const int64_t* wq, const int64_t* vox_off, int64_t V, const int32_t* time_start,
                               const int64_t* offsets, int64_t n_slots, int64_t L, int32_t* n_parts, int32_t* cells_largest,
                               int64_t* area_largest_q, int32_t* n_bad, void* scratch, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(n_bad, 0, sizeof(int32_t), stream);
    if (e != hipSuccess) return e;
    // the 64-bit sums first (8-byte aligned), then the two 32-bit arrays
    int64_t* area = static_cast<int64_t*>(scratch);
    int32_t* parent = reinterpret_cast<int32_t*>(area + (V > 0 ? V : 0));
    int32_t* cells = parent + (V > 0 ? V : 0);
    const int64_t items = V > L ? V : L;
    if (items > 0)
        hipLaunchKernelGGL(parts_init, dim3(blocks_for(items)), dim3(kRowThreads), 0, stream, V, parent, cells, area, L, n_parts,
                           cells_largest, area_largest_q);
    if (n > 0 && n_slots > 0 && L > 0) {
        const ObjectRows rows{start, end, slot, cell_of_row, time_start, offsets, n, C, n_slots, L, vox_off, V};
        const dim3 g(blocks_for(n)), b(kRowThreads);
        if (V > 0) {
            launch_parts_union(rows, row_offsets, nbr, K, parent, V, stream);
            hipLaunchKernelGGL(parts_reduce, g, b, 0, stream, rows, wq, static_cast<const int32_t*>(parent), cells,
                               reinterpret_cast<u64*>(area));
        }
        hipLaunchKernelGGL(parts_count, g, b, 0, stream, rows, static_cast<const int32_t*>(parent),
                           static_cast<const int32_t*>(cells), reinterpret_cast<const u64*>(area), n_parts, cells_largest,
                           reinterpret_cast<u64*>(area_largest_q), n_bad);
    }
    return hipGetLastError();
}

}  // namespace xmhw
