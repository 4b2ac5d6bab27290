// parts_rows.h -- the rows, the voxels and the union-find passes shared by kernels_parts.hip (mhw_track_parts(), DESIGN.md
// 3.12) and kernels_genealogy.hip (mhw_track_genealogy(), 3.13).  A voxel is a day of a selected row: voxel (r, t) has the
// number vox_off[r] + t - start[r].  parts_link_row() unites the voxels of one row with those of its neighbour cells,
// one day at a time; parts_flatten_voxel() points a voxel at its root once no union runs any more.  Both files wrap them
// in kernels of their own (lane = row, lane = voxel).
//
// A row is *fit* iff its slot is in [0, n_slots), its cell in [0, C), start <= end, its days lie within its object's
// entries (which lie within 0..L-1) and its voxel numbers vox_off[r] .. vox_off[r + 1] - 1 are exactly its days within
// [0, V).  A selected row that is not fit is left out of every kernel.
#pragma once
#include "union_find.h"

namespace xmhw {

struct PartRows {
    const int32_t *start, *end, *slot, *cell;
    const int64_t* vox_off;
    const int32_t* time_start;
    const int64_t* offsets;
    int64_t n, C, n_slots, L, V;
};

struct PartRow {
    int32_t s, e, sl, c;
    int64_t vox;                                     // the voxel of day s
    int64_t entry;                                   // the entry of day s
};

// 1: the row is fit and `row` describes it; 0: its slot is outside the selection; -1: selected but not fit
__device__ __forceinline__ int part_row(const PartRows& a, int64_t r, PartRow& row) {
    const int32_t sl = a.slot[r];
    if (sl < 0 || sl >= a.n_slots) return 0;
    const int32_t s = a.start[r], e = a.end[r], c = a.cell[r];
    const int64_t v0 = a.vox_off[r], v1 = a.vox_off[r + 1];
    const int64_t o0 = a.offsets[sl], o1 = a.offsets[sl + 1], t0 = a.time_start[sl];
    const int64_t days = static_cast<int64_t>(e) - s + 1;
    const int64_t p0 = o0 + (static_cast<int64_t>(s) - t0);
    if (c < 0 || c >= a.C || days < 1 || v0 < 0 || v1 - v0 != days || v1 > a.V || o0 < 0 || o1 > a.L || p0 < o0 ||
        p0 + days > o1)
        return -1;
    row = PartRow{s, e, sl, c, v0, p0};
    return 1;
}

// lane = row r < a.n
__device__ __forceinline__ void parts_link_row(const PartRows& a, int64_t r, const int64_t* __restrict__ row_offsets,
                                               const int32_t* __restrict__ nbr, int32_t K, int32_t* __restrict__ parent) {
    PartRow me;
    if (part_row(a, r, me) != 1) return;
    for (int32_t k = 0; k < K; ++k) {
        const int32_t nc = nbr[static_cast<int64_t>(me.c) * K + k];
        if (nc < 0 || nc >= me.c) continue;          // the pair is united from the side of the larger cell
        int64_t lo = row_offsets[nc], last = row_offsets[nc + 1];
        lo = lo < 0 ? 0 : lo;                        // offsets that do not describe the rows read no row outside them
        last = last > a.n ? a.n : last;
        int64_t hi = last;
        while (lo < hi) {                            // the first row of nc with end >= start
            const int64_t mid = lo + (hi - lo) / 2;
            if (a.end[mid] < me.s) lo = mid + 1; else hi = mid;
        }
        for (int64_t j = lo; j < last && a.start[j] <= me.e; ++j) {
            if (a.slot[j] != me.sl) continue;        // another object, or not selected
            PartRow other;
            if (part_row(a, j, other) != 1) continue;
            const int32_t d0 = other.s > me.s ? other.s : me.s, d1 = other.e < me.e ? other.e : me.e;
            for (int32_t t = d0; t <= d1; ++t)       // fit rows: both voxels are within [0, V)
                unite(parent, static_cast<int32_t>(me.vox + (t - me.s)), static_cast<int32_t>(other.vox + (t - other.s)));
        }
    }
}

// lane = voxel v < V
__device__ __forceinline__ void parts_flatten_voxel(int64_t v, int32_t* __restrict__ parent) {
    int32_t x = static_cast<int32_t>(v);
    for (int32_t p = parent_load(parent + x); p != x; p = parent_load(parent + x)) x = p;
    __hip_atomic_store(parent + v, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace xmhw
