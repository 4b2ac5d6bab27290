// object_rows.h -- the one header of the object chain: the selected table rows as mhw_tracks() (kernels_tracks.hip,
// DESIGN.md 3.10), mhw_track_parts() (kernels_parts.hip, 3.12), mhw_track_genealogy() (kernels_genealogy.hip, 3.13) and
// mhw_track_shape() (kernels_shape.hip, 3.14) take them, the rule that says which of them may write which entry, and the
// search of a neighbour cell's rows.  kernels_objects.hip (3.8) takes only kRowThreads and blocks_for() from here.
//
// A voxel is a day of a selected row: voxel (r, t) has the number vox_off[r] + t - start[r].  Only the stages that number
// voxels (parts, genealogy) give vox_off and V; they ask for fit_row<true>, the others for fit_row<false>, which reads
// neither.
//
// A row is *fit* iff its slot is in [0, n_slots), its cell in [0, C), start <= end, its days lie within its object's
// entries (which lie within 0..L-1) and -- with voxels -- its voxel numbers vox_off[r] .. vox_off[r + 1] - 1 are exactly
// its days within [0, V).  A selected row that is not fit is left out of every kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace xmhw {

constexpr int kRowThreads = 256;                     // every kernel of the chain: lane = row (or voxel, entry, slot)

inline unsigned blocks_for(int64_t items) { return static_cast<unsigned>((items + kRowThreads - 1) / kRowThreads); }

struct ObjectRows {
    const int32_t *start, *end, *slot, *cell;
    const int32_t* time_start;
    const int64_t* offsets;
    int64_t n, C, n_slots, L;
    const int64_t* vox_off;                          // the voxel stages only (null and 0 elsewhere): kept last, so that a
    int64_t V;                                       // kernel without voxels finds everything it reads in front of them
};

struct ObjectRow {
    int32_t s, e, sl, c;
    int64_t vox;                                     // the voxel of day s (with voxels)
    int64_t entry;                                   // the entry of day s
};

// 1: the row is fit and `row` describes it; 0: its slot is outside the selection; -1: selected but not fit
template <bool VOXELS>
__device__ __forceinline__ int fit_row(const ObjectRows& a, int64_t r, ObjectRow& row) {
    const int32_t sl = a.slot[r];
    if (sl < 0 || sl >= a.n_slots) return 0;
    const int32_t s = a.start[r], e = a.end[r], c = a.cell[r];
    const int64_t v0 = VOXELS ? a.vox_off[r] : 0, v1 = VOXELS ? a.vox_off[r + 1] : 0;
    const int64_t o0 = a.offsets[sl], o1 = a.offsets[sl + 1], t0 = a.time_start[sl];
    const int64_t days = static_cast<int64_t>(e) - s + 1;
    const int64_t p0 = o0 + (static_cast<int64_t>(s) - t0);
    if (c < 0 || c >= a.C || days < 1 || (VOXELS && (v0 < 0 || v1 - v0 != days || v1 > a.V)) || o0 < 0 || o1 > a.L ||
        p0 < o0 || p0 + days > o1)
        return -1;
    row = ObjectRow{s, e, sl, c, v0, p0};
    return 1;
}

// The first row in [lo, last) whose end reaches `day` (end >= day); `last` where there is none.  The rows of a cell are
// in time order, so their ends ascend.  lo and last come from the row offsets of a cell: offsets that do not describe
// the rows read no row outside them, because both are clamped first, 0 <= lo <= last <= n (last in place).
__device__ __forceinline__ int64_t first_row_reaching(const int32_t* __restrict__ end, int64_t lo, int64_t& last, int64_t n,
                                                      int32_t day) {
    last = last < 0 ? 0 : (last > n ? n : last);
    lo = lo < 0 ? 0 : (lo > last ? last : lo);
    int64_t hi = last;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (end[mid] < day) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// The union-find on the voxels of the fit rows (kernels_parts.hip: parts_link, parts_flatten), for the stages that need
// the parts: parent[v] = v on entry, parent[v] = the smallest voxel of v's part on return.  V > 0.
void launch_parts_union(const ObjectRows& rows, const int64_t* row_offsets, const int32_t* nbr, int32_t K, int32_t* parent,
                        int64_t V, hipStream_t stream);

}  // namespace xmhw
