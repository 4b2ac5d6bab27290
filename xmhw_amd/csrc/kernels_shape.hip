// kernels_shape.hip -- mhw_track_shape(): the outline of every selected object on each of its days.
// The footprint of object i on day t is the set of cells that hold a row of i covering t, as in kernels_parts.hip.  A
// footprint cell has four faces, in the order dim 0 minus, dim 0 plus, dim 1 minus, dim 1 plus; faces[c][4] names what
// lies across each: a compact cell (>= 0), kShapeFaceCoast (land), kShapeFaceBorder (no grid point) or
// kShapeFaceFolded (a wrapping dim of length 1: no face).  A face to a cell is *shared* when that cell is in the
// footprint of the same object on the same day -- nothing is counted -- and *open* otherwise.  Entry offsets[i] + (t -
// time_start[i]) of the ragged arrays of mhw_tracks() receives, for each of the classes open, coast and border, the
// number of such faces and the sum of their lengths lq[c][4], and the number of footprint cells with at least one such
// face.
//
//   memsets        the seven arrays and *n_bad = 0.
//   shape_walk     lane = row.  A coast or border face is the same on every day of the row.  For a face to a cell, a
//                  cursor into the rows of that cell: it starts at the first row with end >= start_r
//                  (first_row_reaching() of object_rows.h, row_offsets clamped to [0, n] there) and moves on while the
//                  row under it ends before the day; rows of a cell are in time order and disjoint, so the row under
//                  the cursor is the only one that can cover the day.  It covers iff it has the lane's slot, is itself fit and has started.
//                  The lane walks its days once, forms the seven addends of a day in registers and issues one integer
//                  atomic without a return value per addend that is not zero: a day on which every face is shared
//                  issues none.
//
// A row is *fit* under the one rule of object_rows.h, without voxels (fit_row<false>): its slot is in [0, n_slots), its cell
// in [0, C), start <= end, and its days lie within its object's entries (which lie within 0..L-1).  A selected row that
// is not fit is left out -- it neither adds nor covers -- and counted in *n_bad; so is, once, a fit row one of whose faces holds a
// value outside [kShapeFaceFolded, C) (that face is passed over).  Nothing outside entries 0..L-1 is ever written.
// Everything is an integer sum: exact, and the same under any schedule.
#include "device_common.h"
#include "kernels.h"
#include "object_rows.h"

namespace xmhw {

namespace {

using u64 = unsigned long long;

// the rows of the cell across one face: [j, last) are those that can still cover a day of the lane's row
struct ShapeCursor {
    int32_t j, last;
    int32_t s, e;                                    // the row under the cursor; s = INT32_MAX past the last row
    bool covers;                                     // it has the lane's slot and is fit
};

__device__ __forceinline__ void shape_cursor_load(const ObjectRows& a, int32_t slot, ShapeCursor& cur) {
    if (cur.j >= cur.last) {
        cur.s = cur.e = INT32_MAX;
        cur.covers = false;
        return;
    }
    cur.s = a.start[cur.j];
    cur.e = a.end[cur.j];
    ObjectRow other;
    cur.covers = a.slot[cur.j] == slot && fit_row<false>(a, cur.j, other) == 1;
}

__global__ __launch_bounds__(kRowThreads) void shape_walk(ObjectRows a, const int64_t* __restrict__ row_offsets,
                                                            const int32_t* __restrict__ faces,
                                                            const int64_t* __restrict__ lq, int32_t* __restrict__ edges,
                                                            u64* __restrict__ perimeter_q, int32_t* __restrict__ cells_edge,
                                                            int32_t* __restrict__ n_bad) {
    const int64_t r = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (r >= a.n) return;
    ObjectRow me;
    const int fit = fit_row<false>(a, r, me);
    if (fit < 0) atomicAdd(n_bad, 1);
    if (fit != 1) return;
    ShapeCursor cur[4];
    u64 len[4];
    bool to_cell[4];
    int32_t n_coast = 0, n_border = 0;
    u64 p_coast = 0, p_border = 0;
    bool bad_face = false;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int32_t f = faces[static_cast<int64_t>(me.c) * 4 + k];
        len[k] = static_cast<u64>(lq[static_cast<int64_t>(me.c) * 4 + k]);
        to_cell[k] = f >= 0 && f < a.C;
        cur[k] = ShapeCursor{0, 0, INT32_MAX, INT32_MAX, false};
        if (f == kShapeFaceCoast) {
            n_coast += 1;
            p_coast += len[k];
        } else if (f == kShapeFaceBorder) {
            n_border += 1;
            p_border += len[k];
        } else if (to_cell[k]) {
            int64_t last = row_offsets[f + 1];
            cur[k].j = static_cast<int32_t>(first_row_reaching(a.end, row_offsets[f], last, a.n, me.s));     // n < 2^31
            cur[k].last = static_cast<int32_t>(last);
            shape_cursor_load(a, me.sl, cur[k]);
        } else if (f != kShapeFaceFolded) {
            bad_face = true;
        }
    }
    if (bad_face) atomicAdd(n_bad, 1);
    int32_t* const e_open = edges + kShapeOpen * a.L;
    int32_t* const e_coast = edges + kShapeCoast * a.L;
    int32_t* const e_border = edges + kShapeBorder * a.L;
    u64* const p_open_at = perimeter_q + kShapeOpen * a.L;
    u64* const p_coast_at = perimeter_q + kShapeCoast * a.L;
    u64* const p_border_at = perimeter_q + kShapeBorder * a.L;
    const int64_t days = static_cast<int64_t>(me.e) - me.s + 1;
    for (int64_t d = 0; d < days; ++d) {
        const int32_t t = static_cast<int32_t>(me.s + d);
        int32_t n_open = 0;
        u64 p_open = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (!to_cell[k]) continue;
            while (cur[k].e < t) {                   // past the last row e = INT32_MAX: the loop ends there at the latest
                cur[k].j += 1;
                shape_cursor_load(a, me.sl, cur[k]);
            }
            if (!(cur[k].covers && cur[k].s <= t)) {
                n_open += 1;
                p_open += len[k];
            }
        }
        if (n_open + n_coast + n_border == 0) continue;
        const int64_t e = me.entry + d;              // within [offsets[slot], offsets[slot + 1]), itself within [0, L)
        atomicAdd(cells_edge + e, 1);
        if (n_open) atomicAdd(e_open + e, n_open);
        if (n_coast) atomicAdd(e_coast + e, n_coast);
        if (n_border) atomicAdd(e_border + e, n_border);
        if (p_open) atomicAdd(p_open_at + e, p_open);
        if (p_coast) atomicAdd(p_coast_at + e, p_coast);
        if (p_border) atomicAdd(p_border_at + e, p_border);
    }
}

}  // namespace

hipError_t launch_object_shape(const int32_t* start, const int32_t* end, const int32_t* slot, const int32_t* cell_of_row,
                               int64_t n, const int64_t* row_offsets, int64_t C, const int32_t* faces, const int64_t* lq,
                               const int32_t* time_start, const int64_t* offsets, int64_t n_slots, int64_t L, int32_t* edges,
                               int64_t* perimeter_q, int32_t* cells_edge, int32_t* n_bad, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(n_bad, 0, sizeof(int32_t), stream);
    if (e != hipSuccess) return e;
    if (L > 0) {
        e = hipMemsetAsync(edges, 0, sizeof(int32_t) * kShapeClasses * static_cast<size_t>(L), stream);
        if (e != hipSuccess) return e;
        e = hipMemsetAsync(perimeter_q, 0, sizeof(int64_t) * kShapeClasses * static_cast<size_t>(L), stream);
        if (e != hipSuccess) return e;
        e = hipMemsetAsync(cells_edge, 0, sizeof(int32_t) * static_cast<size_t>(L), stream);
        if (e != hipSuccess) return e;
    }
    if (n > 0 && n_slots > 0 && L > 0) {
        const ObjectRows rows{start, end, slot, cell_of_row, time_start, offsets, n, C, n_slots, L, nullptr, 0};
        hipLaunchKernelGGL(shape_walk, dim3(blocks_for(n)), dim3(kRowThreads), 0, stream, rows, row_offsets, faces, lq, edges,
                           reinterpret_cast<u64*>(perimeter_q), cells_edge, n_bad);
    }
    return hipGetLastError();
}

}  // namespace xmhw
