// kernels_objects.hip -- mhw_objects(): the per-cell events of detect() grouped into objects connected in space
// and time.  A table row is a run of days [start, end] in one ocean cell; two rows are linked iff their cells are
// different spatial neighbours (nbr[c][K]) and start_a <= end_b + gap and start_b <= end_a + gap.  The connected
// components of that graph are the connected components of the rasterised (time, y, x) voxels.
//
//   objects_init     lane = row: parent[r] = r, cell_of_row[r] = the cell whose offsets hold r (a binary search; the
//                    lanes of a wave walk almost the same path through offsets).
//   objects_link     lane = row.  Rows are numbered cell by cell, so every row of a neighbour cell nc < c is smaller
//                    than the lane's own: only those neighbours are searched, which unites every pair exactly once.
//                    Per neighbour: a binary search of its rows (in time order, ends increasing) for the first with
//                    end >= start - gap, then a walk while start' <= end + gap.  unite() (union_find.h) is a lock-free union-find:
//                    the larger root goes under the smaller by a compare-and-swap that succeeds only while the target
//                    is still its own parent; on failure both ends are found again.  parent[x] <= x always, so a
//                    tree's root is its smallest row under any schedule.  find() reads with relaxed agent-scope atomic
//                    loads and shortens the path behind it (any value ever stored in parent[x] is an ancestor of x).
//                    No wave waits for another: a failed compare-and-swap means another lane made progress.
//   objects_flatten  root[r] = find(r), in place (no union runs any more: the roots are final).
//   objects_reduce   lane = row, a wave owns kObjChunks x 64 consecutive rows.  Rows that follow each other with the
//                    same slot (object) form a run; the runs of a chunk are reduced together by one segmented scan
//                    (shuffles), the run that is still open at the end of a chunk is carried into the next one, and
//                    only the end of a run issues atomics: one set per run, so an object of every row costs one set
//                    per kObjChunks x 64 rows instead of one per row.  Sums, minima and maxima are integers; the
//                    float maximum is an integer maximum of the order-preserving key of device_common.h.
//   objects_peak     the smallest row whose key equals its object's maximum (a read in front of the atomic minimum:
//                    rows arrive roughly in order, so a large tie does not queue on one address).
//   the finish       key -> float64 (NaN where no row had a value): launch_keys_to_f64 (kernels.h).
#include "device_common.h"
#include "kernels.h"
#include "object_rows.h"                           // kRowThreads, blocks_for
#include "union_find.h"                             // parent_load, find_root, unite

namespace xmhw {

namespace {

constexpr int kObjThreads = kRowThreads;
constexpr int kObjChunks = 8;                       // chunks of 64 rows per wave in objects_reduce

__global__ __launch_bounds__(kObjThreads) void objects_init(const int64_t* __restrict__ offsets, int64_t C, int64_t n,
                                                            int32_t* __restrict__ cell_of_row,
                                                            int32_t* __restrict__ parent) {
    const int64_t r = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (r >= n) return;
    int64_t lo = 0, hi = C;                          // the largest c with offsets[c] <= r (empty cells are passed over)
    while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (offsets[mid] <= r) lo = mid; else hi = mid;
    }
    cell_of_row[r] = static_cast<int32_t>(lo);
    parent[r] = static_cast<int32_t>(r);
}

__global__ __launch_bounds__(kObjThreads) void objects_link(const int32_t* __restrict__ start,
                                                            const int32_t* __restrict__ end,
                                                            const int64_t* __restrict__ offsets,
                                                            const int32_t* __restrict__ cell_of_row,
                                                            const int32_t* __restrict__ nbr, int32_t K, int32_t gap,
                                                            int64_t n, int32_t* __restrict__ parent) {
    const int64_t r = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const int32_t c = cell_of_row[r];
    const int64_t s = static_cast<int64_t>(start[r]) - gap, e = static_cast<int64_t>(end[r]) + gap;
    for (int32_t k = 0; k < K; ++k) {
        const int32_t nc = nbr[static_cast<int64_t>(c) * K + k];
        if (nc < 0 || nc >= c) continue;             // the pair is united from the side of the larger cell
        int64_t lo = offsets[nc];
        const int64_t last = offsets[nc + 1];
        int64_t hi = last;
        while (lo < hi) {                            // the first row of nc with end >= s
            const int64_t mid = lo + (hi - lo) / 2;
            if (end[mid] < s) lo = mid + 1; else hi = mid;
        }
        for (int64_t j = lo; j < last && start[j] <= e; ++j) unite(parent, static_cast<int32_t>(r), static_cast<int32_t>(j));
    }
}

__global__ __launch_bounds__(kObjThreads) void objects_flatten(int64_t n, int32_t* __restrict__ parent) {
    const int64_t r = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (r >= n) return;
    int32_t x = static_cast<int32_t>(r);
    for (int32_t p = parent_load(parent + x); p != x; p = parent_load(parent + x)) x = p;
    __hip_atomic_store(parent + r, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

struct ObjPart {
    int32_t cnt, cells, tmin, tmax;
    unsigned long long days, area, key;
};

__device__ __forceinline__ void combine(ObjPart& a, const ObjPart& b) {
    a.cnt += b.cnt;
    a.cells += b.cells;
    a.tmin = b.tmin < a.tmin ? b.tmin : a.tmin;
    a.tmax = b.tmax > a.tmax ? b.tmax : a.tmax;
    a.days += b.days;
    a.area += b.area;
    a.key = b.key > a.key ? b.key : a.key;
}

__device__ __forceinline__ unsigned long long shfl_u64(unsigned long long v, int src) {
    return static_cast<unsigned long long>(__shfl(static_cast<long long>(v), src, 64));
}

__device__ __forceinline__ ObjPart shfl_part(const ObjPart& p, int src) {
    ObjPart q;
    q.cnt = __shfl(p.cnt, src, 64);
    q.cells = __shfl(p.cells, src, 64);
    q.tmin = __shfl(p.tmin, src, 64);
    q.tmax = __shfl(p.tmax, src, 64);
    q.days = shfl_u64(p.days, src);
    q.area = shfl_u64(p.area, src);
    q.key = shfl_u64(p.key, src);
    return q;
}

struct ObjSlots {
    int32_t *n_events, *n_cells, *time_start, *time_end;
    unsigned long long *cell_days, *area_q, *key;
};

__device__ __forceinline__ void flush(const ObjSlots& o, int32_t slot, const ObjPart& p) {
    atomicAdd(o.n_events + slot, p.cnt);
    if (p.cells) atomicAdd(o.n_cells + slot, p.cells);
    atomicMin(o.time_start + slot, p.tmin);
    atomicMax(o.time_end + slot, p.tmax);
    atomicAdd(o.cell_days + slot, p.days);
    if (p.area) atomicAdd(o.area_q + slot, p.area);
    if (p.key) atomicMax(o.key + slot, p.key);
}

__global__ __launch_bounds__(kObjThreads) void objects_reduce(
    const int32_t* __restrict__ start, const int32_t* __restrict__ end, const double* __restrict__ imax, int64_t n,
    const int32_t* __restrict__ cell_of_row, const int64_t* __restrict__ offsets, const int64_t* __restrict__ wq,
    const int32_t* __restrict__ slot, int64_t n_slots, ObjSlots out) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
    const int64_t base = wave * (64 * kObjChunks);
    int32_t cslot = -1;                              // the run left open by the previous chunk (uniform over the wave)
    ObjPart carry{};
    for (int ch = 0; ch < kObjChunks; ++ch) {
        const int64_t r0 = base + ch * 64;
        if (r0 >= n) break;                          // uniform over the wave
        const int64_t r = r0 + lane;
        int32_t sl = -2;                             // no row, or a slot outside [0, n_slots): belongs to no run that is flushed
        ObjPart p{0, 0, 0x7FFFFFFF, -1, 0ull, 0ull, 0ull};
        if (r < n) {
            const int32_t s0 = slot[r];
            if (s0 >= 0 && s0 < n_slots) {
                sl = s0;
                const int32_t c = cell_of_row[r];
                const int32_t a = start[r], b = end[r];
                const unsigned long long d = static_cast<unsigned long long>(static_cast<int64_t>(b) - a + 1);
                int32_t first = 1;                   // no earlier row of the cell is in this object
                for (int64_t j = r - 1, j0 = offsets[c]; j >= j0; --j)
                    if (slot[j] == sl) { first = 0; break; }
                p.cnt = 1;
                p.cells = first;
                p.tmin = a;
                p.tmax = b;
                p.days = d;
                p.area = static_cast<unsigned long long>(wq[c]) * d;
                p.key = f64_key(imax[r] + 0.0);      // -0.0 counts as 0.0; NaN -> 0, below every value
            }
        }
        const int32_t prev = __shfl_up(sl, 1, 64);
        const bool head = lane == 0 || prev != sl;
        const uint64_t heads = __ballot(head);
        const int first_lane = 63 - __builtin_clzll(heads & (~uint64_t{0} >> (63 - lane)));   // where the lane's run starts
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const ObjPart q = shfl_part(p, lane >= d ? lane - d : lane);
            if (lane - d >= first_lane) combine(p, q);
        }
        const int32_t next = __shfl_down(sl, 1, 64);
        const bool tail = lane == 63 || next != sl;  // holds its run's total
        if (cslot >= 0) {
            const int32_t s_first = __shfl(sl, 0, 64);
            if (cslot == s_first) {
                if (tail && first_lane == 0) combine(p, carry);
            } else if (lane == 0) {
                flush(out, cslot, carry);
            }
        }
        if (tail && lane != 63 && sl >= 0) flush(out, sl, p);
        cslot = __shfl(sl, 63, 64);
        carry = shfl_part(p, 63);
    }
    if (cslot >= 0 && lane == 0) flush(out, cslot, carry);
}

__global__ __launch_bounds__(kObjThreads) void objects_peak(const double* __restrict__ imax, int64_t n,
                                                            const int32_t* __restrict__ slot, int64_t n_slots,
                                                            const unsigned long long* __restrict__ key,
                                                            uint32_t* __restrict__ peak_row) {
    const int64_t r = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const int32_t sl = slot[r];
    if (sl < 0 || sl >= n_slots) return;
    const unsigned long long k = f64_key(imax[r] + 0.0);
    if (k == 0 || k != key[sl]) return;
    const uint32_t row = static_cast<uint32_t>(r);
    if (row < __hip_atomic_load(peak_row + sl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(peak_row + sl, row);
}

}  // namespace

hipError_t launch_event_objects(const int32_t* start, const int32_t* end, int64_t n, const int64_t* offsets, int64_t C,
                                const int32_t* nbr, int32_t K, int32_t gap, int32_t* cell_of_row, int32_t* root,
                                hipStream_t stream) {
    if (n <= 0 || C <= 0) return hipSuccess;
    const unsigned g = blocks_for(n);
    hipLaunchKernelGGL(objects_init, dim3(g), dim3(kObjThreads), 0, stream, offsets, C, n, cell_of_row, root);
    hipLaunchKernelGGL(objects_link, dim3(g), dim3(kObjThreads), 0, stream, start, end, offsets, cell_of_row, nbr, K, gap,
                       n, root);
    hipLaunchKernelGGL(objects_flatten, dim3(g), dim3(kObjThreads), 0, stream, n, root);
    return hipGetLastError();
}

hipError_t launch_object_reduce(const int32_t* start, const int32_t* end, const double* imax, int64_t n,
                                const int32_t* cell_of_row, const int64_t* offsets, const int64_t* wq,
                                const int32_t* slot, int64_t n_slots, int32_t* n_events, int32_t* n_cells,
                                int32_t* time_start, int32_t* time_end, int64_t* cell_days, int64_t* area_days_q,
                                double* intensity_max, int32_t* peak_row, hipStream_t stream) {
    if (n_slots <= 0) return hipSuccess;
    const size_t m = static_cast<size_t>(n_slots);
    hipError_t e = hipMemsetAsync(n_events, 0, sizeof(int32_t) * m, stream);
    if (e == hipSuccess) e = hipMemsetAsync(n_cells, 0, sizeof(int32_t) * m, stream);
    if (e == hipSuccess) e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(time_start), 0x7FFFFFFF, m, stream);
    if (e == hipSuccess) e = hipMemsetAsync(time_end, 0xFF, sizeof(int32_t) * m, stream);          // -1
    if (e == hipSuccess) e = hipMemsetAsync(cell_days, 0, sizeof(int64_t) * m, stream);
    if (e == hipSuccess) e = hipMemsetAsync(area_days_q, 0, sizeof(int64_t) * m, stream);
    if (e == hipSuccess) e = hipMemsetAsync(intensity_max, 0, sizeof(double) * m, stream);        // key 0: no value yet
    if (e == hipSuccess) e = hipMemsetAsync(peak_row, 0xFF, sizeof(int32_t) * m, stream);          // -1 = the largest uint32
    if (e != hipSuccess) return e;
    unsigned long long* key = reinterpret_cast<unsigned long long*>(intensity_max);
    if (n > 0) {
        ObjSlots out{n_events, n_cells, time_start, time_end, reinterpret_cast<unsigned long long*>(cell_days),
                     reinterpret_cast<unsigned long long*>(area_days_q), key};
        const int64_t waves = (n + 64 * kObjChunks - 1) / (64 * kObjChunks);
        hipLaunchKernelGGL(objects_reduce, dim3(blocks_for(waves * 64)), dim3(kObjThreads), 0, stream, start, end, imax, n,
                           cell_of_row, offsets, wq, slot, n_slots, out);
        hipLaunchKernelGGL(objects_peak, dim3(blocks_for(n)), dim3(kObjThreads), 0, stream, imax, n, slot, n_slots, key,
                           reinterpret_cast<uint32_t*>(peak_row));
    }
    return launch_keys_to_f64(intensity_max, 1, n_slots, n_slots, stream);
}

}  // namespace xmhw
