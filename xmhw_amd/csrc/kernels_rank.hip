// kernels_rank.hip -- mhw_rank() (xmhw/stats.py:446-510, Hobday's marineHeatWaves.rank()).
//
// Within every ocean cell, every ranked column of the compact event table of detect() is ranked from the
// largest value (rank 1) down, ties broken by position (the later event gets the smaller rank):
//     rank_i = 1 + #{j : v_j > v_i} + #{j > i : v_j == v_i}       (= N - argsort(argsort(v, kind="stable")))
// compared as float64 (-0.0 == 0.0); a NaN value has a NaN rank and takes no part in the others' counts.
// The return period is (n_years + 1) / rank, one float64 division.
//
// Work is cut into items of 64 events of one cell (one wave each, lane = event): item w of the exclusive
// scan item_off of ceil(n_c / 64) belongs to cell c with item_off[c] <= w < item_off[c + 1].  An item
// copies its 64 rows of the table into LDS (coalesced row segments: only the window [cmin, cmin + span) of
// columns that holds the ranked ones), takes its own values into registers, then counts over the cell's
// events 64 rows at a time, every row j read by all lanes at once (an LDS broadcast).  A cell of n <= 64
// events is one item and one copy; a large cell is spread over ceil(n / 64) waves, each O(n).  The ranks go
// back through LDS and leave as contiguous output rows.
// The grid is persistent (twice as many one-wave workgroups as fit at once); a wave takes its next item from a
// counter (one atomic per item), so a wave held up by the items of a large cell leaves the rest to the others.
#include "device_common.h"
#include "kernels.h"

namespace xmhw {
namespace {

constexpr int kItem = 64;                 // events per work item = lanes of the wave
constexpr int kMaxCols = kRankWindow;     // ranked columns of one launch (a window of at most 16 table columns)

__global__ __launch_bounds__(256) void rank_item_counts(const int64_t* __restrict__ offsets, int64_t C,
                                                        int32_t* __restrict__ counts) {
    const int64_t c = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const int64_t n = offsets[c + 1] - offsets[c];
    counts[c] = static_cast<int32_t>((n + kItem - 1) / kItem);
}

// the cell of item w (item_off[c] <= w < item_off[c + 1]), found by the whole wave: each round the 64 lanes
// probe 64 evenly spaced entries of [lo, hi) and keep the stretch between the last probe <= w and the next,
// so a quarter of a million cells take three rounds of dependent loads instead of eighteen
__device__ __forceinline__ int64_t item_cell(const int64_t* __restrict__ item_off, int64_t C, int64_t w, int lane) {
    int64_t lo = 0, hi = C;                        // item_off[lo] <= w < item_off[hi]
    while (hi - lo > 1) {
        const int64_t step = (hi - lo + kItem - 1) / kItem;
        const int64_t idx = lo + lane * step;      // lane 0 probes lo itself: always <= w
        const bool ok = idx < hi && item_off[idx] <= w;
        const uint64_t m = __ballot(ok);
        const int k = 63 - __builtin_clzll(m);
        lo += k * step;
        hi = lo + step < hi ? lo + step : hi;
    }
    return lo;
}

// rows [0, rows) of src (leading dimension ld, from the window's first column) -> tile[row * kMaxCols + col]:
// each pass the wave copies kPass rows, lane % kMaxCols = the column
constexpr int kPass = kItem / kMaxCols;
__device__ __forceinline__ void stage_rows(double* __restrict__ tile, const double* __restrict__ src, int64_t ld,
                                           int rows, int span, int lane) {
    const int col = lane % kMaxCols;
#pragma unroll 4
    for (int r = lane / kMaxCols; r < rows; r += kPass)
        if (col < span) tile[r * kMaxCols + col] = src[static_cast<int64_t>(r) * ld + col];
}

// adds to cnt[k] the rows j of the tile that rank above the lane's own event for column k.
// MODE 0: every row of the tile comes before every own event (count v_j > v_i); 2: after (v_j >= v_i);
// 1: the tile is the item's own rows (row jj follows the lane's event iff jj > lane)
template <int MODE>
__device__ __forceinline__ void count_tile(const double* __restrict__ tile, int rows, const RankColumns& rc,
                                           const double (&v)[kMaxCols], int32_t (&cnt)[kMaxCols], int lane) {
#pragma unroll
    for (int k = 0; k < kMaxCols; ++k) {
        if (k < rc.ncols) {
            const double* col = tile + (rc.col[k] - rc.cmin);
            const double x = v[k];
            int32_t s = 0;
            for (int jj = 0; jj < rows; ++jj) {
                const double y = col[jj * kMaxCols];     // the same address in every lane: a broadcast
                if (MODE == 0) s += y > x;
                else if (MODE == 2) s += y >= x;
                else s += (y > x) | ((y == x) & (jj > lane));
            }
            cnt[k] += s;
        }
    }
}

__global__ __launch_bounds__(kItem) void event_rank(const double* __restrict__ table, int64_t ld_table,
                                                    const int64_t* __restrict__ offsets,
                                                    const int64_t* __restrict__ item_off, int64_t C, RankColumns rc,
                                                    double n_years, double* __restrict__ rank, double* __restrict__ rp,
                                                    int64_t ld_out, unsigned long long* __restrict__ next_item) {
    // kItem rows of the column window, then kItem rows of ranks; the fixed row stride lets the unrolled
    // count loop address its rows by immediate offsets
    __shared__ double tile[kItem * kMaxCols];
    __shared__ int32_t out_col[kMaxCols];
    const int lane = threadIdx.x;
#pragma unroll
    for (int k = 0; k < kMaxCols; ++k)
        if (lane == k) out_col[k] = rc.out[k];
    const int span = rc.span;
    const int ncols = rc.ncols;
    const double np1 = n_years + 1.0;
    const int64_t total = item_off[C];
    for (;;) {
        unsigned long long got = 0;
        if (lane == 0) got = atomicAdd(next_item, 1ull);
        const int64_t w = static_cast<int64_t>(__shfl(got, 0, kItem));
        if (w >= total) break;
        const int64_t c = item_cell(item_off, C, w, lane);
        const int64_t r0 = offsets[c];
        const int64_t n = offsets[c + 1] - r0;
        const int64_t q = w - item_off[c];         // the item's place in its cell
        const int64_t i0 = q * kItem;
        const int m = static_cast<int>(n - i0 < kItem ? n - i0 : kItem);
        __syncthreads();                           // the previous item is done with the tile
        stage_rows(tile, table + (r0 + i0) * ld_table + rc.cmin, ld_table, m, span, lane);
        __syncthreads();
        double v[kMaxCols];
        int32_t cnt[kMaxCols];
#pragma unroll
        for (int k = 0; k < kMaxCols; ++k) {
            v[k] = (k < ncols && lane < m) ? tile[lane * kMaxCols + (rc.col[k] - rc.cmin)] : make_nan();
            cnt[k] = 0;
        }
        count_tile<1>(tile, m, rc, v, cnt, lane);
        // the cell's other rows, 64 at a time
        const int64_t ntiles = (n + kItem - 1) / kItem;
        for (int64_t t = 0; t < ntiles; ++t) {
            if (t == q) continue;
            const int64_t j0 = t * kItem;
            const int mj = static_cast<int>(n - j0 < kItem ? n - j0 : kItem);
            __syncthreads();
            stage_rows(tile, table + (r0 + j0) * ld_table + rc.cmin, ld_table, mj, span, lane);
            __syncthreads();
            if (t < q) count_tile<0>(tile, mj, rc, v, cnt, lane);
            else count_tile<2>(tile, mj, rc, v, cnt, lane);
        }
        // ranks -> tile[row * kMaxCols + k] -> whole output rows
        __syncthreads();
        if (lane < m) {
#pragma unroll
            for (int k = 0; k < kMaxCols; ++k)
                if (k < ncols) tile[lane * kMaxCols + k] = v[k] == v[k] ? 1.0 + static_cast<double>(cnt[k]) : make_nan();
        }
        __syncthreads();
        const int k = lane % kMaxCols;
        if (k < ncols) {
            const int64_t oc = out_col[k];
            for (int r = lane / kMaxCols; r < m; r += kPass) {
                const double x = tile[r * kMaxCols + k];
                const int64_t o = (r0 + i0 + r) * ld_out + oc;
                rank[o] = x;
                rp[o] = np1 / x;
            }
        }
    }
}

}  // namespace

hipError_t launch_event_rank(const double* table, int64_t ld_table, const int64_t* offsets, int64_t C,
                             const RankColumns& rc, double n_years, double* rank, double* rp, int64_t ld_out,
                             int32_t* item_counts, int64_t* item_off, int64_t* scan_scratch,
                             unsigned long long* next_item, hipStream_t stream) {
    if (C <= 0) return hipSuccess;
    hipLaunchKernelGGL(rank_item_counts, dim3(static_cast<unsigned>((C + 255) / 256)), dim3(256), 0, stream, offsets, C,
                       item_counts);
    hipError_t e = launch_offsets_from_counts(item_counts, C, item_off, scan_scratch, stream);
    if (e == hipSuccess) e = hipMemsetAsync(next_item, 0, sizeof(unsigned long long), stream);
    if (e != hipSuccess) return e;
    int dev = 0, cus = 0, per_cu = 0;
    e = hipGetDevice(&dev);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (e == hipSuccess) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, event_rank, kItem, 0);
    if (e != hipSuccess) return e;
    if (per_cu < 1) per_cu = 1;
    if (cus < 1) cus = 1;
    hipLaunchKernelGGL(event_rank, dim3(static_cast<unsigned>(2 * per_cu * cus)), dim3(kItem), 0, stream, table, ld_table,
                       offsets, item_off, C, rc, n_years, rank, rp, ld_out, next_item);
    return hipGetLastError();
}

}  // namespace xmhw
