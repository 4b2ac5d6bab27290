// kernels_coverage.hip -- mhw_coverage(): the first reduction ACROSS cells.  Per day and region, the
// number of cells (and the sum of their integer weights) that are in an event, split by the per-step
// category of mhw_df() (xmhw/features.py:52-66): cats = floor(1 + (ts - thresh) / (thresh - seas)),
// moderate / strong / severe / extreme = cats == 1, == 2, == 3, >= 4.  A day inside a joined gap is in
// an event and, below the threshold or NaN, in none of the four.
//
//   event_day_bits       the walk of events_from_bits (event_walk.h) with another sink: instead of a table
//                        row per event, the steps first..last of every event are set in a bitmap of the
//                        same layout as the exceedance words (inev[w * ldb + c], one thread per cell).
//                        1 bit per sample instead of table rows: the reduction below reads it coalesced.
//   coverage_accumulate  lanes = cells, a workgroup owns `tiles` tiles of 256 cells x a block of `tb` steps.
//                        Only in-event lanes read their sample and climatology rows.  Per step a wave
//                        reduces itself: ballot + popcount for the cell counts, a 64-bit integer butterfly
//                        for the weights, once per region present among its in-event lanes (one pass when
//                        the wave holds one region).  With few regions the wave sums meet in LDS
//                        (acc[step][region][10], integer adds) and the workgroup issues one global 64-bit
//                        add per non-zero entry at the end of the block; with many regions (the LDS block
//                        would not hold one step) the wave leader adds to global memory directly - the
//                        addresses are then spread over the regions.
// All sums are integers: the result does not depend on the order of the adds, the tiling or the slabs.
#include "../../include/xmhw_amd.h"
#include "entry_common.h"
#include "stage_reduce.h"
#include "event_walk.h"

namespace xmhw {

// What the stage computes, on the bitmap of launch_event_day_bits (kernels.h): coverage_accumulate ADDS, for every step t
// and region r < R, the number of in-event cells per state (moderate, strong, severe, extreme, event) to cells[t][r][5]
// and the sum of their weights wq[c] to area_q[t][r][5].  region[c] in [-1, R), -1 = the cell counts nowhere;
// R <= kCoverageMaxRegions.  row_of_t is a DEVICE array here.
constexpr int kCoverageMaxRegions = 1024;

namespace {

constexpr int kCovThreads = 256;
constexpr int kCovStates = 5;                       // moderate, strong, severe, extreme, event
constexpr int kCovSlotsPerRegion = 2 * kCovStates;  // cells[5] then area_q[5]
constexpr int kCovLdsSlots = 2560;                  // 20 KiB of 64-bit accumulators: 7 waves per SIMD
constexpr int kCovLdsMaxRegions = 64;               // above: direct global adds

struct DayBitsSink {
    uint64_t* col = nullptr;      // the cell's column of the bitmap (zeroed before the launch)
    int64_t ldb = 0;
    __device__ __forceinline__ void operator()(int64_t, int64_t first, int64_t last) const {
        for (int64_t w = first >> 6; w <= (last >> 6); ++w) {
            const int lo = w == (first >> 6) ? static_cast<int>(first & 63) : 0;
            const int hi = w == (last >> 6) ? static_cast<int>(last & 63) : 63;
            const uint64_t m = (hi == 63 ? ~uint64_t{0} : ((uint64_t{1} << (hi + 1)) - 1)) & ~((uint64_t{1} << lo) - 1);
            col[w * ldb] |= m;                                   // only this thread touches column c
        }
    }
};

__global__ __launch_bounds__(256) void event_day_bits(const uint64_t* __restrict__ bits, int64_t Tn, int64_t C,
                                                      int64_t ldb, int32_t min_duration, int32_t join_gaps,
                                                      int32_t max_gap, uint64_t* __restrict__ inev, int64_t ldi) {
    const int64_t c = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (c >= C) return;
    EventWalk<DayBitsSink> ew;
    ew.sink.col = inev + c;
    ew.sink.ldb = ldi;
    walk_exceed_bits(bits, c, Tn, ldb, min_duration, join_gaps, max_gap, ew);
}

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += static_cast<unsigned long long>(__shfl_xor(static_cast<long long>(v), d, 64));
    return v;
}

template <typename T>
__global__ __launch_bounds__(kCovThreads) void coverage_accumulate(
    const T* __restrict__ ts, int64_t Tn, int64_t C, int64_t ld, const double* __restrict__ seas,
    const double* __restrict__ thresh, int64_t ldc, const int32_t* __restrict__ row_of_t, int32_t negate,
    const uint64_t* __restrict__ inev, int64_t ldi, const int64_t* __restrict__ wq, const int32_t* __restrict__ region,
    int32_t R, int32_t tb, int32_t tiles, int32_t use_lds, unsigned long long* __restrict__ cells,
    unsigned long long* __restrict__ area) {
    __shared__ unsigned long long acc[kCovLdsSlots];
    const int lane = threadIdx.x & 63;
    const int64_t nblk = (Tn + tb - 1) / tb;
    const int32_t nslots = use_lds ? tb * R * kCovSlotsPerRegion : 0;       // <= kCovLdsSlots (launcher)
    for (int64_t blk = blockIdx.y; blk < nblk; blk += gridDim.y) {
        const int64_t t0 = blk * tb;
        const int64_t t1 = t0 + tb < Tn ? t0 + tb : Tn;
        if (use_lds) {
            for (int32_t i = threadIdx.x; i < nslots; i += kCovThreads) acc[i] = 0;
            __syncthreads();
        }
        for (int32_t tile = 0; tile < tiles; ++tile) {
            const int64_t cbase = (static_cast<int64_t>(blockIdx.x) * tiles + tile) * kCovThreads;
            if (cbase >= C) break;                                           // uniform over the workgroup
            const int64_t c = cbase + threadIdx.x;
            const bool valid = c < C;
            const int32_t rid = valid ? region[c] : -1;
            const bool live = valid && rid >= 0 && rid < R;
            const unsigned long long w = live ? static_cast<unsigned long long>(wq[c]) : 0;
            int64_t wi = -1;
            uint64_t word = 0;
            for (int64_t t = t0; t < t1; ++t) {
                if ((t >> 6) != wi) {
                    wi = t >> 6;
                    word = live ? inev[wi * ldi + c] : 0;
                }
                const bool ev = (word >> (t & 63)) & 1;
                uint64_t todo = __ballot(ev);
                if (todo == 0) continue;                                     // uniform over the wave
                int k = -1;                                                  // 0..3, or in none of the four
                if (ev) {
                    const int64_t r = row_of_t[t];
                    double x = static_cast<double>(ts[t * ld + c]);
                    if (negate) x = -x;
                    const double se = seas[r * ldc + c], th = thresh[r * ldc + c];
                    k = category_index(step_category(x, th, se)) - 1;
                }
                while (todo) {                                               // once per region among the in-event lanes
                    const int leader = __builtin_ctzll(todo);
                    const int32_t r = __shfl(rid, leader, 64);
                    const bool mine = ev && rid == r;
                    todo &= ~__ballot(mine);
#pragma unroll
                    for (int s = 0; s < kCovStates; ++s) {
                        const bool in = mine && (s == kCovStates - 1 || k == s);
                        const uint64_t b = __ballot(in);
                        if (b == 0) continue;
                        const unsigned long long n = static_cast<unsigned long long>(__popcll(b));
                        const unsigned long long a = wave_sum_u64(in ? w : 0);
                        if (lane == 0) {
                            if (use_lds) {
                                unsigned long long* p = acc + (static_cast<int64_t>(t - t0) * R + r) * kCovSlotsPerRegion;
                                atomicAdd(p + s, n);
                                if (a) atomicAdd(p + kCovStates + s, a);
                            } else {
                                const int64_t o = (t * R + r) * kCovStates + s;
                                atomicAdd(cells + o, n);
                                if (a) atomicAdd(area + o, a);
                            }
                        }
                    }
                }
            }
        }
        if (use_lds) {
            __syncthreads();
            const int32_t used = static_cast<int32_t>(t1 - t0) * R * kCovSlotsPerRegion;
            for (int32_t i = threadIdx.x; i < used; i += kCovThreads) {
                const unsigned long long v = acc[i];
                if (v == 0) continue;
                const int32_t cell_slot = i / kCovSlotsPerRegion, j = i % kCovSlotsPerRegion;   // cell_slot = step * R + region
                const int64_t o = (t0 * R + cell_slot) * kCovStates + (j % kCovStates);
                atomicAdd((j < kCovStates ? cells : area) + o, v);
            }
            __syncthreads();
        }
    }
}

}  // namespace

hipError_t launch_event_day_bits(const uint64_t* bits, int64_t Tn, int64_t C, int64_t ldb, int32_t min_duration,
                                 int32_t join_gaps, int32_t max_gap, uint64_t* inev, int64_t ldi, hipStream_t stream) {
    if (C <= 0 || Tn <= 0) return hipSuccess;
    const hipError_t e = zero_rows(inev, sizeof(uint64_t), (Tn + 63) / 64, C, ldi, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(event_day_bits, dim3(static_cast<unsigned>((C + 255) / 256)), dim3(256), 0, stream, bits, Tn, C,
                       ldb, min_duration, join_gaps, max_gap, inev, ldi);
    return hipGetLastError();
}

namespace {

template <typename T>
hipError_t launch_coverage_accumulate(const T* ts, int64_t Tn, int64_t C, int64_t ld, const double* seas,
                                      const double* thresh, int64_t ldc, const int32_t* row_of_t, int32_t negate,
                                      const uint64_t* inev, int64_t ldi, const int64_t* wq, const int32_t* region,
                                      int32_t R, int64_t* cells, int64_t* area_q, hipStream_t stream) {
    if (C <= 0 || Tn <= 0 || R <= 0) return hipSuccess;
    if (R > kCoverageMaxRegions) return hipErrorInvalidValue;
    const int32_t use_lds = R <= kCovLdsMaxRegions;
    int32_t tb = 64;
    if (use_lds) {
        const int32_t fit = kCovLdsSlots / (R * kCovSlotsPerRegion);          // >= 4 for R <= 64
        tb = fit < 64 ? fit : 64;
    }
    // a workgroup walks several tiles of cells so that its LDS block is flushed once for all of them; small
    // grids keep one tile per workgroup to fill the chip
    const int32_t tiles = C >= 65536 ? 8 : 1;
    hipLaunchKernelGGL(coverage_accumulate<T>, stage_grid(C, static_cast<int64_t>(kCovThreads) * tiles, Tn, tb),
                       dim3(kCovThreads), 0, stream, ts, Tn, C, ld, seas, thresh, ldc, row_of_t, negate, inev, ldi, wq,
                       region, R, tb, tiles, use_lds, reinterpret_cast<unsigned long long*>(cells),
                       reinterpret_cast<unsigned long long*>(area_q));
    return hipGetLastError();
}

}  // namespace

}  // namespace xmhw

// ---- the C entries of mhw_coverage() (include/xmhw_amd.h) -------------------------------------------------------------
namespace {

using namespace xmhw::entry;

template <typename T>
int coverage_accumulate(const T* ts, int64_t Tn, int64_t C, int64_t ld, const double* seas, const double* thresh,
                        int64_t ldc, const int32_t* row_of_t, int32_t negate, const uint64_t* bits, int64_t ldb,
                        int32_t min_duration, int32_t join_gaps, int32_t max_gap, const int64_t* wq,
                        const int32_t* region, int32_t R, int64_t* cells, int64_t* area_q, void* stream) {
    if (Tn <= 0 || C < 0 || ld < C || ldc < C || ldb < C) return fail(XMHW_ERR_INVALID, "bad T/C/ld/ldc/ldb");
    if (Tn >= (int64_t{1} << 31)) return fail(XMHW_ERR_INVALID, "T too large");
    if (min_duration < 1 || max_gap < 0) return fail(XMHW_ERR_INVALID, "bad minDuration/maxGap");
    if (R < 1) return fail(XMHW_ERR_INVALID, "R must be >= 1");
    if (R > xmhw::kCoverageMaxRegions)
        return fail(XMHW_ERR_UNSUPPORTED, "coverage: R above the cap of " + std::to_string(xmhw::kCoverageMaxRegions) + " regions");
    if (C == 0) return XMHW_OK;
    if (!ts || !seas || !thresh || !row_of_t || !bits || !wq || !region || !cells || !area_q)
        return fail(XMHW_ERR_INVALID, "NULL buffer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    RowsRef rows;
    if (int rc = upload_table(row_of_t, Tn, "row table upload", &rows)) return rc;
    ScratchRef scratch;
    const uint64_t* inev = nullptr;
    if (int rc = event_day_bitmap(bits, Tn, C, ldb, min_duration, join_gaps, max_gap, st, &scratch, &inev)) return rc;
    return status_of(xmhw::launch_coverage_accumulate<T>(ts, Tn, C, ld, seas, thresh, ldc, rows->d_rows, negate, inev, C, wq,
                                                         region, R, cells, area_q, st),
                     "coverage_accumulate launch");
}

}  // namespace

extern "C" {

int xmhw_coverage_accumulate_f32(const float* ts, int64_t T, int64_t C, int64_t ld, const double* seas,
                                 const double* thresh, int64_t ldc, const int32_t* row_of_t, int32_t negate,
                                 const uint64_t* bits, int64_t ldb, int32_t min_duration, int32_t join_gaps,
                                 int32_t max_gap, const int64_t* wq, const int32_t* region, int32_t R, int64_t* cells,
                                 int64_t* area_q, void* stream) {
    return coverage_accumulate<float>(ts, T, C, ld, seas, thresh, ldc, row_of_t, negate, bits, ldb, min_duration,
                                      join_gaps, max_gap, wq, region, R, cells, area_q, stream);
}
int xmhw_coverage_accumulate_f64(const double* ts, int64_t T, int64_t C, int64_t ld, const double* seas,
                                 const double* thresh, int64_t ldc, const int32_t* row_of_t, int32_t negate,
                                 const uint64_t* bits, int64_t ldb, int32_t min_duration, int32_t join_gaps,
                                 int32_t max_gap, const int64_t* wq, const int32_t* region, int32_t R, int64_t* cells,
                                 int64_t* area_q, void* stream) {
    return coverage_accumulate<double>(ts, T, C, ld, seas, thresh, ldc, row_of_t, negate, bits, ldb, min_duration,
                                       join_gaps, max_gap, wq, region, R, cells, area_q, stream);
}

}  // extern "C"
