// stage_reduce.h -- what the stage kernels share: the reductions over the resident series of mhw_coverage()
// (kernels_coverage.hip), region_series() (kernels_region.hip), mhw_track_intensity() (kernels_track_intensity.hip),
// mhw_days_by() (kernels_class.hip), mhw_cooccurrence() (kernels_cooccur.hip), mhw_displacement()
// (kernels_displacement.hip), heat_stress() (kernels_stress.hip), index_regression() (kernels_regress.hip),
// mhw_composite() (kernels_composite.hip), lag_correlation() (kernels_lagcorr.hip), anomaly_distribution()
// (kernels_distribution.hip), spatial_correlation() (kernels_spatialcorr.hip), coarsen() (kernels_coarsen.hip) and regrid() (kernels_regrid.hip).  Each rule below exists once: the Python oracles and the public documentation state it once as well.  kernels.h, "The
// frame of a class reduction", describes the kernels that use most of it; stage_blocks.h holds the block lengths.
#pragma once
#include "device_common.h"
#include "kernels.h"
#include "stage_blocks.h"

namespace xmhw {

// ---- the fixed point of every sum of values ---------------------------------------------------------------------------
// A value d enters a sum as rint(d * 2^kFixedBits), and only if |d| < 2^kFixedRangeBits: the sum of 2^31 such integers
// stays below 2^54.  Anything else that is not NaN (infinities included) is left out and counted by the stage (n_range).
constexpr int kFixedBits = 16;
constexpr int kFixedRangeBits = 7;
constexpr double kFixedOne = static_cast<double>(1 << kFixedBits);
constexpr double kFixedRange = static_cast<double>(1 << kFixedRangeBits);
static_assert(kClassDaysBits == kFixedBits && kTrackIntensityBits == kFixedBits && kHeatStressBits == kFixedBits,
              "one scale for every stage");

// d against the range: 0 = not a sample (NaN), -1 = out of range, 1 = in range; and the integer of a d in range
__device__ __forceinline__ int fixed_state(double d) { return d == d ? (fabs(d) < kFixedRange ? 1 : -1) : 0; }
__device__ __forceinline__ int64_t fixed_value(double d) { return static_cast<int64_t>(rint(d * kFixedOne)); }

// ---- the category of a step (mhw_df(): floor(1 + (ts - thresh) / (thresh - seas))) ------------------------------------
// 1, 2, 3 or 4 (moderate, strong, severe; extreme = 4 and more), 0 = in none of the four: below the threshold, or NaN,
// which compares false everywhere.  x is the sample as float64, negated for cold spells like th and se.
__device__ __forceinline__ double step_category(double x, double th, double se) { return floor(1.0 + (x - th) / (th - se)); }
__device__ __forceinline__ int category_index(double cat) {
    return cat == 1.0 ? 1 : cat == 2.0 ? 2 : cat == 3.0 ? 3 : cat >= 4.0 ? 4 : 0;
}

// ---- the in-event bitmap (inev[w * ldi + c], one bit per step: event_day_bits, event_table_bits) ----------------------
// A lane walks the steps of its column upwards; the word of 64 steps is loaded when it changes, by a live lane only.
struct EventBits {
    int64_t wi = -1;
    uint64_t word = 0;
    __device__ __forceinline__ bool at(const uint64_t* __restrict__ inev, int64_t ldi, int64_t c, bool live, int64_t t) {
        if ((t >> 6) != wi) {
            wi = t >> 6;
            word = live ? inev[wi * ldi + c] : 0;
        }
        return (word >> (t & 63)) & 1;
    }
};

// ---- the run of one class --------------------------------------------------------------------------------------------
// The class the addends in a lane's registers belong to (uniform over the wave), -1 = none yet.  The stage keeps its own
// accumulator and gives flush(k): add what the lane holds to class k and clear it.  One ClassRun per block of steps.
struct ClassRun {
    int32_t k = -1;
    template <typename Flush>
    __device__ __forceinline__ void enter(int32_t knew, Flush&& flush) {
        if (knew != k) {
            if (k >= 0) flush(k);
            k = knew;
        }
    }
    template <typename Flush>
    __device__ __forceinline__ void leave(Flush&& flush) {
        if (k >= 0) flush(k);
    }
};

// ---- block `blk` of a strided block loop: items base + [blk * tb, min((blk + 1) * tb, n)) -----------------------------
template <typename I>
struct BlockRange {
    I t0, t1;
};
template <typename I>
__device__ __forceinline__ BlockRange<I> block_range(I blk, I tb, I n, I base = 0) {
    const I t0 = base + blk * tb;
    return {t0, n - blk * tb > tb ? t0 + tb : base + n};
}

// ---- the host side of a launch ----------------------------------------------------------------------------------------
// `rows` rows of C items of `item` bytes, leading dimension ldo: zero
inline hipError_t zero_rows(void* p, size_t item, int64_t rows, int64_t C, int64_t ldo, hipStream_t stream) {
    if (rows <= 0 || C <= 0) return hipSuccess;
    return ldo == C ? hipMemsetAsync(p, 0, item * static_cast<size_t>(rows) * static_cast<size_t>(C), stream)
                    : hipMemset2DAsync(p, item * static_cast<size_t>(ldo), 0, item * static_cast<size_t>(C),
                                       static_cast<size_t>(rows), stream);
}

// the grid of a strided block kernel: x = `count` items by `width` per workgroup, y = the blocks of `block` along
// `extent` (the kernel strides over the blocks past kStageMaxBlocks), z as given
inline dim3 stage_grid(int64_t count, int64_t width, int64_t extent, int64_t block, int64_t gz = 1) {
    return dim3(static_cast<unsigned>(ceil_div(count, width)), static_cast<unsigned>(stage_blocks(extent, block)),
                static_cast<unsigned>(gz));
}

}  // namespace xmhw
