// stage_blocks.h -- how the stage kernels split their block axis (time steps, or 64-step words): plain integer
// arithmetic without a device type, so that a host program can include it (tests/c/stage_blocks.cpp pins every value).
//
// A stage kernel is launched as workgroups x blocks: grid.x covers the cells (or waves of grid points), grid.y the
// blocks of the axis, and the kernel strides over the blocks that grid.y cannot hold.  Long blocks keep the flushes of
// a class reduction rare (kernels.h, "The frame of a class reduction"); a slab too small to fill the chip with one block
// per workgroup splits the axis until about kStageWorkgroups workgroups exist.
#pragma once
#include <stdint.h>

namespace xmhw {

constexpr int kStageThreads = 256;                   // the workgroup of every stage kernel
constexpr int64_t kStageWorkgroups = 2048;           // split the block axis until about this many workgroups exist
constexpr int64_t kStageMaxBlocks = 65535;           // grid.y at most: the kernels stride over the blocks

static inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// grid.y of a strided block kernel
static inline int64_t stage_blocks(int64_t extent, int64_t block) {
    const int64_t n = ceil_div(extent, block);
    return n > kStageMaxBlocks ? kStageMaxBlocks : n;
}

// The automatic block length of an axis of `extent` items under `wg` workgroups per block: as many blocks as bring the
// launch to about kStageWorkgroups workgroups; more where a block would exceed about `cap` items (0: no cap); never
// more than `most`, the blocks that the axis allows (it is what states a stage's least block); one at least.  The
// block is the axis divided evenly, rounded up to a multiple of `round`.
static inline int64_t stage_auto_block(int64_t extent, int64_t wg, int64_t most, int64_t cap, int64_t round) {
    int64_t nblk = ceil_div(kStageWorkgroups, wg);
    if (cap > 0 && nblk < ceil_div(extent, cap)) nblk = ceil_div(extent, cap);
    if (nblk > most) nblk = most;
    if (nblk < 1) nblk = 1;
    return ceil_div(ceil_div(extent, nblk), round) * round;
}

// mhw_days_by().  Long blocks keep the flushes rare; a slab too small to fill the chip with one block per 256 cells splits
// the time axis until about 2048 workgroups exist, in blocks of whole 64-step words and of 256 steps at least.  (The count
// of 256-step blocks is rounded up, so an axis a little longer than a multiple of 256 may get blocks a little shorter.)
static inline int64_t class_days_auto_block(int64_t Tn, int64_t C) {
    return stage_auto_block(Tn, ceil_div(C, kStageThreads), ceil_div(Tn, 256), 0, 64);
}

// heat_stress() and its class sums (W = 1).  A block pays W - 1 warm-up steps: blocks of 16 W steps and more keep that
// share below 1/16, and of 256 steps and more keep the flushes rare.  Blocks of about 4096 steps measured faster than one
// block over 14,610 steps on a grid that fills the chip by its cells alone (profiles/r24_heat_stress_bench.json: the
// workgroups finish more evenly), so that is the most a block takes; a slab too small to fill the chip with such blocks
// splits the time axis further, until about 2048 workgroups exist.
static inline int64_t heat_stress_auto_block(int64_t Tn, int64_t C, int32_t W) {
    const int64_t least = 16 * static_cast<int64_t>(W) > 256 ? 16 * static_cast<int64_t>(W) : 256;
    return stage_auto_block(Tn, ceil_div(C, kStageThreads), Tn / least, least > 4096 ? least : 4096, 1);
}

// index_regression().  A block pays one step again (the lag-1 pair of its first step) and one flush, so short blocks are
// cheap, and they measured faster than long ones at every grid size (profiles/r27_index_regress_bench.json: 512 steps
// beat 4096 by 12 % at 32 predictors on a grid that fills the chip by its cells alone -- at 4 waves per SIMD the
// workgroups finish more evenly -- and 256 steps beat 512 only on a small slab): blocks of about 512 steps at most and of
// 256 at least; a slab too small to fill the chip with such blocks splits the time axis until about 2048 workgroups exist.
static inline int64_t index_regress_auto_block(int64_t Tn, int64_t C) {
    return stage_auto_block(Tn, ceil_div(C, kStageThreads), Tn / 256, 512, 1);
}

// mhw_composite(), D = before + after + 1 offsets.  A block builds its window from three bitmap words at most and reads no
// sample for it, and nothing is flushed at its end, so short blocks are cheap: the rule of index_regression() -- blocks of
// about 512 steps at most and of 256 at least; a slab too small to fill the chip with such blocks splits the time axis
// until about 2048 workgroups exist.  Measured (profiles/r28_composite_bench.json, r28_composite_blocks_small.json): on
// a grid that fills the chip by its cells alone the block length moves the time by 4 % at most (111 .. 116 ms from 256
// steps to one block, D = 61: the atomics bind, not the walk); on a slab of 65,536 cells blocks of 256 and 512 steps
// beat 4,096 by 18 % and one block by 43 %.  D does not enter: the warm-up costs the same for every window.
static inline int64_t composite_auto_block(int64_t Tn, int64_t C, int64_t D) {
    (void)D;
    return stage_auto_block(Tn, ceil_div(C, kStageThreads), Tn / 256, 512, 1);
}

// lag_correlation(), lags 0 .. L in groups of kLagCorrGroup (grid.z).  A block clears its ring and reads the L steps before
// it again, for every lag group, and reduces nothing from them: blocks of 16 L steps and more keep that share below 1/16,
// and of 256 steps and more keep the flushes rare.  Long blocks measured faster on a grid that fills the chip by its cells
// alone (profiles/r29_lag_corr_bench.json: blocks of 4,096 steps beat 512 by 2 % at 32 lags and by 4 % at 64 and 256 by
// 6 % and 10 %; one block over 14,610 steps is 2 % slower than 4,096), so about 4,096 steps is the most a block takes, as
// in heat_stress(); a slab whose workgroups x lag groups do not fill the chip with such blocks splits the time axis
// further, until about 2048 workgroups exist.
constexpr int kLagCorrGroup = 8;                     // lags per workgroup up to 8 lags: 11 registers of addends each
constexpr int kLagCorrWideGroup = 16;                // ... and from 9 lags on: half the passes at half the occupancy
static inline int64_t lag_corr_group(int64_t L) { return L >= kLagCorrGroup ? kLagCorrWideGroup : kLagCorrGroup; }
static inline int64_t lag_corr_groups(int64_t L) { return L / lag_corr_group(L) + 1; }
static inline int64_t lag_corr_auto_block(int64_t Tn, int64_t C, int64_t L) {
    const int64_t least = 16 * L > 256 ? 16 * L : 256;
    return stage_auto_block(Tn, ceil_div(C, kStageThreads) * lag_corr_groups(L), Tn / least, least > 4096 ? least : 4096, 1);
}

// anomaly_distribution().  A block pays the clearing of nothing (a flush leaves the LDS column empty) and one flush at its
// end, whose scan covers the dwords the block touched: the rule of class_days_auto_block -- a slab too small to fill the
// chip with one block per 256 cells splits the time axis until about 2048 workgroups exist, in blocks of 256 steps at
// least -- with about 4,096 steps as the most a block takes, as in heat_stress() and lag_correlation(): with 128 KB of LDS
// a CU holds one workgroup at a time, and several blocks per 256 cells let the workgroups finish evenly.  Measured on a
// grid that fills the chip by its cells alone (profiles/r31_distribution_bench.json, one class): forced blocks of 256 /
// 512 / 4,096 steps and one block over 14,610 steps take 73.5 / 71.6 / 70.4 / 72.5 ms at 128 bins and 139.5 / 134.9 /
// 131.9 / 132.8 ms at 256 -- long blocks win by 3 to 6 %, and 4,096 is not slower than one block.
static inline int64_t distribution_auto_block(int64_t Tn, int64_t C) {
    return stage_auto_block(Tn, ceil_div(C, kStageThreads), ceil_div(Tn, 256), 4096, 1);
}

// mhw_displacement(): a workgroup is four waves of 64 longitudes of one grid row.  One block over the steps keeps the
// flushes rare; a grid whose waves do not fill the chip splits the steps until about 2048 workgroups exist.
static inline int64_t displacement_auto_block(int64_t nt, int64_t ny, int64_t nx) {
    return nt > 0 ? stage_auto_block(nt, ceil_div(ny * ceil_div(nx, 64), kStageThreads / 64), nt, 0, 1) : 1;
}

// spatial_correlation(): a workgroup is a tile of `rows` grid rows x 64 longitudes, times the offset groups (grid.z).  A
// block pays no warm-up -- the partners of a step are samples of the same step -- and one flush at its end, so the rule
// is that of displacement_auto_block with the offset groups multiplying the workgroups: one block over the steps keeps
// the flushes rare; a grid whose tiles x groups do not fill the chip splits the steps until about 2048 workgroups exist.
// Short blocks measured faster at the default offsets on a grid that fills the chip by its tiles alone
// (profiles/r32_spatial_corr_bench.json, one class: forced blocks of 256 / 4,096 steps and one block take 242.1 / 238.1 /
// 260.6 ms at 13 offsets and 1,298 / 1,254 / 1,247 ms at 64; on half the grid 120.8 / 121.1 / 144.3 and 619.1 / 615.3 /
// 627.6 ms -- with one or two workgroups per CU and two barriers per step the workgroups finish more evenly), so about
// 256 steps is the most a block takes; 4,096 would do as well or 2 to 3 % better on the full grid.
constexpr int kSpatialCorrGroup = kLagCorrGroup;     // offsets per workgroup up to 8 offsets, the registers of lag_corr
constexpr int kSpatialCorrWideGroup = kLagCorrWideGroup;
static inline int64_t spatial_corr_group(int64_t D) { return D > kSpatialCorrGroup ? kSpatialCorrWideGroup : kSpatialCorrGroup; }
static inline int64_t spatial_corr_groups(int64_t D) { return D > 0 ? ceil_div(D, spatial_corr_group(D)) : 1; }
static inline int64_t spatial_corr_auto_block(int64_t nt, int64_t ny, int64_t nx, int64_t rows, int64_t D) {
    return nt > 0 ? stage_auto_block(nt, ceil_div(ny, rows) * ceil_div(nx, 64) * spatial_corr_groups(D), nt, 256, 1) : 1;
}

// coarsen(): the axis is the ns windows, a workgroup is 256 coarse cells.  A chunk carries nothing over and flushes
// nothing, so short chunks cost a workgroup's start and no more; long ones leave the last workgroups of a launch alone on
// the chip.  A chunk takes the windows that hold about 64 lines x steps of requests per lane (`rows` = fy fine rows by
// `max_len` steps of the longest window each): a workgroup then lives for microseconds, thousands of them per launch; a
// grid too small to fill the chip with such chunks splits the windows until about 2048 workgroups exist.
static inline int64_t coarsen_auto_chunk(int64_t ns, int64_t cells, int64_t rows, int64_t max_len) {
    const int64_t work = rows * max_len > 0 ? rows * max_len : 1;
    const int64_t wg = cells > 0 ? ceil_div(cells, kStageThreads) : 1;
    return ns > 0 ? stage_auto_block(ns, wg, ns, 64 / work > 0 ? 64 / work : 1, 1) : 1;
}

// mhw_cooccurrence(): the axis is the W words of the bitmaps, a workgroup takes one lag group (grid.z).  One block over W
// keeps the flushes rare and needs no first-word loads; a slab whose workgroups x lag groups do not fill the chip splits
// the word axis until about 2048 workgroups exist.
static inline int64_t cooccur_auto_block(int64_t W, int64_t C, int64_t lag_groups) {
    return W > 0 ? stage_auto_block(W, ceil_div(C, kStageThreads) * lag_groups, W, 0, 1) : 1;
}

}  // namespace xmhw
