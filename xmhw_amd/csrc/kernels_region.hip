// kernels_region.hip -- region_series(): the area-weighted regional mean series, the reduction ACROSS cells that
// sums VALUES (mhw_coverage() counts states).  For every step t and region r < R, over the cells c with
// region[c] == r whose sample is not NaN:
//   acc[t][r][0] += 1   acc[t][r][1] += wi[c]   acc[t][r][2] += wi[c] * rint(((double)ts[t][c] - x0) * 2^16)
// A valid sample with |ts - x0| >= 2^7, or infinite, is left out of all three and counted (*n_range).
//
//   region_accumulate  lanes = cells, a workgroup owns `tiles` tiles of 256 cells x a block of `tb` steps, as
//                      coverage_accumulate.  Every lane contributes at every step, and a lane's region and weight
//                      do not change with t, so the region structure of a wave is worked out once per tile:
//                      A  all live lanes of the wave hold one region (boxes, basins, masks: the common case).  Per
//                         step: n_valid = popcount of a ballot; wsum_i = the wave's weight, summed once for the tile,
//                         whenever the ballot equals the live mask (else a wave sum); xsum_q = a 64-bit wave sum.
//                         The wave sums of kRegUnroll = 8 steps are taken together: three exchange stages (lane ^ 1,
//                         lane ^ 2, the halves of the wave) in which a lane keeps half of its values and hands over
//                         the other half, so that 8 values per lane become one after 7 exchanges, then three stages
//                         over that one value; 10 exchanges for 8 steps, all DPP moves or permlane swaps, instead
//                         of 6 per step.  Eight lanes end with one step's total each and add it.
//                      B  2..kRegListMax regions: the same, one pass per region of the list built for the tile.
//                      C  more regions: every lane issues its own adds (no return value).
//                      With R <= kRegLdsMaxRegions the adds meet in LDS (acc[step][region][3]) and the workgroup
//                      issues one global 64-bit add per non-zero entry at the end of a block; above, the lanes
//                      that hold a step's total (A, B) or all lanes (C) add to global memory directly.
//                      *n_range is summed in the workgroup and added once per workgroup when non-zero.
// All sums are integers: the result does not depend on the order of the adds, the tiling or the slabs.
#include "../../include/xmhw_amd.h"
#include "entry_common.h"
#include "stage_reduce.h"

namespace xmhw {

// What the stage computes: region_accumulate ADDS, for every step t and region r < R, over the cells c with
// region[c] == r whose sample is not NaN: acc[t][r][0] += 1, acc[t][r][1] += wi[c], acc[t][r][2] += wi[c] *
// rint(((double)ts[t][c] - x0) * 2^16); a valid sample with |ts - x0| >= 2^7 or infinite is left out and counted in
// *n_range.  region[c] in [-1, R), -1 = the cell counts nowhere; R <= kRegionMaxRegions.  blocked selects how a wave sums:
// 0 = one wave sum per step, 1 = the sums of 8 steps together (below).  Same results.
constexpr int kRegionMaxRegions = 1024;

namespace {

constexpr int kRegThreads = 256;
constexpr int kRegSlots = 3;                        // n_valid, wsum_i, xsum_q
constexpr int kRegLdsSlots = 2560;                  // 20 KiB of 64-bit accumulators, as coverage_accumulate
constexpr int kRegLdsMaxRegions = 64;               // above: direct global adds
constexpr int kRegListMax = 4;                      // regions per wave handled by passes (B); above: per-lane adds (C)
constexpr int kRegUnroll = 8;                       // samples a lane requests before it consumes the first

using u64 = unsigned long long;

template <int CTRL>
__device__ __forceinline__ u64 dpp_u64(u64 v) {
    const int lo = __builtin_amdgcn_update_dpp(0, static_cast<int>(v), CTRL, 0xF, 0xF, true);
    const int hi = __builtin_amdgcn_update_dpp(0, static_cast<int>(v >> 32), CTRL, 0xF, 0xF, true);
    return (static_cast<u64>(static_cast<uint32_t>(hi)) << 32) | static_cast<uint32_t>(lo);
}

// permlane32_swap exchanges lanes 32..63 of its first operand with lanes 0..31 of its second: with (a, b) the sum of the
// two results is a[l] + a[l + 32] in the lower half of the wave and b[l - 32] + b[l] in the upper half
__device__ __forceinline__ u64 swap32_sum(u64 a, u64 b) {
    const auto lo = __builtin_amdgcn_permlane32_swap(static_cast<uint32_t>(a), static_cast<uint32_t>(b), false, false);
    const auto hi = __builtin_amdgcn_permlane32_swap(static_cast<uint32_t>(a >> 32), static_cast<uint32_t>(b >> 32), false, false);
    return ((static_cast<u64>(hi[0]) << 32) | lo[0]) + ((static_cast<u64>(hi[1]) << 32) | lo[1]);
}

// permlane16_swap exchanges the odd rows (of 16 lanes) of its first operand with the even rows of its second: with
// (v, v) the sum of the two results is v[l] + v[l ^ 16] in every lane
__device__ __forceinline__ u64 swap16_sum(u64 v) {
    const auto lo = __builtin_amdgcn_permlane16_swap(static_cast<uint32_t>(v), static_cast<uint32_t>(v), false, false);
    const auto hi = __builtin_amdgcn_permlane16_swap(static_cast<uint32_t>(v >> 32), static_cast<uint32_t>(v >> 32), false, false);
    return ((static_cast<u64>(hi[0]) << 32) | lo[0]) + ((static_cast<u64>(hi[1]) << 32) | lo[1]);
}

// the sum of one value over the wave, in every lane: quad permutes (lane ^ 1, lane ^ 2), the mirrors of a half row and
// of a row of 16 lanes (each pairs every lane with one of the other half, which holds that half's sum), the rows of a
// half wave, the halves.  No LDS traffic.  All 64 lanes must be active.
__device__ __forceinline__ u64 wave_sum(u64 v) {
    v += dpp_u64<0xB1>(v);                           // quad_perm [1, 0, 3, 2]
    v += dpp_u64<0x4E>(v);                           // quad_perm [2, 3, 0, 1]
    v += dpp_u64<0x141>(v);                          // row_half_mirror
    v += dpp_u64<0x140>(v);                          // row_mirror
    v = swap16_sum(v);
    return swap32_sum(v, v);
}

// the sums over the wave of kRegUnroll = 8 values per lane, together.  Stage 1 (partner lane ^ 1): a lane with bit 0
// clear keeps v[0..3] and receives its partner's, a lane with bit 0 set keeps v[4..7]: 4 values left.  Stage 2 (lane ^ 2)
// the same on bit 1: 2 left.  Stage 3: the lower half of the wave keeps v[0], the upper half v[1].  The lane now holds the
// partial sum of step 4 * bit0 + 2 * bit1 + bit5 (step_of_lane) over the 8 lanes that differ from it in bits 0, 1, 5; the
// lanes that differ in bits 2, 3, 4 hold the same step: rotations by 4 and 8 within the row of 16, then the other row.
// Every lane ends with the total of its step.  All 64 lanes must be active.
__device__ __forceinline__ int step_of_lane(int lane) { return ((lane & 1) << 2) | (lane & 2) | ((lane >> 5) & 1); }

__device__ __forceinline__ u64 wave_sum8(u64 (&v)[kRegUnroll], int lane) {
    static_assert(kRegUnroll == 8, "three halving stages");
    const bool b0 = lane & 1, b1 = lane & 2;
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = (b0 ? v[i + 4] : v[i]) + dpp_u64<0xB1>(b0 ? v[i] : v[i + 4]);
#pragma unroll
    for (int i = 0; i < 2; ++i) v[i] = (b1 ? v[i + 2] : v[i]) + dpp_u64<0x4E>(b1 ? v[i] : v[i + 2]);
    u64 r = swap32_sum(v[0], v[1]);
    r += dpp_u64<0x124>(r);                          // row_ror:4
    r += dpp_u64<0x128>(r);                          // row_ror:8
    return swap16_sum(r);
}

// the three adds of one (step, region) entry, in LDS or in global memory (never through a pointer that may be either)
__device__ __forceinline__ void add3(u64* p, u64 n, u64 w, u64 q) {
    atomicAdd(p, n);
    if (w) atomicAdd(p + 1, w);
    if (q) atomicAdd(p + 2, q);
}

template <typename T, bool BLOCKED>
__global__ __launch_bounds__(kRegThreads) void region_accumulate(const T* __restrict__ ts, int64_t Tn, int64_t C, int64_t ld,
                                                                 double x0, const int64_t* __restrict__ wi,
                                                                 const int32_t* __restrict__ region, int32_t R, int32_t tb,
                                                                 int32_t tiles, int32_t use_lds, u64* __restrict__ acc,
                                                                 u64* __restrict__ n_range) {
    __shared__ u64 lacc[kRegLdsSlots];
    __shared__ u64 lrange;
    const int lane = threadIdx.x & 63;
    const int64_t nblk = (Tn + tb - 1) / tb;
    const int32_t nslots = use_lds ? tb * R * kRegSlots : 0;                 // <= kRegLdsSlots (launcher)
    uint32_t out_of_range = 0;                                               // this lane's samples left out
    if (threadIdx.x == 0) lrange = 0;
    for (int64_t blk = blockIdx.y; blk < nblk; blk += gridDim.y) {
        const int64_t t0 = blk * tb;
        const int64_t t1 = t0 + tb < Tn ? t0 + tb : Tn;
        if (use_lds) {
            for (int32_t i = threadIdx.x; i < nslots; i += kRegThreads) lacc[i] = 0;
            __syncthreads();
        }
        for (int32_t tile = 0; tile < tiles; ++tile) {
            const int64_t cbase = (static_cast<int64_t>(blockIdx.x) * tiles + tile) * kRegThreads;
            if (cbase >= C) break;                                           // uniform over the workgroup
            const int64_t c = cbase + threadIdx.x;
            const int32_t rid = c < C ? region[c] : -1;
            const bool live = rid >= 0 && rid < R;
            const u64 w = live ? static_cast<u64>(wi[c]) : 0;
            const uint64_t livemask = __ballot(live);
            if (livemask == 0) continue;                                     // uniform over the wave
            // the regions of the wave, once per tile: up to kRegListMax of them with their lanes and their weight
            int32_t reg[kRegListMax];
            uint64_t mask[kRegListMax];
            u64 wtot[kRegListMax];
            uint64_t todo = livemask;
#pragma unroll
            for (int k = 0; k < kRegListMax; ++k) {
                reg[k] = -1;
                mask[k] = 0;
                wtot[k] = 0;
                if (todo) {                                                  // uniform
                    reg[k] = __shfl(rid, __builtin_ctzll(todo), 64);
                    mask[k] = __ballot(live && rid == reg[k]);
                    wtot[k] = wave_sum(live && rid == reg[k] ? w : 0);
                    todo &= ~mask[k];
                }
            }
            const bool per_lane = todo != 0;                                 // path C
            const uint32_t wl = static_cast<uint32_t>(w), wh = static_cast<uint32_t>(w >> 32);
            const bool wide = __ballot(wh != 0) != 0;                        // weights above 32 bits: outside the budget
            for (int64_t tq = t0; tq < t1; tq += kRegUnroll) {
                T xv[kRegUnroll];
#pragma unroll
                for (int u = 0; u < kRegUnroll; ++u)
                    xv[u] = live && tq + u < t1 ? ts[(tq + u) * ld + c] : static_cast<T>(make_nan());
                u64 q[kRegUnroll];
                uint32_t okbits = 0;                                         // bit u: the sample of step tq + u counts
#pragma unroll
                for (int u = 0; u < kRegUnroll; ++u) {
                    const double d = static_cast<double>(xv[u]) - x0;
                    bool ok = live && d == d;                                // NaN: not a sample
                    if (ok && !(fabs(d) < kFixedRange)) {                    // +-inf included
                        ++out_of_range;
                        ok = false;
                    }
                    // |xq| <= 2^23: w * xq from 32-bit halves, exact modulo 2^64 (xq's upper half is its sign)
                    const int32_t xq = ok ? static_cast<int32_t>(rint(d * kFixedOne)) : 0;
                    const uint32_t xl = static_cast<uint32_t>(xq);
                    uint32_t hi = xq < 0 ? 0u - wl : 0u;
                    if (wide) hi += wh * xl;                                 // uniform
                    q[u] = static_cast<u64>(wl) * xl + (static_cast<u64>(hi) << 32);
                    okbits |= static_cast<uint32_t>(ok) << u;
                }
                if (per_lane) {                                              // uniform
#pragma unroll
                    for (int u = 0; u < kRegUnroll; ++u) {
                        if (!((okbits >> u) & 1)) continue;
                        if (use_lds)
                            add3(lacc + (static_cast<int64_t>(tq + u - t0) * R + rid) * kRegSlots, 1, w, q[u]);
                        else
                            add3(acc + ((tq + u) * R + rid) * kRegSlots, 1, w, q[u]);
                    }
                    continue;
                }
                uint64_t okmask[kRegUnroll];
#pragma unroll
                for (int u = 0; u < kRegUnroll; ++u) okmask[u] = __ballot((okbits >> u) & 1);
                if (BLOCKED) {
                    const int s = step_of_lane(lane);
#pragma unroll 1
                    for (int k = 0; k < kRegListMax; ++k) {
                        if (mask[k] == 0) continue;                          // uniform
                        bool any = false, partial = false;                   // uniform
#pragma unroll
                        for (int u = 0; u < kRegUnroll; ++u) {
                            any |= (okmask[u] & mask[k]) != 0;
                            partial |= (okmask[u] & mask[k]) != mask[k];
                        }
                        if (!any) continue;
                        const bool mine = rid == reg[k];
                        u64 v[kRegUnroll];
#pragma unroll
                        for (int u = 0; u < kRegUnroll; ++u) v[u] = mine ? q[u] : 0;
                        const u64 xs = wave_sum8(v, lane);
                        u64 ws = wtot[k];
                        if (partial) {                                       // a step without all of the region's lanes
#pragma unroll
                            for (int u = 0; u < kRegUnroll; ++u) v[u] = mine && ((okbits >> u) & 1) ? w : 0;
                            ws = wave_sum8(v, lane);
                        }
                        u64 n = 0;
#pragma unroll
                        for (int u = 0; u < kRegUnroll; ++u)
                            if (s == u) n = static_cast<u64>(__popcll(okmask[u] & mask[k]));
                        // one lane per step adds; n != 0 implies tq + s < t1
                        if ((lane & ~0x23) == 0 && n) {
                            if (use_lds)
                                add3(lacc + (static_cast<int64_t>(tq + s - t0) * R + reg[k]) * kRegSlots, n, ws, xs);
                            else
                                add3(acc + ((tq + s) * R + reg[k]) * kRegSlots, n, ws, xs);
                        }
                    }
                } else {
#pragma unroll
                    for (int u = 0; u < kRegUnroll; ++u) {
#pragma unroll
                        for (int k = 0; k < kRegListMax; ++k) {
                            const uint64_t b = okmask[u] & mask[k];
                            if (b == 0) continue;                            // uniform (an unused entry has no lanes)
                            const bool mine = rid == reg[k];
                            const u64 ws = b == mask[k] ? wtot[k] : wave_sum(mine && ((okbits >> u) & 1) ? w : 0);
                            const u64 xs = wave_sum(mine ? q[u] : 0);
                            if (lane == 0) {
                                const u64 n = static_cast<u64>(__popcll(b));
                                if (use_lds)
                                    add3(lacc + (static_cast<int64_t>(tq + u - t0) * R + reg[k]) * kRegSlots, n, ws, xs);
                                else
                                    add3(acc + ((tq + u) * R + reg[k]) * kRegSlots, n, ws, xs);
                            }
                        }
                    }
                }
            }
        }
        if (use_lds) {
            __syncthreads();
            const int32_t used = static_cast<int32_t>(t1 - t0) * R * kRegSlots;
            for (int32_t i = threadIdx.x; i < used; i += kRegThreads) {
                const u64 v = lacc[i];
                if (v) atomicAdd(acc + t0 * R * kRegSlots + i, v);            // the block's entries are contiguous
            }
            __syncthreads();
        }
    }
    __syncthreads();                                                          // lrange is zero for every wave
    if (out_of_range) atomicAdd(&lrange, static_cast<u64>(out_of_range));
    __syncthreads();
    if (threadIdx.x == 0 && lrange) atomicAdd(n_range, lrange);
}

template <typename T>
hipError_t launch_region_accumulate(const T* ts, int64_t Tn, int64_t C, int64_t ld, double x0, const int64_t* wi,
                                    const int32_t* region, int32_t R, int64_t* acc, int64_t* n_range, int32_t blocked,
                                    hipStream_t stream) {
    if (C <= 0 || Tn <= 0 || R <= 0) return hipSuccess;
    if (R > kRegionMaxRegions) return hipErrorInvalidValue;
    const int32_t use_lds = R <= kRegLdsMaxRegions;
    int32_t tb = 64;
    if (use_lds) {
        const int32_t fit = kRegLdsSlots / (R * kRegSlots);                   // >= 13 for R <= 64
        tb = fit < 64 ? fit : 64;
    }
    // a workgroup walks several tiles of cells so that its LDS block is flushed once for all of them; small
    // grids keep one tile per workgroup to fill the chip (as coverage_accumulate)
    const int32_t tiles = C >= 65536 ? 8 : 1;
    const dim3 grid = stage_grid(C, static_cast<int64_t>(kRegThreads) * tiles, Tn, tb), block(kRegThreads);
    u64* a = reinterpret_cast<u64*>(acc);
    u64* nr = reinterpret_cast<u64*>(n_range);
    if (blocked)
        hipLaunchKernelGGL((region_accumulate<T, true>), grid, block, 0, stream, ts, Tn, C, ld, x0, wi, region, R, tb, tiles,
                           use_lds, a, nr);
    else
        hipLaunchKernelGGL((region_accumulate<T, false>), grid, block, 0, stream, ts, Tn, C, ld, x0, wi, region, R, tb, tiles,
                           use_lds, a, nr);
    return hipGetLastError();
}

}  // namespace

}  // namespace xmhw

// ---- the C entries of region_series() (include/xmhw_amd.h) ------------------------------------------------------------
namespace {

using namespace xmhw::entry;

static std::atomic<int> g_region_wave_sum{1};   // region_accumulate sums 8 steps of a wave together (xmhw_set_region_wave_sum)

template <typename T>
int region_accumulate(const T* ts, int64_t Tn, int64_t C, int64_t ld, double x0, const int64_t* wi, const int32_t* region,
                      int32_t R, int64_t* acc, int64_t* n_range, void* stream) {
    if (Tn < 0 || C < 0 || ld < C) return fail(XMHW_ERR_INVALID, "bad T/C/ld");
    if (Tn >= (int64_t{1} << 31)) return fail(XMHW_ERR_INVALID, "T too large");
    if (R < 1) return fail(XMHW_ERR_INVALID, "R must be >= 1");
    if (R > xmhw::kRegionMaxRegions)
        return fail(XMHW_ERR_UNSUPPORTED, "region_accumulate: R above the cap of " + std::to_string(xmhw::kRegionMaxRegions) + " regions");
    if (!(x0 == x0) || std::isinf(x0)) return fail(XMHW_ERR_INVALID, "x0 must be finite");
    if (C == 0 || Tn == 0) return XMHW_OK;
    if (!ts || !wi || !region || !acc || !n_range) return fail(XMHW_ERR_INVALID, "NULL buffer");
    return status_of(xmhw::launch_region_accumulate<T>(ts, Tn, C, ld, x0, wi, region, R, acc, n_range,
                                                       g_region_wave_sum.load(), static_cast<hipStream_t>(stream)),
                     "region_accumulate launch");
}

}  // namespace

extern "C" {

int xmhw_set_region_wave_sum(int32_t variant) {
    if (variant != 0 && variant != 1) return fail(XMHW_ERR_INVALID, "variant must be 0 or 1");
    g_region_wave_sum = variant;
    return XMHW_OK;
}
int xmhw_region_accumulate_f32(const float* ts, int64_t T, int64_t C, int64_t ld, double x0, const int64_t* wi,
                               const int32_t* region, int32_t R, int64_t* acc, int64_t* n_range, void* stream) {
    return region_accumulate<float>(ts, T, C, ld, x0, wi, region, R, acc, n_range, stream);
}
int xmhw_region_accumulate_f64(const double* ts, int64_t T, int64_t C, int64_t ld, double x0, const int64_t* wi,
                               const int32_t* region, int32_t R, int64_t* acc, int64_t* n_range, void* stream) {
    return region_accumulate<double>(ts, T, C, ld, x0, wi, region, R, acc, n_range, stream);
}

}  // extern "C"
