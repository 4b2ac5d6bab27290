// kernels_tracks.hip -- mhw_tracks(): the daily series of every selected object (cells, area, three first moments) as
// one ragged array: object i of the selection owns the entries offsets[i]..offsets[i + 1] - 1, one per day from its
// time_start to its time_end.  Every quantity is constant along a table row, so no voxel is visited:
//
//   tracks_scatter   lane = row.  A row of the selected object i adds (1, vec[0..3][cell]) to the difference arrays at
//                    offsets[i] + start - time_start[i] and subtracts it at offsets[i] + end + 1 - time_start[i], which is
//                    at most offsets[i + 1]: the first entry of the next object, or the sentinel entry L.  Integer
//                    atomics without a return value: the result does not depend on the order.  A row whose slot is
//                    outside [0, n_slots) does nothing; a selected row that is not fit (object_rows.h, fit_row<false>:
//                    its days leave its object's segment, or its cell is outside [0, C)) is left out and counted in
//                    *n_bad (nothing is ever written outside 0..L).
//   tracks_tile_sums   block = one tile of kTile entries of one channel: the tile's sum.
//   tracks_scan_tiles  block = one tile: inclusive scan in place, on top of the carry = the scanned sum of the tile in
//                    front.  Thread = kItems consecutive entries; the thread totals are scanned within the wave by
//                    __shfl_up steps (64-bit, DPP / permute moves), the four wave totals through LDS.
//
// Every object's terms cancel by the end of its own segment, so ONE plain inclusive scan of the concatenated array
// yields all the series (no segment flags), and entry L comes out 0.  The scan is reduce-then-scan in separate launches,
// recursively: tile sums -> scan of the tile sums (the same two kernels one level up) -> tiles rescanned with their
// carry.  No kernel waits for another workgroup.  Channel 0 (cells) is 32-bit at the entry level -- every entry, every
// prefix and every difference of two prefixes is within (-2^31, 2^31) -- and 64-bit in the levels of tile sums.
#include "device_common.h"
#include "kernels.h"
#include "object_rows.h"

namespace xmhw {

namespace {

constexpr int kTrkThreads = kRowThreads;
constexpr int kTrkItems = kTracksTile / kTrkThreads;
static_assert(kTrkItems * kTrkThreads == kTracksTile && kTrkItems == 4, "a thread owns four consecutive entries");
using u64 = unsigned long long;

__global__ __launch_bounds__(kTrkThreads) void tracks_scatter(ObjectRows a, const int64_t* __restrict__ vec, int64_t ldv,
                                                              int32_t* __restrict__ cnt, u64* __restrict__ sums, int64_t ld,
                                                              int32_t* __restrict__ n_bad) {
    const int64_t r = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (r >= a.n) return;
    ObjectRow me;
    const int fit = fit_row<false>(a, r, me);
    if (fit < 0) atomicAdd(n_bad, 1);
    if (fit != 1) return;
    const int32_t c = me.c;
    const int64_t p0 = me.entry, p1 = me.entry + (static_cast<int64_t>(me.e) - me.s + 1);    // p1 <= offsets[i + 1] <= L
    u64 v[4];                                        // the four loads in flight together, ahead of the atomics
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = static_cast<u64>(vec[k * ldv + c]);
    atomicAdd(cnt + p0, 1);
    atomicAdd(cnt + p1, -1);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (v[k] == 0) continue;
        atomicAdd(sums + k * ld + p0, v[k]);
        atomicAdd(sums + k * ld + p1, u64{0} - v[k]);
    }
}

// the four entries of a thread: beyond N they read as 0
template <typename T>
__device__ __forceinline__ void load_items(const T* __restrict__ a, int64_t i0, int64_t N, int64_t (&v)[kTrkItems]) {
    if (i0 + kTrkItems <= N) {                       // a whole thread: four plain loads the compiler may merge
#pragma unroll
        for (int k = 0; k < kTrkItems; ++k) v[k] = static_cast<int64_t>(a[i0 + k]);
    } else {
#pragma unroll
        for (int k = 0; k < kTrkItems; ++k) v[k] = i0 + k < N ? static_cast<int64_t>(a[i0 + k]) : 0;
    }
}

__device__ __forceinline__ int64_t wave_sum(int64_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(static_cast<long long>(v), d, 64);
    return v;
}

template <typename T>
__device__ __forceinline__ void tile_sum(const T* __restrict__ a, int64_t N, int64_t* __restrict__ out) {
    __shared__ int64_t part[kTrkThreads / 64];
    const int64_t i0 = static_cast<int64_t>(blockIdx.x) * kTracksTile + threadIdx.x * kTrkItems;
    int64_t v[kTrkItems];
    load_items(a, i0, N, v);
    const int64_t s = wave_sum(v[0] + v[1] + v[2] + v[3]);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) out[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}

template <typename T>
__device__ __forceinline__ void tile_scan(T* __restrict__ a, int64_t N, const int64_t* __restrict__ carry) {
    __shared__ int64_t part[kTrkThreads / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t i0 = static_cast<int64_t>(blockIdx.x) * kTracksTile + threadIdx.x * kTrkItems;
    int64_t v[kTrkItems];
    load_items(a, i0, N, v);
    v[1] += v[0];
    v[2] += v[1];
    v[3] += v[2];
    int64_t s = v[3];                                // inclusive scan of the thread totals over the wave
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int64_t q = __shfl_up(static_cast<long long>(s), d, 64);
        if (lane >= d) s += q;
    }
    if (lane == 63) part[wave] = s;
    __syncthreads();
    int64_t base = s - v[3];                         // what lies in front of the thread: within the wave,
    for (int w = 0; w < wave; ++w) base += part[w];  // in the waves before it,
    if (carry && blockIdx.x > 0) base += carry[blockIdx.x - 1];     // and in the tiles before this one
#pragma unroll
    for (int k = 0; k < kTrkItems; ++k)
        if (i0 + k < N) a[i0 + k] = static_cast<T>(v[k] + base);
}

// blockIdx.y = channel.  With a32 set, channel 0 is the 32-bit array and channel y > 0 is a64 + (y - 1) * ld; without,
// channel y is a64 + y * ld (the levels of tile sums).  Tile sums of channel y: out + y * ldo.
__global__ __launch_bounds__(kTrkThreads) void tracks_tile_sums(const int32_t* __restrict__ a32, const int64_t* __restrict__ a64,
                                                                int64_t ld, int64_t N, int64_t* __restrict__ out, int64_t ldo) {
    const int y = blockIdx.y;
    if (a32 && y == 0) tile_sum(a32, N, out);
    else tile_sum(a64 + (a32 ? y - 1 : y) * ld, N, out + y * ldo);
}

__global__ __launch_bounds__(kTrkThreads) void tracks_scan_tiles(int32_t* __restrict__ a32, int64_t* __restrict__ a64, int64_t ld,
                                                                 int64_t N, const int64_t* __restrict__ carry, int64_t ldo) {
    const int y = blockIdx.y;
    if (a32 && y == 0) tile_scan(a32, N, carry);
    else tile_scan(a64 + (a32 ? y - 1 : y) * ld, N, carry ? carry + y * ldo : nullptr);
}

inline int64_t tiles_of(int64_t N) { return (N + kTracksTile - 1) / kTracksTile; }

// inclusive scan in place of the five channels of length N; `scratch` holds the levels of tile sums
void scan_level(int32_t* a32, int64_t* a64, int64_t ld, int64_t N, int64_t* scratch, hipStream_t stream) {
    const int64_t tiles = tiles_of(N);
    const dim3 grid(static_cast<unsigned>(tiles), kTracksChannels), block(kTrkThreads);
    if (tiles == 1) {
        hipLaunchKernelGGL(tracks_scan_tiles, grid, block, 0, stream, a32, a64, ld, N, static_cast<const int64_t*>(nullptr),
                           int64_t{0});
        return;
    }
    hipLaunchKernelGGL(tracks_tile_sums, grid, block, 0, stream, static_cast<const int32_t*>(a32),
                       static_cast<const int64_t*>(a64), ld, N, scratch, tiles);
    scan_level(nullptr, scratch, tiles, tiles, scratch + kTracksChannels * tiles, stream);
    hipLaunchKernelGGL(tracks_scan_tiles, grid, block, 0, stream, a32, a64, ld, N, static_cast<const int64_t*>(scratch), tiles);
}

}  // namespace

size_t object_tracks_scratch_bytes(int64_t L1) {
    size_t words = 0;
    for (int64_t N = L1; N > kTracksTile;) {
        N = tiles_of(N);
        words += static_cast<size_t>(kTracksChannels) * static_cast<size_t>(N);
    }
    return sizeof(int64_t) * (words ? words : 1);
}

hipError_t launch_object_tracks(const int32_t* start, const int32_t* end, int64_t n, const int32_t* slot,
                                const int32_t* cell_of_row, int64_t C, const int64_t* vec, int64_t ldv,
                                const int32_t* time_start, const int64_t* offsets, int64_t n_slots, int64_t L,
                                int32_t* n_cells, int64_t* sums, int64_t ld, int32_t* n_bad, int64_t* scratch,
                                hipStream_t stream) {
    const size_t L1 = static_cast<size_t>(L) + 1;
    hipError_t e = hipMemsetAsync(n_cells, 0, sizeof(int32_t) * L1, stream);
    for (int k = 0; k < 4 && e == hipSuccess; ++k) e = hipMemsetAsync(sums + k * ld, 0, sizeof(int64_t) * L1, stream);
    if (e == hipSuccess) e = hipMemsetAsync(n_bad, 0, sizeof(int32_t), stream);
    if (e != hipSuccess) return e;
    if (n > 0 && n_slots > 0 && L > 0) {
        const ObjectRows rows{start, end, slot, cell_of_row, time_start, offsets, n, C, n_slots, L, nullptr, 0};
        hipLaunchKernelGGL(tracks_scatter, dim3(blocks_for(n)), dim3(kTrkThreads), 0, stream, rows, vec, ldv, n_cells,
                           reinterpret_cast<u64*>(sums), ld, n_bad);
        scan_level(n_cells, sums, ld, L + 1, scratch, stream);
    }
    return hipGetLastError();
}

}  // namespace xmhw
