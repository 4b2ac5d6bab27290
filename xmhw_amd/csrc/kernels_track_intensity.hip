// kernels_track_intensity.hip -- mhw_track_intensity(): how hot every selected object was on each of its days.  The
// first reduction that joins the resident series, the climatology and the object partition, so it is the first object
// stage that visits voxels.  Entry offsets[i] + (t - time_start[i]) of the ragged arrays of
// mhw_tracks() receives, over the voxels of object i on day t (cells with a row of i that covers t):
//   n_valid, wsum_i, isum_q   the number of voxels with a non-NaN anomaly a = x - seas (x = the sample, negated for cold
//                             spells: the expression of event_stats), the sum of their integer weights wi[c] and of
//                             wi[c] * rint(a * 2^16);
//   key                       the largest order-preserving key of a + 0.0 (device_common.h), 0 = none;
//   cat_cells[4]              the voxels whose per-step category floor(1 + (x - thresh) / (thresh - seas)) is 1, 2, 3, >= 4.
//
//   track_intensity_accumulate  lane = cell, a wave = 64 consecutive cells (256 contiguous bytes of a float32 row), a
//                     workgroup = 256 cells x one chunk of kTrackIntensityChunk steps.  A lane finds the first row of its
//                     cell that ends at or behind the chunk's first step by a binary search, then walks rows and steps
//                     together; row_of_t[t] is uniform over the wave.  Only a lane inside a selected row loads its
//                     sample and climatology rows.  Neighbouring lanes often address the same entry (objects are
//                     spatially coherent), so runs of equal target entries are combined in the wave by one segmented
//                     scan (shuffles) and only the last lane of a run issues the atomics: a step of a wave that lies
//                     in one object costs one set of atomics instead of 64.  Integer atomics without a return value:
//                     the result does not depend on the order, the chunks or the slabs.  No kernel waits for another
//                     workgroup.  A voxel with |a| >= 2^7 or infinite is left out and counted (*n_range); a voxel of a
//                     row whose days leave its object's entries is left out and counted (*n_bad): nothing outside
//                     entries 0..L-1 is ever written.
//   the finish                  key -> float64 (NaN where no voxel had a value): launch_keys_to_f64 (kernels.h).
#include "../../include/xmhw_amd.h"
#include "entry_common.h"
#include "stage_reduce.h"

namespace xmhw {

namespace {

constexpr int kTiThreads = 256;
using u64 = unsigned long long;

struct TiAcc {
    int32_t* n_valid;
    u64 *wsum, *isum, *key;
    int32_t* cat;
    int64_t ldcat;
    u64 *n_range, *n_bad;
};

// what a voxel adds: cnt packs five counts of at most 64 in 8 bits each (valid, then the four categories)
struct TiPart {
    u64 cnt, w, is, key;
};

__device__ __forceinline__ void combine(TiPart& a, const TiPart& b) {
    a.cnt += b.cnt;
    a.w += b.w;
    a.is += b.is;
    a.key = b.key > a.key ? b.key : a.key;
}

__device__ __forceinline__ u64 shfl_u64(u64 v, int src) {
    return static_cast<u64>(__shfl(static_cast<long long>(v), src, 64));
}

__device__ __forceinline__ void flush(const TiAcc& o, int64_t p, const TiPart& v) {
    if (v.cnt == 0) return;                          // no valid voxel and no category: nothing to add
    const int32_t nv = static_cast<int32_t>(v.cnt & 0xFF);
    if (nv) atomicAdd(o.n_valid + p, nv);
    if (v.w) atomicAdd(o.wsum + p, v.w);
    if (v.is) atomicAdd(o.isum + p, v.is);
    if (v.key) atomicMax(o.key + p, v.key);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int32_t n = static_cast<int32_t>((v.cnt >> (8 * (k + 1))) & 0xFF);
        if (n) atomicAdd(o.cat + k * o.ldcat + p, n);
    }
}

template <typename T, bool COMBINE>
__global__ __launch_bounds__(kTiThreads) void track_intensity_accumulate(
    const T* __restrict__ ts, int64_t Tn, int64_t n, int64_t ld, const double* __restrict__ seas,
    const double* __restrict__ thresh, int64_t ldc, const int32_t* __restrict__ row_of_t, int32_t negate,
    const int32_t* __restrict__ rstart, const int32_t* __restrict__ rend, const int32_t* __restrict__ rslot,
    int64_t n_rows, const int64_t* __restrict__ roff, const int64_t* __restrict__ wi, const int32_t* __restrict__ time_start,
    const int64_t* __restrict__ offsets, int64_t n_slots, int64_t L, TiAcc out) {
    const int lane = threadIdx.x & 63;
    const int64_t c = static_cast<int64_t>(blockIdx.x) * kTiThreads + threadIdx.x;
    const bool cell = c < n;
    const int64_t nchunks = (Tn + kTrackIntensityChunk - 1) / kTrackIntensityChunk;
    const u64 w = cell ? static_cast<u64>(wi[c]) : 0;
    int64_t jbeg = cell ? roff[c] : 0, jend = cell ? roff[c + 1] : 0;
    jbeg = jbeg < 0 ? 0 : jbeg;                      // offsets that do not describe the rows read no row outside them
    jend = jend > n_rows ? n_rows : jend;
    for (int64_t ch = blockIdx.y; ch < nchunks; ch += gridDim.y) {
        const int64_t t0 = ch * kTrackIntensityChunk;
        const int64_t t1 = t0 + kTrackIntensityChunk < Tn ? t0 + kTrackIntensityChunk : Tn;
        int64_t j = jbeg, hi = jend;
        while (j < hi) {                             // the first row of the cell with end >= t0
            const int64_t mid = j + (hi - j) / 2;
            if (rend[mid] < t0) j = mid + 1; else hi = mid;
        }
        int64_t s = t1, e = -1, base = 0;            // the row the lane stands on: days s..e, entry = base + t
        bool fresh = true, selected = false, fits = false;
        for (int64_t t = t0; t < t1; ++t) {
            while (j < jend && !fresh && e < t) { ++j; fresh = true; }
            if (fresh && j < jend) {
                s = rstart[j];
                e = rend[j];
                const int32_t sl = rslot[j];
                selected = sl >= 0 && sl < n_slots && s < t1;       // (a row behind the chunk is loaded again by the next)
                if (selected) {
                    const int64_t o0 = offsets[sl], o1 = offsets[sl + 1];
                    base = o0 - time_start[sl];
                    fits = o0 >= 0 && o1 <= L && base + s >= o0 && base + e < o1;
                }
                fresh = false;
            }
            const bool in = j < jend && selected && s <= t && t <= e;
            if (__ballot(in) == 0) continue;         // uniform over the wave: the row of samples is not read
            TiPart v{0, 0, 0, 0};
            int64_t p = -1;
            if (in) {
                if (!fits) {
                    atomicAdd(out.n_bad, u64{1});
                } else {
                    const int64_t r = row_of_t[t];
                    double x = static_cast<double>(ts[t * ld + c]);
                    if (negate) x = -x;
                    const double se = seas[r * ldc + c], th = thresh[r * ldc + c];
                    const double a = x - se;
                    if (a == a) {
                        if (!(fabs(a) < kFixedRange)) {
                            atomicAdd(out.n_range, u64{1});
                        } else {
                            p = base + t;
                            const double cat = step_category(x, th, se);
                            const int k = cat == 1.0 ? 1 : cat == 2.0 ? 2 : cat == 3.0 ? 3 : cat >= 4.0 ? 4 : 0;
                            v.cnt = 1 | (k ? u64{1} << (8 * k) : 0);
                            v.w = w;
                            v.is = w * static_cast<u64>(fixed_value(a));
                            v.key = f64_key(a + 0.0);                              // -0.0 counts as 0.0
                        }
                    }
                }
            }
            if (!COMBINE) {
                if (p >= 0) flush(out, p, v);
                continue;
            }
            const int64_t prev = __shfl_up(static_cast<long long>(p), 1, 64);
            const bool head = lane == 0 || prev != p;
            const uint64_t heads = __ballot(head);
            const int first_lane = 63 - __builtin_clzll(heads & (~uint64_t{0} >> (63 - lane)));   // where the lane's run starts
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int src = lane >= d ? lane - d : lane;
                const TiPart q{shfl_u64(v.cnt, src), shfl_u64(v.w, src), shfl_u64(v.is, src), shfl_u64(v.key, src)};
                if (lane - d >= first_lane) combine(v, q);
            }
            const int64_t next = __shfl_down(static_cast<long long>(p), 1, 64);
            if (p >= 0 && (lane == 63 || next != p)) flush(out, p, v);             // the last lane of a run holds its total
        }
    }
}

hipError_t launch_track_intensity_init(int64_t L, int32_t* n_valid, int64_t* wsum_i, int64_t* isum_q, double* intensity_max,
                                       int32_t* cat_cells, int64_t ldcat, int64_t* n_range, int64_t* n_bad,
                                       hipStream_t stream) {
    const size_t m = static_cast<size_t>(L);
    hipError_t e = hipMemsetAsync(n_range, 0, sizeof(int64_t), stream);
    if (e == hipSuccess) e = hipMemsetAsync(n_bad, 0, sizeof(int64_t), stream);
    if (m == 0 || e != hipSuccess) return e;
    e = hipMemsetAsync(n_valid, 0, sizeof(int32_t) * m, stream);
    if (e == hipSuccess) e = hipMemsetAsync(wsum_i, 0, sizeof(int64_t) * m, stream);
    if (e == hipSuccess) e = hipMemsetAsync(isum_q, 0, sizeof(int64_t) * m, stream);
    if (e == hipSuccess) e = hipMemsetAsync(intensity_max, 0, sizeof(double) * m, stream);        // key 0: no value yet
    for (int k = 0; k < 4 && e == hipSuccess; ++k) e = hipMemsetAsync(cat_cells + k * ldcat, 0, sizeof(int32_t) * m, stream);
    return e;
}

template <typename T>
hipError_t launch_track_intensity_accumulate(const T* ts, int64_t Tn, int64_t n, int64_t ld, const double* seas,
                                             const double* thresh, int64_t ldc, const int32_t* row_of_t, int32_t negate,
                                             const int32_t* start, const int32_t* end, const int32_t* slot,
                                             int64_t n_rows, const int64_t* row_offsets, const int64_t* wi, const int32_t* time_start,
                                             const int64_t* offsets, int64_t n_slots, int64_t L, int32_t* n_valid,
                                             int64_t* wsum_i, int64_t* isum_q, double* intensity_max, int32_t* cat_cells,
                                             int64_t ldcat, int64_t* n_range, int64_t* n_bad, int32_t combine_runs,
                                             hipStream_t stream) {
    if (n <= 0 || Tn <= 0 || n_rows <= 0 || n_slots <= 0 || L <= 0) return hipSuccess;
    const TiAcc out{n_valid, reinterpret_cast<u64*>(wsum_i), reinterpret_cast<u64*>(isum_q),
                    reinterpret_cast<u64*>(intensity_max), cat_cells, ldcat, reinterpret_cast<u64*>(n_range),
                    reinterpret_cast<u64*>(n_bad)};
    const dim3 grid = stage_grid(n, kTiThreads, Tn, kTrackIntensityChunk), block(kTiThreads);
    if (combine_runs)
        hipLaunchKernelGGL((track_intensity_accumulate<T, true>), grid, block, 0, stream, ts, Tn, n, ld, seas, thresh, ldc,
                           row_of_t, negate, start, end, slot, n_rows, row_offsets, wi, time_start, offsets, n_slots, L, out);
    else
        hipLaunchKernelGGL((track_intensity_accumulate<T, false>), grid, block, 0, stream, ts, Tn, n, ld, seas, thresh, ldc,
                           row_of_t, negate, start, end, slot, n_rows, row_offsets, wi, time_start, offsets, n_slots, L, out);
    return hipGetLastError();
}

hipError_t launch_track_intensity_finish(int64_t L, double* intensity_max, hipStream_t stream) {
    if (L <= 0) return hipSuccess;
    return launch_keys_to_f64(intensity_max, 1, L, L, stream);
}

}  // namespace

}  // namespace xmhw

// ---- the C entries of mhw_track_intensity() (include/xmhw_amd.h) ------------------------------------------------------
namespace {

using namespace xmhw::entry;

static std::atomic<int> g_track_intensity_combine{1};   // runs of equal entries summed in the wave (xmhw_set_track_intensity_combine)

template <typename T>
int track_intensity_accumulate(const T* ts, int64_t Tn, int64_t n, int64_t ld, const double* seas, const double* thresh,
                               int64_t ldc, int64_t D, const int32_t* row_of_t, int32_t negate, const int32_t* start,
                               const int32_t* end, const int32_t* slot, int64_t n_rows, const int64_t* row_offsets,
                               const int64_t* wi, const int32_t* time_start, const int64_t* offsets, int64_t n_slots,
                               int64_t L, int32_t* n_valid, int64_t* wsum_i, int64_t* isum_q, double* intensity_max,
                               int32_t* cat_cells, int64_t ldcat, int64_t* n_range, int64_t* n_bad, void* stream) {
    if (Tn <= 0 || n < 0 || ld < n || ldc < n || D < 1) return fail(XMHW_ERR_INVALID, "bad T/n/ld/ldc/D");
    if (n_rows < 0 || n_slots < 0 || L < 0 || ldcat < L) return fail(XMHW_ERR_INVALID, "bad n_rows/n_slots/L/ldcat");
    if (Tn > 0x7FFFFFFFll || n > 0x7FFFFFFFll || n_rows > 0x7FFFFFFFll || n_slots > 0x7FFFFFFFll || L > 0x7FFFFFFFll)
        return fail(XMHW_ERR_UNSUPPORTED, "track_intensity: 2^31 steps, cells, rows, slots or series entries and more");
    if (n == 0 || n_rows == 0 || n_slots == 0 || L == 0) return XMHW_OK;
    if (!ts || !seas || !thresh || !row_of_t || !start || !end || !slot || !row_offsets || !wi || !time_start || !offsets)
        return fail(XMHW_ERR_INVALID, "NULL buffer");
    if (!n_valid || !wsum_i || !isum_q || !intensity_max || !cat_cells || !n_range || !n_bad)
        return fail(XMHW_ERR_INVALID, "NULL output buffer");
    if (int rc = check_labels(row_of_t, Tn, 0, D, kRowsOutside)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    RowsRef rows;
    if (int rc = upload_table(row_of_t, Tn, "row table upload", &rows)) return rc;
    return status_of(xmhw::launch_track_intensity_accumulate<T>(ts, Tn, n, ld, seas, thresh, ldc, rows->d_rows, negate,
                                                                start, end, slot, n_rows, row_offsets, wi, time_start,
                                                                offsets, n_slots, L, n_valid, wsum_i, isum_q, intensity_max,
                                                                cat_cells, ldcat, n_range, n_bad,
                                                                g_track_intensity_combine.load(), st),
                     "track_intensity_accumulate launch");
}

}  // namespace

extern "C" {

int xmhw_set_track_intensity_combine(int32_t on) {
    if (on != 0 && on != 1) return fail(XMHW_ERR_INVALID, "on must be 0 or 1");
    g_track_intensity_combine = on;
    return XMHW_OK;
}
int xmhw_track_intensity_init(int64_t L, int32_t* n_valid, int64_t* wsum_i, int64_t* isum_q, double* intensity_max,
                              int32_t* cat_cells, int64_t ldcat, int64_t* n_range, int64_t* n_bad, void* stream) {
    if (L < 0 || ldcat < L) return fail(XMHW_ERR_INVALID, "bad L/ldcat");
    if (L > 0x7FFFFFFFll) return fail(XMHW_ERR_UNSUPPORTED, "track_intensity: 2^31 series entries and more");
    if (!n_range || !n_bad || (L > 0 && (!n_valid || !wsum_i || !isum_q || !intensity_max || !cat_cells)))
        return fail(XMHW_ERR_INVALID, "NULL output buffer");
    return status_of(xmhw::launch_track_intensity_init(L, n_valid, wsum_i, isum_q, intensity_max, cat_cells, ldcat, n_range,
                                                       n_bad, static_cast<hipStream_t>(stream)),
                     "track_intensity_init");
}
int xmhw_track_intensity_accumulate_f32(const float* ts, int64_t T, int64_t n, int64_t ld, const double* seas,
                                        const double* thresh, int64_t ldc, int64_t D, const int32_t* row_of_t, int32_t negate,
                                        const int32_t* start, const int32_t* end, const int32_t* slot, int64_t n_rows,
                                        const int64_t* row_offsets, const int64_t* wi, const int32_t* time_start,
                                        const int64_t* offsets, int64_t n_slots, int64_t L, int32_t* n_valid, int64_t* wsum_i,
                                        int64_t* isum_q, double* intensity_max, int32_t* cat_cells, int64_t ldcat,
                                        int64_t* n_range, int64_t* n_bad, void* stream) {
    return track_intensity_accumulate<float>(ts, T, n, ld, seas, thresh, ldc, D, row_of_t, negate, start, end, slot, n_rows,
                                             row_offsets, wi, time_start, offsets, n_slots, L, n_valid, wsum_i, isum_q,
                                             intensity_max, cat_cells, ldcat, n_range, n_bad, stream);
}
int xmhw_track_intensity_accumulate_f64(const double* ts, int64_t T, int64_t n, int64_t ld, const double* seas,
                                        const double* thresh, int64_t ldc, int64_t D, const int32_t* row_of_t, int32_t negate,
                                        const int32_t* start, const int32_t* end, const int32_t* slot, int64_t n_rows,
                                        const int64_t* row_offsets, const int64_t* wi, const int32_t* time_start,
                                        const int64_t* offsets, int64_t n_slots, int64_t L, int32_t* n_valid, int64_t* wsum_i,
                                        int64_t* isum_q, double* intensity_max, int32_t* cat_cells, int64_t ldcat,
                                        int64_t* n_range, int64_t* n_bad, void* stream) {
    return track_intensity_accumulate<double>(ts, T, n, ld, seas, thresh, ldc, D, row_of_t, negate, start, end, slot, n_rows,
                                              row_offsets, wi, time_start, offsets, n_slots, L, n_valid, wsum_i, isum_q,
                                              intensity_max, cat_cells, ldcat, n_range, n_bad, stream);
}
int xmhw_track_intensity_finish(int64_t L, double* intensity_max, void* stream) {
    if (L < 0) return fail(XMHW_ERR_INVALID, "bad L");
    if (L > 0x7FFFFFFFll) return fail(XMHW_ERR_UNSUPPORTED, "track_intensity: 2^31 series entries and more");
    if (L == 0) return XMHW_OK;
    if (!intensity_max) return fail(XMHW_ERR_INVALID, "NULL output buffer");
    return status_of(xmhw::launch_track_intensity_finish(L, intensity_max, static_cast<hipStream_t>(stream)),
                     "track_intensity_finish launch");
}

}  // extern "C"
