// kernels_class.hip -- mhw_days_by(): per cell and per CLASS of time steps (month, season, year, phase of a climate
// mode: class_of_t[t] in [-1, K), -1 = the step counts nowhere), the number of in-event steps by category and the
// sum / maximum of their anomaly.  mhw_coverage()'s kernel turned by ninety degrees: reduce over time, keep the cell.
// For every class k and cell c, over the in-event steps t (the bitmap of event_day_bits, kernels_coverage.hip) with
// class_of_t[t] == k, x = the sample as float64 (negated for cold spells), a = x - seas[row(t)] (the expression of
// event_stats), cat = floor(1 + (x - thresh) / (thresh - seas)):
//   days[k][0..3][c]     steps with cat == 1, == 2, == 3, >= 4
//   days[k][4][c]        all in-event steps
//   days[k][5][c]        n_valid: in-event steps with a not NaN and |a| < 2^7
//   isum_q[k][c]         sum of rint(a * 2^16) over the valid steps
//   key[k][c]            the largest order-preserving key of a + 0.0 over the valid steps (device_common.h), 0 = none
// A step with a not NaN and |a| >= 2^7 (or infinite) stays in days[k][0..4] and is counted in *n_range.
//
//   class_days_accumulate  the frame of a class reduction (kernels.h), eight addends per lane (a wave reads 256
//                     contiguous bytes of a float32 row).  Calendar classes come in runs of ~30 and more steps, so
//                     flushes are rare; a class that changes every step flushes every step and is still exact.  The
//                     in-event word of 64 steps is read once per word; only in-event lanes read their sample and
//                     climatology rows; a step whose class is -1, or on which no lane of the wave is in an event, reads
//                     nothing.
//   keys_to_f64       key -> float64 (NaN where no step, voxel or row had a value), in place: the finish of this stage,
//                     of mhw_track_intensity() and of mhw_objects() (launch_keys_to_f64, kernels.h).
#include "../../include/xmhw_amd.h"
#include "entry_common.h"
#include "stage_reduce.h"

namespace xmhw {

namespace {

constexpr int kCdThreads = 256;
using u64 = unsigned long long;

struct CdOut {
    int32_t* days;                                   // [K][6][ldo]
    u64 *isum, *key;                                 // [K][ldo]
    int64_t ldo;
    u64* n_range;
};

// the addends of one lane for the current class
struct CdAcc {
    int32_t n[kClassDaysChannels];
    u64 is, key;
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int j = 0; j < kClassDaysChannels; ++j) n[j] = 0;
        is = 0;
        key = 0;
    }
};

__device__ __forceinline__ void flush(const CdOut& o, int32_t k, int64_t c, CdAcc& v) {
    if (v.n[4] == 0) return;                         // every addend belongs to an in-event step
    int32_t* d = o.days + (static_cast<int64_t>(k) * kClassDaysChannels) * o.ldo + c;
#pragma unroll
    for (int j = 0; j < kClassDaysChannels; ++j)
        if (v.n[j]) atomicAdd(d + j * o.ldo, v.n[j]);
    const int64_t p = static_cast<int64_t>(k) * o.ldo + c;
    if (v.is) atomicAdd(o.isum + p, v.is);
    if (v.key) atomicMax(o.key + p, v.key);
    v.clear();
}

template <typename T>
__global__ __launch_bounds__(kCdThreads) void class_days_accumulate(
    const T* __restrict__ ts, int64_t Tn, int64_t C, int64_t ld, const double* __restrict__ seas,
    const double* __restrict__ thresh, int64_t ldc, const int32_t* __restrict__ row_of_t,
    const int32_t* __restrict__ class_of_t, int32_t K, int32_t negate, const uint64_t* __restrict__ inev, int64_t ldi,
    int64_t tb, CdOut out) {
    const int64_t c = static_cast<int64_t>(blockIdx.x) * kCdThreads + threadIdx.x;
    const bool live = c < C;
    const int64_t nblk = (Tn + tb - 1) / tb;
    CdAcc v;
    v.clear();
    u64 n_range = 0;
    for (int64_t blk = blockIdx.y; blk < nblk; blk += gridDim.y) {
        const int64_t t0 = blk * tb;
        const int64_t t1 = Tn - t0 > tb ? t0 + tb : Tn;
        int32_t kcur = -1;                           // the class the addends belong to (uniform over the wave)
        int64_t wi = -1;
        uint64_t word = 0;
        for (int64_t t = t0; t < t1; ++t) {
            const int32_t k = class_of_t[t];
            if (k < 0 || k >= K) continue;           // counts nowhere (labels are checked on the host): reads nothing
            if ((t >> 6) != wi) {
                wi = t >> 6;
                word = live ? inev[wi * ldi + c] : 0;
            }
            const bool ev = (word >> (t & 63)) & 1;
            if (__ballot(ev) == 0) continue;         // uniform over the wave: the row of samples is not read
            if (k != kcur) {
                if (kcur >= 0) flush(out, kcur, c, v);
                kcur = k;
            }
            if (!ev) continue;
            const int64_t r = row_of_t[t];
            double x = static_cast<double>(ts[t * ld + c]);
            if (negate) x = -x;
            const double se = seas[r * ldc + c], th = thresh[r * ldc + c];
            const double a = x - se;
            const double cat = step_category(x, th, se);
            v.n[0] += cat == 1.0;
            v.n[1] += cat == 2.0;
            v.n[2] += cat == 3.0;
            v.n[3] += cat >= 4.0;
            v.n[4] += 1;
            if (a == a) {
                if (!(fabs(a) < kFixedRange)) {
                    ++n_range;
                } else {
                    v.n[5] += 1;
                    v.is += static_cast<u64>(fixed_value(a));
                    const u64 key = f64_key(a + 0.0);                       // -0.0 counts as 0.0
                    v.key = key > v.key ? key : v.key;
                }
            }
        }
        if (kcur >= 0) flush(out, kcur, c, v);
    }
    if (n_range) atomicAdd(out.n_range, n_range);
}

// keys -> float64, 0 -> NaN, in place: row blockIdx.y of `rows` rows of `cols` keys, leading dimension ld
__global__ __launch_bounds__(kCdThreads) void keys_to_f64(int64_t cols, int64_t ld, u64* __restrict__ key) {
    const int64_t c = static_cast<int64_t>(blockIdx.x) * kCdThreads + threadIdx.x;
    if (c >= cols) return;
    const int64_t p = static_cast<int64_t>(blockIdx.y) * ld + c;
    const u64 q = key[p];
    const double v = q ? key_f64(q) : make_nan();
    key[p] = static_cast<u64>(__double_as_longlong(v));
}

}  // namespace

hipError_t launch_keys_to_f64(double* key, int64_t rows, int64_t cols, int64_t ld, hipStream_t stream) {
    if (rows <= 0 || cols <= 0) return hipSuccess;
    if (rows > kStageMaxBlocks) return hipErrorInvalidValue;
    hipLaunchKernelGGL(keys_to_f64, dim3(static_cast<unsigned>(ceil_div(cols, kCdThreads)), static_cast<unsigned>(rows)),
                       dim3(kCdThreads), 0, stream, cols, ld, reinterpret_cast<u64*>(key));
    return hipGetLastError();
}

namespace {

hipError_t launch_class_days_init(int32_t K, int64_t C, int32_t* days, int64_t* isum_q, double* intensity_max, int64_t ldo,
                                  int64_t* n_range, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(n_range, 0, sizeof(int64_t), stream);
    if (e == hipSuccess) e = zero_rows(days, sizeof(int32_t), static_cast<int64_t>(K) * kClassDaysChannels, C, ldo, stream);
    if (e == hipSuccess) e = zero_rows(isum_q, sizeof(int64_t), K, C, ldo, stream);
    if (e == hipSuccess) e = zero_rows(intensity_max, sizeof(double), K, C, ldo, stream);      // key 0: no value yet
    return e;
}

template <typename T>
hipError_t launch_class_days_accumulate(const T* ts, int64_t Tn, int64_t C, int64_t ld, const double* seas,
                                        const double* thresh, int64_t ldc, const int32_t* row_of_t,
                                        const int32_t* class_of_t, int32_t K, int32_t negate, const uint64_t* inev,
                                        int64_t ldi, int64_t block_steps, int32_t* days, int64_t* isum_q,
                                        double* intensity_max, int64_t ldo, int64_t* n_range, hipStream_t stream) {
    if (C <= 0 || Tn <= 0 || K <= 0) return hipSuccess;
    const int64_t tb = block_steps > 0 ? block_steps : class_days_auto_block(Tn, C);
    const CdOut out{days, reinterpret_cast<u64*>(isum_q), reinterpret_cast<u64*>(intensity_max), ldo,
                    reinterpret_cast<u64*>(n_range)};
    hipLaunchKernelGGL(class_days_accumulate<T>, stage_grid(C, kCdThreads, Tn, tb), dim3(kCdThreads), 0, stream, ts, Tn, C,
                       ld, seas, thresh, ldc, row_of_t, class_of_t, K, negate, inev, ldi, tb, out);
    return hipGetLastError();
}

hipError_t launch_class_days_finish(int32_t K, int64_t C, double* intensity_max, int64_t ldo, hipStream_t stream) {
    if (K <= 0 || C <= 0) return hipSuccess;
    return launch_keys_to_f64(intensity_max, K, C, ldo, stream);       // K <= kClassDaysMaxClasses rows
}

}  // namespace

}  // namespace xmhw

// ---- the C entries of mhw_days_by() (include/xmhw_amd.h) --------------------------------------------------------------
namespace {

using namespace xmhw::entry;

static std::atomic<int> g_class_days_block{0};   // steps a workgroup takes per block, 0 = automatic (xmhw_set_class_days_block)

static int class_days_check_k(int32_t K) {
    if (K < 1 || K > xmhw::kClassDaysMaxClasses)
        return fail(XMHW_ERR_UNSUPPORTED, "class_days: K must be in [1, " + std::to_string(xmhw::kClassDaysMaxClasses) + "]");
    return XMHW_OK;
}

template <typename T>
int class_days_accumulate(const T* ts, int64_t Tn, int64_t C, int64_t ld, const double* seas, const double* thresh,
                          int64_t ldc, const int32_t* row_of_t, int32_t negate, const uint64_t* bits, int64_t ldb,
                          int32_t min_duration, int32_t join_gaps, int32_t max_gap, const int32_t* class_of_t, int32_t K,
                          int32_t* days, int64_t* isum_q, double* intensity_max, int64_t ldo, int64_t* n_range,
                          void* stream) {
    if (class_days_check_k(K) != XMHW_OK) return XMHW_ERR_UNSUPPORTED;
    if (Tn > 0x7FFFFFFFll || C > 0x7FFFFFFFll) return fail(XMHW_ERR_UNSUPPORTED, "class_days: 2^31 steps or cells and more");
    if (Tn <= 0 || C < 0 || ld < C || ldc < C || ldb < C || ldo < C) return fail(XMHW_ERR_INVALID, "bad T/C/ld/ldc/ldb/ldo");
    if (min_duration < 1 || max_gap < 0) return fail(XMHW_ERR_INVALID, "bad minDuration/maxGap");
    if (!class_of_t) return fail(XMHW_ERR_INVALID, "NULL class_of_t");
    if (int rc = check_labels(class_of_t, Tn, -1, K, kClassesOutside)) return rc;
    if (C == 0) return XMHW_OK;
    if (!ts || !seas || !thresh || !row_of_t || !bits || !days || !isum_q || !intensity_max || !n_range)
        return fail(XMHW_ERR_INVALID, "NULL buffer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    RowsRef rows;
    if (int rc = upload_table(row_of_t, Tn, "row table upload", &rows)) return rc;
    RowsRef classes;                                   // the same content-keyed cache: one more int32[T] table
    if (int rc = upload_table(class_of_t, Tn, "class table upload", &classes)) return rc;
    ScratchRef scratch;
    const uint64_t* inev = nullptr;
    if (int rc = event_day_bitmap(bits, Tn, C, ldb, min_duration, join_gaps, max_gap, st, &scratch, &inev)) return rc;
    return status_of(xmhw::launch_class_days_accumulate<T>(ts, Tn, C, ld, seas, thresh, ldc, rows->d_rows, classes->d_rows,
                                                           K, negate, inev, C, g_class_days_block.load(), days, isum_q,
                                                           intensity_max, ldo, n_range, st),
                     "class_days_accumulate launch");
}

}  // namespace

extern "C" {

int xmhw_set_class_days_block(int32_t steps) { return set_knob(g_class_days_block, steps, "steps must be >= 0"); }
int xmhw_class_days_init(int32_t K, int64_t C, int32_t* days, int64_t* isum_q, double* intensity_max, int64_t ldo,
                         int64_t* n_range, void* stream) {
    if (class_days_check_k(K) != XMHW_OK) return XMHW_ERR_UNSUPPORTED;
    if (C > 0x7FFFFFFFll) return fail(XMHW_ERR_UNSUPPORTED, "class_days: 2^31 cells and more");
    if (C < 0 || ldo < C) return fail(XMHW_ERR_INVALID, "bad C/ldo");
    if (!n_range || (C > 0 && (!days || !isum_q || !intensity_max))) return fail(XMHW_ERR_INVALID, "NULL output buffer");
    return status_of(xmhw::launch_class_days_init(K, C, days, isum_q, intensity_max, ldo, n_range,
                                                  static_cast<hipStream_t>(stream)),
                     "class_days_init");
}
int xmhw_class_days_accumulate_f32(const float* ts, int64_t T, int64_t C, int64_t ld, const double* seas, const double* thresh,
                                   int64_t ldc, const int32_t* row_of_t, int32_t negate, const uint64_t* bits, int64_t ldb,
                                   int32_t min_duration, int32_t join_gaps, int32_t max_gap, const int32_t* class_of_t,
                                   int32_t K, int32_t* days, int64_t* isum_q, double* intensity_max, int64_t ldo,
                                   int64_t* n_range, void* stream) {
    return class_days_accumulate<float>(ts, T, C, ld, seas, thresh, ldc, row_of_t, negate, bits, ldb, min_duration, join_gaps,
                                        max_gap, class_of_t, K, days, isum_q, intensity_max, ldo, n_range, stream);
}
int xmhw_class_days_accumulate_f64(const double* ts, int64_t T, int64_t C, int64_t ld, const double* seas, const double* thresh,
                                   int64_t ldc, const int32_t* row_of_t, int32_t negate, const uint64_t* bits, int64_t ldb,
                                   int32_t min_duration, int32_t join_gaps, int32_t max_gap, const int32_t* class_of_t,
                                   int32_t K, int32_t* days, int64_t* isum_q, double* intensity_max, int64_t ldo,
                                   int64_t* n_range, void* stream) {
    return class_days_accumulate<double>(ts, T, C, ld, seas, thresh, ldc, row_of_t, negate, bits, ldb, min_duration, join_gaps,
                                         max_gap, class_of_t, K, days, isum_q, intensity_max, ldo, n_range, stream);
}
int xmhw_class_days_finish(int32_t K, int64_t C, double* intensity_max, int64_t ldo, void* stream) {
    if (class_days_check_k(K) != XMHW_OK) return XMHW_ERR_UNSUPPORTED;
    if (C > 0x7FFFFFFFll) return fail(XMHW_ERR_UNSUPPORTED, "class_days: 2^31 cells and more");
    if (C < 0 || ldo < C) return fail(XMHW_ERR_INVALID, "bad C/ldo");
    if (C == 0) return XMHW_OK;
    if (!intensity_max) return fail(XMHW_ERR_INVALID, "NULL output buffer");
    return status_of(xmhw::launch_class_days_finish(K, C, intensity_max, ldo, static_cast<hipStream_t>(stream)),
                     "class_days_finish launch");
}

}  // extern "C"
