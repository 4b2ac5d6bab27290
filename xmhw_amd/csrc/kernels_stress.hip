// kernels_stress.hip -- heat_stress(): accumulated thermal stress (the Degree Heating Week of NOAA Coral Reef Watch) and
// the per-class sums of the plain series that its baseline, the Maximum Monthly Mean, is made of.
//
// Class sums.  For every class k (class_of_t[t] in [-1, K), -1 = the step counts nowhere) and cell c, over the steps of
// class k with d = float64(sample) - x0 not NaN and |d| < 2^7:
//   n_valid[k][c]        the contributing steps
//   sum_q[k][c]          the sum of rint(d * 2^16)
// Any other non-NaN d is left out and counted in *n_range.
//
// Heat stress.  x = the sample as float64, b = base[row_of_t[t]][c], both negated for cold spells, h = x - b.  The step
// is HOT iff h == h, h >= h0 and h < 2^7; q(t) = rint(h * 2^16) on hot steps and 0 otherwise; S(t) = the sum of q over the
// steps max(0, t - W + 1) .. t (W <= 255: S < 2^31).  A step with h >= 2^7 or infinite is not hot and is counted in
// *n_range, whatever its class.  For every class k and cell c, over the steps of class k:
//   counts[k][0][c]      steps with h not NaN
//   counts[k][1][c]      hot steps
//   counts[k][2 + l][c]  steps with S(t) >= level_q[l], l < L <= 6 (the channels 2 + L .. 7 stay 0)
//   hsum_q[k][c]         the sum of q(t)
//   key[k][c]            the largest S(t) << 32 | ~t: the peak of S and the first step that attains it (0 = no step)
// and snap_q[j][c] = S(at[j]) whatever the class of that step.  A step of class -1 feeds the window and is reduced nowhere.
//
//   class_sums_accumulate, heat_stress_accumulate
//                     the frame of a class reduction (kernels.h) without the event bitmap; no barrier, no scratch.  A
//                     run of class -1 changes no class and costs no flush.
//                     The samples of several steps are requested together before the first of them is used: eight in
//                     registers for the class sums; 64 B per lane (16 float32 or 8 float64 steps) for the stress kernel,
//                     parked in the lane's own column of a 16 KB LDS stage and walked by a loop that is not unrolled --
//                     unrolled, the body with its flush, snapshot and window branches runs out of scalar registers.
//   the window        Inside a block S += q(t) - q(t - W).  q(t - W) is RE-DERIVED from the sample (and, for a base of many
//                     rows, the base row) of step t - W: a second stream W rows behind the first.  Why, of the three ways:
//                     * a window of W steps of one wave is W x 256 B of float32 samples (21 KB at W = 84, 65 KB at 255),
//                       the same bytes as a ring of q in LDS.  The 4 MiB L2 of an XCD is 128 KB per CU, less than the
//                       CU's 160 KB of LDS, so the second stream lives in L2 only at the occupancy a ring would allow
//                       (7 waves per CU at W = 84, 2 at W = 255).  At full occupancy (32 waves per CU) the windows of the
//                       resident workgroups are 2048 x 84 KB = 172 MB: the stream is served by the 256 MiB Infinity Cache,
//                       which delivers uniformly gathered rows above the HBM rate, and costs HBM nothing.
//                     * the ring in LDS reads HBM once whatever W and the type, but 7 (or 2) waves per CU must then keep
//                       some 48 KB of loads in flight per CU to stream from HBM, and W = 255 leaves no room for that.
//                     * registers cannot hold a window whose length is a run-time argument.
//                     The re-read is one path for every W and both sample types, with the occupancy of a streaming kernel,
//                     and it is skipped outright where it cannot matter: while a lane's S is 0 every q in its window is
//                     0 (q >= 0), so q(t - W) = 0 without a read -- heat stress is rare, and most steps of most cells
//                     take that path.  DESIGN.md 3.19 has the measured cost and what would follow if it binds.
//   time blocks       A block that starts at t0 > 0 first rebuilds the part of S(t0) that lies before it from the steps
//                     t0 - W + 1 .. t0 - 1: blocks are independent and exact, at W - 1 extra steps each.  The automatic
//                     block is at least 16 W steps (warm-up share below 1/16) and 256 steps, and about 4096 steps at
//                     most: measured faster than one block over the whole series (heat_stress_auto_block).
//   snapshots         plain stores by the block that owns the step.
//   heat_stress_finish     key -> peak_q = key >> 32, peak_t = ~key (low word); key 0 -> 0 and -1.
#include "../../include/xmhw_amd.h"
#include "entry_common.h"
#include "stage_reduce.h"

namespace xmhw {

namespace {

constexpr int kHsThreads = 256;
constexpr int kHsBatch = 4;                          // steps whose samples are requested together
using u64 = unsigned long long;

// ---- class sums ------------------------------------------------------------------------------------

struct CsOut {
    int32_t* n_valid;                                // [K][ldo]
    u64* sum;                                        // [K][ldo]
    int64_t ldo;
    u64* n_range;
};

__device__ __forceinline__ void cs_flush(const CsOut& o, int32_t k, int64_t c, int32_t& n, u64& s) {
    const int64_t p = static_cast<int64_t>(k) * o.ldo + c;
    if (n) atomicAdd(o.n_valid + p, n);
    if (s) atomicAdd(o.sum + p, s);
    n = 0;
    s = 0;
}

template <typename T>
__global__ __launch_bounds__(kHsThreads) void class_sums_accumulate(const T* __restrict__ ts, int64_t Tn, int64_t C,
                                                                    int64_t ld, double x0,
                                                                    const int32_t* __restrict__ class_of_t, int32_t K,
                                                                    int64_t tb, CsOut out) {
    const int64_t c = static_cast<int64_t>(blockIdx.x) * kHsThreads + threadIdx.x;
    if (c >= C) return;
    const int64_t nblk = (Tn + tb - 1) / tb;
    int32_t n = 0;
    u64 s = 0, n_range = 0;
    const auto flush_class = [&](int32_t k) { cs_flush(out, k, c, n, s); };
    for (int64_t blk = blockIdx.y; blk < nblk; blk += gridDim.y) {
        const auto [t0, t1] = block_range(blk, tb, Tn);
        ClassRun run;
        for (int64_t tc = t0; tc < t1; tc += kHsBatch) {
            int32_t kk[kHsBatch];
            T x[kHsBatch];
#pragma unroll
            for (int u = 0; u < kHsBatch; ++u) {
                const int64_t t = tc + u;
                kk[u] = t < t1 ? class_of_t[t] : -1;
                if (kk[u] >= K) kk[u] = -1;          // (labels are checked on the host)
                x[u] = kk[u] >= 0 ? ts[t * ld + c] : static_cast<T>(0);      // a step of class -1 reads nothing
            }
#pragma unroll
            for (int u = 0; u < kHsBatch; ++u) {
                const int32_t k = kk[u];
                if (k < 0) continue;
                run.enter(k, flush_class);
                const double d = static_cast<double>(x[u]) - x0;
                const int fixed = fixed_state(d);
                if (fixed < 0) ++n_range;
                if (fixed > 0) {
                    n += 1;
                    s += static_cast<u64>(fixed_value(d));
                }
            }
        }
        run.leave(flush_class);
    }
    if (n_range) atomicAdd(out.n_range, n_range);
}

// ---- heat stress -----------------------------------------------------------------------------------

template <typename T>
struct HsIn {
    const T* ts;
    int64_t ld;
    const double* base;                              // [D][ldb]
    int64_t ldb;
    const int32_t* row_of_t;
    int32_t one_row;                                 // D == 1: the base is a constant per cell, read once
    int32_t negate;
    double h0;
};

struct HsLevels {
    int32_t q[kHeatStressMaxLevels];                 // clamped to int32: S is one
    int32_t L;
};

struct HsOut {
    int32_t* counts;                                 // [K][8][ldo]
    u64 *hsum, *key;                                 // [K][ldo]
    int32_t* snap;                                   // [J][ldo]
    int64_t ldo;
    u64* n_range;
};

// the addends of one lane for the current class
struct HsAcc {
    int32_t n[kHeatStressChannels];
    u64 hs, key;
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int j = 0; j < kHeatStressChannels; ++j) n[j] = 0;
        hs = 0;
        key = 0;
    }
};

__device__ __forceinline__ void hs_flush(const HsOut& o, int32_t k, int64_t c, HsAcc& v) {
    if (v.key == 0) return;                          // every step of a class raises the key: no step, no addend
    int32_t* d = o.counts + (static_cast<int64_t>(k) * kHeatStressChannels) * o.ldo + c;
#pragma unroll
    for (int j = 0; j < kHeatStressChannels; ++j)
        if (v.n[j]) atomicAdd(d + j * o.ldo, v.n[j]);
    const int64_t p = static_cast<int64_t>(k) * o.ldo + c;
    if (v.hs) atomicAdd(o.hsum + p, v.hs);
    atomicMax(o.key + p, v.key);
    v.clear();
}

// h of step t from its sample; b0 = the (negated) base of a one-row baseline
template <typename T>
__device__ __forceinline__ double hs_h(const HsIn<T>& in, T sample, double b0, int64_t t, int64_t c) {
    double x = static_cast<double>(sample);
    double b = b0;
    if (!in.one_row) {
        b = in.base[static_cast<int64_t>(in.row_of_t[t]) * in.ldb + c];
        if (in.negate) b = -b;
    }
    if (in.negate) x = -x;
    return x - b;
}
__device__ __forceinline__ int32_t hs_q(double h, double h0) {
    return (h >= h0 && h < kFixedRange) ? static_cast<int32_t>(rint(h * kFixedOne)) : 0;      // NaN compares false
}
template <typename T>
__device__ __forceinline__ int32_t hs_q_at(const HsIn<T>& in, double b0, int64_t t, int64_t c) {
    return hs_q(hs_h(in, in.ts[t * in.ld + c], b0, t, c), in.h0);
}

template <typename T>
__global__ __launch_bounds__(kHsThreads) void heat_stress_accumulate(HsIn<T> in, int64_t Tn, int64_t C, int32_t W,
                                                                     const int32_t* __restrict__ class_of_t, int32_t K,
                                                                     HsLevels lv, const int32_t* __restrict__ at, int32_t J,
                                                                     int64_t tb, HsOut out) {
    constexpr int kStage = 64 / sizeof(T);           // 16 float32 or 8 float64 steps: 64 B per lane, 16 KB per workgroup
    __shared__ T stage[kStage][kHsThreads];
    const int64_t c = static_cast<int64_t>(blockIdx.x) * kHsThreads + threadIdx.x;
    if (c >= C) return;
    double b0 = 0.0;
    if (in.one_row) {
        b0 = in.base[c];
        if (in.negate) b0 = -b0;
    }
    // T < 2^31: steps and blocks are 32-bit here, addresses are not
    const int32_t Ts = static_cast<int32_t>(Tn), bs = static_cast<int32_t>(tb < Tn ? tb : Tn);
    const int32_t nblk = (Ts - 1) / bs + 1;
    HsAcc v;
    v.clear();
    u64 n_range = 0;
    for (int32_t blk = blockIdx.y; blk < nblk; blk += gridDim.y) {
        const auto [t0, t1] = block_range<int32_t>(blk, bs, Ts);
        // the part of S(t0) before the block: the steps t0 - W + 1 .. t0 - 1
        int32_t S = 0;
        for (int32_t i = t0 - W + 1 > 0 ? t0 - W + 1 : 0; i < t0; ++i) S += hs_q_at(in, b0, i, c);
        int32_t j = 0;                               // the next snapshot step (uniform)
        while (j < J && at[j] < t0) ++j;
        int32_t kcur = -1;                           // the class the addends belong to (uniform over the wave)
        for (int32_t tc = t0, n = 0; tc < t1; tc += n) {
            // the samples of the next kStage steps, requested together, wait in the lane's own column of the stage
            n = t1 - tc > kStage ? kStage : t1 - tc;
            const T* p = in.ts + static_cast<int64_t>(tc) * in.ld + c;
#pragma unroll
            for (int u = 0; u < kStage; ++u) {
                if (u < n) stage[u][threadIdx.x] = *p;
                p += in.ld;
            }
            for (int32_t u = 0; u < n; ++u) {
                const int32_t t = tc + u;
                const double h = hs_h(in, stage[u][threadIdx.x], b0, t, c);
                const bool valid = h == h;
                const int32_t q = hs_q(h, in.h0);              // hot iff q != 0: h0 >= 2^-16
                // the step that leaves the window; S == 0 here means that every q of the window is 0, that one included
                if (t > t0 && t >= W && S > 0) S -= hs_q_at(in, b0, t - W, c);
                S += q;
                if (valid && !(h < kFixedRange && h > -INFINITY)) ++n_range;  // h >= 2^7 or infinite
                if (j < J && at[j] == t) {
                    out.snap[static_cast<int64_t>(j) * out.ldo + c] = S;
                    ++j;
                }
                const int32_t k = class_of_t[t];
                if (k < 0 || k >= K) continue;       // reduced nowhere (labels are checked on the host)
                if (k != kcur) {
                    if (kcur >= 0) hs_flush(out, kcur, c, v);
                    kcur = k;
                }
                v.n[0] += valid;
                v.n[1] += q != 0;
#pragma unroll
                for (int l = 0; l < kHeatStressMaxLevels; ++l) v.n[2 + l] += l < lv.L && S >= lv.q[l];
                v.hs += static_cast<u64>(q);
                const u64 key = (static_cast<u64>(static_cast<uint32_t>(S)) << 32) | ~static_cast<uint32_t>(t);
                v.key = key > v.key ? key : v.key;
            }
        }
        if (kcur >= 0) hs_flush(out, kcur, c, v);
    }
    if (n_range) atomicAdd(out.n_range, n_range);
}

__global__ __launch_bounds__(kHsThreads) void heat_stress_finish(int32_t K, int64_t C, int64_t ldo, const u64* __restrict__ key,
                                                                 int32_t* __restrict__ peak_q, int32_t* __restrict__ peak_t) {
    const int64_t c = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (c >= C) return;
    for (int32_t k = blockIdx.y; k < K; k += gridDim.y) {
        const int64_t p = static_cast<int64_t>(k) * ldo + c;
        const u64 q = key[p];
        peak_q[p] = q ? static_cast<int32_t>(q >> 32) : 0;
        peak_t[p] = q ? static_cast<int32_t>(~static_cast<uint32_t>(q)) : -1;
    }
}

hipError_t launch_class_sums_init(int32_t K, int64_t C, int32_t* n_valid, int64_t* sum_q, int64_t ldo, int64_t* n_range,
                                  hipStream_t stream) {
    hipError_t e = hipMemsetAsync(n_range, 0, sizeof(int64_t), stream);
    if (e == hipSuccess) e = zero_rows(n_valid, sizeof(int32_t), K, C, ldo, stream);
    if (e == hipSuccess) e = zero_rows(sum_q, sizeof(int64_t), K, C, ldo, stream);
    return e;
}

template <typename T>
hipError_t launch_class_sums_accumulate(const T* ts, int64_t Tn, int64_t C, int64_t ld, double x0, const int32_t* class_of_t,
                                        int32_t K, int64_t block_steps, int32_t* n_valid, int64_t* sum_q, int64_t ldo,
                                        int64_t* n_range, hipStream_t stream) {
    if (C <= 0 || Tn <= 0 || K <= 0) return hipSuccess;
    const int64_t tb = block_steps > 0 ? block_steps : heat_stress_auto_block(Tn, C, 1);
    const CsOut out{n_valid, reinterpret_cast<u64*>(sum_q), ldo, reinterpret_cast<u64*>(n_range)};
    hipLaunchKernelGGL(class_sums_accumulate<T>, stage_grid(C, kHsThreads, Tn, tb), dim3(kHsThreads), 0, stream, ts, Tn, C,
                       ld, x0, class_of_t, K, tb, out);
    return hipGetLastError();
}

hipError_t launch_heat_stress_init(int32_t K, int64_t C, int32_t* counts, int64_t* hsum_q, int64_t* peak_key, int64_t ldo,
                                   int64_t* n_range, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(n_range, 0, sizeof(int64_t), stream);
    if (e == hipSuccess) e = zero_rows(counts, sizeof(int32_t), static_cast<int64_t>(K) * kHeatStressChannels, C, ldo, stream);
    if (e == hipSuccess) e = zero_rows(hsum_q, sizeof(int64_t), K, C, ldo, stream);
    if (e == hipSuccess) e = zero_rows(peak_key, sizeof(int64_t), K, C, ldo, stream);          // key 0: no step yet
    return e;
}

template <typename T>
hipError_t launch_heat_stress_accumulate(const T* ts, int64_t Tn, int64_t C, int64_t ld, const double* base, int64_t ldb,
                                         int64_t D, const int32_t* row_of_t, int32_t negate, int32_t W, double h0,
                                         const int32_t* class_of_t, int32_t K, const int64_t* level_q, int32_t L,
                                         const int32_t* at, int32_t J, int64_t block_steps, int32_t* counts, int64_t* hsum_q,
                                         int64_t* peak_key, int32_t* snap_q, int64_t ldo, int64_t* n_range,
                                         hipStream_t stream) {
    if (C <= 0 || Tn <= 0 || K <= 0) return hipSuccess;
    const int64_t tb = block_steps > 0 ? block_steps : heat_stress_auto_block(Tn, C, W);
    const HsIn<T> in{ts, ld, base, ldb, row_of_t, D == 1, negate != 0, h0};
    HsLevels lv{};
    lv.L = L;
    for (int32_t l = 0; l < L && l < kHeatStressMaxLevels; ++l)        // 0 <= S < 2^31 - 1: the clamped level compares alike
        lv.q[l] = static_cast<int32_t>(level_q[l] > INT32_MAX ? INT32_MAX : level_q[l] < INT32_MIN ? INT32_MIN : level_q[l]);
    const HsOut out{counts, reinterpret_cast<u64*>(hsum_q), reinterpret_cast<u64*>(peak_key), snap_q, ldo,
                    reinterpret_cast<u64*>(n_range)};
    hipLaunchKernelGGL(heat_stress_accumulate<T>, stage_grid(C, kHsThreads, Tn, tb), dim3(kHsThreads), 0, stream, in, Tn, C,
                       W, class_of_t, K, lv, at, J, tb, out);
    return hipGetLastError();
}

hipError_t launch_heat_stress_finish(int32_t K, int64_t C, const int64_t* peak_key, int32_t* peak_q, int32_t* peak_t,
                                     int64_t ldo, hipStream_t stream) {
    if (K <= 0 || C <= 0) return hipSuccess;
    const int64_t gx = (C + kHsThreads - 1) / kHsThreads;
    hipLaunchKernelGGL(heat_stress_finish, dim3(static_cast<unsigned>(gx), static_cast<unsigned>(K < 1024 ? K : 1024)),
                       dim3(kHsThreads), 0, stream, K, C, ldo, reinterpret_cast<const u64*>(peak_key), peak_q, peak_t);
    return hipGetLastError();
}

}  // namespace

}  // namespace xmhw

// ---- the C entries of heat_stress() and its class sums (include/xmhw_amd.h) -------------------------------------------
namespace {

using namespace xmhw::entry;

static std::atomic<int> g_heat_stress_block{0};   // steps a workgroup takes per block, 0 = automatic (xmhw_set_heat_stress_block)

static int heat_stress_check_shape(const char* who, int32_t K, int64_t Tn, int64_t C) {
    if (K < 1 || K > xmhw::kHeatStressMaxClasses)
        return fail(XMHW_ERR_UNSUPPORTED,
                    std::string(who) + ": K must be in [1, " + std::to_string(xmhw::kHeatStressMaxClasses) + "]");
    if (Tn > 0x7FFFFFFFll || C > 0x7FFFFFFFll)
        return fail(XMHW_ERR_UNSUPPORTED, std::string(who) + ": 2^31 steps or cells and more");
    return XMHW_OK;
}

template <typename T>
int class_sums_accumulate(const T* ts, int64_t Tn, int64_t C, int64_t ld, double x0, const int32_t* class_of_t, int32_t K,
                          int32_t* n_valid, int64_t* sum_q, int64_t ldo, int64_t* n_range, void* stream) {
    if (heat_stress_check_shape("class_sums", K, Tn, C) != XMHW_OK) return XMHW_ERR_UNSUPPORTED;
    if (Tn <= 0 || C < 0 || ld < C || ldo < C) return fail(XMHW_ERR_INVALID, "bad T/C/ld/ldo");
    if (!std::isfinite(x0)) return fail(XMHW_ERR_INVALID, "x0 must be finite");
    if (!class_of_t) return fail(XMHW_ERR_INVALID, "NULL class_of_t");
    if (int rc = check_labels(class_of_t, Tn, -1, K, kClassesOutside)) return rc;
    if (C == 0) return XMHW_OK;
    if (!ts || !n_valid || !sum_q || !n_range) return fail(XMHW_ERR_INVALID, "NULL buffer");
    RowsRef classes;
    if (int rc = upload_table(class_of_t, Tn, "class table upload", &classes)) return rc;
    return status_of(xmhw::launch_class_sums_accumulate<T>(ts, Tn, C, ld, x0, classes->d_rows, K, g_heat_stress_block.load(),
                                                           n_valid, sum_q, ldo, n_range, static_cast<hipStream_t>(stream)),
                     "class_sums_accumulate launch");
}

template <typename T>
int heat_stress_accumulate(const T* ts, int64_t Tn, int64_t C, int64_t ld, const double* base, int64_t ldb, int64_t D,
                           const int32_t* row_of_t, int32_t negate, int32_t W, double h0, const int32_t* class_of_t,
                           int32_t K, const int64_t* level_q, int32_t L, const int32_t* at, int32_t J, int32_t* counts,
                           int64_t* hsum_q, int64_t* peak_key, int32_t* snap_q, int64_t ldo, int64_t* n_range,
                           void* stream) {
    if (heat_stress_check_shape("heat_stress", K, Tn, C) != XMHW_OK) return XMHW_ERR_UNSUPPORTED;
    if (W < 1 || W > xmhw::kHeatStressMaxWindow)
        return fail(XMHW_ERR_UNSUPPORTED, "heat_stress: W must be in [1, " + std::to_string(xmhw::kHeatStressMaxWindow) + "]");
    if (L > xmhw::kHeatStressMaxLevels)
        return fail(XMHW_ERR_UNSUPPORTED, "heat_stress: at most " + std::to_string(xmhw::kHeatStressMaxLevels) + " levels");
    if (J > xmhw::kHeatStressMaxSnapshots)
        return fail(XMHW_ERR_UNSUPPORTED,
                    "heat_stress: at most " + std::to_string(xmhw::kHeatStressMaxSnapshots) + " snapshot steps");
    if (Tn <= 0 || C < 0 || ld < C || ldb < C || ldo < C || D < 1 || L < 0 || J < 0)
        return fail(XMHW_ERR_INVALID, "bad T/C/ld/ldb/ldo/D/L/J");
    if (!(h0 >= 1.0 / 65536.0 && h0 < 128.0)) return fail(XMHW_ERR_INVALID, "h0 outside [2^-16, 2^7)");
    if (!class_of_t || !row_of_t || (L > 0 && !level_q) || (J > 0 && !at)) return fail(XMHW_ERR_INVALID, "NULL host table");
    if (int rc = check_labels(class_of_t, Tn, -1, K, kClassesOutside)) return rc;
    if (int rc = check_labels(row_of_t, Tn, 0, D, kRowsOutside)) return rc;
    for (int32_t l = 1; l < L; ++l)
        if (level_q[l] <= level_q[l - 1]) return fail(XMHW_ERR_INVALID, "level_q not strictly ascending");
    for (int32_t j = 0; j < J; ++j)
        if (at[j] < 0 || at[j] >= Tn || (j > 0 && at[j] <= at[j - 1]))
            return fail(XMHW_ERR_INVALID, "snapshot steps not strictly ascending in [0, T)");
    if (C == 0) return XMHW_OK;
    if (!ts || !base || !counts || !hsum_q || !peak_key || !n_range || (J > 0 && !snap_q))
        return fail(XMHW_ERR_INVALID, "NULL buffer");
    RowsRef rows;
    if (int rc = upload_table(row_of_t, Tn, "row table upload", &rows)) return rc;
    RowsRef classes;                                   // the same content-keyed cache: one more int32[T] table
    if (int rc = upload_table(class_of_t, Tn, "class table upload", &classes)) return rc;
    RowsRef steps;                                     // ... and the snapshot steps, int32[J]
    if (J > 0)
        if (int rc = upload_table(at, J, "snapshot table upload", &steps)) return rc;
    return status_of(xmhw::launch_heat_stress_accumulate<T>(ts, Tn, C, ld, base, ldb, D, rows->d_rows, negate, W, h0,
                                                            classes->d_rows, K, level_q, L, J > 0 ? steps->d_rows : nullptr, J,
                                                            g_heat_stress_block.load(), counts, hsum_q, peak_key, snap_q, ldo,
                                                            n_range, static_cast<hipStream_t>(stream)),
                     "heat_stress_accumulate launch");
}

}  // namespace

extern "C" {

int xmhw_set_heat_stress_block(int32_t steps) { return set_knob(g_heat_stress_block, steps, "steps must be >= 0"); }
int xmhw_class_sums_init(int32_t K, int64_t C, int32_t* n_valid, int64_t* sum_q, int64_t ldo, int64_t* n_range, void* stream) {
    if (heat_stress_check_shape("class_sums", K, 1, C) != XMHW_OK) return XMHW_ERR_UNSUPPORTED;
    if (C < 0 || ldo < C) return fail(XMHW_ERR_INVALID, "bad C/ldo");
    if (!n_range || (C > 0 && (!n_valid || !sum_q))) return fail(XMHW_ERR_INVALID, "NULL output buffer");
    return status_of(xmhw::launch_class_sums_init(K, C, n_valid, sum_q, ldo, n_range, static_cast<hipStream_t>(stream)),
                     "class_sums_init");
}
int xmhw_class_sums_accumulate_f32(const float* ts, int64_t T, int64_t C, int64_t ld, double x0, const int32_t* class_of_t,
                                   int32_t K, int32_t* n_valid, int64_t* sum_q, int64_t ldo, int64_t* n_range, void* stream) {
    return class_sums_accumulate<float>(ts, T, C, ld, x0, class_of_t, K, n_valid, sum_q, ldo, n_range, stream);
}
int xmhw_class_sums_accumulate_f64(const double* ts, int64_t T, int64_t C, int64_t ld, double x0, const int32_t* class_of_t,
                                   int32_t K, int32_t* n_valid, int64_t* sum_q, int64_t ldo, int64_t* n_range, void* stream) {
    return class_sums_accumulate<double>(ts, T, C, ld, x0, class_of_t, K, n_valid, sum_q, ldo, n_range, stream);
}
int xmhw_heat_stress_init(int32_t K, int64_t C, int32_t* counts, int64_t* hsum_q, int64_t* peak_key, int64_t ldo,
                          int64_t* n_range, void* stream) {
    if (heat_stress_check_shape("heat_stress", K, 1, C) != XMHW_OK) return XMHW_ERR_UNSUPPORTED;
    if (C < 0 || ldo < C) return fail(XMHW_ERR_INVALID, "bad C/ldo");
    if (!n_range || (C > 0 && (!counts || !hsum_q || !peak_key))) return fail(XMHW_ERR_INVALID, "NULL output buffer");
    return status_of(xmhw::launch_heat_stress_init(K, C, counts, hsum_q, peak_key, ldo, n_range,
                                                   static_cast<hipStream_t>(stream)),
                     "heat_stress_init");
}
int xmhw_heat_stress_accumulate_f32(const float* ts, int64_t T, int64_t C, int64_t ld, const double* base, int64_t ldb,
                                    int64_t D, const int32_t* row_of_t, int32_t negate, int32_t W, double h0,
                                    const int32_t* class_of_t, int32_t K, const int64_t* level_q, int32_t L, const int32_t* at,
                                    int32_t J, int32_t* counts, int64_t* hsum_q, int64_t* peak_key, int32_t* snap_q,
                                    int64_t ldo, int64_t* n_range, void* stream) {
    return heat_stress_accumulate<float>(ts, T, C, ld, base, ldb, D, row_of_t, negate, W, h0, class_of_t, K, level_q, L, at, J,
                                         counts, hsum_q, peak_key, snap_q, ldo, n_range, stream);
}
int xmhw_heat_stress_accumulate_f64(const double* ts, int64_t T, int64_t C, int64_t ld, const double* base, int64_t ldb,
                                    int64_t D, const int32_t* row_of_t, int32_t negate, int32_t W, double h0,
                                    const int32_t* class_of_t, int32_t K, const int64_t* level_q, int32_t L, const int32_t* at,
                                    int32_t J, int32_t* counts, int64_t* hsum_q, int64_t* peak_key, int32_t* snap_q,
                                    int64_t ldo, int64_t* n_range, void* stream) {
    return heat_stress_accumulate<double>(ts, T, C, ld, base, ldb, D, row_of_t, negate, W, h0, class_of_t, K, level_q, L, at, J,
                                          counts, hsum_q, peak_key, snap_q, ldo, n_range, stream);
}
int xmhw_heat_stress_finish(int32_t K, int64_t C, const int64_t* peak_key, int32_t* peak_q, int32_t* peak_t, int64_t ldo,
                            void* stream) {
    if (heat_stress_check_shape("heat_stress", K, 1, C) != XMHW_OK) return XMHW_ERR_UNSUPPORTED;
    if (C < 0 || ldo < C) return fail(XMHW_ERR_INVALID, "bad C/ldo");
    if (C == 0) return XMHW_OK;
    if (!peak_key || !peak_q || !peak_t) return fail(XMHW_ERR_INVALID, "NULL buffer");
    return status_of(xmhw::launch_heat_stress_finish(K, C, peak_key, peak_q, peak_t, ldo, static_cast<hipStream_t>(stream)),
                     "heat_stress_finish launch");
}

}  // extern "C"
