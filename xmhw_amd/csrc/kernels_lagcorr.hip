// kernels_lagcorr.hip -- lag_correlation(): per-cell lagged auto- and cross-correlation sums.  The
// definition of the sums is in include/xmhw_amd.h, "lag_correlation()"; in short, with ax(t), ay(t) the scaled anomalies of
// two series, valid as fixed_state() says, qx, qy their fixed-point integers: for every cell, every step t of class
// k >= 0 and every lag l in [0, L] with t - l >= 0 and both ax(t) and ay(t - l) valid, the six sums n, sx, sy, sxx, syy,
// sxy at [k][l][c] over the pairs (qx(t), qy(t - l)).
//
//   lag_corr_accumulate<T, DEPTH, G>
//                     the frame of a class reduction (kernels.h): lane = cell, a workgroup is 256 cells x a block of
//                     steps x a group of G lags (grid.z); the 11 registers of addends per lag of the current class are
//                     flushed by integer atomics without a return value when the wave-uniform class changes and at the
//                     end of the block, non-zero addends only.  No barrier, no scratch.  G = 8 (126 VGPRs, 4 waves per
//                     SIMD) serves up to 8 lags in one pass; from 9 lags on G = 16 (237 VGPRs, 2 waves) halves the passes
//                     over the samples, and the samples of step t + 1 are requested before step t is worked on.
//   the history       lag_ring.h: qy of the last DEPTH steps in the lane's own column of an LDS ring, slot-major
//                     (ring[slot][lane]: a wave reads 64 consecutive words, no bank conflict; only the lane itself ever
//                     touches its column, so no barrier), and a 64-bit validity mask in registers.  A partner that is not
//                     valid holds qy = 0 and a zero bit: its products vanish and the hot loop has no per-lag branch.  A
//                     lane whose own step is not valid skips the lags altogether.
//   a lag             one LDS read; the mask bits of the group are taken once per step, a lag's bit becomes a gate of all
//                     ones or zero, qx & gate feeds n, sx and -- times qx -- sxx: three v_mad_i64_i32 (sxx, syy, sxy),
//                     two 64-bit adds (sx, sy), eight 32-bit operations.
//   a block           clears its ring, then stores steps max(0, t0 - L) .. t0 - 1 of y and pushes their validity; it
//                     reduces and counts nothing from them: blocks are independent.
//   the counters      the lag group 0 alone counts the out-of-range steps, each once.
#include "../../include/xmhw_amd.h"
#include "entry_common.h"
#include "stage_reduce.h"
#include "lag_ring.h"

namespace xmhw {

// What the stage computes (lag_ring.h holds the ring): per cell, class of the LATER step and lag l in [0, L], the sums over
// the pairs (qx(t), qy(t - l)) whose two anomalies are valid -- n int32, sx, sy, sxx, syy, sxy int64, [K][L + 1][ldo],
// ADDED; the definition is in include/xmhw_amd.h, "lag_correlation()".  y may be x.  n_range[0] counts the steps of class
// >= 0 whose ax is not NaN and out of range, n_range[1] the steps of any class whose ay is.  row_of_t and class_of_t are
// DEVICE arrays here.  block_steps: the steps a workgroup takes per block, 0 = automatic; same results for every value.
constexpr int kLagCorrMaxLag = 63;                   // one validity bit per lag in a 64-bit mask
constexpr int kLagCorrMaxClasses = 64;
constexpr int kLagCorrMaxSteps = 1 << 17;            // T below it: 2^17 * 2^46 = 2^63
constexpr int kLagCorrBits = 16;
constexpr int kLagCorrRangeBits = 7;
constexpr int kLagCorrMaxShift = 24;

static_assert(kLagCorrBits == kFixedBits && kLagCorrRangeBits == kFixedRangeBits, "one scale for every stage");
static_assert(kLagCorrMaxLag == kLagRingMaxLag, "the mask holds one bit per lag");

namespace {

constexpr int kLcThreads = 256;
using u64 = unsigned long long;

template <typename T>
struct LcIn {
    const T *x, *y;
    int64_t ldx, ldy;
    const double *bx, *by;                           // [Dr][ldbx], [Dr][ldby]
    int64_t ldbx, ldby;
    const int32_t* row_of_t;
    int32_t one_row;                                 // Dr == 1: the bases are constants per cell, read once
    int32_t same;                                    // y is x in every respect: ax(t) is ay(t), read once
    double scale_x, scale_y;                         // 2^-shift
};

struct LcOut {
    int32_t* n;                                      // [K][L + 1][ldo]
    u64 *sx, *sy, *sxx, *syy, *sxy;
    int64_t ldo;
    u64* n_range;                                    // [2]: x, y
};

// the addends of one lane for the current class: the lags l0 .. l0 + G - 1
template <int G>
struct LcAcc {
    int32_t n[G];
    int64_t sx[G], sy[G], sxx[G], syy[G], sxy[G];
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int j = 0; j < G; ++j) {
            n[j] = 0;
            sx[j] = sy[j] = sxx[j] = syy[j] = sxy[j] = 0;
        }
    }
};

template <int G>
__device__ __forceinline__ void lc_flush(const LcOut& o, int32_t k, int64_t c, int32_t l0, int32_t L, LcAcc<G>& v) {
#pragma unroll
    for (int j = 0; j < G; ++j) {
        if (l0 + j > L || v.n[j] == 0) continue;     // no pair, no addend: an invalid partner holds qy = 0
        const int64_t p = (static_cast<int64_t>(k) * (L + 1) + l0 + j) * o.ldo + c;
        atomicAdd(o.n + p, v.n[j]);
        if (v.sx[j]) atomicAdd(o.sx + p, static_cast<u64>(v.sx[j]));
        if (v.sy[j]) atomicAdd(o.sy + p, static_cast<u64>(v.sy[j]));
        if (v.sxx[j]) atomicAdd(o.sxx + p, static_cast<u64>(v.sxx[j]));
        if (v.syy[j]) atomicAdd(o.syy + p, static_cast<u64>(v.syy[j]));
        if (v.sxy[j]) atomicAdd(o.sxy + p, static_cast<u64>(v.sxy[j]));
    }
    v.clear();
}

template <typename T, int DEPTH, int G>
__global__ __launch_bounds__(kLcThreads) void lag_corr_accumulate(LcIn<T> in, int64_t Tn, int64_t C,
                                                                  const int32_t* __restrict__ class_of_t, int32_t K, int32_t L,
                                                                  int64_t tb, LcOut out) {
    static_assert(DEPTH % G == 0 && DEPTH <= 64, "whole lag groups inside the ring");
    constexpr bool kAhead = G == kLagCorrWideGroup;  // two waves per SIMD there, and registers to spare
    __shared__ int32_t ring[DEPTH * kLcThreads];
    const int64_t c = static_cast<int64_t>(blockIdx.x) * kLcThreads + threadIdx.x;
    if (c >= C) return;                              // (no barrier below)
    int32_t* const mine = ring + threadIdx.x;        // the lane's column: slot s at mine[s * kLcThreads]
    const int32_t l0 = static_cast<int32_t>(blockIdx.z) * G;
    const bool counts = blockIdx.z == 0;
    const double bx0 = in.one_row ? in.bx[c] : 0.0, by0 = in.one_row ? in.by[c] : 0.0;
    // T < 2^17: steps and blocks are 32-bit here, addresses are not
    const int32_t Ts = static_cast<int32_t>(Tn), bs = static_cast<int32_t>(tb < Tn ? tb : Tn);
    const int32_t nblk = (Ts - 1) / bs + 1;
    LcAcc<G> v;
    v.clear();
    u64 range_x = 0, range_y = 0;
    const auto flush_class = [&](int32_t k) { lc_flush<G>(out, k, c, l0, L, v); };
    // a sample and its base as they are read; the anomaly is formed where it is used
    struct Raw {
        T s;
        double b;
    };
    const auto load_x = [&](int32_t t) -> Raw {
        return {in.x[static_cast<int64_t>(t) * in.ldx + c],
                in.one_row ? bx0 : in.bx[static_cast<int64_t>(in.row_of_t[t]) * in.ldbx + c]};
    };
    const auto load_y = [&](int32_t t) -> Raw {
        return {in.y[static_cast<int64_t>(t) * in.ldy + c],
                in.one_row ? by0 : in.by[static_cast<int64_t>(in.row_of_t[t]) * in.ldby + c]};
    };
    const auto label = [&](int32_t t) -> int32_t {
        const int32_t k = class_of_t[t];
        return k < K ? k : -1;                       // (labels are checked on the host)
    };
    for (int32_t blk = blockIdx.y; blk < nblk; blk += gridDim.y) {
        const auto [t0, t1] = block_range<int32_t>(blk, bs, Ts);
        // the history of the block: an empty ring, then the steps before it, which are reduced and counted nowhere
#pragma unroll
        for (int s = 0; s < DEPTH; ++s) mine[s * kLcThreads] = 0;
        uint64_t mask = 0;
        for (int32_t t = lag_warmup_begin(t0, L); t < t0; ++t) {
            const Raw r = load_y(t);
            const double ay = (static_cast<double>(r.s) - r.b) * in.scale_y;
            const bool valid = fixed_state(ay) > 0;
            mine[lag_ring_slot(t, 0, DEPTH) * kLcThreads] = valid ? static_cast<int32_t>(fixed_value(ay)) : 0;
            mask = lag_mask_push(mask, valid, L);
        }
        ClassRun run;
        // step t of class k (wave-uniform) with its samples ry and, for k >= 0 and two fields, rx
        const auto step = [&](int32_t t, int32_t k, const Raw& ry, const Raw& rx) {
            const double ay = (static_cast<double>(ry.s) - ry.b) * in.scale_y;
            const int state_y = fixed_state(ay);
            mine[lag_ring_slot(t, 0, DEPTH) * kLcThreads] = state_y > 0 ? static_cast<int32_t>(fixed_value(ay)) : 0;
            mask = lag_mask_push(mask, state_y > 0, L);
            if (counts && state_y < 0) ++range_y;
            if (k < 0) return;                       // uniform over the wave: x was not read
            run.enter(k, flush_class);
            const double ax = in.same ? ay : (static_cast<double>(rx.s) - rx.b) * in.scale_x;
            const int state_x = in.same ? state_y : fixed_state(ax);
            if (counts && state_x < 0) ++range_x;
            if (state_x <= 0) return;                // the lane's own step is not valid: nothing for any lag
            const int32_t qx = static_cast<int32_t>(fixed_value(ax));
            const uint32_t bits = lag_mask_group(mask, l0);
#pragma unroll
            for (int j = 0; j < G; ++j) {
                const int32_t qy = mine[lag_ring_slot(t, l0 + j, DEPTH) * kLcThreads];
                const int32_t gate = -static_cast<int32_t>((bits >> j) & 1u);        // all ones iff the partner is valid
                const int32_t qxg = qx & gate;
                v.n[j] -= gate;
                v.sx[j] += qxg;
                v.sxx[j] += static_cast<int64_t>(qxg) * qx;
                v.sy[j] += qy;
                v.syy[j] += static_cast<int64_t>(qy) * qy;
                v.sxy[j] += static_cast<int64_t>(qx) * qy;
            }
        };
        const auto needs_x = [&](int32_t k) { return k >= 0 && !in.same; };
        if constexpr (kAhead) {
            // the samples of step t + 1 are requested before step t is worked on: at two waves per SIMD the other wave
            // alone does not cover a trip to memory
            int32_t k = label(t0);
            Raw ry = load_y(t0), rx = needs_x(k) ? load_x(t0) : Raw{};
            for (int32_t t = t0; t < t1; ++t) {
                const int32_t kc = k;
                const Raw cy = ry, cx = rx;
                if (t + 1 < t1) {
                    k = label(t + 1);
                    ry = load_y(t + 1);
                    if (needs_x(k)) rx = load_x(t + 1);
                }
                step(t, kc, cy, cx);
            }
        } else {
            for (int32_t t = t0; t < t1; ++t) {
                const int32_t k = label(t);
                step(t, k, load_y(t), needs_x(k) ? load_x(t) : Raw{});
            }
        }
        run.leave(flush_class);
    }
    if (range_x) atomicAdd(out.n_range, range_x);
    if (range_y) atomicAdd(out.n_range + 1, range_y);
}

template <typename T, int DEPTH, int G>
void lc_launch(const LcIn<T>& in, int64_t Tn, int64_t C, const int32_t* class_of_t, int32_t K, int32_t L, int64_t tb,
               const LcOut& out, hipStream_t stream) {
    hipLaunchKernelGGL((lag_corr_accumulate<T, DEPTH, G>), stage_grid(C, kLcThreads, Tn, tb, lag_corr_groups(L)), dim3(kLcThreads),
                       0, stream, in, Tn, C, class_of_t, K, L, tb, out);
}

hipError_t launch_lag_corr_init(int32_t K, int32_t L, int64_t C, int32_t* n, int64_t* sx, int64_t* sy, int64_t* sxx,
                                int64_t* syy, int64_t* sxy, int64_t ldo, int64_t* n_range, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(n_range, 0, 2 * sizeof(int64_t), stream);
    const int64_t rows = static_cast<int64_t>(K) * (L + 1);
    if (e == hipSuccess) e = zero_rows(n, sizeof(int32_t), rows, C, ldo, stream);
    for (int64_t* p : {sx, sy, sxx, syy, sxy})
        if (e == hipSuccess) e = zero_rows(p, sizeof(int64_t), rows, C, ldo, stream);
    return e;
}

template <typename T>
hipError_t launch_lag_corr_accumulate(const T* x, int64_t ldx, const T* y, int64_t ldy, int64_t Tn, int64_t C,
                                      const double* base_x, int64_t ldbx, const double* base_y, int64_t ldby, int64_t Dr,
                                      const int32_t* row_of_t, int32_t shift_x, int32_t shift_y, const int32_t* class_of_t,
                                      int32_t K, int32_t L, int64_t block_steps, int32_t* n, int64_t* sx, int64_t* sy,
                                      int64_t* sxx, int64_t* syy, int64_t* sxy, int64_t ldo, int64_t* n_range,
                                      hipStream_t stream) {
    if (C <= 0 || Tn <= 0 || K <= 0) return hipSuccess;
    if (L < 0 || L > kLagCorrMaxLag || Tn >= kLagCorrMaxSteps || shift_x < 0 || shift_x > kLagCorrMaxShift || shift_y < 0 ||
        shift_y > kLagCorrMaxShift)
        return hipErrorInvalidValue;
    const int64_t tb = block_steps > 0 ? block_steps : lag_corr_auto_block(Tn, C, L);
    const bool same = x == y && ldx == ldy && base_x == base_y && ldbx == ldby && shift_x == shift_y;
    const LcIn<T> in{x, y, ldx, ldy, base_x, base_y, ldbx, ldby, row_of_t, Dr == 1, same, ldexp(1.0, -shift_x),
                     ldexp(1.0, -shift_y)};
    const auto u = [](int64_t* p) { return reinterpret_cast<u64*>(p); };
    const LcOut out{n, u(sx), u(sy), u(sxx), u(syy), u(sxy), ldo, u(n_range)};
    constexpr int G8 = kLagCorrGroup, G16 = kLagCorrWideGroup;
    if (lag_corr_group(L) == G8) {
        lc_launch<T, 16, G8>(in, Tn, C, class_of_t, K, L, tb, out, stream);
    } else {
        switch (lag_ring_depth(L)) {
            case 16: lc_launch<T, 16, G16>(in, Tn, C, class_of_t, K, L, tb, out, stream); break;
            case 32: lc_launch<T, 32, G16>(in, Tn, C, class_of_t, K, L, tb, out, stream); break;
            default: lc_launch<T, 64, G16>(in, Tn, C, class_of_t, K, L, tb, out, stream); break;
        }
    }
    return hipGetLastError();
}

}  // namespace

}  // namespace xmhw

// ---- the C entries of lag_correlation() (include/xmhw_amd.h) ----------------------------------------------------------
namespace {

using namespace xmhw::entry;

static std::atomic<int> g_lag_corr_block{0};    // steps a workgroup takes per block, 0 = automatic (xmhw_set_lag_corr_block)

static int lag_corr_check_shape(int32_t K, int32_t L, int32_t shift_x, int32_t shift_y, int64_t Tn, int64_t C) {
    if (K < 1 || K > xmhw::kLagCorrMaxClasses)
        return fail(XMHW_ERR_UNSUPPORTED, "lag_corr: K must be in [1, " + std::to_string(xmhw::kLagCorrMaxClasses) + "]");
    if (L < 0 || L > xmhw::kLagCorrMaxLag)
        return fail(XMHW_ERR_UNSUPPORTED, "lag_corr: max_lag must be in [0, " + std::to_string(xmhw::kLagCorrMaxLag) + "]");
    if (shift_x < 0 || shift_x > xmhw::kLagCorrMaxShift || shift_y < 0 || shift_y > xmhw::kLagCorrMaxShift)
        return fail(XMHW_ERR_UNSUPPORTED, "lag_corr: shifts must be in [0, " + std::to_string(xmhw::kLagCorrMaxShift) + "]");
    if (Tn >= xmhw::kLagCorrMaxSteps) return fail(XMHW_ERR_UNSUPPORTED, "lag_corr: 2^17 steps and more");
    if (C > 0x7FFFFFFFll) return fail(XMHW_ERR_UNSUPPORTED, "lag_corr: 2^31 cells and more");
    return XMHW_OK;
}

template <typename T>
int lag_corr_accumulate(const T* x, int64_t ldx, const T* y, int64_t ldy, int64_t Tn, int64_t C, const double* base_x,
                        int64_t ldbx, const double* base_y, int64_t ldby, int64_t Dr, const int32_t* row_of_t, int32_t shift_x,
                        int32_t shift_y, const int32_t* class_of_t, int32_t K, int32_t max_lag, int32_t* n, int64_t* sx,
                        int64_t* sy, int64_t* sxx, int64_t* syy, int64_t* sxy, int64_t ldo, int64_t* n_range, void* stream) {
    if (lag_corr_check_shape(K, max_lag, shift_x, shift_y, Tn, C) != XMHW_OK) return XMHW_ERR_UNSUPPORTED;
    if (Tn < 0 || C < 0 || ldx < C || ldy < C || ldbx < C || ldby < C || ldo < C || Dr < 1)
        return fail(XMHW_ERR_INVALID, "bad T/C/ldx/ldy/ldbx/ldby/ldo/D");
    if (Tn > 0 && (!class_of_t || !row_of_t)) return fail(XMHW_ERR_INVALID, "NULL host table");
    if (int rc = check_labels(class_of_t, Tn, -1, K, kClassesOutside)) return rc;
    if (int rc = check_labels(row_of_t, Tn, 0, Dr, kRowsOutside)) return rc;
    if (C == 0 || Tn == 0) return XMHW_OK;
    if (!x || !y || !base_x || !base_y || !n || !sx || !sy || !sxx || !syy || !sxy || !n_range)
        return fail(XMHW_ERR_INVALID, "NULL buffer");
    RowsRef rows;
    if (int rc = upload_table(row_of_t, Tn, "row table upload", &rows)) return rc;
    RowsRef classes;                                   // the same content-keyed cache: one more int32[T] table
    if (int rc = upload_table(class_of_t, Tn, "class table upload", &classes)) return rc;
    return status_of(xmhw::launch_lag_corr_accumulate<T>(x, ldx, y, ldy, Tn, C, base_x, ldbx, base_y, ldby, Dr, rows->d_rows,
                                                         shift_x, shift_y, classes->d_rows, K, max_lag,
                                                         g_lag_corr_block.load(), n, sx, sy, sxx, syy, sxy, ldo, n_range,
                                                         static_cast<hipStream_t>(stream)),
                     "lag_corr_accumulate launch");
}

}  // namespace

extern "C" {

int xmhw_set_lag_corr_block(int32_t steps) { return set_knob(g_lag_corr_block, steps, "steps must be >= 0"); }
int xmhw_lag_corr_init(int32_t K, int32_t max_lag, int64_t C, int32_t* n, int64_t* sx, int64_t* sy, int64_t* sxx, int64_t* syy,
                       int64_t* sxy, int64_t ldo, int64_t* n_range, void* stream) {
    if (lag_corr_check_shape(K, max_lag, 0, 0, 1, C) != XMHW_OK) return XMHW_ERR_UNSUPPORTED;
    if (C < 0 || ldo < C) return fail(XMHW_ERR_INVALID, "bad C/ldo");
    if (!n_range || (C > 0 && (!n || !sx || !sy || !sxx || !syy || !sxy))) return fail(XMHW_ERR_INVALID, "NULL output buffer");
    return status_of(xmhw::launch_lag_corr_init(K, max_lag, C, n, sx, sy, sxx, syy, sxy, ldo, n_range,
                                                static_cast<hipStream_t>(stream)),
                     "lag_corr_init");
}
int xmhw_lag_corr_accumulate_f32(const float* x, int64_t ldx, const float* y, int64_t ldy, int64_t T, int64_t C,
                                 const double* base_x, int64_t ldbx, const double* base_y, int64_t ldby, int64_t Dr,
                                 const int32_t* row_of_t, int32_t shift_x, int32_t shift_y, const int32_t* class_of_t, int32_t K,
                                 int32_t max_lag, int32_t* n, int64_t* sx, int64_t* sy, int64_t* sxx, int64_t* syy, int64_t* sxy,
                                 int64_t ldo, int64_t* n_range, void* stream) {
    return lag_corr_accumulate<float>(x, ldx, y, ldy, T, C, base_x, ldbx, base_y, ldby, Dr, row_of_t, shift_x, shift_y,
                                      class_of_t, K, max_lag, n, sx, sy, sxx, syy, sxy, ldo, n_range, stream);
}
int xmhw_lag_corr_accumulate_f64(const double* x, int64_t ldx, const double* y, int64_t ldy, int64_t T, int64_t C,
                                 const double* base_x, int64_t ldbx, const double* base_y, int64_t ldby, int64_t Dr,
                                 const int32_t* row_of_t, int32_t shift_x, int32_t shift_y, const int32_t* class_of_t, int32_t K,
                                 int32_t max_lag, int32_t* n, int64_t* sx, int64_t* sy, int64_t* sxx, int64_t* syy, int64_t* sxy,
                                 int64_t ldo, int64_t* n_range, void* stream) {
    return lag_corr_accumulate<double>(x, ldx, y, ldy, T, C, base_x, ldbx, base_y, ldby, Dr, row_of_t, shift_x, shift_y,
                                       class_of_t, K, max_lag, n, sx, sy, sxx, syy, sxy, ldo, n_range, stream);
}

}  // extern "C"
