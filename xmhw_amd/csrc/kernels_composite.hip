// kernels_composite.hip -- mhw_composite(): event-centred composites (superposed epoch analysis) of a field, per cell
// (DESIGN.md 3.21).
//
// ts[T][ld] is the series, base[Dr][ldb] with row_of_t[T] its base (one row: a constant per cell, read once), A the anchor
// bitmap in the layout of launch_event_table_bits (bits[w * lda + c], the bits at t >= T zero), class_of_t[T] labels in
// [-1, K), before >= 0 and after >= 0 with D = before + after + 1 <= 128, shift in [0, 24].  For every cell c, every
// anchor step s of c with k = class_of_t[s] >= 0 and every offset d in [-before, after] with 0 <= s + d < T:
//   a = (float64(ts[s + d][c]) - base[row_of_t[s + d]][c]) * 2^-shift      (the scaling is exact)
//   a NaN adds nothing; |a| >= 2^7 or infinite adds 1 to *n_range; otherwise q = rint(a * 2^16) and, with i = d + before,
//   n[k][i][c] += 1, s[k][i][c] += q, ss[k][i][c] += q^2.
// The class is that of the ANCHOR step, not of the sample.  T < 2^17, |q| <= 2^23, q^2 <= 2^46 and at most T anchors per
// entry: every sum stays inside 64 bits.  The atomics add the two's-complement bits as unsigned integers.  Everything is
// an integer sum: the result does not depend on blocks, slabs, launch shape or schedule.
//
//   composite_accumulate<T, WORDS>
//                     the frame of a class reduction (kernels.h): lane = cell, a workgroup is 256 cells x a block of
//                     steps, grid.y strides over the blocks.  WORDS = 1 (D <= 64) or 2 (D <= 128).
//   the window        composite_window.h: D bits per lane, bit i set iff the cell has an anchor at step t + before - i.
//                     A block that starts at t0 builds it from the bitmap words that cover [t0 - after, t0 + before] and
//                     reads no sample: blocks are independent.  A look-ahead cursor over the lane's bitmap column supplies
//                     the bit of step t + 1 + before.
//   the step          __ballot(window != 0) == 0 skips it: the row of samples and the base row are not requested.  A
//                     lane with a non-zero window loads its sample (and its base row, unless the base is one row), forms
//                     q once and walks the set bits of its window: for bit i the class of step t + before - i, and for a
//                     class >= 0 three integer atomics without a return value at (k * D + i) * ldo + c.  Lanes of a wave
//                     at the same i hit consecutive addresses.  Nothing accumulates in registers: each (anchor, offset)
//                     pair is visited exactly once.  No barrier, no LDS, no scratch.
#include "../../include/xmhw_amd.h"
#include "entry_common.h"
#include "stage_reduce.h"
#include "composite_window.h"

namespace xmhw {

// What the stage computes: event-centred composites of a field, per cell.  anchor_bits is a bitmap of
// launch_event_table_bits whose set bits are the anchor steps of every cell (leading dimension lda).  With
// D = before + after + 1, for every cell c, anchor step s of c with k = class_of_t[s] >= 0 and offset d in [-before, after]
// with 0 <= s + d < Tn, and a = (sample(s + d) - base[row_of_t[s + d]][c]) * 2^-shift: launch_composite_accumulate ADDS,
// with i = d + before and for an a that is not NaN and |a| < 2^7, 1 to n[k][i][c], q = rint(a * 2^kCompositeBits) to
// s[k][i][c] and q^2 to ss[k][i][c]; any other non-NaN a adds 1 to *n_range.  The class is that of the anchor step.  Cells
// are the fastest axis, leading dimension ldo >= C; the outputs are [K][D][ldo].  row_of_t and class_of_t are DEVICE arrays
// here.  block_steps: the steps a workgroup takes per block, 0 = automatic; same results for every value.
constexpr int kCompositeMaxOffsets = 128;            // D at most: a window of two words
constexpr int kCompositeMaxClasses = 64;
constexpr int kCompositeMaxSteps = 1 << 17;          // T below it, the cap of index_regression(): 2^17 * 2^46 = 2^63
constexpr int kCompositeBits = 16;
constexpr int kCompositeRangeBits = 7;
constexpr int kCompositeMaxShift = 24;

static_assert(kCompositeBits == kFixedBits && kCompositeRangeBits == kFixedRangeBits, "one scale for every stage");

namespace {

constexpr int kCoThreads = 256;
using u64 = unsigned long long;

template <typename T>
struct CoIn {
    const T* ts;
    int64_t ld;
    const double* base;                              // [Dr][ldb]
    int64_t ldb;
    const int32_t* row_of_t;
    int32_t one_row;                                 // Dr == 1: the base is a constant per cell, read once
    double scale;                                    // 2^-shift
    const uint64_t* bits;                            // the anchor bitmap
    int64_t lda;
};

struct CoOut {
    int32_t* n;                                      // [K][D][ldo]
    u64 *s, *ss;
    int64_t ldo;
    u64* n_range;
};

template <typename T, int WORDS>
__global__ __launch_bounds__(kCoThreads) void composite_accumulate(CoIn<T> in, int64_t Tn, int64_t C,
                                                                   const int32_t* __restrict__ class_of_t, int32_t K,
                                                                   int32_t before, int32_t D, int64_t tb, CoOut out) {
    const int64_t c = static_cast<int64_t>(blockIdx.x) * kCoThreads + threadIdx.x;
    if (c >= C) return;
    const double b0 = in.one_row ? in.base[c] : 0.0;
    // T < 2^17: steps and blocks are 32-bit here, addresses are not
    const int32_t Ts = static_cast<int32_t>(Tn), bs = static_cast<int32_t>(tb < Tn ? tb : Tn);
    const int32_t nblk = (Ts - 1) / bs + 1;
    const int32_t W = (Ts + 63) >> 6;
    const uint64_t last = composite_low_bits(Ts - 64 * (W - 1));      // the steps of the last word that exist
    // word w of the lane's bitmap column; no anchor below step 0 and from step T on, whatever the bitmap holds there
    const auto load = [&](int32_t w) -> uint64_t {
        if (w < 0 || w >= W) return 0;
        const uint64_t x = in.bits[static_cast<int64_t>(w) * in.lda + c];
        return w == W - 1 ? x & last : x;
    };
    u64 n_range = 0;
    for (int32_t blk = blockIdx.y; blk < nblk; blk += gridDim.y) {
        const auto [t0, t1] = block_range<int32_t>(blk, bs, Ts);
        CompositeWindow<WORDS> win = composite_window_at<WORDS>(load, t0, before, D);
        CompositeCursor ahead;
        for (int32_t t = t0; t < t1; ++t) {
            if (t > t0) win.push(ahead.bit(load, t + before), D);
            if (__ballot(win.any()) == 0) continue;  // uniform over the wave: the row of samples is not requested
            if (!win.any()) continue;
            const double b = in.one_row ? b0 : in.base[static_cast<int64_t>(in.row_of_t[t]) * in.ldb + c];
            const double a = (static_cast<double>(in.ts[static_cast<int64_t>(t) * in.ld + c]) - b) * in.scale;
            const int state = fixed_state(a);
            if (state == 0) continue;                // NaN adds nothing
            const int64_t q = state > 0 ? fixed_value(a) : 0;
            const u64 qq = static_cast<u64>(q * q);
#pragma unroll
            for (int h = 0; h < WORDS; ++h) {
                uint64_t m = win.w[h];
                while (m) {
                    const int32_t i = 64 * h + __builtin_ctzll(m);
                    m &= m - 1;
                    const int32_t k = class_of_t[t + before - i];
                    if (k < 0 || k >= K) continue;   // (labels are checked on the host)
                    if (state < 0) {
                        ++n_range;
                        continue;
                    }
                    const int64_t p = (static_cast<int64_t>(k) * D + i) * out.ldo + c;
                    atomicAdd(out.n + p, 1);
                    if (q) {
                        atomicAdd(out.s + p, static_cast<u64>(q));
                        atomicAdd(out.ss + p, qq);
                    }
                }
            }
        }
    }
    if (n_range) atomicAdd(out.n_range, n_range);
}

template <typename T, int WORDS>
void co_launch(const CoIn<T>& in, int64_t Tn, int64_t C, const int32_t* class_of_t, int32_t K, int32_t before, int32_t D,
               int64_t tb, const CoOut& out, hipStream_t stream) {
    hipLaunchKernelGGL((composite_accumulate<T, WORDS>), stage_grid(C, kCoThreads, Tn, tb), dim3(kCoThreads), 0, stream, in,
                       Tn, C, class_of_t, K, before, D, tb, out);
}

hipError_t launch_composite_init(int32_t K, int32_t D, int64_t C, int32_t* n, int64_t* s, int64_t* ss, int64_t ldo,
                                 int64_t* n_range, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(n_range, 0, sizeof(int64_t), stream);
    const int64_t rows = static_cast<int64_t>(K) * D;
    if (e == hipSuccess) e = zero_rows(n, sizeof(int32_t), rows, C, ldo, stream);
    for (int64_t* p : {s, ss})
        if (e == hipSuccess) e = zero_rows(p, sizeof(int64_t), rows, C, ldo, stream);
    return e;
}

template <typename T>
hipError_t launch_composite_accumulate(const T* ts, int64_t Tn, int64_t C, int64_t ld, const double* base, int64_t ldb,
                                       int64_t Dr, const int32_t* row_of_t, int32_t shift, const uint64_t* anchor_bits,
                                       int64_t lda, const int32_t* class_of_t, int32_t K, int32_t before, int32_t after,
                                       int64_t block_steps, int32_t* n, int64_t* s, int64_t* ss, int64_t ldo,
                                       int64_t* n_range, hipStream_t stream) {
    if (C <= 0 || Tn <= 0 || K <= 0) return hipSuccess;
    const int64_t D = static_cast<int64_t>(before) + after + 1;
    if (before < 0 || after < 0 || D > kCompositeMaxOffsets || Tn >= kCompositeMaxSteps || shift < 0 ||
        shift > kCompositeMaxShift)
        return hipErrorInvalidValue;
    const int64_t tb = block_steps > 0 ? block_steps : composite_auto_block(Tn, C, D);
    const CoIn<T> in{ts, ld, base, ldb, row_of_t, Dr == 1, ldexp(1.0, -shift), anchor_bits, lda};
    const auto u = [](int64_t* p) { return reinterpret_cast<u64*>(p); };
    const CoOut out{n, u(s), u(ss), ldo, u(n_range)};
    if (D <= 64)
        co_launch<T, 1>(in, Tn, C, class_of_t, K, before, static_cast<int32_t>(D), tb, out, stream);
    else
        co_launch<T, 2>(in, Tn, C, class_of_t, K, before, static_cast<int32_t>(D), tb, out, stream);
    return hipGetLastError();
}

}  // namespace

}  // namespace xmhw

// ---- the C entries of mhw_composite() (include/xmhw_amd.h) ------------------------------------------------------------
namespace {

using namespace xmhw::entry;

static std::atomic<int> g_composite_block{0};   // steps a workgroup takes per block, 0 = automatic (xmhw_set_composite_block)

static int composite_check_shape(int32_t K, int64_t D, int32_t shift, int64_t Tn, int64_t C) {
    if (K < 1 || K > xmhw::kCompositeMaxClasses)
        return fail(XMHW_ERR_UNSUPPORTED, "composite: K must be in [1, " + std::to_string(xmhw::kCompositeMaxClasses) + "]");
    if (D < 1 || D > xmhw::kCompositeMaxOffsets)
        return fail(XMHW_ERR_UNSUPPORTED,
                    "composite: before + after + 1 must be in [1, " + std::to_string(xmhw::kCompositeMaxOffsets) + "]");
    if (shift < 0 || shift > xmhw::kCompositeMaxShift)
        return fail(XMHW_ERR_UNSUPPORTED, "composite: shift must be in [0, " + std::to_string(xmhw::kCompositeMaxShift) + "]");
    if (Tn >= xmhw::kCompositeMaxSteps) return fail(XMHW_ERR_UNSUPPORTED, "composite: 2^17 steps and more");
    if (C > 0x7FFFFFFFll) return fail(XMHW_ERR_UNSUPPORTED, "composite: 2^31 cells and more");
    return XMHW_OK;
}

template <typename T>
int composite_accumulate(const T* ts, int64_t Tn, int64_t C, int64_t ld, const double* base, int64_t ldb, int64_t Dr,
                         const int32_t* row_of_t, int32_t shift, const uint64_t* anchor_bits, int64_t lda,
                         const int32_t* class_of_t, int32_t K, int32_t before, int32_t after, int32_t* n, int64_t* s,
                         int64_t* ss, int64_t ldo, int64_t* n_range, void* stream) {
    if (before < 0 || after < 0) return fail(XMHW_ERR_UNSUPPORTED, "composite: before and after must be >= 0");
    if (composite_check_shape(K, static_cast<int64_t>(before) + after + 1, shift, Tn, C) != XMHW_OK)
        return XMHW_ERR_UNSUPPORTED;
    if (Tn < 0 || C < 0 || ld < C || ldb < C || lda < C || ldo < C || Dr < 1)
        return fail(XMHW_ERR_INVALID, "bad T/C/ld/ldb/lda/ldo/D");
    if (Tn > 0 && (!class_of_t || !row_of_t)) return fail(XMHW_ERR_INVALID, "NULL host table");
    if (int rc = check_labels(class_of_t, Tn, -1, K, kClassesOutside)) return rc;
    if (int rc = check_labels(row_of_t, Tn, 0, Dr, kRowsOutside)) return rc;
    if (C == 0 || Tn == 0) return XMHW_OK;
    if (!ts || !base || !anchor_bits || !n || !s || !ss || !n_range) return fail(XMHW_ERR_INVALID, "NULL buffer");
    RowsRef rows;
    if (int rc = upload_table(row_of_t, Tn, "row table upload", &rows)) return rc;
    RowsRef classes;                                   // the same content-keyed cache: one more int32[T] table
    if (int rc = upload_table(class_of_t, Tn, "class table upload", &classes)) return rc;
    return status_of(xmhw::launch_composite_accumulate<T>(ts, Tn, C, ld, base, ldb, Dr, rows->d_rows, shift, anchor_bits, lda,
                                                          classes->d_rows, K, before, after, g_composite_block.load(), n, s,
                                                          ss, ldo, n_range, static_cast<hipStream_t>(stream)),
                     "composite_accumulate launch");
}

}  // namespace

extern "C" {

int xmhw_set_composite_block(int32_t steps) { return set_knob(g_composite_block, steps, "steps must be >= 0"); }
int xmhw_composite_init(int32_t K, int32_t D, int64_t C, int32_t* n, int64_t* s, int64_t* ss, int64_t ldo, int64_t* n_range,
                        void* stream) {
    if (composite_check_shape(K, D, 0, 1, C) != XMHW_OK) return XMHW_ERR_UNSUPPORTED;
    if (C < 0 || ldo < C) return fail(XMHW_ERR_INVALID, "bad C/ldo");
    if (!n_range || (C > 0 && (!n || !s || !ss))) return fail(XMHW_ERR_INVALID, "NULL output buffer");
    return status_of(xmhw::launch_composite_init(K, D, C, n, s, ss, ldo, n_range, static_cast<hipStream_t>(stream)),
                     "composite_init");
}
int xmhw_composite_accumulate_f32(const float* ts, int64_t T, int64_t C, int64_t ld, const double* base, int64_t ldb,
                                  int64_t Dr, const int32_t* row_of_t, int32_t shift, const uint64_t* anchor_bits, int64_t lda,
                                  const int32_t* class_of_t, int32_t K, int32_t before, int32_t after, int32_t* n, int64_t* s,
                                  int64_t* ss, int64_t ldo, int64_t* n_range, void* stream) {
    return composite_accumulate<float>(ts, T, C, ld, base, ldb, Dr, row_of_t, shift, anchor_bits, lda, class_of_t, K, before,
                                       after, n, s, ss, ldo, n_range, stream);
}
int xmhw_composite_accumulate_f64(const double* ts, int64_t T, int64_t C, int64_t ld, const double* base, int64_t ldb,
                                  int64_t Dr, const int32_t* row_of_t, int32_t shift, const uint64_t* anchor_bits, int64_t lda,
                                  const int32_t* class_of_t, int32_t K, int32_t before, int32_t after, int32_t* n, int64_t* s,
                                  int64_t* ss, int64_t ldo, int64_t* n_range, void* stream) {
    return composite_accumulate<double>(ts, T, C, ld, base, ldb, Dr, row_of_t, shift, anchor_bits, lda, class_of_t, K, before,
                                        after, n, s, ss, ldo, n_range, stream);
}

}  // extern "C"
