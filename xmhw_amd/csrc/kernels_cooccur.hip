// kernels_cooccur.hip -- mhw_cooccurrence(): per cell, per CLASS of time steps and per LAG, the joint event days of two
// detections (compound extremes: joint frequency and likelihood multiplication factor; verification: the 2x2
// contingency table per cell and lead).
//
// Two event tables A and B lie on the same time axis of T steps.  For column c and step t, A[t][c] = 1 iff some table
// row of that cell has start <= t <= end (gap days of joined events included, as detect() stores them).  B is defined
// the same way.  For a lag l (any int32) the pair (t, l) is VALID iff 0 <= t + l < T.  Then:
//   Bl[t] = B[t + l] on valid pairs and 0 otherwise.
//   J[t]  = A[t] & Bl[t], with J[-1] = 0.
// class_of_t[T] holds int32 labels in [-1, K); -1 counts nowhere.  A pair belongs to the class of t, which is A's step.
// For every class k, lag index i and column c, summed over the valid pairs with class_of_t[t] == k:
//   counts[k][i][0][c]  both     A[t] & Bl[t]
//   counts[k][i][1][c]  a_only   A[t] & ~Bl[t]
//   counts[k][i][2][c]  b_only   ~A[t] & Bl[t]
//   counts[k][i][3][c]  onsets   J[t] & ~J[t-1]: the first steps of joint runs
// The onset test looks at t - 1 whatever the class of t - 1 is.  `neither` is not computed on the device: it is
// n_pairs[k][i] - both - a_only - b_only, where n_pairs (the number of valid pairs of class k) is computed on the host
// from the labels and the lag.  All counts are int32 and <= T < 2^31.  A lag with |l| >= T gives zeros everywhere.
// Everything is an integer sum: the result does not depend on the time blocks, the lag groups, the slabs or the schedule.
//
//   event_table_bits   table -> bitmap, one bit per sample, word-major, cells-minor (the layout of exceed_bits and
//                      event_day_bits).  Lane = column: a lane owns its column, walks its rows once (they are in time
//                      order) and writes every word of the column with a plain vector store, zero where there is no
//                      event; a wave stores 512 contiguous bytes per word.  `reach`, the largest end seen so far,
//                      carries a row over the word edges, so rows that overlap are handled as well.
//   cooccur_accumulate lane = cell, workgroup = 256 cells x a block of whole 64-step words, grid.z = a group of at most
//                      8 lags: 32 int32 addends of the current class in registers.  class_of_t arrives as a per-word
//                      SEGMENT list (seg_off[W + 1], seg_class[], seg_mask[]): a segment is a run of one non-negative
//                      class inside one word, so a calendar class gives 1-2 segments per word and labels that change
//                      every step give 64 one-bit segments.  Segments, lags, shifts and range masks are uniform over the
//                      wave: every decision about them is scalar.  Per word and lag, with l = 64 q + r:
//                      Bl = B[w + q] >> r | B[w + q + 1] << (64 - r) (r == 0 on its own path), word indices outside
//                      [0, W) read as 0, a range mask removes the invalid pairs; the word B[w + q + 1] stays in
//                      registers for the next word.  J's carry bit comes from the previous word of both bitmaps: inside
//                      a block it is kept from the previous iteration, at a block's first word it costs one more load of
//                      each bitmap and is never a value carried across workgroups.  Per segment and lag four popcounts
//                      (v_bcnt_u32_b32 pairs that add into the addend).  The lag loop is the OUTER one and each lag
//                      walks the word's segments on its own: the four result words of one lag live in registers, not
//                      those of eight (64 VGPRs).  Every lag enters a word with the same current class and leaves it with
//                      the class of the word's last segment, so the flushes are the same as with a shared walk.  A flush
//                      is int32 atomics without a return value, non-zero addends only, to addresses consecutive across
//                      lanes; it happens when the next segment's class differs and at the end of the block.  One code
//                      path: atomics also where a workgroup owns all of T, as in kernels_class.hip (a second path would
//                      need its own tests for nothing measurable).  No LDS, no cross-lane traffic, no scratch, and
//                      nothing waits for another workgroup.
#include "../../include/xmhw_amd.h"
#include "entry_common.h"
#include "stage_reduce.h"

namespace xmhw {

namespace {

constexpr int kCoThreads = 256;
using u64 = unsigned long long;

// bits a .. b (inclusive, 0 <= a <= b <= 63)
__device__ __forceinline__ u64 bit_range(int a, int b) {
    const u64 m = (b - a == 63) ? ~0ull : ((1ull << (b - a + 1)) - 1ull);
    return m << a;
}

__global__ __launch_bounds__(kCoThreads) void event_table_bits(const int32_t* __restrict__ start,
                                                                const int32_t* __restrict__ end,
                                                                const int64_t* __restrict__ offsets,
                                                                const int64_t* __restrict__ cell, int64_t C, int64_t Tn,
                                                                uint64_t* __restrict__ bits, int64_t ldb) {
    const int64_t j = static_cast<int64_t>(blockIdx.x) * kCoThreads + threadIdx.x;
    if (j >= C) return;
    const int64_t W = (Tn + 63) / 64;
    const int64_t cj = cell[j];
    int64_t cur = offsets[cj];
    const int64_t r1 = offsets[cj + 1];
    int64_t reach = -1;                              // the largest end among the rows consumed so far
    const int tail = static_cast<int>(Tn - (W - 1) * 64);                  // steps in the last word, 1..64
    for (int64_t w = 0; w < W; ++w) {
        const int64_t lo = w * 64, hi = lo + 63;
        u64 word = 0;
        if (reach >= lo) word = bit_range(0, static_cast<int>((reach < hi ? reach : hi) - lo));
        while (cur < r1) {
            const int64_t s = start[cur];
            if (s > hi) break;
            const int64_t e = end[cur];
            if (e >= lo) word |= bit_range(static_cast<int>((s > lo ? s : lo) - lo), static_cast<int>((e < hi ? e : hi) - lo));
            reach = e > reach ? e : reach;
            ++cur;
        }
        if (w == W - 1 && tail < 64) word &= (1ull << tail) - 1ull;        // the bits at t >= T are 0 whatever the table says
        bits[w * ldb + j] = word;
    }
}

// word w of a bitmap column, 0 outside [0, W) (w is uniform over the wave)
__device__ __forceinline__ u64 word_at(const uint64_t* __restrict__ p, int64_t ld, int64_t W, int64_t w, int64_t c, bool live) {
    return (live && w >= 0 && w < W) ? p[w * ld + c] : 0ull;
}

// the valid pairs of word w under lag l: bits j with 0 <= 64 w + j + l < T and 64 w + j < T (uniform over the wave)
__device__ __forceinline__ u64 valid_mask(int64_t w, int64_t lag, int64_t Tn) {
    int64_t a = (lag < 0 ? -lag : 0) - w * 64;                             // first valid bit
    int64_t b = (lag > 0 ? Tn - lag : Tn) - w * 64;                        // one past the last
    if (a < 0) a = 0;
    if (b > 64) b = 64;
    if (a >= b) return 0ull;
    return bit_range(static_cast<int>(a), static_cast<int>(b - 1));
}

__device__ __forceinline__ u64 shifted(u64 blo, u64 bhi, int r) {
    return r == 0 ? blo : (blo >> r) | (bhi << (64 - r));                  // r is uniform: a scalar branch; a shift by 64 is undefined
}

__device__ __forceinline__ void flush4(int32_t* __restrict__ p, int64_t ldo, int32_t (&v)[kCooccurChannels]) {
#pragma unroll
    for (int ch = 0; ch < kCooccurChannels; ++ch) {
        if (v[ch]) atomicAdd(p + ch * ldo, v[ch]);
        v[ch] = 0;
    }
}

// every table is its own __restrict__ argument: the uniform loads of segments and lags may then go through the scalar cache
// although the kernel writes (atomics) to counts
struct CoShape {
    int64_t lda, ldb, Tn, W, C, wb, ldo;             // wb: words per block
    int32_t L;
};

__global__ __launch_bounds__(kCoThreads) void cooccur_accumulate(
    const uint64_t* __restrict__ a_bits, const uint64_t* __restrict__ b_bits, const int32_t* __restrict__ seg_off,
    const int32_t* __restrict__ seg_class, const uint64_t* __restrict__ seg_mask, const int32_t* __restrict__ lags,
    int32_t* __restrict__ counts, CoShape g) {
    const int64_t c = static_cast<int64_t>(blockIdx.x) * kCoThreads + threadIdx.x;
    const bool live = c < g.C;
    const int32_t i0 = static_cast<int32_t>(blockIdx.z) * kCooccurLagGroup;
    const int32_t nl = g.L - i0 < kCooccurLagGroup ? g.L - i0 : kCooccurLagGroup;
    const int64_t nblk = (g.W + g.wb - 1) / g.wb;
    int32_t acc[kCooccurLagGroup][kCooccurChannels];
#pragma unroll
    for (int i = 0; i < kCooccurLagGroup; ++i)
#pragma unroll
        for (int ch = 0; ch < kCooccurChannels; ++ch) acc[i][ch] = 0;
    for (int64_t blk = blockIdx.y; blk < nblk; blk += gridDim.y) {
        const auto [w0, w1] = block_range(blk, g.wb, g.W);
        // the state at the block's first word: per lag the word B[w0 + q] and the top bit of J[w0 - 1]
        u64 bnext[kCooccurLagGroup];
        uint32_t carry = 0;                          // bit i: J's last bit of the previous word under lag i
        const u64 aprev = word_at(a_bits, g.lda, g.W, w0 - 1, c, live);
#pragma unroll
        for (int i = 0; i < kCooccurLagGroup; ++i) {
            bnext[i] = 0;
            if (i < nl) {
                const int64_t lag = lags[i0 + i];
                const int64_t q = lag >> 6;
                const int r = static_cast<int>(lag & 63);
                const u64 b1 = word_at(b_bits, g.ldb, g.W, w0 + q, c, live);
                const u64 v = w0 > 0 ? valid_mask(w0 - 1, lag, g.Tn) : 0ull;
                if (v >> 63) {                       // uniform: the pair (64 w0 - 1, lag) is valid
                    const u64 b0 = word_at(b_bits, g.ldb, g.W, w0 - 1 + q, c, live);
                    carry |= static_cast<uint32_t>((aprev & shifted(b0, b1, r)) >> 63) << i;
                }
                bnext[i] = b1;
            }
        }
        int32_t kcur = -1;                           // the class the addends belong to (uniform over the wave)
        for (int64_t w = w0; w < w1; ++w) {
            const u64 aw = word_at(a_bits, g.lda, g.W, w, c, live);
            const int32_t s0 = seg_off[w], s1 = seg_off[w + 1];
            int32_t kend = kcur;
#pragma unroll
            for (int i = 0; i < kCooccurLagGroup; ++i) {
                if (i < nl) {
                    const int64_t lag = lags[i0 + i];
                    const int64_t q = lag >> 6;
                    const int r = static_cast<int>(lag & 63);
                    const u64 blo = bnext[i];
                    const u64 bhi = word_at(b_bits, g.ldb, g.W, w + q + 1, c, live);
                    bnext[i] = bhi;
                    const u64 v = valid_mask(w, lag, g.Tn);
                    const u64 bl = shifted(blo, bhi, r) & v;
                    const u64 av = aw & v;
                    const u64 both = av & bl;
                    const u64 a_only = av & ~bl;
                    const u64 b_only = bl & ~av;
                    const u64 onset = both & ~((both << 1) | ((carry >> i) & 1u));
                    carry = (carry & ~(1u << i)) | (static_cast<uint32_t>(both >> 63) << i);
                    int32_t k = kcur;
                    for (int32_t s = s0; s < s1; ++s) {
                        const int32_t ks = seg_class[s];
                        const u64 m = seg_mask[s];
                        if (ks != k) {
                            if (k >= 0 && live)
                                flush4(counts + ((static_cast<int64_t>(k) * g.L + i0 + i) * kCooccurChannels) * g.ldo + c,
                                       g.ldo, acc[i]);
                            k = ks;
                        }
                        acc[i][0] += __popcll(both & m);
                        acc[i][1] += __popcll(a_only & m);
                        acc[i][2] += __popcll(b_only & m);
                        acc[i][3] += __popcll(onset & m);
                    }
                    kend = k;
                }
            }
            kcur = kend;
        }
        if (kcur >= 0 && live) {
#pragma unroll
            for (int i = 0; i < kCooccurLagGroup; ++i)
                if (i < nl)
                    flush4(counts + ((static_cast<int64_t>(kcur) * g.L + i0 + i) * kCooccurChannels) * g.ldo + c, g.ldo,
                           acc[i]);
        }
    }
}

hipError_t launch_event_table_bits(const int32_t* start, const int32_t* end, const int64_t* offsets, const int64_t* cell,
                                   int64_t C, int64_t Tn, uint64_t* bits, int64_t ldb, hipStream_t stream) {
    if (C <= 0 || Tn <= 0) return hipSuccess;
    const int64_t gx = (C + kCoThreads - 1) / kCoThreads;
    hipLaunchKernelGGL(event_table_bits, dim3(static_cast<unsigned>(gx)), dim3(kCoThreads), 0, stream, start, end, offsets,
                       cell, C, Tn, bits, ldb);
    return hipGetLastError();
}

hipError_t launch_cooccur_init(int32_t K, int32_t L, int64_t C, int32_t* counts, int64_t ldo, hipStream_t stream) {
    return zero_rows(counts, sizeof(int32_t), static_cast<int64_t>(K) * L * kCooccurChannels, C, ldo, stream);
}

hipError_t launch_cooccur_accumulate(const uint64_t* a_bits, int64_t lda, const uint64_t* b_bits, int64_t ldb, int64_t Tn,
                                     int64_t C, const int32_t* seg_off, const int32_t* seg_class, const uint64_t* seg_mask,
                                     const int32_t* lags, int32_t L, int64_t block_words, int32_t* counts, int64_t ldo,
                                     hipStream_t stream) {
    if (C <= 0 || Tn <= 0 || L <= 0) return hipSuccess;
    const int64_t W = (Tn + 63) / 64;
    const int64_t gz = ceil_div(L, kCooccurLagGroup);
    int64_t wb = block_words > 0 ? block_words : cooccur_auto_block(W, C, gz);
    if (wb > W) wb = W;
    const CoShape g{lda, ldb, Tn, W, C, wb, ldo, L};
    hipLaunchKernelGGL(cooccur_accumulate, stage_grid(C, kCoThreads, W, wb, gz), dim3(kCoThreads), 0, stream, a_bits, b_bits,
                       seg_off, seg_class, seg_mask, lags, counts, g);
    return hipGetLastError();
}

}  // namespace

}  // namespace xmhw

// ---- the C entries of mhw_cooccurrence() (include/xmhw_amd.h) ---------------------------------------------------------
namespace {

using namespace xmhw::entry;

static std::atomic<int> g_cooccur_block{0};      // words a workgroup takes per block, 0 = automatic (xmhw_set_cooccur_block)

static int cooccur_check_shape(int32_t K, int32_t L, int64_t Tn, int64_t C) {
    if (K < 1 || K > xmhw::kCooccurMaxClasses)
        return fail(XMHW_ERR_UNSUPPORTED, "cooccur: K must be in [1, " + std::to_string(xmhw::kCooccurMaxClasses) + "]");
    if (L < 1 || L > xmhw::kCooccurMaxLags)
        return fail(XMHW_ERR_UNSUPPORTED, "cooccur: L must be in [1, " + std::to_string(xmhw::kCooccurMaxLags) + "]");
    if (Tn > 0x7FFFFFFFll || C > 0x7FFFFFFFll) return fail(XMHW_ERR_UNSUPPORTED, "cooccur: 2^31 steps or cells and more");
    return XMHW_OK;
}

}  // namespace

extern "C" {

int xmhw_event_table_bits(const int32_t* start, const int32_t* end, const int64_t* offsets, const int64_t* cell, int64_t C,
                          int64_t T, uint64_t* bits, int64_t ldb, void* stream) {
    if (T > 0x7FFFFFFFll || C > 0x7FFFFFFFll) return fail(XMHW_ERR_UNSUPPORTED, "event_table_bits: 2^31 steps or cells and more");
    if (T < 0 || C < 0 || ldb < C) return fail(XMHW_ERR_INVALID, "bad T/C/ldb");
    if (C == 0 || T == 0) return XMHW_OK;
    if (!offsets || !cell || !bits) return fail(XMHW_ERR_INVALID, "NULL buffer");
    return status_of(xmhw::launch_event_table_bits(start, end, offsets, cell, C, T, bits, ldb,
                                                   static_cast<hipStream_t>(stream)),
                     "event_table_bits launch");
}
int xmhw_set_cooccur_block(int32_t words) { return set_knob(g_cooccur_block, words, "words must be >= 0"); }
int xmhw_cooccur_init(int32_t K, int32_t L, int64_t C, int32_t* counts, int64_t ldo, void* stream) {
    if (cooccur_check_shape(K, L, 0, C) != XMHW_OK) return XMHW_ERR_UNSUPPORTED;
    if (C < 0 || ldo < C) return fail(XMHW_ERR_INVALID, "bad C/ldo");
    if (C == 0) return XMHW_OK;
    if (!counts) return fail(XMHW_ERR_INVALID, "NULL output buffer");
    return status_of(xmhw::launch_cooccur_init(K, L, C, counts, ldo, static_cast<hipStream_t>(stream)), "cooccur_init");
}
int xmhw_cooccur_accumulate(const uint64_t* a_bits, int64_t lda, const uint64_t* b_bits, int64_t ldb, int64_t T, int64_t C,
                            const int32_t* class_of_t, int32_t K, const int32_t* lags, int32_t L, int32_t* counts,
                            int64_t ldo, void* stream) {
    if (cooccur_check_shape(K, L, T, C) != XMHW_OK) return XMHW_ERR_UNSUPPORTED;
    if (T < 0 || C < 0 || lda < C || ldb < C || ldo < C) return fail(XMHW_ERR_INVALID, "bad T/C/lda/ldb/ldo");
    if (!lags || (T > 0 && !class_of_t)) return fail(XMHW_ERR_INVALID, "NULL class_of_t or lags");
    if (int rc = check_labels(class_of_t, T, -1, K, kClassesOutside)) return rc;
    if (C == 0 || T == 0) return XMHW_OK;
    if (!a_bits || !b_bits || !counts) return fail(XMHW_ERR_INVALID, "NULL buffer");
    RowsRef classes;                                   // the content-keyed cache of int32 tables
    if (int rc = upload_table(class_of_t, T, "class table upload", &classes)) return rc;
    if (int rc = status_of(cooccur_segments(classes, T), "segment table upload")) return rc;
    RowsRef lag_table;
    if (int rc = upload_table(lags, L, "lag table upload", &lag_table)) return rc;
    return status_of(xmhw::launch_cooccur_accumulate(a_bits, lda, b_bits, ldb, T, C, classes->seg_off, classes->seg_class,
                                                     classes->seg_mask, lag_table->d_rows, L, g_cooccur_block.load(), counts,
                                                     ldo, static_cast<hipStream_t>(stream)),
                     "cooccur_accumulate launch");
}

}  // extern "C"
