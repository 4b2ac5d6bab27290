// kernels_distribution.hip -- anomaly_distribution(): per-cell histograms, quantiles and moments of the anomaly (DESIGN.md
// 3.23).  The definition is in include/xmhw_amd.h, "anomaly_distribution()"; in short, with d(t) the scaled anomaly of a
// cell, valid as fixed_state() says, and q its fixed-point integer: per class k of the step and cell c, over the valid
// steps, the counts hist[k][0 .. B + 1][c] of the rows of hist_bin.h, n, the sums of q and q^2 in 64 bits, of q^3 and q^4
// in 128 bits (wide_sum.h) and the keys of the largest d and of the largest -d.
//
//   distribution_accumulate<T>
//                     the frame of a class reduction (kernels.h): lane = cell, a workgroup is 256 cells x a block of
//                     steps; the addends of the current class stay in registers, and this is the first stage whose
//                     accumulator's address is the sample.
//   the histogram     of a lane lives in LDS, in the lane's own column: two 16-bit counters to a dword, dword
//                     (b >> 1) * 256 + lane -- the bank is the lane, whatever the sample, and only the lane itself ever
//                     touches its column, so there is no conflict and no barrier.  One LDS addition without a return
//                     value per sample.  The dynamic LDS size follows B: 32 KB up to 64 bins, 64 KB up to 128, 128 KB up
//                     to 256, so that few bins keep several workgroups on a CU.  UNDER and OVER are register counters.
//   the order         the bin index is formed from the sample in registers, compared against [0, B), and only then becomes
//                     an LDS address: no value derived from data reaches an address unchecked.  A NaN or a d out of range
//                     never gets that far (fixed_state()).
//   a flush           on a class change, at the end of a block and after kHistHalfMax steps of a run (a half holds no
//                     more): the register addends by integer atomics as in the other stages -- the 128-bit ones by the
//                     carry rule of wide_sum.h --, then the lane exchanges the dwords of its column with 0, from the lowest
//                     to the highest dword that the WAVE touched in the run (two registers, reduced over the wave: the
//                     loop bounds are uniform and the rows of a trip coalesce), and adds every non-zero half to
//                     hist[k][row][c].  A calendar class that lasts 30 steps scans a few dwords, not B / 2.
//   the loads         of kDsAhead steps are requested before the first of them is worked on: with 128 KB of LDS a CU holds
//                     one workgroup, one wave per SIMD, and nothing else covers a trip to memory.
//   a lane past C     stays in the kernel (the wave reduction wants every lane) and takes every sample as NaN.
//   distribution_finish
//                     lane = cell, a loop over the classes: one upward walk over the B + 2 rows of the cell with a
//                     running count serves the P ranks (the row with running < r <= running + h holds rank r: below =
//                     running, count = h; the ranks need no order for that) and the L levels (n - running at row 1 + e),
//                     and the float64 of the smallest d is 0 - that of the largest -d.
#include "../../include/xmhw_amd.h"
#include "entry_common.h"
#include "stage_reduce.h"
#include "hist_bin.h"
#include "wide_sum.h"

namespace xmhw {

// What the stage computes (hist_bin.h, wide_sum.h hold the pieces): per cell and class of the step, over the steps
// whose anomaly d = (sample - base[row_of_t[t]][c]) * 2^-shift is valid, with q = rint(d * 2^kDistributionBits): the counts
// hist[k][0 .. B + 1][c] of the rows of the bins (lo_q, width_q, B) -- row 0 UNDER, row B + 1 OVER --, n[k][c], s1 and s2
// [k][c] the sums of q and q^2, s3 and s4 [k][0..1][c] the sums of q^3 and q^4 as 128-bit integers (low words, high words),
// all ADDED, and kmax, kmin [k][c] RAISED to the key of the largest d and of the largest -d; the definition is in
// include/xmhw_amd.h, "anomaly_distribution()".  *n_range counts the steps of a class whose d is not NaN and out of range.
// launch_distribution_finish turns the keys into float64 (kmin: the smallest d; NaN for none) and writes, from the
// histogram, qbin, qbelow and qcount [k][P][c] of the ranks of p_q[P] and n_at_least[k][L][c] of the edges edge[L].  row_of_t and
// class_of_t are DEVICE arrays, p_q and edge HOST arrays here.  block_steps: the steps a workgroup takes per block,
// 0 = automatic; same results for every value.
constexpr int kDistributionMaxBins = 256;            // two 16-bit counters to a dword: 128 KB of LDS per workgroup
constexpr int kDistributionMaxClasses = 64;
constexpr int kDistributionMaxQuantiles = 16;
constexpr int kDistributionMaxLevels = 8;
constexpr int kDistributionMaxSteps = 1 << 17;       // T below it, as the cap of lag_correlation(): 2^17 * 2^46 = 2^63
constexpr int kDistributionBits = 16;
constexpr int kDistributionRangeBits = 7;
constexpr int kDistributionMaxShift = 24;

static_assert(kDistributionBits == kFixedBits && kDistributionRangeBits == kFixedRangeBits, "one scale for every stage");
static_assert(kDistributionMaxBins == kHistMaxBins, "a column of 128 dwords at most");

namespace {

constexpr int kDsThreads = 256;
constexpr int kDsAhead = 8;
using u64 = unsigned long long;

template <typename T>
struct DsIn {
    const T* x;
    int64_t ld;
    const double* base;                              // [Dr][ldb]
    int64_t ldb;
    const int32_t* row_of_t;
    int32_t one_row;                                 // Dr == 1: the base is a constant per cell, read once
    double scale;                                    // 2^-shift
};

struct DsOut {
    int32_t* hist;                                   // [K][B + 2][ldo]
    int32_t* n;                                      // [K][ldo]
    u64 *s1, *s2;                                    // [K][ldo]
    u64 *s3, *s4;                                    // [K][2][ldo]: low words, high words
    u64 *kmin, *kmax;                                // [K][ldo]: the keys of the largest -d and the largest d
    int64_t ldo;
    u64* n_range;
};

// the addends of one lane for the current class
struct DsAcc {
    int32_t n;
    uint32_t under, over;
    int64_t s1, s2;
    Wide s3, s4;
    u64 kmin, kmax;
    int32_t dlo, dhi;                                // the lowest and highest dword of the column touched in the run
    __device__ __forceinline__ void clear() {
        n = 0;
        under = over = 0;
        s1 = s2 = 0;
        s3 = s4 = Wide{0, 0};
        kmin = kmax = 0;
        dlo = 0x7FFFFFFF;
        dhi = -1;
    }
};

__device__ __forceinline__ void ds_flush_wide(u64* p, int64_t ldo, const Wide& v) {
    if (v.lo == 0 && v.hi == 0) return;
    u64 high = static_cast<u64>(v.hi);
    if (v.lo) high = wide_flush_high(v, atomicAdd(p, static_cast<u64>(v.lo)));
    if (high) atomicAdd(p + ldo, high);
}

template <typename T>
__global__ __launch_bounds__(kDsThreads) void distribution_accumulate(DsIn<T> in, int64_t Tn, int64_t C,
                                                                      const int32_t* __restrict__ class_of_t, int32_t K,
                                                                      int64_t tb, HistBins bins, DsOut out) {
    extern __shared__ uint32_t ds_columns[];         // [hist_dwords(B)][kDsThreads]
    const int64_t c = static_cast<int64_t>(blockIdx.x) * kDsThreads + threadIdx.x;
    const bool live = c < C;                         // (no early return: the flush reduces over the wave)
    uint32_t* const mine = ds_columns + threadIdx.x; // the lane's column: dword i at mine[i * kDsThreads]
    const int32_t ndw = hist_dwords(bins.B);
    for (int32_t i = 0; i < ndw; ++i) mine[i * kDsThreads] = 0;        // once: a flush leaves zeros behind
    const double b0 = live && in.one_row ? in.base[c] : 0.0;
    // T < 2^17: steps and blocks are 32-bit here, addresses are not
    const int32_t Ts = static_cast<int32_t>(Tn), bs = static_cast<int32_t>(tb < Tn ? tb : Tn);
    const int32_t nblk = (Ts - 1) / bs + 1;
    const int64_t rows = bins.B + 2;
    DsAcc v;
    v.clear();
    u64 range = 0;
    int32_t run_steps = 0;                           // the steps of the run since its last flush (uniform over the wave)
    const auto flush_class = [&](int32_t k) {
        run_steps = 0;
        int32_t lo = v.dlo, hi = v.dhi;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const int32_t lo2 = __shfl_xor(lo, d, 64), hi2 = __shfl_xor(hi, d, 64);
            lo = lo2 < lo ? lo2 : lo;
            hi = hi2 > hi ? hi2 : hi;
        }
        int32_t* const h = out.hist + static_cast<int64_t>(k) * rows * out.ldo + c;      // row r at h[r * ldo]
        if (v.n) {                                   // (a lane past C never has a sample)
            const int64_t p = static_cast<int64_t>(k) * out.ldo + c;
            atomicAdd(out.n + p, v.n);
            if (v.s1) atomicAdd(out.s1 + p, static_cast<u64>(v.s1));
            atomicAdd(out.s2 + p, static_cast<u64>(v.s2));
            ds_flush_wide(out.s3 + 2 * static_cast<int64_t>(k) * out.ldo + c, out.ldo, v.s3);
            ds_flush_wide(out.s4 + 2 * static_cast<int64_t>(k) * out.ldo + c, out.ldo, v.s4);
            atomicMax(out.kmin + p, v.kmin);
            atomicMax(out.kmax + p, v.kmax);
            if (v.under) atomicAdd(h, static_cast<int32_t>(v.under));
            if (v.over) atomicAdd(h + (rows - 1) * out.ldo, static_cast<int32_t>(v.over));
        }
        // lo .. hi lie inside [0, ndw): they come from bin indices that were checked against [0, B)
        for (int32_t i = lo; i <= hi; ++i) {
            const uint32_t w = __hip_atomic_exchange(mine + i * kDsThreads, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (w & 0xFFFFu) atomicAdd(h + (1 + 2 * static_cast<int64_t>(i)) * out.ldo, static_cast<int32_t>(w & 0xFFFFu));
            if (w >> 16) atomicAdd(h + (2 + 2 * static_cast<int64_t>(i)) * out.ldo, static_cast<int32_t>(w >> 16));
        }
        v.clear();
    };
    // a sample and its base as they are read; the anomaly is formed where it is used
    struct Raw {
        T s;
        double b;
    };
    const auto load = [&](int32_t t) -> Raw {
        if (!live) return {static_cast<T>(make_nan()), 0.0};
        return {in.x[static_cast<int64_t>(t) * in.ld + c],
                in.one_row ? b0 : in.base[static_cast<int64_t>(in.row_of_t[t]) * in.ldb + c]};
    };
    const auto label = [&](int32_t t) -> int32_t {
        const int32_t k = class_of_t[t];
        return k < K ? k : -1;                       // (labels are checked on the host)
    };
    for (int32_t blk = blockIdx.y; blk < nblk; blk += gridDim.y) {
        const auto [t0, t1] = block_range<int32_t>(blk, bs, Ts);
        ClassRun run;
        // step t of class k >= 0 (wave-uniform) with its sample
        const auto step = [&](int32_t k, const Raw& r) {
            run.enter(k, flush_class);
            if (run_steps == kHistHalfMax) flush_class(k);
            ++run_steps;
            const double d = (static_cast<double>(r.s) - r.b) * in.scale;
            const int state = fixed_state(d);
            if (state < 0) ++range;
            if (state <= 0) return;
            const int32_t q = static_cast<int32_t>(fixed_value(d));
            const int64_t q2 = static_cast<int64_t>(q) * q;
            ++v.n;
            v.s1 += q;
            v.s2 += q2;
            wide_mac_i32(v.s3, static_cast<uint64_t>(q2), q);
            wide_mac_u64(v.s4, static_cast<uint64_t>(q2), static_cast<uint64_t>(q2));
            const u64 up = f64_key(d + 0.0), down = f64_key(0.0 - d);  // -0.0 counts as 0.0
            v.kmax = up > v.kmax ? up : v.kmax;
            v.kmin = down > v.kmin ? down : v.kmin;
            const int32_t b = hist_bin_floor(bins, q);
            if (b < 0) {
                ++v.under;
            } else if (b >= bins.B) {
                ++v.over;
            } else {                                 // 0 <= b < B: the one place a sample becomes an address
                const int32_t dw = hist_half_dword(b);
                __hip_atomic_fetch_add(mine + dw * kDsThreads, hist_half_addend(b), __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_WORKGROUP);
                v.dlo = dw < v.dlo ? dw : v.dlo;
                v.dhi = dw > v.dhi ? dw : v.dhi;
            }
        };
        for (int32_t t = t0; t < t1; t += kDsAhead) {
            int32_t k[kDsAhead];
            Raw r[kDsAhead];
#pragma unroll
            for (int j = 0; j < kDsAhead; ++j) {
                k[j] = t + j < t1 ? label(t + j) : -1;
                r[j] = k[j] >= 0 ? load(t + j) : Raw{};    // uniform over the wave: a step without a class is not read
            }
#pragma unroll
            for (int j = 0; j < kDsAhead; ++j)
                if (k[j] >= 0) step(k[j], r[j]);
        }
        run.leave(flush_class);
    }
    if (range) atomicAdd(out.n_range, range);
}

struct DsFinish {
    uint64_t p_q[kDistributionMaxQuantiles];
    int32_t edge[kDistributionMaxLevels];
    int32_t P, L;
};

__global__ __launch_bounds__(kDsThreads) void distribution_finish(int32_t K, int32_t B, int64_t C,
                                                                  const int32_t* __restrict__ hist,
                                                                  const int32_t* __restrict__ n, DsFinish f,
                                                                  int32_t* __restrict__ qbin, int32_t* __restrict__ qbelow,
                                                                  int32_t* __restrict__ qcount, int32_t* __restrict__ n_at_least,
                                                                  double* __restrict__ kmin,
                                                                  int64_t ldo) {
    const int64_t c = static_cast<int64_t>(blockIdx.x) * kDsThreads + threadIdx.x;
    if (c >= C) return;
    const int64_t rows = B + 2;
    for (int32_t k = 0; k < K; ++k) {
        const int64_t p = static_cast<int64_t>(k) * ldo + c;
        kmin[p] = 0.0 - kmin[p];                     // the key was that of the largest -d; NaN stays NaN
        const int32_t nn = n[p];
        int64_t rank[kDistributionMaxQuantiles];
#pragma unroll
        for (int j = 0; j < kDistributionMaxQuantiles; ++j) rank[j] = j < f.P ? hist_rank(f.p_q[j], nn) : 0;
        if (nn == 0) {
#pragma unroll
            for (int j = 0; j < kDistributionMaxQuantiles; ++j)
                if (j < f.P) {
                    qbin[(static_cast<int64_t>(k) * f.P + j) * ldo + c] = INT32_MIN;
                    qbelow[(static_cast<int64_t>(k) * f.P + j) * ldo + c] = 0;
                    qcount[(static_cast<int64_t>(k) * f.P + j) * ldo + c] = 0;
                }
        }
        const int32_t* const h = hist + static_cast<int64_t>(k) * rows * ldo + c;
        int64_t running = 0;
        for (int32_t row = 0; row < rows; ++row) {
            const int32_t here = h[static_cast<int64_t>(row) * ldo];
#pragma unroll
            for (int l = 0; l < kDistributionMaxLevels; ++l)
                if (l < f.L && row == 1 + f.edge[l])
                    n_at_least[(static_cast<int64_t>(k) * f.L + l) * ldo + c] = static_cast<int32_t>(nn - running);
#pragma unroll
            for (int j = 0; j < kDistributionMaxQuantiles; ++j)
                if (j < f.P && running < rank[j] && rank[j] <= running + here) {      // (never for n == 0: here is 0)
                    qbin[(static_cast<int64_t>(k) * f.P + j) * ldo + c] = row - 1;
                    qbelow[(static_cast<int64_t>(k) * f.P + j) * ldo + c] = static_cast<int32_t>(running);
                    qcount[(static_cast<int64_t>(k) * f.P + j) * ldo + c] = here;
                }
            running += here;
        }
    }
}

// the dynamic LDS of B bins: 32, 64 or 128 KB
size_t ds_lds_bytes(int32_t B) { return (B <= 64 ? 32u : B <= 128 ? 64u : 128u) * 1024u; }

hipError_t launch_distribution_init(int32_t K, int32_t B, int64_t C, int32_t* hist, int32_t* n, int64_t* s1, int64_t* s2,
                                    int64_t* s3, int64_t* s4, uint64_t* kmin, uint64_t* kmax, int64_t ldo, int64_t* n_range,
                                    hipStream_t stream) {
    hipError_t e = hipMemsetAsync(n_range, 0, sizeof(int64_t), stream);
    if (e == hipSuccess) e = zero_rows(hist, sizeof(int32_t), static_cast<int64_t>(K) * (B + 2), C, ldo, stream);
    if (e == hipSuccess) e = zero_rows(n, sizeof(int32_t), K, C, ldo, stream);
    for (void* p : {static_cast<void*>(s1), static_cast<void*>(s2), static_cast<void*>(kmin), static_cast<void*>(kmax)})
        if (e == hipSuccess) e = zero_rows(p, sizeof(int64_t), K, C, ldo, stream);          // key 0: no value yet
    for (int64_t* p : {s3, s4})
        if (e == hipSuccess) e = zero_rows(p, sizeof(int64_t), 2 * static_cast<int64_t>(K), C, ldo, stream);
    return e;
}

template <typename T>
hipError_t launch_distribution_accumulate(const T* ts, int64_t Tn, int64_t C, int64_t ld, const double* base, int64_t ldb,
                                          int64_t Dr, const int32_t* row_of_t, int32_t shift, const int32_t* class_of_t,
                                          int32_t K, int64_t lo_q, int32_t width_q, int32_t B, int64_t block_steps,
                                          int32_t* hist, int32_t* n, int64_t* s1, int64_t* s2, int64_t* s3, int64_t* s4,
                                          uint64_t* kmin, uint64_t* kmax, int64_t ldo, int64_t* n_range, hipStream_t stream) {
    if (C <= 0 || Tn <= 0 || K <= 0) return hipSuccess;
    if (B < 1 || B > kDistributionMaxBins || width_q < 1 || lo_q < -kHistMaxEdge || lo_q > kHistMaxEdge ||
        Tn >= kDistributionMaxSteps || shift < 0 || shift > kDistributionMaxShift)
        return hipErrorInvalidValue;
    const int64_t tb = block_steps > 0 ? block_steps : distribution_auto_block(Tn, C);
    const DsIn<T> in{ts, ld, base, ldb, row_of_t, Dr == 1, ldexp(1.0, -shift)};
    const auto u = [](void* p) { return reinterpret_cast<u64*>(p); };
    const DsOut out{hist, n, u(s1), u(s2), u(s3), u(s4), u(kmin), u(kmax), ldo, u(n_range)};
    const size_t lds = ds_lds_bytes(B);
    // more than 64 KB of dynamic LDS is asked for before the launch
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&distribution_accumulate<T>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds));
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((distribution_accumulate<T>), stage_grid(C, kDsThreads, Tn, tb), dim3(kDsThreads), lds, stream, in, Tn,
                       C, class_of_t, K, tb, hist_bins(lo_q, width_q, B), out);
    return hipGetLastError();
}

hipError_t launch_distribution_finish(int32_t K, int32_t B, int64_t C, const int32_t* hist, const int32_t* n, double* kmin,
                                      double* kmax, const uint64_t* p_q, int32_t P, const int32_t* edge, int32_t L,
                                      int32_t* qbin, int32_t* qbelow, int32_t* qcount, int32_t* n_at_least, int64_t ldo,
                                      hipStream_t stream) {
    if (C <= 0 || K <= 0) return hipSuccess;
    if (B < 1 || B > kDistributionMaxBins || P < 0 || P > kDistributionMaxQuantiles || L < 0 || L > kDistributionMaxLevels)
        return hipErrorInvalidValue;
    hipError_t e = launch_keys_to_f64(kmax, K, C, ldo, stream);        // K <= kDistributionMaxClasses rows
    if (e == hipSuccess) e = launch_keys_to_f64(kmin, K, C, ldo, stream);
    if (e != hipSuccess) return e;
    DsFinish f{};
    for (int32_t j = 0; j < P; ++j) f.p_q[j] = p_q[j];
    for (int32_t l = 0; l < L; ++l) f.edge[l] = edge[l];
    f.P = P;
    f.L = L;
    hipLaunchKernelGGL(distribution_finish, dim3(static_cast<unsigned>(ceil_div(C, kDsThreads))), dim3(kDsThreads), 0, stream, K,
                       B, C, hist, n, f, qbin, qbelow, qcount, n_at_least, kmin, ldo);
    return hipGetLastError();
}

}  // namespace

}  // namespace xmhw

// ---- the C entries of anomaly_distribution() (include/xmhw_amd.h) -----------------------------------------------------
namespace {

using namespace xmhw::entry;

static std::atomic<int> g_distribution_block{0};    // steps a workgroup takes per block, 0 = automatic (xmhw_set_distribution_block)

static_assert(XMHW_DISTRIBUTION_MAX_BINS == xmhw::kDistributionMaxBins &&
                  XMHW_DISTRIBUTION_MAX_CLASSES == xmhw::kDistributionMaxClasses &&
                  XMHW_DISTRIBUTION_MAX_QUANTILES == xmhw::kDistributionMaxQuantiles &&
                  XMHW_DISTRIBUTION_MAX_LEVELS == xmhw::kDistributionMaxLevels &&
                  XMHW_DISTRIBUTION_MAX_STEPS == xmhw::kDistributionMaxSteps &&
                  XMHW_DISTRIBUTION_BITS == xmhw::kDistributionBits &&
                  XMHW_DISTRIBUTION_RANGE_BITS == xmhw::kDistributionRangeBits &&
                  XMHW_DISTRIBUTION_MAX_SHIFT == xmhw::kDistributionMaxShift,
              "the public limits of anomaly_distribution() are the kernel's");

static int distribution_check_shape(int32_t K, int32_t B, int64_t Tn, int64_t C) {
    if (K < 1 || K > xmhw::kDistributionMaxClasses)
        return fail(XMHW_ERR_UNSUPPORTED,
                    "distribution: K must be in [1, " + std::to_string(xmhw::kDistributionMaxClasses) + "]");
    if (B < 1 || B > xmhw::kDistributionMaxBins)
        return fail(XMHW_ERR_UNSUPPORTED, "distribution: B must be in [1, " + std::to_string(xmhw::kDistributionMaxBins) + "]");
    if (Tn >= xmhw::kDistributionMaxSteps) return fail(XMHW_ERR_UNSUPPORTED, "distribution: 2^17 steps and more");
    if (C > 0x7FFFFFFFll) return fail(XMHW_ERR_UNSUPPORTED, "distribution: 2^31 cells and more");
    return XMHW_OK;
}

template <typename T>
int distribution_accumulate(const T* ts, int64_t Tn, int64_t C, int64_t ld, const double* base, int64_t ldb, int64_t Dr,
                            const int32_t* row_of_t, int32_t shift, const int32_t* class_of_t, int32_t K, int64_t lo_q,
                            int32_t width_q, int32_t B, int32_t* hist, int32_t* n, int64_t* s1, int64_t* s2, int64_t* s3,
                            int64_t* s4, uint64_t* kmin, uint64_t* kmax, int64_t ldo, int64_t* n_range, void* stream) {
    if (distribution_check_shape(K, B, Tn, C) != XMHW_OK) return XMHW_ERR_UNSUPPORTED;
    if (width_q < 1) return fail(XMHW_ERR_UNSUPPORTED, "distribution: width_q must be >= 1");
    if (lo_q < -(int64_t{1} << 23) || lo_q > (int64_t{1} << 23))
        return fail(XMHW_ERR_UNSUPPORTED, "distribution: lo_q must be in [-2^23, 2^23]");
    if (shift < 0 || shift > xmhw::kDistributionMaxShift)
        return fail(XMHW_ERR_UNSUPPORTED,
                    "distribution: shift must be in [0, " + std::to_string(xmhw::kDistributionMaxShift) + "]");
    if (Tn < 0 || C < 0 || ld < C || ldb < C || ldo < C || Dr < 1) return fail(XMHW_ERR_INVALID, "bad T/C/ld/ldb/ldo/D");
    if (Tn > 0 && (!class_of_t || !row_of_t)) return fail(XMHW_ERR_INVALID, "NULL host table");
    if (int rc = check_labels(class_of_t, Tn, -1, K, kClassesOutside)) return rc;
    if (int rc = check_labels(row_of_t, Tn, 0, Dr, kRowsOutside)) return rc;
    if (C == 0 || Tn == 0) return XMHW_OK;
    if (!ts || !base || !hist || !n || !s1 || !s2 || !s3 || !s4 || !kmin || !kmax || !n_range)
        return fail(XMHW_ERR_INVALID, "NULL buffer");
    RowsRef rows;
    if (int rc = upload_table(row_of_t, Tn, "row table upload", &rows)) return rc;
    RowsRef classes;                                   // the same content-keyed cache: one more int32[T] table
    if (int rc = upload_table(class_of_t, Tn, "class table upload", &classes)) return rc;
    return status_of(xmhw::launch_distribution_accumulate<T>(ts, Tn, C, ld, base, ldb, Dr, rows->d_rows, shift, classes->d_rows,
                                                             K, lo_q, width_q, B, g_distribution_block.load(), hist, n, s1,
                                                             s2, s3, s4, kmin, kmax, ldo, n_range,
                                                             static_cast<hipStream_t>(stream)),
                     "distribution_accumulate launch");
}

}  // namespace

extern "C" {

int xmhw_set_distribution_block(int32_t steps) { return set_knob(g_distribution_block, steps, "steps must be >= 0"); }
int xmhw_distribution_init(int32_t K, int32_t B, int64_t C, int32_t* hist, int32_t* n, int64_t* s1, int64_t* s2, int64_t* s3,
                           int64_t* s4, uint64_t* kmin, uint64_t* kmax, int64_t ldo, int64_t* n_range, void* stream) {
    if (distribution_check_shape(K, B, 1, C) != XMHW_OK) return XMHW_ERR_UNSUPPORTED;
    if (C < 0 || ldo < C) return fail(XMHW_ERR_INVALID, "bad C/ldo");
    if (!n_range || (C > 0 && (!hist || !n || !s1 || !s2 || !s3 || !s4 || !kmin || !kmax)))
        return fail(XMHW_ERR_INVALID, "NULL output buffer");
    return status_of(xmhw::launch_distribution_init(K, B, C, hist, n, s1, s2, s3, s4, kmin, kmax, ldo, n_range,
                                                    static_cast<hipStream_t>(stream)),
                     "distribution_init");
}
int xmhw_distribution_accumulate_f32(const float* ts, int64_t T, int64_t C, int64_t ld, const double* base, int64_t ldb,
                                     int64_t Dr, const int32_t* row_of_t, int32_t shift, const int32_t* class_of_t, int32_t K,
                                     int64_t lo_q, int32_t width_q, int32_t B, int32_t* hist, int32_t* n, int64_t* s1,
                                     int64_t* s2, int64_t* s3, int64_t* s4, uint64_t* kmin, uint64_t* kmax, int64_t ldo,
                                     int64_t* n_range, void* stream) {
    return distribution_accumulate<float>(ts, T, C, ld, base, ldb, Dr, row_of_t, shift, class_of_t, K, lo_q, width_q, B, hist,
                                          n, s1, s2, s3, s4, kmin, kmax, ldo, n_range, stream);
}
int xmhw_distribution_accumulate_f64(const double* ts, int64_t T, int64_t C, int64_t ld, const double* base, int64_t ldb,
                                     int64_t Dr, const int32_t* row_of_t, int32_t shift, const int32_t* class_of_t, int32_t K,
                                     int64_t lo_q, int32_t width_q, int32_t B, int32_t* hist, int32_t* n, int64_t* s1,
                                     int64_t* s2, int64_t* s3, int64_t* s4, uint64_t* kmin, uint64_t* kmax, int64_t ldo,
                                     int64_t* n_range, void* stream) {
    return distribution_accumulate<double>(ts, T, C, ld, base, ldb, Dr, row_of_t, shift, class_of_t, K, lo_q, width_q, B, hist,
                                           n, s1, s2, s3, s4, kmin, kmax, ldo, n_range, stream);
}
int xmhw_distribution_finish(int32_t K, int32_t B, int64_t C, const int32_t* hist, const int32_t* n, double* kmin, double* kmax,
                             const uint64_t* p_q, int32_t P, const int32_t* edge, int32_t L, int32_t* qbin, int32_t* qbelow,
                             int32_t* qcount, int32_t* n_at_least, int64_t ldo, void* stream) {
    if (distribution_check_shape(K, B, 1, C) != XMHW_OK) return XMHW_ERR_UNSUPPORTED;
    if (P < 0 || P > xmhw::kDistributionMaxQuantiles)
        return fail(XMHW_ERR_UNSUPPORTED,
                    "distribution: P must be in [0, " + std::to_string(xmhw::kDistributionMaxQuantiles) + "]");
    if (L < 0 || L > xmhw::kDistributionMaxLevels)
        return fail(XMHW_ERR_UNSUPPORTED, "distribution: L must be in [0, " + std::to_string(xmhw::kDistributionMaxLevels) + "]");
    if (C < 0 || ldo < C) return fail(XMHW_ERR_INVALID, "bad C/ldo");
    if ((P > 0 && !p_q) || (L > 0 && !edge)) return fail(XMHW_ERR_INVALID, "NULL host table");
    for (int32_t j = 0; j < P; ++j)
        if (p_q[j] > (uint64_t{1} << 32)) return fail(XMHW_ERR_INVALID, "p_q outside [0, 2^32]");
    for (int32_t l = 0; l < L; ++l)
        if (edge[l] < 0 || edge[l] > B) return fail(XMHW_ERR_INVALID, "edge outside [0, B]");
    if (C == 0) return XMHW_OK;
    if (!hist || !n || !kmin || !kmax || (P > 0 && (!qbin || !qbelow || !qcount)) || (L > 0 && !n_at_least))
        return fail(XMHW_ERR_INVALID, "NULL buffer");
    return status_of(xmhw::launch_distribution_finish(K, B, C, hist, n, kmin, kmax, p_q, P, edge, L, qbin, qbelow, qcount, n_at_least,
                                                      ldo, static_cast<hipStream_t>(stream)),
                     "distribution_finish launch");
}

}  // extern "C"
