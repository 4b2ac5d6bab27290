// kernels_regress.hip -- index_regression(): the integer sums behind lagged regression and correlation maps of the
// anomalies of every cell on a few climate indices.
//
// a = float64(sample) - base[row_of_t[t]][c]; the step is VALID iff a is not NaN and |a| < 2^7; q(t) = rint(a * 2^16) on
// valid steps.  zq[t][0..J) is the predictor row of the step: int32, fixed point already, |zq| < 2^23, uniform over the
// cells.  For every class k (class_of_t[t] in [-1, K), -1 = the step counts nowhere and is not read) and cell c:
//   n[k][c], sa[k][c], saa[k][c]     over the valid steps of class k: their count, the sum of q, the sum of q^2
//   n1[k][c], saa1[k][c]             over the valid steps t >= 1 of class k whose step t - 1 is valid and of class k as
//                                    well: their count and the sum of q(t) q(t - 1)
//   saz[k][j][c]                     over the valid steps of class k: the sum of q(t) zq[t][j]
//   mz[k][j][c], mzz[k][j][c]        over the steps of class k that are NOT valid: the sums of zq[t][j] and zq[t][j]^2
// A non-NaN a with |a| >= 2^7 (or infinite) is one of the steps that are not valid and is counted in *n_range.
// |q| <= 2^23, |zq| < 2^23 and T < 2^17: every sum stays inside int64.  The atomics add the two's-complement bits as
// unsigned 64-bit integers.
//
//   index_regress_accumulate<T, G>
//                     the frame of a class reduction (kernels.h): lane = cell, a workgroup is 256 cells x a block of
//                     steps, the samples (and base rows) of four steps are requested together before the first is used,
//                     the addends of the current class stay in registers and are flushed by integer atomics without a
//                     return value when the wave-uniform class changes and at the end of the block.  No barrier, no
//                     scratch.  From G = 8 on the steps of a batch run one at a time (below) and the compiler parks the
//                     batch in the lane's own column of a 12 KB LDS stage, as heat_stress_accumulate does by hand; the
//                     scalar registers it reports as spilled (to vector lanes, not to memory) are flush addresses, read
//                     back in the flush alone.
//   the predictors    G = 4, 8, 16 or 32 accumulators per lane, indexed at compile time; J is padded to G with zero
//                     columns in the device table, which is step-major: the row of a step is G consecutive int32 at an
//                     address that is uniform over the wave, so the compiler fetches it through the scalar cache
//                     (s_load_dwordx4 / x8 / x16) and the multiply-add takes the predictor as a scalar operand.  The hot
//                     instruction is one v_mad_i64_i32 per predictor, step and lane.  A lane whose step is not valid
//                     multiplies q = 0: the hot path has no per-lane branch.
//   invalid steps     the rare path: 2 J atomics straight to global memory, in a loop that is not unrolled.
//   the lag-1 pair    kprev = the class of the previous step if that step was valid, -1 otherwise (per lane), qprev its
//                     q.  A block that starts at t0 > 0 derives both from step t0 - 1, which it reads once and reduces
//                     nowhere: blocks are independent.
#include "../../include/xmhw_amd.h"
#include "entry_common.h"
#include "stage_reduce.h"

namespace xmhw {

// What the stage computes: the sums behind lagged regression maps of anomalies on indices.  With
// a = sample - base[row_of_t[t]][c], the step VALID iff a is not NaN and |a| < 2^7, q = rint(a * 2^kIndexRegressBits) on
// valid steps, and the predictor row zq[t][0..J) of the step, launch_index_regress_accumulate ADDS per class k of the step
// and cell c: over the valid steps n[k][c] += 1, sa += q, saa += q^2, saz[k][j][c] += q * zq[t][j]; over the valid steps
// whose step t - 1 is valid and of class k as well n1 += 1, saa1 += q(t) q(t - 1); over the steps of class k that are NOT
// valid mz[k][j][c] += zq[t][j], mzz[k][j][c] += zq[t][j]^2; and counts the non-NaN a with |a| >= 2^7 of the steps with a
// class in *n_range.  Cells are the fastest axis, leading dimension ldo >= C.  row_of_t and class_of_t are DEVICE arrays
// here, and so is zq: int32 [T][G], step-major, G = index_regress_group(J) columns of which those past J are zero.
// block_steps: the steps a workgroup takes per block, 0 = automatic; same results for every value.
constexpr int kIndexRegressMaxPredictors = 32;
constexpr int kIndexRegressMaxClasses = 64;
constexpr int kIndexRegressMaxSteps = 1 << 17;       // T below it: 2^17 * 2^23 * 2^23 = 2^63
constexpr int kIndexRegressBits = 16;
constexpr int kIndexRegressPredictorBits = 23;       // |zq| < 2^23
// the predictor columns of the kernel instantiation that takes J predictors: 4, 8, 16 or 32
inline int index_regress_group(int32_t J) { return J <= 4 ? 4 : J <= 8 ? 8 : J <= 16 ? 16 : 32; }

static_assert(kIndexRegressBits == kFixedBits, "one scale for every stage");

namespace {

constexpr int kIrThreads = 256;
constexpr int kIrBatch = 4;                          // steps whose samples are requested together
constexpr int kIrRolled = 8;                         // predictors from which the steps of a batch are not unrolled
using u64 = unsigned long long;

template <typename T>
struct IrIn {
    const T* ts;
    int64_t ld;
    const double* base;                              // [D][ldb]
    int64_t ldb;
    const int32_t* row_of_t;
    int32_t one_row;                                 // D == 1: the base is a constant per cell, read once
};

struct IrOut {
    int32_t *n, *n1;                                 // [K][ldo]
    u64 *sa, *saa, *saa1;                            // [K][ldo]
    u64 *saz, *mz, *mzz;                             // [K][J][ldo]
    int64_t ldo;
    int32_t J;
    u64* n_range;
};

// the addends of one lane for the current class
template <int G>
struct IrAcc {
    int32_t n, n1;
    int64_t sa, saa, saa1;
    int64_t saz[G];
    __device__ __forceinline__ void clear() {
        n = n1 = 0;
        sa = saa = saa1 = 0;
#pragma unroll
        for (int j = 0; j < G; ++j) saz[j] = 0;
    }
};

template <int G>
__device__ __forceinline__ void ir_flush(const IrOut& o, int32_t k, int64_t c, IrAcc<G>& v) {
    if (v.n) {                                       // no valid step, no addend
        const int64_t p = static_cast<int64_t>(k) * o.ldo + c;
        atomicAdd(o.n + p, v.n);
        if (v.sa) atomicAdd(o.sa + p, static_cast<u64>(v.sa));
        if (v.saa) atomicAdd(o.saa + p, static_cast<u64>(v.saa));
        if (v.n1) atomicAdd(o.n1 + p, v.n1);
        if (v.saa1) atomicAdd(o.saa1 + p, static_cast<u64>(v.saa1));
        u64* d = o.saz + static_cast<int64_t>(k) * o.J * o.ldo + c;
#pragma unroll
        for (int j = 0; j < G; ++j)
            if (j < o.J && v.saz[j]) atomicAdd(d + j * o.ldo, static_cast<u64>(v.saz[j]));
    }
    v.clear();
}

// x[u] of a batch kept in registers, for a u that is not a compile-time constant
template <typename V>
__device__ __forceinline__ V ir_pick(const V (&x)[kIrBatch], int u) {
    V r = x[0];
#pragma unroll
    for (int i = 1; i < kIrBatch; ++i) r = u == i ? x[i] : r;
    return r;
}

// the deficits of a step of class k that is not valid
__device__ __forceinline__ void ir_deficit(const IrOut& o, int32_t k, int64_t c, const int32_t* __restrict__ z) {
    const int64_t p = static_cast<int64_t>(k) * o.J * o.ldo + c;
#pragma unroll 1
    for (int32_t j = 0; j < o.J; ++j) {
        const int64_t zj = z[j];
        if (zj == 0) continue;
        atomicAdd(o.mz + p + j * o.ldo, static_cast<u64>(zj));
        atomicAdd(o.mzz + p + j * o.ldo, static_cast<u64>(zj * zj));
    }
}

template <typename T, int G>
__global__ __launch_bounds__(kIrThreads) void index_regress_accumulate(IrIn<T> in, int64_t Tn, int64_t C,
                                                                       const int32_t* __restrict__ class_of_t, int32_t K,
                                                                       const int32_t* __restrict__ zq, int64_t tb,
                                                                       IrOut out) {
    constexpr int kIrUnroll = G >= kIrRolled ? 1 : kIrBatch;
    const int64_t c = static_cast<int64_t>(blockIdx.x) * kIrThreads + threadIdx.x;
    if (c >= C) return;
    const double b0 = in.one_row ? in.base[c] : 0.0;
    // T < 2^17: steps and blocks are 32-bit here, addresses are not
    const int32_t Ts = static_cast<int32_t>(Tn), bs = static_cast<int32_t>(tb < Tn ? tb : Tn);
    const int32_t nblk = (Ts - 1) / bs + 1;
    IrAcc<G> v;
    v.clear();
    u64 n_range = 0;
    const auto flush_class = [&](int32_t k) { ir_flush<G>(out, k, c, v); };
    const auto anomaly = [&](T sample, int32_t t) {
        return static_cast<double>(sample) -
               (in.one_row ? b0 : in.base[static_cast<int64_t>(in.row_of_t[t]) * in.ldb + c]);
    };
    for (int32_t blk = blockIdx.y; blk < nblk; blk += gridDim.y) {
        const auto [t0, t1] = block_range<int32_t>(blk, bs, Ts);
        // the step before the block, for the lag-1 pair of step t0 alone
        int32_t kprev = -1, qprev = 0;
        if (t0 > 0) {
            const int32_t k = class_of_t[t0 - 1];
            if (k >= 0 && k < K) {
                const double a = anomaly(in.ts[static_cast<int64_t>(t0 - 1) * in.ld + c], t0 - 1);
                if (fixed_state(a) > 0) {
                    kprev = k;
                    qprev = static_cast<int32_t>(fixed_value(a));
                }
            }
        }
        ClassRun run;
        for (int32_t tc = t0; tc < t1; tc += kIrBatch) {
            int32_t kk[kIrBatch];
            double a[kIrBatch];
#pragma unroll
            for (int u = 0; u < kIrBatch; ++u) {
                const int32_t t = tc + u;
                kk[u] = t < t1 ? class_of_t[t] : -1;
                if (kk[u] >= K) kk[u] = -1;          // (labels are checked on the host)
                // a step of class -1 reads nothing
                a[u] = kk[u] >= 0 ? anomaly(in.ts[static_cast<int64_t>(t) * in.ld + c], t) : 0.0;
            }
            // One step at a time from G = kIrRolled predictors on: unrolled, the predictor rows of all four steps are
            // fetched ahead and the body runs out of scalar registers (139 of them spilled to vector lanes at G = 32).
            // The step's anomaly is then picked from the batch by selects, which fold away where the loop is unrolled.
#pragma unroll kIrUnroll
            for (int u = 0; u < kIrBatch; ++u) {
                const int32_t k = ir_pick(kk, u);
                if (k < 0) {
                    kprev = -1;
                    continue;
                }
                run.enter(k, flush_class);
                const int32_t* __restrict__ z = zq + static_cast<int64_t>(tc + u) * G;
                const double au = ir_pick(a, u);
                const int state = fixed_state(au);
                const int32_t q = state > 0 ? static_cast<int32_t>(fixed_value(au)) : 0;
                const bool pair = state > 0 && kprev == k;
#pragma unroll
                for (int j = 0; j < G; ++j) v.saz[j] += static_cast<int64_t>(q) * z[j];
                v.n += state > 0;
                v.sa += q;
                v.saa += static_cast<int64_t>(q) * q;
                v.n1 += pair;
                v.saa1 += static_cast<int64_t>(q) * (pair ? qprev : 0);
                if (state <= 0) {
                    if (state < 0) ++n_range;
                    ir_deficit(out, k, c, z);
                }
                kprev = state > 0 ? k : -1;
                qprev = q;
            }
        }
        run.leave(flush_class);
    }
    if (n_range) atomicAdd(out.n_range, n_range);
}

template <typename T, int G>
void ir_launch(const IrIn<T>& in, int64_t Tn, int64_t C, const int32_t* class_of_t, int32_t K, const int32_t* zq, int64_t tb,
               const IrOut& out, hipStream_t stream) {
    hipLaunchKernelGGL((index_regress_accumulate<T, G>), stage_grid(C, kIrThreads, Tn, tb), dim3(kIrThreads), 0, stream, in, Tn,
                       C, class_of_t, K, zq, tb, out);
}

hipError_t launch_index_regress_init(int32_t K, int32_t J, int64_t C, int32_t* n, int64_t* sa, int64_t* saa, int32_t* n1,
                                     int64_t* saa1, int64_t* saz, int64_t* mz, int64_t* mzz, int64_t ldo, int64_t* n_range,
                                     hipStream_t stream) {
    hipError_t e = hipMemsetAsync(n_range, 0, sizeof(int64_t), stream);
    for (int32_t* p : {n, n1})
        if (e == hipSuccess) e = zero_rows(p, sizeof(int32_t), K, C, ldo, stream);
    for (int64_t* p : {sa, saa, saa1})
        if (e == hipSuccess) e = zero_rows(p, sizeof(int64_t), K, C, ldo, stream);
    for (int64_t* p : {saz, mz, mzz})
        if (e == hipSuccess) e = zero_rows(p, sizeof(int64_t), static_cast<int64_t>(K) * J, C, ldo, stream);
    return e;
}

template <typename T>
hipError_t launch_index_regress_accumulate(const T* ts, int64_t Tn, int64_t C, int64_t ld, const double* base, int64_t ldb,
                                           int64_t D, const int32_t* row_of_t, const int32_t* class_of_t, int32_t K,
                                           const int32_t* zq, int32_t J, int64_t block_steps, int32_t* n, int64_t* sa,
                                           int64_t* saa, int32_t* n1, int64_t* saa1, int64_t* saz, int64_t* mz, int64_t* mzz,
                                           int64_t ldo, int64_t* n_range, hipStream_t stream) {
    if (C <= 0 || Tn <= 0 || K <= 0 || J <= 0) return hipSuccess;
    if (Tn >= kIndexRegressMaxSteps || J > kIndexRegressMaxPredictors) return hipErrorInvalidValue;
    const int64_t tb = block_steps > 0 ? block_steps : index_regress_auto_block(Tn, C);
    const IrIn<T> in{ts, ld, base, ldb, row_of_t, D == 1};
    const auto u = [](int64_t* p) { return reinterpret_cast<u64*>(p); };
    const IrOut out{n, n1, u(sa), u(saa), u(saa1), u(saz), u(mz), u(mzz), ldo, J, u(n_range)};
    switch (index_regress_group(J)) {
        case 4: ir_launch<T, 4>(in, Tn, C, class_of_t, K, zq, tb, out, stream); break;
        case 8: ir_launch<T, 8>(in, Tn, C, class_of_t, K, zq, tb, out, stream); break;
        case 16: ir_launch<T, 16>(in, Tn, C, class_of_t, K, zq, tb, out, stream); break;
        default: ir_launch<T, 32>(in, Tn, C, class_of_t, K, zq, tb, out, stream); break;
    }
    return hipGetLastError();
}

}  // namespace

}  // namespace xmhw

// ---- the C entries of index_regression() (include/xmhw_amd.h) ---------------------------------------------------------
namespace {

using namespace xmhw::entry;

static std::atomic<int> g_index_regress_block{0};   // steps a workgroup takes per block, 0 = automatic (xmhw_set_index_regress_block)

static int index_regress_check_shape(int32_t K, int32_t J, int64_t Tn, int64_t C) {
    if (K < 1 || K > xmhw::kIndexRegressMaxClasses)
        return fail(XMHW_ERR_UNSUPPORTED,
                    "index_regress: K must be in [1, " + std::to_string(xmhw::kIndexRegressMaxClasses) + "]");
    if (J < 1 || J > xmhw::kIndexRegressMaxPredictors)
        return fail(XMHW_ERR_UNSUPPORTED,
                    "index_regress: J must be in [1, " + std::to_string(xmhw::kIndexRegressMaxPredictors) + "]");
    if (Tn >= xmhw::kIndexRegressMaxSteps) return fail(XMHW_ERR_UNSUPPORTED, "index_regress: 2^17 steps and more");
    if (C > 0x7FFFFFFFll) return fail(XMHW_ERR_UNSUPPORTED, "index_regress: 2^31 cells and more");
    return XMHW_OK;
}

template <typename T>
int index_regress_accumulate(const T* ts, int64_t Tn, int64_t C, int64_t ld, const double* base, int64_t ldb, int64_t D,
                             const int32_t* row_of_t, const int32_t* class_of_t, int32_t K, const int32_t* zq, int32_t J,
                             int32_t* n, int64_t* sa, int64_t* saa, int32_t* n1, int64_t* saa1, int64_t* saz, int64_t* mz,
                             int64_t* mzz, int64_t ldo, int64_t* n_range, void* stream) {
    if (index_regress_check_shape(K, J, Tn, C) != XMHW_OK) return XMHW_ERR_UNSUPPORTED;
    if (Tn <= 0 || C < 0 || ld < C || ldb < C || ldo < C || D < 1) return fail(XMHW_ERR_INVALID, "bad T/C/ld/ldb/ldo/D");
    if (!class_of_t || !row_of_t || !zq) return fail(XMHW_ERR_INVALID, "NULL host table");
    if (int rc = check_labels(class_of_t, Tn, -1, K, kClassesOutside)) return rc;
    if (int rc = check_labels(row_of_t, Tn, 0, D, kRowsOutside)) return rc;
    constexpr int32_t zlim = 1 << xmhw::kIndexRegressPredictorBits;
    if (int rc = check_labels(zq, Tn * J, -zlim + 1, zlim, "zq outside (-2^23, 2^23)")) return rc;
    if (C == 0) return XMHW_OK;
    if (!ts || !base || !n || !sa || !saa || !n1 || !saa1 || !saz || !mz || !mzz || !n_range)
        return fail(XMHW_ERR_INVALID, "NULL buffer");
    RowsRef rows;
    if (int rc = upload_table(row_of_t, Tn, "row table upload", &rows)) return rc;
    RowsRef classes;                                   // the same content-keyed cache: one more int32[T] table
    if (int rc = upload_table(class_of_t, Tn, "class table upload", &classes)) return rc;
    // ... and the predictors, step-major, J padded with zero columns to the kernel's group: int32[T][G]
    const int G = xmhw::index_regress_group(J);
    std::vector<int32_t> padded(static_cast<size_t>(Tn) * G, 0);
    for (int64_t t = 0; t < Tn; ++t) std::copy(zq + t * J, zq + (t + 1) * J, padded.begin() + t * G);
    RowsRef predictors;
    if (int rc = upload_table(padded.data(), Tn * G, "predictor table upload", &predictors)) return rc;
    return status_of(xmhw::launch_index_regress_accumulate<T>(ts, Tn, C, ld, base, ldb, D, rows->d_rows, classes->d_rows, K,
                                                              predictors->d_rows, J, g_index_regress_block.load(), n, sa, saa,
                                                              n1, saa1, saz, mz, mzz, ldo, n_range,
                                                              static_cast<hipStream_t>(stream)),
                     "index_regress_accumulate launch");
}

}  // namespace

extern "C" {

int xmhw_set_index_regress_block(int32_t steps) { return set_knob(g_index_regress_block, steps, "steps must be >= 0"); }
int xmhw_index_regress_init(int32_t K, int32_t J, int64_t C, int32_t* n, int64_t* sa, int64_t* saa, int32_t* n1, int64_t* saa1,
                            int64_t* saz, int64_t* mz, int64_t* mzz, int64_t ldo, int64_t* n_range, void* stream) {
    if (index_regress_check_shape(K, J, 1, C) != XMHW_OK) return XMHW_ERR_UNSUPPORTED;
    if (C < 0 || ldo < C) return fail(XMHW_ERR_INVALID, "bad C/ldo");
    if (!n_range || (C > 0 && (!n || !sa || !saa || !n1 || !saa1 || !saz || !mz || !mzz)))
        return fail(XMHW_ERR_INVALID, "NULL output buffer");
    return status_of(xmhw::launch_index_regress_init(K, J, C, n, sa, saa, n1, saa1, saz, mz, mzz, ldo, n_range,
                                                     static_cast<hipStream_t>(stream)),
                     "index_regress_init");
}
int xmhw_index_regress_accumulate_f32(const float* ts, int64_t T, int64_t C, int64_t ld, const double* base, int64_t ldb,
                                      int64_t D, const int32_t* row_of_t, const int32_t* class_of_t, int32_t K,
                                      const int32_t* zq, int32_t J, int32_t* n, int64_t* sa, int64_t* saa, int32_t* n1,
                                      int64_t* saa1, int64_t* saz, int64_t* mz, int64_t* mzz, int64_t ldo, int64_t* n_range,
                                      void* stream) {
    return index_regress_accumulate<float>(ts, T, C, ld, base, ldb, D, row_of_t, class_of_t, K, zq, J, n, sa, saa, n1, saa1,
                                           saz, mz, mzz, ldo, n_range, stream);
}
int xmhw_index_regress_accumulate_f64(const double* ts, int64_t T, int64_t C, int64_t ld, const double* base, int64_t ldb,
                                      int64_t D, const int32_t* row_of_t, const int32_t* class_of_t, int32_t K,
                                      const int32_t* zq, int32_t J, int32_t* n, int64_t* sa, int64_t* saa, int32_t* n1,
                                      int64_t* saa1, int64_t* saz, int64_t* mz, int64_t* mzz, int64_t ldo, int64_t* n_range,
                                      void* stream) {
    return index_regress_accumulate<double>(ts, T, C, ld, base, ldb, D, row_of_t, class_of_t, K, zq, J, n, sa, saa, n1, saa1,
                                            saz, mz, mzz, ldo, n_range, stream);
}

}  // extern "C"
