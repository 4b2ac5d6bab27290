// kernels_fit.hip -- detrend(): per-cell least-squares fit over the time axis and removal of its leading columns
// (xmhw_amd/detrend.py states the model).
//
// Input: the resident series ts[T][ld] (time-major, cells contiguous), the design matrix basis[T][P] float64 shared
// by all cells (built on the host), an optional weight[T] in {0, 1} (the fit period).  A sample contributes when its
// step has weight 1 and it is not NaN.  beta solves the normal equations G beta = r, G = sum b b', r = sum b y over
// the contributing samples, by Cholesky and two triangular solves -- float64 throughout, no FMA (-ffp-contract=off).
//
// series_gram: one workgroup.  Gfull = sum over the steps with weight 1 of b b' (P(P+1)/2 entries, each summed in
// time order by one thread from rows staged in LDS) and nw = the number of such steps.  The Gram matrix of a cell
// without a missing sample IS Gfull: it is computed once per call, not once per cell.
//
// series_fit<T, P>: one lane per cell (coalesced rows), one wave per workgroup, the whole time axis in one walk,
// so that every sum of a cell runs in time order and depends on the cell's own samples only.  Per sample:
// part[k] += b[k] * y (P multiply-adds; a NaN enters as 0.0, which leaves every sum as it is), part being the sum of
// the eight rows t0 .. t0 + 7 (t0 a multiple of eight: a function of T alone), started at 0.0; each batch joins r by a
// compensated (Kahan) add.  A plain running sum loses eps * |r| at every sample, and with r_const of the order of
// 1e5 K that alone moved the x^3 coefficient of a two-year cubic by 1e-11 max|y|; this way the adds
// that round are between numbers of a batch's size.  Gfull is a compensated sum as well.  Only on a step
// where some lane of the wave misses its sample, the lanes that miss it add the outer product b b' to their own
// A[P(P+1)/2]; at the end G = Gfull - A.  A cell with more missing than contributing samples would lose digits in
// that difference (a cell that is valid on twelve days of forty years: all of them), so for such cells -- a rule on
// the cell's own counts -- a second kernel (series_fit_direct; waves without such a cell leave at once) sums A = sum of b b' over the
// contributing samples directly (compensated adds, one walk over the series per row of A), and G = A.  The basis row of a step is wave-uniform (scalar loads).
//
// series_remove<T, R>: y' = y - sum_{k<R} beta_k basis[t][k], the sum in float64 in column order, one subtraction,
// one rounding to T; NaN stays NaN, a failed cell (beta = NaN) becomes NaN everywhere.  Elementwise: workgroups of
// 256 consecutive cells x a chunk of rows.
#include "device_common.h"
#include "kernels.h"

namespace xmhw {
namespace {

constexpr int kWave = 64;
constexpr int kBatch = 8;                  // rows requested before the first is consumed
constexpr int kGramRows = 256;             // rows of the basis staged in LDS at a time (256 x 10 x 8 B = 20 KB)
constexpr int kGramThreads = 256;
constexpr double kPivotRatio = 1e-6;

__host__ __device__ constexpr int tri(int i, int j) { return i * (i + 1) / 2 + j; }     // j <= i

// gram[0 .. P(P+1)/2): Gfull in tri() order; gram[kFitGramWords - 1]: nw as a double
__global__ __launch_bounds__(kGramThreads) void series_gram(const double* __restrict__ basis, int64_t Tn, int P,
                                                            const uint8_t* __restrict__ weight, double* __restrict__ gram) {
    __shared__ double rows[kGramRows * kFitMaxTerms];
    __shared__ uint8_t wrow[kGramRows];
    const int tid = threadIdx.x;
    const int ne = P * (P + 1) / 2;
    int i = 0, j = 0;
    if (tid < ne) {
        while (tri(i + 1, 0) <= tid) ++i;
        j = tid - tri(i, 0);
    }
    double s = 0.0, comp = 0.0;           // compensated (Kahan) sum: Gfull carries no rounding of its 14,610 adds
    int64_t nw = 0;
    for (int64_t t0 = 0; t0 < Tn; t0 += kGramRows) {
        const int n = static_cast<int>(Tn - t0 < kGramRows ? Tn - t0 : kGramRows);
        for (int k = tid; k < n * P; k += kGramThreads) rows[k] = basis[t0 * P + k];
        for (int k = tid; k < n; k += kGramThreads) wrow[k] = weight ? weight[t0 + k] : uint8_t(1);
        __syncthreads();
        if (tid < ne) {
            for (int t = 0; t < n; ++t)
                if (wrow[t]) {
                    const double term = rows[t * P + i] * rows[t * P + j] - comp;
                    const double next = s + term;
                    comp = (next - s) - term;
                    s = next;
                }
        } else if (tid == kGramThreads - 1) {
            for (int t = 0; t < n; ++t) nw += wrow[t] != 0;
        }
        __syncthreads();
    }
    if (tid < ne) gram[tid] = s;
    if (tid == kGramThreads - 1) gram[kFitGramWords - 1] = static_cast<double>(nw);
}

// the walk over the time axis: r (with its compensation rc), n, bad, and A = the outer products of the MISSING samples
template <typename T, int P>
__device__ __forceinline__ void fit_walk(const T* __restrict__ col, int64_t Tn, int64_t ld, const double* __restrict__ basis,
                                         const uint8_t* __restrict__ weight, double (&r)[P], double (&rc)[P],
                                         double (&A)[P * (P + 1) / 2], int& n, bool& bad) {
    for (int64_t t0 = 0; t0 < Tn; t0 += kBatch) {
        const int nb = static_cast<int>(Tn - t0 < kBatch ? Tn - t0 : kBatch);
        if (weight) {                                          // a batch outside the fit period is not read
            bool any = false;
            for (int u = 0; u < nb; ++u) any |= weight[t0 + u] != 0;
            if (!any) continue;
        }
        T v[kBatch];
#pragma unroll
        for (int u = 0; u < kBatch; ++u) v[u] = u < nb ? col[(t0 + u) * ld] : T(0);
        double part[P];                                        // r of this batch of rows, summed from 0.0
#pragma unroll
        for (int k = 0; k < P; ++k) part[k] = 0.0;
#pragma unroll
        for (int u = 0; u < kBatch; ++u) {
            if (u >= nb) break;
            const int64_t t = t0 + u;
            if (weight && !weight[t]) continue;
            const double* __restrict__ b = basis + t * P;
            const bool valid = v[u] == v[u];
            const double y = valid ? static_cast<double>(v[u]) : 0.0;
            n += valid;
            bad |= valid && isinf(v[u]);
#pragma unroll
            for (int k = 0; k < P; ++k) part[k] += b[k] * y;
            if (__ballot(!valid) != 0) {
#pragma unroll
                for (int i = 0; i < P; ++i) {
                    const double bi = valid ? 0.0 : b[i];
#pragma unroll
                    for (int j = 0; j <= i; ++j) A[tri(i, j)] += bi * b[j];
                }
            }
        }
#pragma unroll
        for (int k = 0; k < P; ++k) {                          // the batch joins the running sum by a compensated add
            const double term = part[k] - rc[k];
            const double next = r[k] + term;
            rc[k] = (next - r[k]) - term;
            r[k] = next;
        }
    }
}

// the second walk, for the lanes with `direct` set: rows I .. P-1 of A = the sum of b b' over the CONTRIBUTING samples,
// one walk over the series per row of A (I + 1 entries with their compensations: few registers; it is the rare
// path), every sample joined by a compensated (Kahan) add.
template <typename T, int P, int I>
__device__ __forceinline__ void direct_rows(const T* __restrict__ col, int64_t Tn, int64_t ld,
                                            const double* __restrict__ basis, const uint8_t* __restrict__ weight,
                                            bool direct, double (&A)[P * (P + 1) / 2]) {
    if constexpr (I < P) {
        double tot[I + 1], comp[I + 1];
#pragma unroll
        for (int j = 0; j <= I; ++j) tot[j] = comp[j] = 0.0;
        for (int64_t t0 = 0; t0 < Tn; t0 += kBatch) {
            const int nb = static_cast<int>(Tn - t0 < kBatch ? Tn - t0 : kBatch);
            if (weight) {
                bool any = false;
                for (int u = 0; u < nb; ++u) any |= weight[t0 + u] != 0;
                if (!any) continue;
            }
            T v[kBatch];
#pragma unroll
            for (int u = 0; u < kBatch; ++u) v[u] = u < nb ? col[(t0 + u) * ld] : T(0);
#pragma unroll
            for (int u = 0; u < kBatch; ++u) {
                if (u >= nb) break;
                const int64_t t = t0 + u;
                if (weight && !weight[t]) continue;
                const double* __restrict__ b = basis + t * P;
                const double bi = (direct && v[u] == v[u]) ? b[I] : 0.0;
#pragma unroll
                for (int j = 0; j <= I; ++j) {
                    const double term = bi * b[j] - comp[j];
                    const double next = tot[j] + term;
                    comp[j] = (next - tot[j]) - term;
                    tot[j] = next;
                }
            }
        }
#pragma unroll
        for (int j = 0; j <= I; ++j) A[tri(I, j)] = direct ? tot[j] : A[tri(I, j)];
        direct_rows<T, P, I + 1>(col, Tn, ld, basis, weight, direct, A);
    }
}

// G (in A) -> its Cholesky factor in place (columns in the order of the basis), then L z = r, L' beta = z in r.
// Returns false when a pivot fails.
template <int P>
__device__ __forceinline__ bool solve_cell(double (&A)[P * (P + 1) / 2], double (&r)[P]) {
    bool ok = true;
#pragma unroll
    for (int j = 0; j < P; ++j) {
        const double gjj = A[tri(j, j)];
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < j; ++k) s += A[tri(j, k)] * A[tri(j, k)];
        const double d = gjj - s;
        ok = ok && (d > kPivotRatio * gjj);                    // NaN and negative pivots fail
        const double l = sqrt(d);
        A[tri(j, j)] = l;
#pragma unroll
        for (int i = j + 1; i < P; ++i) {
            double q = 0.0;
#pragma unroll
            for (int k = 0; k < j; ++k) q += A[tri(i, k)] * A[tri(j, k)];
            A[tri(i, j)] = (A[tri(i, j)] - q) / l;
        }
    }
#pragma unroll
    for (int i = 0; i < P; ++i) {
        double q = 0.0;
#pragma unroll
        for (int k = 0; k < i; ++k) q += A[tri(i, k)] * r[k];
        r[i] = (r[i] - q) / A[tri(i, i)];
    }
#pragma unroll
    for (int i = P - 1; i >= 0; --i) {
        double q = 0.0;
#pragma unroll
        for (int k = P - 1; k > i; --k) q += A[tri(k, i)] * r[k];
        r[i] = (r[i] - q) / A[tri(i, i)];
    }
    return ok;
}

// flags[C]: 1 for a cell that sums its own Gram matrix; series_fit leaves r in its coef column for series_fit_direct
template <typename T, int P>
__global__ __launch_bounds__(kWave) void series_fit(const T* __restrict__ ts, int64_t Tn, int64_t C, int64_t ld,
                                                    const double* __restrict__ basis, const uint8_t* __restrict__ weight,
                                                    int32_t need, const double* __restrict__ gram, uint8_t* __restrict__ flags,
                                                    double* __restrict__ coef, int64_t ldc, int32_t* __restrict__ nvalid) {
    constexpr int NE = P * (P + 1) / 2;
    const int64_t cell = static_cast<int64_t>(blockIdx.x) * kWave + threadIdx.x;
    if (cell >= C) return;
    const T* __restrict__ col = ts + cell;
    double r[P], rc[P], A[NE];
#pragma unroll
    for (int k = 0; k < P; ++k) r[k] = rc[k] = 0.0;
#pragma unroll
    for (int e = 0; e < NE; ++e) A[e] = 0.0;
    int n = 0;
    bool bad = false;
    fit_walk<T, P>(col, Tn, ld, basis, weight, r, rc, A, n, bad);
    const int64_t nw = static_cast<int64_t>(gram[kFitGramWords - 1]);
    const int64_t nmiss = nw - n;
    const bool enough = n >= need && !bad;
    const bool direct = enough && nmiss > n;
    flags[cell] = direct ? 1 : 0;
    if (nvalid) nvalid[cell] = n;
    if (direct) {
#pragma unroll
        for (int k = 0; k < P; ++k) coef[k * ldc + cell] = r[k];
        return;
    }
#pragma unroll
    for (int e = 0; e < NE; ++e) A[e] = gram[e] - A[e];
    const bool ok = solve_cell<P>(A, r) && enough;
    const double nan = make_nan();
#pragma unroll
    for (int k = 0; k < P; ++k) coef[k * ldc + cell] = ok ? r[k] : nan;
}

template <typename T, int P>
__global__ __launch_bounds__(kWave) void series_fit_direct(const T* __restrict__ ts, int64_t Tn, int64_t C, int64_t ld,
                                                           const double* __restrict__ basis,
                                                           const uint8_t* __restrict__ weight,
                                                           const uint8_t* __restrict__ flags, double* __restrict__ coef,
                                                           int64_t ldc) {
    constexpr int NE = P * (P + 1) / 2;
    const int64_t cell = static_cast<int64_t>(blockIdx.x) * kWave + threadIdx.x;
    if (cell >= C) return;
    const bool direct = flags[cell] != 0;
    if (__ballot(direct) == 0) return;
    double r[P], A[NE];
#pragma unroll
    for (int e = 0; e < NE; ++e) A[e] = 1.0;                   // (lanes without the flag: never written back)
    direct_rows<T, P, 0>(ts + cell, Tn, ld, basis, weight, direct, A);
    if (!direct) return;
#pragma unroll
    for (int k = 0; k < P; ++k) r[k] = coef[k * ldc + cell];
    const bool ok = solve_cell<P>(A, r);
    const double nan = make_nan();
#pragma unroll
    for (int k = 0; k < P; ++k) coef[k * ldc + cell] = ok ? r[k] : nan;
}

constexpr int kRemoveThreads = 256;
constexpr int kRemoveRows = 64;            // rows of one workgroup

template <typename T, int R>
__global__ __launch_bounds__(kRemoveThreads) void series_remove(T* __restrict__ ts, int64_t Tn, int64_t C, int64_t ld,
                                                                const double* __restrict__ basis, int P,
                                                                const double* __restrict__ coef, int64_t ldc) {
    const int64_t cell = static_cast<int64_t>(blockIdx.x) * kRemoveThreads + threadIdx.x;
    if (cell >= C) return;
    double beta[R];
#pragma unroll
    for (int k = 0; k < R; ++k) beta[k] = coef[k * ldc + cell];
    const int64_t tbeg = static_cast<int64_t>(blockIdx.y) * kRemoveRows;
    const int64_t tend = tbeg + kRemoveRows < Tn ? tbeg + kRemoveRows : Tn;
    T* __restrict__ col = ts + cell;
    for (int64_t t0 = tbeg; t0 < tend; t0 += kBatch) {
        const int nb = static_cast<int>(tend - t0 < kBatch ? tend - t0 : kBatch);
        T v[kBatch];
#pragma unroll
        for (int u = 0; u < kBatch; ++u) v[u] = u < nb ? col[(t0 + u) * ld] : T(0);
#pragma unroll
        for (int u = 0; u < kBatch; ++u) {
            if (u >= nb) break;
            const double* __restrict__ b = basis + (t0 + u) * P;
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < R; ++k) s += beta[k] * b[k];
            col[(t0 + u) * ld] = static_cast<T>(static_cast<double>(v[u]) - s);
        }
    }
}

template <typename T, int P>
void launch_fit_p(unsigned blocks, hipStream_t stream, const T* ts, int64_t Tn, int64_t C, int64_t ld, const double* basis,
                  const uint8_t* weight, int32_t need, const double* gram, uint8_t* flags, double* coef, int64_t ldc,
                  int32_t* nvalid) {
    hipLaunchKernelGGL((series_fit<T, P>), dim3(blocks), dim3(kWave), 0, stream, ts, Tn, C, ld, basis, weight, need, gram,
                       flags, coef, ldc, nvalid);
    hipLaunchKernelGGL((series_fit_direct<T, P>), dim3(blocks), dim3(kWave), 0, stream, ts, Tn, C, ld, basis, weight, flags,
                       coef, ldc);
}
template <typename T, int R>
void launch_remove_r(dim3 grid, hipStream_t stream, T* ts, int64_t Tn, int64_t C, int64_t ld, const double* basis, int P,
                     const double* coef, int64_t ldc) {
    hipLaunchKernelGGL((series_remove<T, R>), grid, dim3(kRemoveThreads), 0, stream, ts, Tn, C, ld, basis, P, coef, ldc);
}

}  // namespace

template <typename T>
hipError_t launch_series_fit(const T* ts, int64_t Tn, int64_t C, int64_t ld, const double* basis, int32_t P,
                             const uint8_t* weight, int32_t need, double* gram, uint8_t* flags, double* coef, int64_t ldc,
                             int32_t* nvalid, hipStream_t stream) {
    if (C <= 0 || Tn <= 0) return hipSuccess;
    if (P < 1 || P > kFitMaxTerms) return hipErrorInvalidValue;
    const int64_t blocks = (C + kWave - 1) / kWave;
    if (blocks > 0x7FFFFFFFll) return hipErrorInvalidValue;
    hipLaunchKernelGGL(series_gram, dim3(1), dim3(kGramThreads), 0, stream, basis, Tn, P, weight, gram);
    const unsigned g = static_cast<unsigned>(blocks);
#define XMHW_FIT_CASE(N) \
    case N: launch_fit_p<T, N>(g, stream, ts, Tn, C, ld, basis, weight, need, gram, flags, coef, ldc, nvalid); break;
    switch (P) {
        XMHW_FIT_CASE(1) XMHW_FIT_CASE(2) XMHW_FIT_CASE(3) XMHW_FIT_CASE(4) XMHW_FIT_CASE(5)
        XMHW_FIT_CASE(6) XMHW_FIT_CASE(7) XMHW_FIT_CASE(8) XMHW_FIT_CASE(9) XMHW_FIT_CASE(10)
    }
#undef XMHW_FIT_CASE
    return hipGetLastError();
}

template <typename T>
hipError_t launch_series_remove(T* ts, int64_t Tn, int64_t C, int64_t ld, const double* basis, int32_t P, int32_t R,
                                const double* coef, int64_t ldc, hipStream_t stream) {
    if (C <= 0 || Tn <= 0) return hipSuccess;
    if (P < 1 || P > kFitMaxTerms || R < 1 || R > P) return hipErrorInvalidValue;
    const int64_t bx = (C + kRemoveThreads - 1) / kRemoveThreads, by = (Tn + kRemoveRows - 1) / kRemoveRows;
    if (bx > 0x7FFFFFFFll || by > 65535) return hipErrorInvalidValue;
    const dim3 grid(static_cast<unsigned>(bx), static_cast<unsigned>(by));
#define XMHW_REMOVE_CASE(N) case N: launch_remove_r<T, N>(grid, stream, ts, Tn, C, ld, basis, P, coef, ldc); break;
    switch (R) {
        XMHW_REMOVE_CASE(1) XMHW_REMOVE_CASE(2) XMHW_REMOVE_CASE(3) XMHW_REMOVE_CASE(4) XMHW_REMOVE_CASE(5)
        XMHW_REMOVE_CASE(6) XMHW_REMOVE_CASE(7) XMHW_REMOVE_CASE(8) XMHW_REMOVE_CASE(9) XMHW_REMOVE_CASE(10)
    }
#undef XMHW_REMOVE_CASE
    return hipGetLastError();
}

template hipError_t launch_series_fit<float>(const float*, int64_t, int64_t, int64_t, const double*, int32_t, const uint8_t*,
                                             int32_t, double*, uint8_t*, double*, int64_t, int32_t*, hipStream_t);
template hipError_t launch_series_fit<double>(const double*, int64_t, int64_t, int64_t, const double*, int32_t,
                                              const uint8_t*, int32_t, double*, uint8_t*, double*, int64_t, int32_t*, hipStream_t);
template hipError_t launch_series_remove<float>(float*, int64_t, int64_t, int64_t, const double*, int32_t, int32_t,
                                                const double*, int64_t, hipStream_t);
template hipError_t launch_series_remove<double>(double*, int64_t, int64_t, int64_t, const double*, int32_t, int32_t,
                                                 const double*, int64_t, hipStream_t);

}  // namespace xmhw
