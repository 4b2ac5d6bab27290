// kernels_trend.hip -- mean_trend() (Oliver's marineHeatWaves.meanTrend(); xmhw_amd/trend.py states the semantics).
//
// Input: the planes of block_average(), y[stat][block][cell] float64 (cells contiguous, leading dimension ld), the
// abscissa x[block] (years centred on the whole period, strictly increasing) and, for OLS, tcrit[dof].  A NaN block
// is left out of its series; m = the number of valid blocks of one (cell, statistic) item.  Output planes
// out[what][stat][cell] (leading dimension ldo).  A valid +-Inf, or m == 0: every output of the item is NaN.
//
// trend_ols: one thread per item, lane = cell (coalesced rows).  A workgroup of 64 cells stages its nb x 64 values in
// LDS once (each lane its own column: no bank conflict, no barrier needed beyond the wave's own order) and walks them
// three times: sums, centred products, residuals -- the order of operations of trend.py, no FMA.  Above
// kOlsStageBlocks blocks the three walks read global memory instead.
//
// trend_theil_sen<CAP>: one wave per tile of 16 cells of one statistic.  The tile's nb rows are loaded as 128-byte
// row segments into LDS; then, cell by cell, the wave
//   1. compacts the valid (x, y) into LDS in block order (ballot prefix), m of them; m == 0 ends the item at once;
//   2. ranks every y among the others (m^2 / 64 broadcast reads per lane): the count of equal values c_b gives the tie
//      term, the position in the total order the two middle y;
//   3. walks the N = m(m-1)/2 pairs i < j, lane-strided: one float64 division per pair, the slope's order-preserving
//      64-bit key stored in LDS, sign(y_j - y_i) summed in an integer;
//   4. selects the keys of rank (N-1)/2 and N/2 by a radix select over the stored keys: eight bits per pass from
//      the top, a 256-bin histogram in LDS (integer adds; lanes that share the first active lane's digit are counted
//      by one add), a wave scan of the bins; the passes stop as soon as one candidate is left.
// Everything is integer or a single IEEE operation, in an order that does not depend on scheduling: the same input
// gives the same bytes.  CAP bounds nb for the static LDS arrays (the slopes of CAP blocks: CAP(CAP-1)/2 keys).
#include "device_common.h"
#include "kernels.h"

namespace xmhw {
namespace {

constexpr int kWave = 64;
constexpr int kOlsStageBlocks = 96;        // nb x 64 cells x 8 B = 48 KB of LDS at most

struct GlobalCol {
    const double* p;
    int64_t stride;
    __device__ __forceinline__ double at(int b) const { return p[static_cast<int64_t>(b) * stride]; }
};
struct LdsCol {
    const double* p;
    __device__ __forceinline__ double at(int b) const { return p[b * kWave]; }
};

template <typename Col>
__device__ __forceinline__ void ols_item(const Col& col, const double* __restrict__ x, const double* __restrict__ tcrit,
                                         int nb, double& mean, double& trend, double& dtrend) {
    const double nan = make_nan();
    mean = trend = dtrend = nan;
    int m = 0;
    bool bad = false;
    double sx = 0.0, sy = 0.0;
    for (int b = 0; b < nb; ++b) {
        const double v = col.at(b);
        if (v == v) {
            ++m;
            sx += x[b];
            sy += v;
            bad |= isinf(v);
        }
    }
    if (m == 0 || bad) return;
    const double md = static_cast<double>(m);
    const double xb = sx / md, yb = sy / md;
    if (m == 1) {
        mean = yb;
        return;
    }
    double sxx = 0.0, sxy = 0.0;
    for (int b = 0; b < nb; ++b) {
        const double v = col.at(b);
        if (v == v) {
            const double dx = x[b] - xb;
            sxx += dx * dx;
            sxy += dx * (v - yb);
        }
    }
    trend = sxy / sxx;
    mean = yb - trend * xb;
    if (m == 2) return;
    double ssr = 0.0;
    for (int b = 0; b < nb; ++b) {
        const double v = col.at(b);
        if (v == v) {
            const double r = v - (mean + trend * x[b]);
            ssr += r * r;
        }
    }
    const double s = sqrt(ssr / (md - 2.0));
    dtrend = tcrit[m - 2] * s / sqrt(sxx);
}

template <bool STAGED>
__global__ __launch_bounds__(kWave) void trend_ols(const double* __restrict__ y, int nstat, int nb, int64_t C, int64_t ld,
                                                   const double* __restrict__ x, const double* __restrict__ tcrit,
                                                   double* __restrict__ out, int64_t ldo) {
    extern __shared__ double stage[];      // [nb][64] when STAGED
    const int lane = threadIdx.x;
    const int64_t tiles = (C + kWave - 1) / kWave;
    const int64_t stat = blockIdx.x / tiles;
    const int64_t cell = (blockIdx.x % tiles) * kWave + lane;
    if (cell >= C) return;
    const double* src = y + stat * nb * ld + cell;
    double mean, trend, dtrend;
    if (STAGED) {
        for (int b = 0; b < nb; ++b) stage[b * kWave + lane] = src[static_cast<int64_t>(b) * ld];
        ols_item(LdsCol{stage + lane}, x, tcrit, nb, mean, trend, dtrend);
    } else {
        ols_item(GlobalCol{src, ld}, x, tcrit, nb, mean, trend, dtrend);
    }
    const int64_t plane = static_cast<int64_t>(nstat) * ldo;
    double* dst = out + stat * ldo + cell;
    dst[0] = mean;
    dst[plane] = trend;
    dst[2 * plane] = dtrend;
}

// ---- Theil-Sen / Mann-Kendall ---------------------------------------------------------------------------------------
constexpr int kTile = 16;                  // cells of one workgroup: rows of 128 bytes
constexpr int kTileLd = kTile + 1;         // row stride of the tile in LDS (odd: a column walk spreads over the banks)

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
    return v;
}
__device__ __forceinline__ uint64_t wave_min(uint64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint64_t w = __shfl_xor(v, o, kWave);
        v = w < v ? w : v;
    }
    return v;
}
__device__ __forceinline__ uint64_t lanes_below(int lane) { return (1ull << lane) - 1ull; }

// the key of rank k (0-based) among keys[0..n), and in *next the key of rank k + 1 (n > k + 1 not required: *next is
// only meaningful if it is).  hist: 256 words of LDS.  Every lane returns the same values.
__device__ __forceinline__ uint64_t radix_select(const uint64_t* __restrict__ keys, int n, int k, uint32_t* __restrict__ hist,
                                                 int lane, uint64_t* next) {
    uint64_t prefix = 0, mask = 0;
    int left = n;                          // candidates: keys with (key & mask) == prefix
    for (int shift = 56; shift >= 0; shift -= 8) {
        reinterpret_cast<uint4*>(hist)[lane] = make_uint4(0, 0, 0, 0);
        __syncthreads();
        for (int p0 = 0; p0 < n; p0 += kWave) {
            const int p = p0 + lane;
            const uint64_t key = p < n ? keys[p] : 0;
            bool act = p < n && (key & mask) == prefix;
            const uint32_t digit = static_cast<uint32_t>(key >> shift) & 255u;
            // the lanes that share the first active lane's digit: one add for all of them
            const uint64_t am = __ballot(act);
            if (am) {
                const int first = __builtin_ctzll(am);
                const uint32_t d0 = __shfl(digit, first, kWave);
                const uint64_t same = __ballot(act && digit == d0);
                if (lane == first) atomicAdd(&hist[d0], static_cast<uint32_t>(__builtin_popcountll(same)));
                act = act && digit != d0;
            }
            if (act) atomicAdd(&hist[digit], 1u);
        }
        __syncthreads();
        // bins 4 lane .. 4 lane + 3; the bin that holds rank k
        const uint4 h = reinterpret_cast<const uint4*>(hist)[lane];
        const int mine = static_cast<int>(h.x + h.y + h.z + h.w);
        int incl = mine;
#pragma unroll
        for (int o = 1; o < kWave; o <<= 1) {
            const int t = __shfl_up(incl, o, kWave);
            if (lane >= o) incl += t;
        }
        const uint64_t over = __ballot(k < incl);          // never empty: the last lane's incl is `left` > k
        const int L = __builtin_ctzll(over);
        int kk = k - (__shfl(incl, L, kWave) - __shfl(mine, L, kWave));
        const int h0 = static_cast<int>(__shfl(h.x, L, kWave)), h1 = static_cast<int>(__shfl(h.y, L, kWave));
        const int h2 = static_cast<int>(__shfl(h.z, L, kWave)), h3 = static_cast<int>(__shfl(h.w, L, kWave));
        int d = 0, cnt = h0;
        if (kk >= cnt) { kk -= cnt; d = 1; cnt = h1;
            if (kk >= cnt) { kk -= cnt; d = 2; cnt = h2;
                if (kk >= cnt) { kk -= cnt; d = 3; cnt = h3; } } }
        prefix |= static_cast<uint64_t>(4 * L + d) << shift;
        mask |= 255ull << shift;
        k = kk;
        left = cnt;
        __syncthreads();                                   // the bins are read: the next pass may clear them
        if (left == 1) break;
    }
    // one pass over the keys: the candidate itself (if the passes stopped early) and the smallest key above it
    uint64_t found = ~0ull, above = ~0ull;
    for (int p = lane; p < n; p += kWave) {
        const uint64_t key = keys[p];
        if ((key & mask) == prefix) found = key;           // left == 1: one key; left > 1: mask is full, all equal
    }
    found = wave_min(found);
    if (k + 1 < left) {                                    // rank k + 1 is another copy of the same key
        *next = found;
        return found;
    }
    for (int p = lane; p < n; p += kWave) {
        const uint64_t key = keys[p];
        if (key > found && key < above) above = key;
    }
    *next = wave_min(above);
    return found;
}

template <int CAP>
__global__ __launch_bounds__(kWave) void trend_theil_sen(const double* __restrict__ y, int nstat, int nb, int64_t C,
                                                         int64_t ld, const double* __restrict__ x,
                                                         double* __restrict__ out, int64_t ldo) {
    constexpr int kPairs = CAP * (CAP - 1) / 2;
    __shared__ double tile[CAP * kTileLd];
    __shared__ uint64_t keys[kPairs];
    __shared__ double yv[CAP], xv[CAP];
    __shared__ __attribute__((aligned(16))) uint32_t hist[256];
    __shared__ double ymid[2];
    __shared__ double res[4][kTile];
    const int lane = threadIdx.x;
    const int64_t tiles = (C + kTile - 1) / kTile;
    const int64_t stat = blockIdx.x / tiles;
    const int64_t c0 = (blockIdx.x % tiles) * kTile;
    const int ncell = static_cast<int>(C - c0 < kTile ? C - c0 : kTile);
    const double nan = make_nan();
    {
        const int c = lane % kTile;
        const double* src = y + stat * nb * ld + c0 + c;
        for (int r = lane / kTile; r < nb; r += kWave / kTile)
            tile[r * kTileLd + c] = c < ncell ? src[static_cast<int64_t>(r) * ld] : nan;
    }
    __syncthreads();
    for (int c = 0; c < ncell; ++c) {
        // 1. the valid blocks, in block order
        int m = 0;
        bool bad = false;
        for (int b0 = 0; b0 < nb; b0 += kWave) {
            const int b = b0 + lane;
            const double v = b < nb ? tile[b * kTileLd + c] : nan;
            const bool ok = v == v;
            const uint64_t vm = __ballot(ok);
            if (ok) {
                const int pos = m + __builtin_popcountll(vm & lanes_below(lane));
                yv[pos] = v;
                xv[pos] = x[b];
            }
            bad |= __ballot(ok && isinf(v)) != 0;
            m += __builtin_popcountll(vm);
        }
        double trend = nan, mean = nan, mk_s = nan, mk_var = nan;
        if (m == 0 || bad) {
            // land, a statistic that is NaN in every block, or an infinite value: nothing to compute
        } else if (m == 1) {
            __syncthreads();
            mean = yv[0];
        } else {
            __syncthreads();
            // 2. ties and the two middle y
            int tie = 0;
            for (int b = lane; b < m; b += kWave) {
                const double v = yv[b];
                const uint64_t kv = f64_key(v);
                int eq = 0, below = 0;
                for (int j = 0; j < m; ++j) {
                    const double w = yv[j];                // the same address in every lane: a broadcast
                    const uint64_t kw = f64_key(w);
                    eq += w == v;
                    below += (kw < kv) | ((kw == kv) & (j < b));
                }
                tie += (eq - 1) * (2 * eq + 5);
                if (below == (m - 1) / 2) ymid[0] = v;
                if (below == m / 2) ymid[1] = v;
            }
            tie = wave_sum(tie);
            // 3. the pairs i < j in row-major order, lane-strided
            const int N = m * (m - 1) / 2;
            int s = 0;
            int i = 0, j = 1 + lane;
            for (int p = lane; p < N; p += kWave) {
                while (j >= m) {                           // p < N: ends with i < j < m
                    j -= m;
                    ++i;
                    j += i + 1;
                }
                const double yi = yv[i], yj = yv[j];
                const double slope = (yj - yi) / (xv[j] - xv[i]);
                keys[p] = f64_key(slope);
                s += (yj > yi) - (yj < yi);
                j += kWave;
            }
            s = wave_sum(s);
            __syncthreads();
            // 4. the two middle slopes
            uint64_t k_hi;
            const uint64_t k_lo = radix_select(keys, N, (N - 1) / 2, hist, lane, &k_hi);
            if ((N & 1) != 0) k_hi = k_lo;
            trend = (key_f64(k_lo) + key_f64(k_hi)) / 2.0;
            const double ymed = (ymid[0] + ymid[1]) / 2.0;
            const double xmed = (xv[(m - 1) / 2] + xv[m / 2]) / 2.0;      // x is increasing: xv is sorted
            mean = ymed - trend * xmed;
            if (m >= 3) {
                mk_s = static_cast<double>(s);
                const int64_t mm = m;
                mk_var = static_cast<double>(mm * (mm - 1) * (2 * mm + 5) - tie) / 18.0;
            }
        }
        if (lane == 0) {
            res[0][c] = trend;
            res[1][c] = mean;
            res[2][c] = mk_s;
            res[3][c] = mk_var;
        }
        __syncthreads();                                   // yv / xv / ymid / keys are free for the next cell
    }
    const int w = lane / kTile, c = lane % kTile;
    if (c < ncell) out[(static_cast<int64_t>(w) * nstat + stat) * ldo + c0 + c] = res[w][c];
}

template <int CAP>
void launch_ts(unsigned blocks, hipStream_t stream, const double* y, int nstat, int nb, int64_t C, int64_t ld,
               const double* x, double* out, int64_t ldo) {
    hipLaunchKernelGGL(trend_theil_sen<CAP>, dim3(blocks), dim3(kWave), 0, stream, y, nstat, nb, C, ld, x, out, ldo);
}

}  // namespace

hipError_t launch_trend_ols(const double* y, int32_t nstat, int32_t nb, int64_t C, int64_t ld, const double* x,
                            const double* tcrit, double* out, int64_t ldo, hipStream_t stream) {
    if (nstat <= 0 || C <= 0) return hipSuccess;
    const int64_t blocks = static_cast<int64_t>(nstat) * ((C + kWave - 1) / kWave);
    if (blocks > 0x7FFFFFFFll) return hipErrorInvalidValue;
    if (nb <= kOlsStageBlocks)
        hipLaunchKernelGGL(trend_ols<true>, dim3(static_cast<unsigned>(blocks)), dim3(kWave),
                           sizeof(double) * kWave * static_cast<size_t>(nb), stream, y, nstat, nb, C, ld, x, tcrit, out, ldo);
    else
        hipLaunchKernelGGL(trend_ols<false>, dim3(static_cast<unsigned>(blocks)), dim3(kWave), 0, stream, y, nstat, nb, C,
                           ld, x, tcrit, out, ldo);
    return hipGetLastError();
}

hipError_t launch_trend_theil_sen(const double* y, int32_t nstat, int32_t nb, int64_t C, int64_t ld, const double* x,
                                  double* out, int64_t ldo, hipStream_t stream) {
    if (nstat <= 0 || C <= 0) return hipSuccess;
    if (nb > kTrendMaxBlocks) return hipErrorInvalidValue;
    const int64_t blocks = static_cast<int64_t>(nstat) * ((C + kTile - 1) / kTile);
    if (blocks > 0x7FFFFFFFll) return hipErrorInvalidValue;
    const unsigned g = static_cast<unsigned>(blocks);
    if (nb <= 8) launch_ts<8>(g, stream, y, nstat, nb, C, ld, x, out, ldo);
    else if (nb <= 16) launch_ts<16>(g, stream, y, nstat, nb, C, ld, x, out, ldo);
    else if (nb <= 24) launch_ts<24>(g, stream, y, nstat, nb, C, ld, x, out, ldo);
    else if (nb <= 32) launch_ts<32>(g, stream, y, nstat, nb, C, ld, x, out, ldo);
    else if (nb <= 40) launch_ts<40>(g, stream, y, nstat, nb, C, ld, x, out, ldo);
    else if (nb <= 48) launch_ts<48>(g, stream, y, nstat, nb, C, ld, x, out, ldo);
    else if (nb <= 64) launch_ts<64>(g, stream, y, nstat, nb, C, ld, x, out, ldo);
    else if (nb <= 96) launch_ts<96>(g, stream, y, nstat, nb, C, ld, x, out, ldo);
    else launch_ts<kTrendMaxBlocks>(g, stream, y, nstat, nb, C, ld, x, out, ldo);
    return hipGetLastError();
}

}  // namespace xmhw
