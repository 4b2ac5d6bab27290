// kernels_coarsen.hip -- coarsen(): weighted block means in space and time.  The definition is in
// include/xmhw_amd.h, "coarsen()"; in short, for the coarse cell (J, I) and the window s of steps win[s] .. win[s + 1] - 1,
// over the in-grid fine samples of the block fy x fx behind the cell that have wi > 0 and are not NaN:
//   xq = rint(((double)x - x0) * 2^16), left out and counted (*n_range) when |x - x0| >= 2^7 or infinite
//   n += 1, wsum += wi, xsum += wi * xq            (exact integers: |xsum| <= 2^59 under the cap of 4096 samples)
//   W = the sum of wi over the in-grid points of the block, land included
//   out = x0 + ((double)xsum / (double)wsum) / 65536.0 where n >= 1 and wsum * 65536 >= a * len * W, NaN elsewhere
//
//   coarsen_windows<T, VW, WIDE, COLS>
//                     lane = one coarse cell, flat index c = J * ncx + I (coarsen_index.h), 256 lanes a workgroup; grid.y
//                     covers chunks of windows and strides over the chunks it cannot hold.  Nothing is carried from one
//                     launch to the next and nothing is shared: no LDS, no cross-lane traffic, no atomics but one
//                     wave-reduced add to *n_range when the wave's count is not zero.
//   a line            what a lane reads with one request: its VW = fx consecutive samples of one fine row (fx = 1, 2, 4:
//                     WIDE in one load of the lane's full width -- 4, 8, 16 bytes of float32, two loads of 16 for four
//                     float64 --, else VW loads of one sample), or, for any other fx (COLS), one sample: the lines of
//                     a block are then its fy * fx points, a run-time column loop.  A wave reads 64 * fx contiguous
//                     samples per row and step either way.  A lane whose block hangs over the last column reads its
//                     in-grid samples one by one whatever the class: no load reaches past the row.
//   a window          of kCoBatch = 4 steps and more: line by line, the line's weights in registers across the steps,
//                     the samples of four steps requested together.  A shorter window (the purely spatial coarsening
//                     among them): four lines together, their weights in registers across the steps.  Up to
//                     4 x 16 bytes of samples per lane are in flight, the 64 B of kernels_stress.hip.
//   the weights       int32, read as the samples are (same lines, same widths): ny * nx * 4 bytes that the workgroups
//                     of all chunks share -- they live in L2 and are no second stream from HBM.  W falls out of them.
//   per sample        f32 -> f64, subtract, d == d and |d| < 2^7, scale, rint, convert, the gates, one v_mad_i64_i32 (xsum),
//                     one 64-bit add (wsum) and one 32-bit add (n): the chain region_series() has, without its wave sums.
//   what binds        the bytes a wave has in flight between two windows, not this chain (measured).
#include "../../include/xmhw_amd.h"
#include "entry_common.h"
#include "stage_reduce.h"
#include "coarsen_index.h"

namespace xmhw {

// What the stage computes (coarsen_index.h holds the index rules): the weighted means of the blocks fy x fx of the
// UNCOMPACTED ny x nx grid
// over the windows win[s] .. win[s + 1] - 1 of the nt rows at ts -- out [ns][ldo] in the sample type, WRITTEN; wsum int64 and
// n int32 likewise where not NULL; *n_range ADDED to; the definition is in include/xmhw_amd.h, "coarsen()".  win_dev is a
// DEVICE array of ns + 1 boundaries here, max_len the longest window of it.  variant: kCoarsenVariantAuto, or a narrower
// instantiation than the call's alignment allows (tests and measurements); chunk_windows: the windows a workgroup takes per
// chunk, 0 = automatic (coarsen_auto_chunk); same results for every value of either.
constexpr int kCoarsenBits = 16;
constexpr int kCoarsenRangeBits = 7;
constexpr int kCoarsenMaxWeightBits = 24;
constexpr int kCoarsenVariantAuto = 0;               // the widest loads the call's alignment allows
constexpr int kCoarsenVariantNarrow = 1;             // fx = 2, 4 with loads of one sample
constexpr int kCoarsenVariantGeneric = 2;            // the run-time column loop whatever fx

static_assert(kCoarsenBits == kFixedBits && kCoarsenRangeBits == kFixedRangeBits, "one scale for every stage");

namespace {

using u64 = unsigned long long;

constexpr int kCoThreads = kStageThreads;
constexpr int kCoBatch = 4;                          // steps (long windows) or lines (short ones) requested together

template <typename T>
struct CoIn {
    const T* ts;                                     // [nt][ld]
    int64_t ld;
    int32_t ny, nx, fy, fx, ncy, ncx;
    const int32_t* wi;                               // [ny * nx]
    double x0;
    int32_t a;                                       // the least covered share, in 65536ths
    const int32_t* win;                              // [ns + 1], device
    int32_t ns, per;                                 // windows, windows per chunk
};

template <typename T>
struct CoOut {
    T* out;                                          // [ns][ldo]
    int64_t ldo;
    int64_t* wsum;                                   // [ns][ldo] or NULL
    int32_t* n;                                      // [ns][ldo] or NULL
    u64* n_range;
};

template <typename P, int VW>
struct alignas(sizeof(P) * VW > 16 ? 16 : sizeof(P) * VW) CoPack {
    P v[VW];
};

// the `live` (0 .. VW) leading items of a line at p; the others are zero
template <typename P, int VW, bool WIDE>
__device__ __forceinline__ void co_load(const P* __restrict__ p, int32_t live, P (&x)[VW]) {
    if (WIDE && live == VW) {                        // (the class says that p is aligned: coarsen_class)
        const CoPack<P, VW> pack = *reinterpret_cast<const CoPack<P, VW>*>(p);
#pragma unroll
        for (int k = 0; k < VW; ++k) x[k] = pack.v[k];
        return;
    }
#pragma unroll
    for (int k = 0; k < VW; ++k) x[k] = k < live ? p[k] : static_cast<P>(0);
}

struct CoSums {
    int32_t n;
    int64_t wsum, xsum;
    u64 range;
};

template <typename T, int VW>
__device__ __forceinline__ void co_add(const T (&x)[VW], const int32_t (&w)[VW], double x0, CoSums& v) {
#pragma unroll
    for (int k = 0; k < VW; ++k) {
        const double d = static_cast<double>(x[k]) - x0;
        bool ok = w[k] > 0 && d == d;                // land, a point outside the grid (w = 0), NaN: no sample
        const bool in_range = fabs(d) < kFixedRange; // +-inf included
        v.range += ok && !in_range;
        ok = ok && in_range;
        const int32_t xq = ok ? static_cast<int32_t>(rint(d * kFixedOne)) : 0;
        const int32_t wk = ok ? w[k] : 0;
        v.n += ok;
        v.wsum += wk;
        v.xsum += static_cast<int64_t>(wk) * xq;
    }
}

template <typename T, int VW, bool WIDE, bool COLS>
__global__ __launch_bounds__(kCoThreads) void coarsen_windows(CoIn<T> in, CoOut<T> out) {
    static_assert(!COLS || VW == 1, "the column loop reads one sample a line");
    const int64_t cells = static_cast<int64_t>(in.ncy) * in.ncx;
    const int64_t c = static_cast<int64_t>(blockIdx.x) * kCoThreads + threadIdx.x;
    // a lane without a cell owns a block of 0 x 0 points: it reads nothing and stays for the wave's count at the end
    const CoarsenBlock b = coarsen_block(c, in.ny, in.nx, in.fy, in.fx, in.ncy, in.ncx);
    const bool live = c < cells;
    const int64_t origin = static_cast<int64_t>(b.j0) * in.nx + b.i0;
    const T* const base = in.ts + origin;
    const int32_t* const wbase = in.wi + origin;
    const int32_t lines = COLS ? in.fy * in.fx : in.fy;      // uniform; <= 4096
    // line q of the block: its offset from the origin and how many of its items are the lane's (0: none)
    const auto line_at = [&](int32_t q, int64_t* off) -> int32_t {
        if (COLS) {
            const int32_t r = q / in.fx, i = q - r * in.fx;
            *off = static_cast<int64_t>(r) * in.nx + i;
            return r < b.h && i < b.w ? 1 : 0;
        }
        *off = static_cast<int64_t>(q) * in.nx;
        return q < b.h ? b.w : 0;                    // b.w <= fx == VW
    };
    u64 range = 0;
    const int64_t nchunks = coarsen_chunks(in.ns, in.per);
    for (int64_t chunk = blockIdx.y; chunk < nchunks; chunk += gridDim.y) {
        int32_t s0, s1;
        coarsen_chunk(chunk, in.ns, in.per, &s0, &s1);
        for (int32_t s = s0; s < s1; ++s) {
            const int32_t t0 = in.win[s], t1 = in.win[s + 1];
            const int32_t len = t1 - t0;
            CoSums v = {0, 0, 0, 0};
            int64_t W = 0;
            if (len >= kCoBatch) {
                for (int32_t q = 0; q < lines; ++q) {
                    int64_t off;
                    const int32_t mine = line_at(q, &off);
                    int32_t w[VW];
                    co_load<int32_t, VW, WIDE>(wbase + off, mine, w);
#pragma unroll
                    for (int k = 0; k < VW; ++k) W += w[k];
                    const T* p = base + off + static_cast<int64_t>(t0) * in.ld;
                    for (int32_t t = t0; t < t1; t += kCoBatch) {
                        T x[kCoBatch][VW];
#pragma unroll
                        for (int u = 0; u < kCoBatch; ++u)
                            co_load<T, VW, WIDE>(p + u * in.ld, t + u < t1 ? mine : 0, x[u]);
#pragma unroll
                        for (int u = 0; u < kCoBatch; ++u)
                            if (t + u < t1) co_add<T, VW>(x[u], w, in.x0, v);
                        p += kCoBatch * in.ld;
                    }
                }
            } else {
                for (int32_t q0 = 0; q0 < lines; q0 += kCoBatch) {
                    int64_t off[kCoBatch];
                    int32_t mine[kCoBatch];
                    int32_t w[kCoBatch][VW];
#pragma unroll
                    for (int u = 0; u < kCoBatch; ++u) {
                        mine[u] = q0 + u < lines ? line_at(q0 + u, &off[u]) : 0;
                        if (q0 + u >= lines) off[u] = 0;
                        co_load<int32_t, VW, WIDE>(wbase + off[u], mine[u], w[u]);
                    }
#pragma unroll
                    for (int u = 0; u < kCoBatch; ++u)
#pragma unroll
                        for (int k = 0; k < VW; ++k) W += w[u][k];
                    const T* p = base + static_cast<int64_t>(t0) * in.ld;
                    for (int32_t t = t0; t < t1; ++t) {
                        T x[kCoBatch][VW];
#pragma unroll
                        for (int u = 0; u < kCoBatch; ++u) co_load<T, VW, WIDE>(p + off[u], mine[u], x[u]);
#pragma unroll
                        for (int u = 0; u < kCoBatch; ++u) co_add<T, VW>(x[u], w[u], in.x0, v);
                        p += in.ld;
                    }
                }
            }
            range += v.range;
            if (live) {
                const bool valid = v.n >= 1 && v.wsum * 65536 >= static_cast<int64_t>(in.a) * len * W;
                const double mean = in.x0 + (static_cast<double>(v.xsum) / static_cast<double>(v.wsum)) / kFixedOne;
                const int64_t at = static_cast<int64_t>(s) * out.ldo + c;
                out.out[at] = valid ? static_cast<T>(mean) : static_cast<T>(make_nan());
                if (out.wsum) out.wsum[at] = v.wsum;
                if (out.n) out.n[at] = v.n;
            }
        }
    }
    // the wave's count, added once and only when it is not zero (every lane of the wave is here: nothing returned early)
    if (__ballot(range != 0) != 0) {
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const uint32_t lo = __shfl_xor(static_cast<uint32_t>(range), m, 64);
            const uint32_t hi = __shfl_xor(static_cast<uint32_t>(range >> 32), m, 64);
            range += (static_cast<u64>(hi) << 32) | lo;
        }
        if ((threadIdx.x & 63) == 0) atomicAdd(out.n_range, range);
    }
}

template <typename T, int VW, bool WIDE, bool COLS>
hipError_t co_launch(const CoIn<T>& in, const CoOut<T>& out, hipStream_t stream) {
    const int64_t cells = static_cast<int64_t>(in.ncy) * in.ncx;
    const dim3 grid(static_cast<unsigned>(ceil_div(cells, kCoThreads)),
                    static_cast<unsigned>(stage_blocks(in.ns, in.per)));
    hipLaunchKernelGGL((coarsen_windows<T, VW, WIDE, COLS>), grid, dim3(kCoThreads), 0, stream, in, out);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_coarsen(const T* ts, int64_t ld, int32_t ny, int32_t nx, int32_t fy, int32_t fx, int32_t ncy, int32_t ncx,
                          const int32_t* wi, double x0, int32_t a, const int32_t* win_dev, int32_t ns, int32_t max_len,
                          int32_t variant, int32_t chunk_windows, T* out, int64_t ldo, int64_t* wsum, int32_t* n,
                          int64_t* n_range, hipStream_t stream) {
    if (ns <= 0 || ncy <= 0 || ncx <= 0) return hipSuccess;
    if (!coarsen_grid_ok(ny, nx, fy, fx, ncy, ncx) || max_len < 1 ||
        static_cast<int64_t>(fy) * fx * max_len > kCoarsenMaxVolume || static_cast<int64_t>(ny) * nx > INT32_MAX)
        return hipErrorInvalidValue;
    const int64_t cells = static_cast<int64_t>(ncy) * ncx;
    const int64_t per = chunk_windows > 0 ? chunk_windows : coarsen_auto_chunk(ns, cells, fy, max_len);
    const CoIn<T> in{ts, ld, ny, nx, fy, fx, ncy, ncx, wi, x0, a, win_dev, ns, static_cast<int32_t>(per < ns ? per : ns)};
    const CoOut<T> o{out, ldo, wsum, n, reinterpret_cast<u64*>(n_range)};
    switch (coarsen_class(reinterpret_cast<uint64_t>(ts), reinterpret_cast<uint64_t>(wi), ld, nx, sizeof(T), fx,
                          variant == kCoarsenVariantNarrow, variant == kCoarsenVariantGeneric)) {
        case kCoarsenFx1: return co_launch<T, 1, false, false>(in, o, stream);
        case kCoarsenFx2: return co_launch<T, 2, false, false>(in, o, stream);
        case kCoarsenFx2Wide: return co_launch<T, 2, true, false>(in, o, stream);
        case kCoarsenFx4: return co_launch<T, 4, false, false>(in, o, stream);
        case kCoarsenFx4Wide: return co_launch<T, 4, true, false>(in, o, stream);
        default: return co_launch<T, 1, false, true>(in, o, stream);
    }
}

}  // namespace

}  // namespace xmhw

// ---- the C entries of coarsen() (include/xmhw_amd.h) ------------------------------------------------------------------
namespace {

using namespace xmhw::entry;

static std::atomic<int> g_coarsen_variant{0};      // which loads coarsen() may use, 0 = the widest (xmhw_set_coarsen_variant)
static std::atomic<int> g_coarsen_chunk{0};        // windows a workgroup takes per chunk, 0 = automatic (xmhw_set_coarsen_chunk)

static_assert(XMHW_COARSEN_MAX_VOLUME == xmhw::kCoarsenMaxVolume && XMHW_COARSEN_MAX_WEIGHT_BITS == xmhw::kCoarsenMaxWeightBits &&
                  XMHW_REGION_SERIES_BITS == xmhw::kCoarsenBits,
              "the public limits of coarsen() are the kernel's");

template <typename T>
int coarsen(const T* ts, int64_t nt, int64_t ld, int32_t ny, int32_t nx, int32_t fy, int32_t fx, int32_t ncy, int32_t ncx,
            const int32_t* wi, double x0, int32_t a, const int32_t* win, int32_t ns, T* out, int64_t ldo, int64_t* wsum,
            int32_t* n, int64_t* n_range, void* stream) {
    // the caps: the volume of the largest block x window, over the windows of positive length of a table that is there
    int64_t max_len = 1;
    if (win)
        for (int32_t s = 0; s < ns; ++s) max_len = std::max<int64_t>(max_len, static_cast<int64_t>(win[s + 1]) - win[s]);
    if (fy >= 1 && fx >= 1 && static_cast<int64_t>(fy) * fx * max_len > xmhw::kCoarsenMaxVolume)
        return fail(XMHW_ERR_UNSUPPORTED, "coarsen: fy * fx * the longest window is above the cap of " +
                                              std::to_string(xmhw::kCoarsenMaxVolume) + " samples");
    if (ny > 0 && nx > 0 && static_cast<int64_t>(ny) * nx > INT32_MAX)
        return fail(XMHW_ERR_UNSUPPORTED, "coarsen: a grid of 2^31 points and more");
    if (nt < 0 || ny < 0 || nx < 0 || ld < static_cast<int64_t>(ny) * nx) return fail(XMHW_ERR_INVALID, "bad nt/ny/nx/ld");
    if (fy < 1 || fx < 1) return fail(XMHW_ERR_INVALID, "coarsen: the factors must be >= 1");
    if (!xmhw::coarsen_grid_ok(ny, nx, fy, fx, ncy, ncx))
        return fail(XMHW_ERR_INVALID, "coarsen: ncy, ncx must lie in [0, ceil(ny / fy)], [0, ceil(nx / fx)]");
    if (ldo < static_cast<int64_t>(ncy) * ncx) return fail(XMHW_ERR_INVALID, "bad ldo");
    if (ns < 0 || (ns > 0 && !win)) return fail(XMHW_ERR_INVALID, "bad ns / NULL window table");
    if (ns > 0 && (win[0] < 0 || win[ns] > nt)) return fail(XMHW_ERR_INVALID, "coarsen: the windows leave [0, nt]");
    for (int32_t s = 0; s < ns; ++s)
        if (win[s + 1] <= win[s]) return fail(XMHW_ERR_INVALID, "coarsen: the window table must be strictly increasing");
    if (a < 0 || a > 65536) return fail(XMHW_ERR_INVALID, "coarsen: a must be in [0, 65536]");
    if (!std::isfinite(x0)) return fail(XMHW_ERR_INVALID, "coarsen: x0 must be finite");
    if (ns == 0 || ncy == 0 || ncx == 0) return XMHW_OK;
    if (!ts || !wi || !out || !n_range) return fail(XMHW_ERR_INVALID, "NULL buffer");
    RowsRef table;
    if (int rc = upload_table(win, static_cast<int64_t>(ns) + 1, "window table upload", &table)) return rc;
    return status_of(xmhw::launch_coarsen<T>(ts, ld, ny, nx, fy, fx, ncy, ncx, wi, x0, a, table->d_rows, ns,
                                             static_cast<int32_t>(max_len), g_coarsen_variant.load(), g_coarsen_chunk.load(),
                                             out, ldo, wsum, n, n_range, static_cast<hipStream_t>(stream)),
                     "coarsen launch");
}

}  // namespace

extern "C" {

int xmhw_set_coarsen_variant(int32_t variant) {
    if (variant < xmhw::kCoarsenVariantAuto || variant > xmhw::kCoarsenVariantGeneric)
        return fail(XMHW_ERR_INVALID, "variant must be 0, 1 or 2");
    g_coarsen_variant = variant;
    return XMHW_OK;
}
int xmhw_set_coarsen_chunk(int32_t windows) { return set_knob(g_coarsen_chunk, windows, "windows must be >= 0"); }
int xmhw_coarsen_class(const void* ts, const int32_t* wi, int64_t ld, int32_t nx, int32_t itemsize, int32_t fx) {
    const int32_t variant = g_coarsen_variant.load();
    return xmhw::coarsen_class(reinterpret_cast<uint64_t>(ts), reinterpret_cast<uint64_t>(wi), ld, nx, itemsize, fx,
                               variant == xmhw::kCoarsenVariantNarrow, variant == xmhw::kCoarsenVariantGeneric);
}
int xmhw_coarsen_f32(const float* ts, int64_t nt, int64_t ld, int32_t ny, int32_t nx, int32_t fy, int32_t fx, int32_t ncy,
                     int32_t ncx, const int32_t* wi, double x0, int32_t a, const int32_t* win, int32_t ns, float* out,
                     int64_t ldo, int64_t* wsum, int32_t* n, int64_t* n_range, void* stream) {
    return coarsen<float>(ts, nt, ld, ny, nx, fy, fx, ncy, ncx, wi, x0, a, win, ns, out, ldo, wsum, n, n_range, stream);
}
int xmhw_coarsen_f64(const double* ts, int64_t nt, int64_t ld, int32_t ny, int32_t nx, int32_t fy, int32_t fx, int32_t ncy,
                     int32_t ncx, const int32_t* wi, double x0, int32_t a, const int32_t* win, int32_t ns, double* out,
                     int64_t ldo, int64_t* wsum, int32_t* n, int64_t* n_range, void* stream) {
    return coarsen<double>(ts, nt, ld, ny, nx, fy, fx, ncy, ncx, wi, x0, a, win, ns, out, ldo, wsum, n, n_range, stream);
}

}  // extern "C"
