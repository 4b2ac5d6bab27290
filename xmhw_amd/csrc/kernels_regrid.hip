// kernels_regrid.hip -- regrid(): first-order conservative remapping between two rectilinear grids.  The
// definition is in include/xmhw_amd.h, "regrid()"; in short, for the step t and the destination cell (J, I), over the pairs
// (r, k) of its row run and its column run with w = ay * ax > 0 whose sample x[t][row_first[J] + r][(col_first[I] + k) mod nx]
// is not NaN:
//   xq = rint(((double)x - x0) * 2^16), left out and counted (*n_range, per pair) when |x - x0| >= 2^7 or infinite
//   n += 1, wsum += w, xsum += w * xq              (exact integers: |xsum| <= 2^59 under the caps)
//   out = x0 + ((double)xsum / (double)wsum) / 65536.0 where n >= 1 and wsum * 65536 >= a * wy[J] * wx[I], NaN elsewhere
//
//   regrid_steps<T, KX, STAGED>
//                     workgroup = one destination row J x 256 destination columns (regrid_index.h), a wave = 64 consecutive
//                     columns of that row: the row's run and its ay are uniform over the workgroup and come through the
//                     scalar cache.  A lane keeps its column run (first, count; its ax in registers where the longest
//                     column run of the call is KX = 1, 2 or 4; KX = 0 reads ax in a run-time loop) for the whole launch.
//                     grid.y covers chunks of steps and strides over the chunks it cannot hold.  Nothing is carried from
//                     one launch to the next; the only atomic is one wave-reduced add to *n_range when the wave's count is
//                     not zero.
//   the sample word   a sample becomes ONE dword: xq (|xq| <= 2^23), or one of two sentinels below -2^23, kRgNaN (no
//                     sample) and kRgRange (a sample out of range); the sums are taken from such words on both paths, so
//                     the two paths cannot differ by a bit.
//   direct            the lane loads its samples from global memory, one per (r, k), and converts each; the samples of
//                     kRgBatch = 4 steps are requested together.  Any table within the caps.
//   staged            per step, the workgroup loads the source footprint of its tile -- the row run x the tile's
//                     contiguous column span, wrapped at a periodic seam -- with coalesced loads, converts every sample
//                     once into an LDS dword and, after a barrier, every lane reads its rows x columns words at its own
//                     offset.  Possible where the largest footprint of the call fits (regrid_fits); the automatic choice
//                     takes it where it measured faster (regrid_auto_staged).
//   the sums          separable: per source row sw = sum ax, sx = sum ax * xq over the lane's columns (|sx| <= 2^41), then
//                     wsum += ay * sw, xsum += ay * sx; a row with ay = 0 is skipped (uniform).
#include <cstring>

#include "../../include/xmhw_amd.h"
#include "entry_common.h"
#include "stage_reduce.h"
#include "regrid_index.h"

namespace xmhw {

// What the stage computes (regrid_index.h holds the index rules): first-order conservative remapping of the UNCOMPACTED
// ny x nx series at ts
// onto the my x mx destination grid under two CSR overlap tables -- out [nt][ldo] in the sample type, WRITTEN; wsum int64 and
// n int32 likewise where not NULL; *n_range ADDED to; the definition is in include/xmhw_amd.h, "regrid()".  table_dev is the
// ONE device table that holds the ten int32 tables of the call at the places `lay` names (regrid_layout); max_rows, max_cols
// the longest run per axis and max_width the widest tile span (regrid_max_width), taken from the host tables.  variant:
// kRegridVariantAuto, Direct or Staged (staged where the footprint fits, tests and measurements); chunk_steps: the steps a
// workgroup takes per chunk, 0 = automatic (regrid_auto_chunk); same results for every value of either.
constexpr int kRegridBits = 16;
constexpr int kRegridRangeBits = 7;
constexpr int kRegridVariantAuto = 0;
constexpr int kRegridVariantDirect = 1;
constexpr int kRegridVariantStaged = 2;

static_assert(kRegridBits == kFixedBits && kRegridRangeBits == kFixedRangeBits, "one scale for every stage");

namespace {

using u64 = unsigned long long;

constexpr int kRgThreads = kRegridTile;
constexpr int kRgBatch = 4;                          // steps the direct path requests together
constexpr int32_t kRgNaN = INT32_MIN;                // the sample words that are no xq
constexpr int32_t kRgRange = INT32_MIN + 1;
static_assert(kRgThreads == kStageThreads, "the workgroup of every stage kernel");

template <typename T>
struct RgIn {
    const T* ts;                                     // [nt][ld]
    int64_t ld, nt, per;                             // steps, steps per chunk
    int32_t ny, nx, my, mx;
    const int32_t *row_first, *row_ptr, *ay, *wy;    // device
    const int32_t *col_first, *col_ptr, *ax, *wx;
    const int32_t *tile_c0, *tile_w;                 // the span of every column tile (staged)
    int32_t periodic;
    double x0;
    int32_t a;                                       // the least covered share, in 65536ths
};

template <typename T>
struct RgOut {
    T* out;                                          // [nt][ldo]
    int64_t ldo;
    int64_t* wsum;                                   // [nt][ldo] or NULL
    int32_t* n;                                      // [nt][ldo] or NULL
    u64* n_range;
};

struct RgSums {
    int32_t n;
    int64_t wsum, xsum;
};

template <typename T>
__device__ __forceinline__ int32_t rg_word(T x, double x0) {
    const double d = static_cast<double>(x) - x0;
    const int32_t q = static_cast<int32_t>(rint((fabs(d) < kFixedRange ? d : 0.0) * kFixedOne));
    return d == d ? (fabs(d) < kFixedRange ? q : kRgRange) : kRgNaN;      // +-inf is out of range
}

// one sample word under the column weight w into the sums of a source row
__device__ __forceinline__ void rg_add(int32_t q, int32_t w, int32_t& sw, int64_t& sx, int32_t& nk, int32_t& rk) {
    const bool ok = w > 0 && q > kRgRange;
    rk += w > 0 && q == kRgRange;
    nk += ok;
    sw += ok ? w : 0;
    sx += ok ? static_cast<int64_t>(w) * q : 0;
}

template <typename T, int KX, bool STAGED>
__global__ __launch_bounds__(kRgThreads) void regrid_steps(RgIn<T> in, RgOut<T> out) {
    constexpr int B = STAGED ? 1 : kRgBatch;
    constexpr int KR = KX > 0 ? KX : 1;
    extern __shared__ int32_t rg_lds[];
    const bool periodic = in.periodic != 0;
    int32_t J = 0, I0 = 0;
    if (!regrid_tile(blockIdx.x, in.my, in.mx, &J, &I0)) return;         // (uniform; the grid holds tiles only)
    const int32_t I = I0 + static_cast<int32_t>(threadIdx.x);
    const bool live = I < in.mx;
    // the row run: uniform over the workgroup
    const int32_t rf = in.row_first[J], rp = in.row_ptr[J], rny = in.row_ptr[J + 1] - rp;
    // the lane's column run; a lane without a cell owns an empty one and stays for the barriers and the wave's count
    const int32_t cf = live ? in.col_first[I] : 0, cp = live ? in.col_ptr[I] : 0;
    const int32_t cnx = live ? in.col_ptr[I + 1] - cp : 0;
    int32_t axr[KR];
#pragma unroll
    for (int k = 0; k < KR; ++k) axr[k] = KX > 0 && k < cnx ? in.ax[cp + k] : 0;
    const int64_t least = live ? static_cast<int64_t>(in.a) * in.wy[J] * in.wx[I] : 0;
    // staged: the tile's span and the lane's place in it
    int32_t c0 = 0, width = 0, off = 0;
    if (STAGED) {
        const int32_t tile = I0 / kRegridTile;
        c0 = in.tile_c0[tile];
        width = in.tile_w[tile];
        off = cnx > 0 ? regrid_lane_offset(cf, c0, in.nx, periodic) : 0;
    }
    u64 range = 0;
    const int64_t nchunks = regrid_chunks(in.nt, in.per);
    for (int64_t chunk = blockIdx.y; chunk < nchunks; chunk += gridDim.y) {
        int64_t t0, t1;
        regrid_chunk(chunk, in.nt, in.per, &t0, &t1);
        for (int64_t t = t0; t < t1; t += B) {
            const T* const step = in.ts + t * in.ld;
            if (STAGED) {
                __syncthreads();                     // the words of the step before have been read
                for (int32_t r = 0; r < rny; ++r) {
                    if (in.ay[rp + r] == 0) continue;                     // (uniform) nobody reads that row
                    const T* const src = step + static_cast<int64_t>(rf + r) * in.nx;
                    for (int32_t s = threadIdx.x; s < width; s += kRgThreads) {
                        const int32_t col = regrid_source_col(c0, s, in.nx, periodic);   // in the grid: the call fits
                        rg_lds[r * width + s] = rg_word<T>(src[col > 0 ? col : 0], in.x0);
                    }
                }
                __syncthreads();
            }
            RgSums v[B];
#pragma unroll
            for (int u = 0; u < B; ++u) v[u] = {0, 0, 0};
            for (int32_t r = 0; r < rny; ++r) {
                const int32_t ayr = in.ay[rp + r];
                if (ayr == 0) continue;              // (uniform) w = 0 for the whole row
                const T* const src = step + static_cast<int64_t>(rf + r) * in.nx;
                const int32_t* const words = rg_lds + r * width + off;
                int32_t sw[B], nk[B], rk[B];
                int64_t sx[B];
#pragma unroll
                for (int u = 0; u < B; ++u) sw[u] = nk[u] = rk[u] = 0, sx[u] = 0;
                // the sample word of entry k of the lane's run at step t + u (k < cnx)
                const auto word_at = [&](int32_t k, int u) -> int32_t {
                    if (STAGED) return words[k];
                    if (t + u >= t1) return kRgNaN;
                    int32_t col = cf + k;
                    col = periodic && col >= in.nx ? col - in.nx : col;
                    return rg_word<T>(src[u * in.ld + col], in.x0);
                };
                if (KX > 0) {
                    int32_t q[B][KR];
#pragma unroll
                    for (int u = 0; u < B; ++u)
#pragma unroll
                        for (int k = 0; k < KR; ++k) q[u][k] = k < cnx ? word_at(k, u) : kRgNaN;
#pragma unroll
                    for (int u = 0; u < B; ++u)
#pragma unroll
                        for (int k = 0; k < KR; ++k) rg_add(q[u][k], axr[k], sw[u], sx[u], nk[u], rk[u]);
                } else {
                    for (int32_t k = 0; k < cnx; ++k) {
                        const int32_t w = in.ax[cp + k];
                        int32_t q[B];
#pragma unroll
                        for (int u = 0; u < B; ++u) q[u] = word_at(k, u);
#pragma unroll
                        for (int u = 0; u < B; ++u) rg_add(q[u], w, sw[u], sx[u], nk[u], rk[u]);
                    }
                }
#pragma unroll
                for (int u = 0; u < B; ++u) {
                    v[u].n += nk[u];
                    v[u].wsum += static_cast<int64_t>(ayr) * sw[u];
                    v[u].xsum += ayr * sx[u];
                    range += static_cast<u64>(rk[u]);
                }
            }
            if (live) {
#pragma unroll
                for (int u = 0; u < B; ++u) {
                    if (t + u >= t1) continue;
                    const bool valid = v[u].n >= 1 && v[u].wsum * 65536 >= least;
                    const double mean = in.x0 + (static_cast<double>(v[u].xsum) / static_cast<double>(v[u].wsum)) / kFixedOne;
                    const int64_t at = (t + u) * out.ldo + static_cast<int64_t>(J) * in.mx + I;
                    out.out[at] = valid ? static_cast<T>(mean) : static_cast<T>(make_nan());
                    if (out.wsum) out.wsum[at] = v[u].wsum;
                    if (out.n) out.n[at] = v[u].n;
                }
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

template <typename T, int KX, bool STAGED>
hipError_t rg_launch(const RgIn<T>& in, const RgOut<T>& out, size_t lds_bytes, hipStream_t stream) {
    const dim3 grid(static_cast<unsigned>(regrid_tiles_x(in.mx) * in.my), static_cast<unsigned>(stage_blocks(in.nt, in.per)));
    hipLaunchKernelGGL((regrid_steps<T, KX, STAGED>), grid, dim3(kRgThreads), lds_bytes, stream, in, out);
    return hipGetLastError();
}

template <typename T, bool STAGED>
hipError_t rg_launch_kx(int32_t max_cols, const RgIn<T>& in, const RgOut<T>& out, size_t lds_bytes, hipStream_t stream) {
    if (max_cols <= 1) return rg_launch<T, 1, STAGED>(in, out, lds_bytes, stream);
    if (max_cols <= 2) return rg_launch<T, 2, STAGED>(in, out, lds_bytes, stream);
    if (max_cols <= 4) return rg_launch<T, 4, STAGED>(in, out, lds_bytes, stream);
    return rg_launch<T, 0, STAGED>(in, out, lds_bytes, stream);
}

template <typename T>
hipError_t launch_regrid(const T* ts, int64_t nt, int64_t ld, int32_t ny, int32_t nx, int32_t my, int32_t mx,
                         const int32_t* table_dev, const RegridLayout& lay, int32_t max_rows, int32_t max_cols,
                         int32_t max_width, int32_t periodic, double x0, int32_t a, int32_t variant, int64_t chunk_steps,
                         T* out, int64_t ldo, int64_t* wsum, int32_t* n, int64_t* n_range, hipStream_t stream) {
    if (nt <= 0 || my <= 0 || mx <= 0) return hipSuccess;
    if (ny < 1 || nx < 1 || static_cast<int64_t>(ny) * nx > INT32_MAX || static_cast<int64_t>(my) * mx > INT32_MAX ||
        max_rows < 0 || max_rows > kRegridMaxRun || max_cols < 0 || max_cols > kRegridMaxRun || !table_dev)
        return hipErrorInvalidValue;
    const int32_t klass = regrid_class(max_rows, max_width, mx < kRegridTile ? mx : kRegridTile, nx, periodic != 0, variant);
    if (klass == kRegridNone) return hipErrorInvalidValue;
    const int64_t workgroups = regrid_tiles_x(mx) * my;
    const int64_t work = static_cast<int64_t>(max_rows > 0 ? max_rows : 1) * (max_cols > 0 ? max_cols : 1);
    int64_t per = chunk_steps > 0 ? chunk_steps : regrid_auto_chunk(nt, workgroups, work);
    per = per < nt ? per : nt;
    const RgIn<T> in{ts, ld, nt, per, ny, nx, my, mx,
                     table_dev + lay.row_first, table_dev + lay.row_ptr, table_dev + lay.ay, table_dev + lay.wy,
                     table_dev + lay.col_first, table_dev + lay.col_ptr, table_dev + lay.ax, table_dev + lay.wx,
                     table_dev + lay.tile_c0, table_dev + lay.tile_w, periodic, x0, a};
    const RgOut<T> o{out, ldo, wsum, n, reinterpret_cast<u64*>(n_range)};
    if (klass == kRegridStaged)
        return rg_launch_kx<T, true>(max_cols, in, o, sizeof(int32_t) * static_cast<size_t>(max_rows) * static_cast<size_t>(max_width),
                                     stream);
    return rg_launch_kx<T, false>(max_cols, in, o, 0, stream);
}

}  // namespace

}  // namespace xmhw

// ---- the C entries of regrid() (include/xmhw_amd.h) -------------------------------------------------------------------
namespace {

using namespace xmhw::entry;

static std::atomic<int> g_regrid_variant{0};       // the path regrid() takes, 0 = automatic (xmhw_set_regrid_variant)
static std::atomic<int> g_regrid_chunk{0};         // steps a workgroup takes per chunk, 0 = automatic (xmhw_set_regrid_chunk)

static_assert(XMHW_REGRID_MAX_RUN == xmhw::kRegridMaxRun && XMHW_REGRID_MAX_WEIGHT == xmhw::kRegridMaxWeight &&
                  XMHW_REGRID_MAX_EXTENT == xmhw::kRegridMaxExtent && XMHW_REGION_SERIES_BITS == xmhw::kRegridBits,
              "the public limits of regrid() are the kernel's");

// one axis of a regrid() call: m destination runs over n source points
struct RegridAxis {
    const int32_t *first, *ptr, *w, *full;
    int32_t m, n;
    bool periodic;
    const char* name;
};
// can the tables be read as CSR tables: all there, the pointers from 0 and non-decreasing?
bool regrid_axis_readable(const RegridAxis& x) {
    if (x.m < 0) return false;
    if (x.m == 0) return true;
    if (!x.first || !x.ptr || !x.full || x.ptr[0] != 0) return false;
    for (int32_t k = 0; k < x.m; ++k)
        if (x.ptr[k + 1] < x.ptr[k]) return false;
    return x.ptr[x.m] == 0 || x.w;
}
// the caps of an axis (of tables that can be read): "" or what is above them
std::string regrid_axis_cap(const RegridAxis& x) {
    if (!regrid_axis_readable(x)) return "";
    for (int32_t k = 0; k < x.m; ++k) {
        if (x.ptr[k + 1] - x.ptr[k] > xmhw::kRegridMaxRun)
            return std::string("regrid: a ") + x.name + " run of more than " + std::to_string(xmhw::kRegridMaxRun) + " entries";
        if (x.full[k] > xmhw::kRegridMaxExtent) return std::string("regrid: a ") + x.name + " extent above 2^18";
    }
    for (int32_t e = 0; e < x.ptr[x.m]; ++e)
        if (x.w[e] > xmhw::kRegridMaxWeight) return std::string("regrid: a ") + x.name + " weight above 2^12";
    return "";
}
// the shape of an axis: "" or what is malformed
std::string regrid_axis_bad(const RegridAxis& x) {
    if (!regrid_axis_readable(x)) return std::string("regrid: bad ") + x.name + " tables (NULL, or pointers not from 0 and non-decreasing)";
    for (int32_t k = 0; k < x.m; ++k) {
        const int64_t cnt = x.ptr[k + 1] - x.ptr[k];
        int64_t sum = 0;
        for (int32_t e = x.ptr[k]; e < x.ptr[k + 1]; ++e) {
            if (x.w[e] < 0) return std::string("regrid: a negative ") + x.name + " weight";
            sum += x.w[e];
        }
        if (sum > x.full[k]) return std::string("regrid: the ") + x.name + " weights of a run exceed its extent";
        const int64_t first = x.first[k];
        const bool inside = x.periodic ? first >= 0 && first < x.n && cnt <= x.n : first >= 0 && first + cnt <= x.n;
        if (cnt > 0 && !inside) return std::string("regrid: a ") + x.name + " run leaves the source grid";
    }
    return "";
}

template <typename T>
int regrid(const T* ts, int64_t nt, int64_t ld, int32_t ny, int32_t nx, int32_t my, int32_t mx, const int32_t* row_first,
           const int32_t* row_ptr, const int32_t* ay, const int32_t* wy, const int32_t* col_first, const int32_t* col_ptr,
           const int32_t* ax, const int32_t* wx, int32_t periodic, double x0, int32_t a, T* out, int64_t ldo, int64_t* wsum,
           int32_t* n, int64_t* n_range, void* stream) {
    const RegridAxis rows{row_first, row_ptr, ay, wy, my, ny, false, "row"};
    const RegridAxis cols{col_first, col_ptr, ax, wx, mx, nx, periodic != 0, "column"};
    // the caps, over the tables that can be read
    for (const RegridAxis* x : {&rows, &cols}) {
        const std::string cap = regrid_axis_cap(*x);
        if (!cap.empty()) return fail(XMHW_ERR_UNSUPPORTED, cap);
    }
    if ((ny > 0 && nx > 0 && static_cast<int64_t>(ny) * nx > INT32_MAX) || (my > 0 && mx > 0 && static_cast<int64_t>(my) * mx > INT32_MAX))
        return fail(XMHW_ERR_UNSUPPORTED, "regrid: a grid of 2^31 points and more");
    if (nt < 0 || ny < 0 || nx < 0 || ld < static_cast<int64_t>(ny) * nx) return fail(XMHW_ERR_INVALID, "bad nt/ny/nx/ld");
    if (my < 0 || mx < 0 || ldo < static_cast<int64_t>(my) * mx) return fail(XMHW_ERR_INVALID, "bad my/mx/ldo");
    for (const RegridAxis* x : {&rows, &cols}) {
        const std::string bad = regrid_axis_bad(*x);
        if (!bad.empty()) return fail(XMHW_ERR_INVALID, bad);
    }
    if (a < 0 || a > 65536) return fail(XMHW_ERR_INVALID, "regrid: a must be in [0, 65536]");
    if (!std::isfinite(x0)) return fail(XMHW_ERR_INVALID, "regrid: x0 must be finite");
    if (nt == 0 || my == 0 || mx == 0) return XMHW_OK;
    if (!ts || !out || !n_range) return fail(XMHW_ERR_INVALID, "NULL buffer");
    // the ten tables as one: one upload, one cache slot, reused by the time blocks of a call
    const xmhw::RegridLayout lay = xmhw::regrid_layout(my, mx, row_ptr[my], col_ptr[mx]);
    std::vector<int32_t> packed(static_cast<size_t>(lay.total), 0);
    const auto put = [&](int64_t at, const int32_t* src, int64_t count) {
        if (count > 0) std::memcpy(packed.data() + at, src, sizeof(int32_t) * static_cast<size_t>(count));
    };
    put(lay.row_first, row_first, my);
    put(lay.row_ptr, row_ptr, static_cast<int64_t>(my) + 1);
    put(lay.ay, ay, row_ptr[my]);
    put(lay.wy, wy, my);
    put(lay.col_first, col_first, mx);
    put(lay.col_ptr, col_ptr, static_cast<int64_t>(mx) + 1);
    put(lay.ax, ax, col_ptr[mx]);
    put(lay.wx, wx, mx);
    int32_t max_width = 0;
    for (int32_t I0 = 0; I0 < mx; I0 += xmhw::kRegridTile) {
        const xmhw::RegridSpan sp = xmhw::regrid_tile_span(col_first, col_ptr, mx, nx, periodic != 0, I0);
        packed[static_cast<size_t>(lay.tile_c0 + I0 / xmhw::kRegridTile)] = sp.c0;
        packed[static_cast<size_t>(lay.tile_w + I0 / xmhw::kRegridTile)] = sp.width;
        max_width = std::max(max_width, sp.width);
    }
    RowsRef table;
    if (int rc = upload_table(packed.data(), lay.total, "overlap table upload", &table)) return rc;
    return status_of(xmhw::launch_regrid<T>(ts, nt, ld, ny, nx, my, mx, table->d_rows, lay, xmhw::regrid_max_run(row_ptr, my),
                                            xmhw::regrid_max_run(col_ptr, mx), max_width, periodic != 0, x0, a,
                                            g_regrid_variant.load(), g_regrid_chunk.load(), out, ldo, wsum, n, n_range,
                                            static_cast<hipStream_t>(stream)),
                     "regrid launch");
}

}  // namespace

extern "C" {

int xmhw_set_regrid_variant(int32_t variant) {
    if (variant < xmhw::kRegridVariantAuto || variant > xmhw::kRegridVariantStaged)
        return fail(XMHW_ERR_INVALID, "variant must be 0, 1 or 2");
    g_regrid_variant = variant;
    return XMHW_OK;
}
int xmhw_set_regrid_chunk(int32_t steps) { return set_knob(g_regrid_chunk, steps, "steps must be >= 0"); }
int xmhw_regrid_class(int32_t nx, int32_t my, int32_t mx, const int32_t* row_ptr, const int32_t* col_first, const int32_t* col_ptr,
                      int32_t periodic) {
    const RegridAxis rows{nullptr, row_ptr, nullptr, nullptr, my, 0, false, "row"};
    const RegridAxis cols{col_first, col_ptr, nullptr, nullptr, mx, nx, periodic != 0, "column"};
    // (the pointer tables alone: first, weights and extents are not read for the row axis)
    if (my < 0 || mx < 0 || nx < 1 || (my > 0 && !row_ptr) || (mx > 0 && (!col_ptr || !col_first))) return xmhw::kRegridNone;
    for (const RegridAxis* x : {&rows, &cols})
        for (int32_t k = 0; k < x->m; ++k)
            if (x->ptr[k + 1] < x->ptr[k] || x->ptr[k + 1] - x->ptr[k] > xmhw::kRegridMaxRun) return xmhw::kRegridNone;
    for (int32_t I = 0; I < mx; ++I) {
        const int64_t cnt = col_ptr[I + 1] - col_ptr[I], first = col_first[I];
        if (cnt > 0 && !(periodic ? first >= 0 && first < nx && cnt <= nx : first >= 0 && first + cnt <= nx)) return xmhw::kRegridNone;
    }
    return xmhw::regrid_class(xmhw::regrid_max_run(row_ptr, my), xmhw::regrid_max_width(col_first, col_ptr, mx, nx, periodic != 0),
                              mx < xmhw::kRegridTile ? mx : xmhw::kRegridTile, nx, periodic != 0, g_regrid_variant.load());
}
int xmhw_regrid_f32(const float* ts, int64_t nt, int64_t ld, int32_t ny, int32_t nx, int32_t my, int32_t mx,
                    const int32_t* row_first, const int32_t* row_ptr, const int32_t* ay, const int32_t* wy,
                    const int32_t* col_first, const int32_t* col_ptr, const int32_t* ax, const int32_t* wx, int32_t periodic,
                    double x0, int32_t a, float* out, int64_t ldo, int64_t* wsum, int32_t* n, int64_t* n_range, void* stream) {
    return regrid<float>(ts, nt, ld, ny, nx, my, mx, row_first, row_ptr, ay, wy, col_first, col_ptr, ax, wx, periodic, x0, a, out,
                         ldo, wsum, n, n_range, stream);
}
int xmhw_regrid_f64(const double* ts, int64_t nt, int64_t ld, int32_t ny, int32_t nx, int32_t my, int32_t mx,
                    const int32_t* row_first, const int32_t* row_ptr, const int32_t* ay, const int32_t* wy,
                    const int32_t* col_first, const int32_t* col_ptr, const int32_t* ax, const int32_t* wx, int32_t periodic,
                    double x0, int32_t a, double* out, int64_t ldo, int64_t* wsum, int32_t* n, int64_t* n_range, void* stream) {
    return regrid<double>(ts, nt, ld, ny, nx, my, mx, row_first, row_ptr, ay, wy, col_first, col_ptr, ax, wx, periodic, x0, a, out,
                          ldo, wsum, n, n_range, stream);
}

}  // extern "C"
