// kernels_spatialcorr.hip -- spatial_correlation(): per-cell correlation sums with grid neighbours.  The
// definition is in include/xmhw_amd.h, "spatial_correlation()"; in short, with a(t, p) the scaled anomaly of grid point p
// at step t, valid as fixed_state() says, and q its fixed-point integer: for every point p = (j, i), every step t of class
// k >= 0 and every offset e = (dj, di) whose partner p' = (j + dj, i + di) lies in the grid (the column wraps across a
// periodic seam) with a(t, p) and a(t, p') both valid, the six sums n, sx, sy, sxx, syy, sxy at [k][e][p] over the pairs
// (q(t, p), q(t, p')).
//
//   spatial_corr_accumulate<T, ROWS, G>
//                     the frame of a class reduction (kernels.h) on the UNCOMPACTED grid: a workgroup owns a tile of ROWS
//                     (8; 4 for measurements) grid rows x 64 longitudes (a wave = 64 consecutive longitudes of one row), walks a block of steps
//                     and takes a group of G offsets (grid.z); the 11 registers of addends per offset of the current class
//                     are flushed by integer atomics without a return value when the class changes and at the end of the
//                     block, non-zero addends only.  G = 8 serves up to 8 offsets, G = 16 more (stage_blocks.h).
//   the tile          halo_tile.h: the tile plus the halo the GROUP's offsets reach (their bounding box, not the cap of
//                     32 points), one dword per point.  Three LDS arrays over its slots: the grid point of the slot (-1
//                     outside the grid; wrapped across a periodic seam), written once per workgroup; the base of the slot
//                     as float64 where the base is one row (read once, for the halo points too); and q of the current step.
//   a step            every slot is converted once, slot s by lane s mod the workgroup: sample and base -> q, or one of two
//                     sentinels below -2^23 (not a sample: NaN, land, outside the grid; out of range).  The samples of a
//                     lane's first kScAhead slots are requested one labelled step ahead, into registers, so that they
//                     travel across the barriers and the sums of the step before; a box with more slots than that reads
//                     the rest as it converts them.  One barrier; then a lane reads its own dword
//                     (qx, its validity, its range state) and, per offset, one dword at a wave-uniform distance from its
//                     own: 64 consecutive dwords per wave, the bank is the lane.  The validity of a pair is a gate of
//                     all ones or zero -- no branch --: three v_mad_i64_i32 (sxx, syy, sxy), two 64-bit adds, a few
//                     32-bit operations, as in kernels_lagcorr.hip.
//   the next step     a SECOND BARRIER after the reads protects the tile: one q array instead of two keeps the LDS of
//                     the largest box (72 x 128 slots) at 144 KB with the point and base arrays, inside the 160 KB of a
//                     CU, and at the default offsets (16 x 72 slots, 18 KB) the registers decide how many workgroups
//                     share a CU either way; the barrier joins eight (or four) waves that have just done the same work.
//   steps of class -1 are not read: the label is uniform over the workgroup, so every wave skips the same barriers.
//   the counter       the lanes of offset group 0 count the out-of-range samples of their OWN point, each once.
#include "../../include/xmhw_amd.h"
#include "entry_common.h"
#include "stage_reduce.h"
#include "halo_tile.h"

namespace xmhw {

// What the stage computes (halo_tile.h holds the tile): per grid point of the UNCOMPACTED ny x nx grid, class of the
// step and offset e = (dj, di) of the table djdi[D][2], the sums over the pairs (q(t, p), q(t, p + e)) of one step whose two
// anomalies are valid -- n int32, sx, sy, sxx, syy, sxy int64, [K][D][ldo], ADDED; the definition is in
// include/xmhw_amd.h, "spatial_correlation()".  ts is row t0 of the series, the block t0 .. t0 + nt - 1; row_of_t and
// class_of_t are DEVICE arrays over all T steps here; the offsets come twice, padded with (0, 0) to whole groups
// (spatial_corr_group): djdi_dev for the kernel, djdi_host for the size of its LDS tile.  *n_range counts the samples of a
// class >= 0 that are not NaN and out of range, each once.  tile_rows: kSpatialCorrRows or kSpatialCorrShortRows grid rows per
// workgroup; block_steps: the steps a workgroup takes per block, 0 = automatic; same results for every value of either.
constexpr int kSpatialCorrMaxOffsets = 64;
constexpr int kSpatialCorrReach = 32;                // |dj|, |di| at most
constexpr int kSpatialCorrMaxClasses = 64;
constexpr int kSpatialCorrMaxSteps = 1 << 17;        // T below it: 2^17 * 2^46 = 2^63
constexpr int kSpatialCorrMaxAxis = 32767;
constexpr int kSpatialCorrBits = 16;
constexpr int kSpatialCorrRangeBits = 7;
constexpr int kSpatialCorrMaxShift = 24;
constexpr int kSpatialCorrRows = 8;                  // the tile: 8 rows x 64 longitudes, 512 lanes
constexpr int kSpatialCorrShortRows = 4;             // ... or 4 x 64, 256 lanes (measurements: the slower of the two)

static_assert(kSpatialCorrBits == kFixedBits && kSpatialCorrRangeBits == kFixedRangeBits, "one scale for every stage");
static_assert(kSpatialCorrReach == kHaloReach, "the halo box clamps at the public reach");

namespace {

using u64 = unsigned long long;

constexpr int32_t kScNoSample = INT32_MIN;           // NaN, land, outside the grid
constexpr int32_t kScOutOfRange = INT32_MIN + 1;     // not NaN and |a| >= 2^7
constexpr int32_t kScLeast = -(1 << 24);             // every q lies above it, both sentinels below
constexpr int kScAhead = 4;                          // slots per lane whose samples are requested a step ahead

template <typename T>
struct ScIn {
    const T* ts;                                     // row t0 of the series: [nt][ld]
    int64_t ld;
    const double* base;                              // [Dr][ldb]
    int64_t ldb;
    const int32_t* row_of_t;                         // [T], by absolute step
    const int32_t* class_of_t;
    int32_t one_row;
    double scale;                                    // 2^-shift
    int32_t t0, nt;
    int32_t ny, nx, periodic;
    const int32_t* djdi;                             // [groups * G][2], padded with (0, 0)
    int32_t D, K;
    int32_t slots;                                   // the slots of each LDS array
};

struct ScOut {
    int32_t* n;                                      // [K][D][ldo]
    u64 *sx, *sy, *sxx, *syy, *sxy;
    int64_t ldo;
    u64* n_range;
};

template <int G>
struct ScAcc {
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
__device__ __forceinline__ void sc_flush(const ScOut& o, int32_t k, int64_t p, int32_t e0, int32_t D, ScAcc<G>& v) {
    if (p >= 0) {
#pragma unroll
        for (int j = 0; j < G; ++j) {
            if (e0 + j >= D || v.n[j] == 0) continue;    // no pair, no addend: an invalid pair holds zeros
            const int64_t at = (static_cast<int64_t>(k) * D + e0 + j) * o.ldo + p;
            atomicAdd(o.n + at, v.n[j]);
            if (v.sx[j]) atomicAdd(o.sx + at, static_cast<u64>(v.sx[j]));
            if (v.sy[j]) atomicAdd(o.sy + at, static_cast<u64>(v.sy[j]));
            if (v.sxx[j]) atomicAdd(o.sxx + at, static_cast<u64>(v.sxx[j]));
            if (v.syy[j]) atomicAdd(o.syy + at, static_cast<u64>(v.syy[j]));
            if (v.sxy[j]) atomicAdd(o.sxy + at, static_cast<u64>(v.sxy[j]));
        }
    }
    v.clear();
}

template <typename T, int ROWS, int G>
__global__ __launch_bounds__(ROWS * kHaloCols) void spatial_corr_accumulate(ScIn<T> in, int64_t tb, ScOut out) {
    extern __shared__ __attribute__((aligned(8))) unsigned char sc_lds[];
    // [slots] float64 bases (one-row base only), [slots] int32 grid points, [slots] int32 q
    double* const base_of = reinterpret_cast<double*>(sc_lds);
    int32_t* const point_of = reinterpret_cast<int32_t*>(sc_lds + (in.one_row ? sizeof(double) * in.slots : 0));
    int32_t* const tile = point_of + in.slots;
    const int32_t rr = threadIdx.x / kHaloCols, cc = threadIdx.x % kHaloCols;     // the wave is the tile row
    const int32_t e0 = static_cast<int32_t>(blockIdx.z) * G;
    int32_t j0 = 0, i0 = 0;
    if (!halo_origin(blockIdx.x, in.ny, in.nx, ROWS, &j0, &i0)) return;          // (uniform: before every barrier)
    const HaloBox box = halo_box(in.djdi + 2 * e0, G);
    const int32_t H = halo_height(box, ROWS), W = halo_width(box);
    if (H * W > in.slots) return;                    // (uniform) never: the launcher sized the arrays by the same rule
    // what the lane owns and where it reads
    const int64_t own = halo_own_point(ROWS, j0, i0, rr, cc, in.ny, in.nx);
    const int32_t own_slot = halo_read_slot(box, ROWS, rr, cc, 0, 0);            // >= 0: the box holds (0, 0)
    int32_t delta[G];                                // wave-uniform: the partner's slot minus the lane's own
    uint32_t alive = 0;                              // the offsets of the group that lie in the box (all of them)
#pragma unroll
    for (int j = 0; j < G; ++j) {
        const int32_t dj = in.djdi[2 * (e0 + j)], di = in.djdi[2 * (e0 + j) + 1];
        const int32_t s = halo_read_slot(box, ROWS, rr, cc, dj, di);
        delta[j] = s >= 0 ? s - own_slot : 0;
        alive |= (s >= 0 && e0 + j < in.D ? 1u : 0u) << j;
    }
    // the grid point of every slot, once; and the one-row base
    for (int32_t r = rr; r < H; r += ROWS)
        for (int32_t c = cc; c < W; c += kHaloCols) {
            const int32_t s = halo_slot(box, ROWS, r, c);
            const int64_t p = halo_point(box, ROWS, j0, i0, r, c, in.ny, in.nx, in.periodic != 0);
            point_of[s] = static_cast<int32_t>(p);   // ny, nx <= 32767: below 2^30
            if (in.one_row) base_of[s] = p >= 0 ? in.base[p] : 0.0;
        }
    const bool counts = blockIdx.z == 0 && own >= 0;
    const int32_t bs = static_cast<int32_t>(tb < in.nt ? tb : in.nt);
    const int32_t nblk = (in.nt - 1) / bs + 1;
    const int32_t HW = H * W;                        // <= in.slots: every slot index below lies inside the three arrays
    constexpr int32_t NT = ROWS * kHaloCols;
    ScAcc<G> v;
    v.clear();
    u64 range = 0;
    const auto flush_class = [&](int32_t k) { sc_flush<G>(out, k, own, e0, in.D, v); };
    const auto label = [&](int32_t tl) -> int32_t {
        const int32_t k = in.class_of_t[in.t0 + tl];
        return k < in.K ? k : -1;                    // (labels are checked on the host)
    };
    // the next step of the block at or after tl whose class counts (uniform over the workgroup), or b1
    const auto labelled_from = [&](int32_t tl, int32_t b1) -> int32_t {
        while (tl < b1 && label(tl) < 0) ++tl;
        return tl;
    };
    // the slots tid, tid + NT, ... of the tile are the lane's to convert; the first kScAhead of them are requested a
    // step ahead, into registers
    T ahead[kScAhead];
    double ahead_base[kScAhead];
    const auto request = [&](int32_t tl) {
        const T* const row = in.ts + static_cast<int64_t>(tl) * in.ld;
        const double* const brow = in.one_row ? nullptr : in.base + static_cast<int64_t>(in.row_of_t[in.t0 + tl]) * in.ldb;
#pragma unroll
        for (int i = 0; i < kScAhead; ++i) {
            const int32_t s = static_cast<int32_t>(threadIdx.x) + i * NT;
            const int32_t p = s < HW ? point_of[s] : -1;
            if (p >= 0) {
                ahead[i] = row[p];
                if (!in.one_row) ahead_base[i] = brow[p];
            }
        }
    };
    const auto encode = [&](double a) -> int32_t {
        const int state = fixed_state(a);
        return state > 0 ? static_cast<int32_t>(fixed_value(a)) : state < 0 ? kScOutOfRange : kScNoSample;
    };
    __syncthreads();                                 // the point and base arrays are written
    for (int32_t blk = blockIdx.y; blk < nblk; blk += gridDim.y) {
        const auto [b0, b1] = block_range<int32_t>(blk, bs, in.nt);
        ClassRun run;
        int32_t tl = labelled_from(b0, b1);          // steps of class -1 are not read
        if (tl < b1) request(tl);
        while (tl < b1) {
            run.enter(label(tl), flush_class);
            // every slot once: sample and base -> q or a sentinel
#pragma unroll
            for (int i = 0; i < kScAhead; ++i) {
                const int32_t s = static_cast<int32_t>(threadIdx.x) + i * NT;
                if (s < HW)
                    tile[s] = point_of[s] >= 0 ? encode((static_cast<double>(ahead[i]) - (in.one_row ? base_of[s] : ahead_base[i])) * in.scale)
                                               : kScNoSample;
            }
            if (HW > kScAhead * NT) {                // a box that wide: the rest of the slots as they come
                const T* const row = in.ts + static_cast<int64_t>(tl) * in.ld;
                const double* const brow = in.one_row ? nullptr : in.base + static_cast<int64_t>(in.row_of_t[in.t0 + tl]) * in.ldb;
                for (int32_t s = static_cast<int32_t>(threadIdx.x) + kScAhead * NT; s < HW; s += NT) {
                    const int32_t p = point_of[s];
                    tile[s] = p >= 0 ? encode((static_cast<double>(row[p]) - (in.one_row ? base_of[s] : brow[p])) * in.scale) : kScNoSample;
                }
            }
            const int32_t next = labelled_from(tl + 1, b1);
            if (next < b1) request(next);            // in flight across the barriers and the sums of this step
            __syncthreads();                         // the tile of step tl is written
            const int32_t mine = tile[own_slot];
            const int32_t gate_x = own >= 0 && mine > kScLeast ? -1 : 0;
            const int32_t qx = mine & gate_x;
            if (counts && mine == kScOutOfRange) ++range;
#pragma unroll
            for (int j = 0; j < G; ++j) {
                const int32_t theirs = tile[own_slot + delta[j]];
                const int32_t gate = (theirs > kScLeast && ((alive >> j) & 1u) ? -1 : 0) & gate_x;   // all ones iff the pair is valid
                const int32_t qxg = qx & gate, qy = theirs & gate;
                v.n[j] -= gate;
                v.sx[j] += qxg;
                v.sxx[j] += static_cast<int64_t>(qxg) * qxg;
                v.sy[j] += qy;
                v.syy[j] += static_cast<int64_t>(qy) * qy;
                v.sxy[j] += static_cast<int64_t>(qxg) * qy;
            }
            __syncthreads();                         // ... and read: the next step may overwrite it
            tl = next;
        }
        run.leave(flush_class);
    }
    if (range) atomicAdd(out.n_range, range);
}

// the LDS bytes of a launch: the largest box of the groups
template <int ROWS>
size_t sc_lds_layout(const int32_t* djdi_host, int32_t groups, int32_t G, bool one_row, int32_t* slots) {
    int32_t most = 0;
    for (int32_t g = 0; g < groups; ++g) {
        const int32_t s = halo_slots(halo_box(djdi_host + 2 * g * G, G), ROWS);
        most = s > most ? s : most;
    }
    *slots = most;
    return static_cast<size_t>(most) * (2 * sizeof(int32_t) + (one_row ? sizeof(double) : 0));
}

template <typename T, int ROWS, int G>
hipError_t sc_launch(ScIn<T> in, const int32_t* djdi_host, int32_t groups, int64_t block_steps, const ScOut& out,
                     hipStream_t stream) {
    const size_t lds = sc_lds_layout<ROWS>(djdi_host, groups, G, in.one_row != 0, &in.slots);
    if (lds > (size_t{64} << 10)) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&spatial_corr_accumulate<T, ROWS, G>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds));
        if (e != hipSuccess) return e;
    }
    const int64_t tiles = halo_tiles_x(in.nx) * halo_tiles_y(in.ny, ROWS);
    const int64_t tb = block_steps > 0 ? block_steps : spatial_corr_auto_block(in.nt, in.ny, in.nx, ROWS, in.D);
    const dim3 grid(static_cast<unsigned>(tiles), static_cast<unsigned>(stage_blocks(in.nt, tb)), static_cast<unsigned>(groups));
    hipLaunchKernelGGL((spatial_corr_accumulate<T, ROWS, G>), grid, dim3(ROWS * kHaloCols), lds, stream, in, tb, out);
    return hipGetLastError();
}

hipError_t launch_spatial_corr_init(int32_t K, int32_t D, int64_t N, int32_t* n, int64_t* sx, int64_t* sy, int64_t* sxx,
                                    int64_t* syy, int64_t* sxy, int64_t ldo, int64_t* n_range, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(n_range, 0, sizeof(int64_t), stream);
    const int64_t rows = static_cast<int64_t>(K) * D;
    if (e == hipSuccess) e = zero_rows(n, sizeof(int32_t), rows, N, ldo, stream);
    for (int64_t* p : {sx, sy, sxx, syy, sxy})
        if (e == hipSuccess) e = zero_rows(p, sizeof(int64_t), rows, N, ldo, stream);
    return e;
}

template <typename T>
hipError_t launch_spatial_corr_accumulate(const T* ts, int64_t ld, int64_t t0, int64_t nt, int32_t ny, int32_t nx,
                                          bool periodic, const double* base, int64_t ldb, int64_t Dr, const int32_t* row_of_t,
                                          int32_t shift, const int32_t* class_of_t, int32_t K, const int32_t* djdi_dev,
                                          const int32_t* djdi_host, int32_t D, int32_t tile_rows, int64_t block_steps,
                                          int32_t* n, int64_t* sx, int64_t* sy, int64_t* sxx, int64_t* syy, int64_t* sxy,
                                          int64_t ldo, int64_t* n_range, hipStream_t stream) {
    if (nt <= 0 || ny <= 0 || nx <= 0 || K <= 0) return hipSuccess;
    if (D < 1 || D > kSpatialCorrMaxOffsets || shift < 0 || shift > kSpatialCorrMaxShift || t0 < 0 ||
        t0 + nt > kSpatialCorrMaxSteps || ny > kSpatialCorrMaxAxis || nx > kSpatialCorrMaxAxis)
        return hipErrorInvalidValue;
    const int32_t G = static_cast<int32_t>(spatial_corr_group(D)), groups = static_cast<int32_t>(spatial_corr_groups(D));
    const ScIn<T> in{ts, ld, base, ldb, row_of_t, class_of_t, Dr == 1, ldexp(1.0, -shift), static_cast<int32_t>(t0),
                     static_cast<int32_t>(nt), ny, nx, periodic ? 1 : 0, djdi_dev, D, K, 0};
    const auto u = [](int64_t* p) { return reinterpret_cast<u64*>(p); };
    const ScOut out{n, u(sx), u(sy), u(sxx), u(syy), u(sxy), ldo, u(n_range)};
    const bool small = tile_rows == kSpatialCorrShortRows;
    if (G == kSpatialCorrGroup)
        return small ? sc_launch<T, kSpatialCorrShortRows, kSpatialCorrGroup>(in, djdi_host, groups, block_steps, out, stream)
                     : sc_launch<T, kSpatialCorrRows, kSpatialCorrGroup>(in, djdi_host, groups, block_steps, out, stream);
    return small ? sc_launch<T, kSpatialCorrShortRows, kSpatialCorrWideGroup>(in, djdi_host, groups, block_steps, out, stream)
                 : sc_launch<T, kSpatialCorrRows, kSpatialCorrWideGroup>(in, djdi_host, groups, block_steps, out, stream);
}

}  // namespace

}  // namespace xmhw

// ---- the C entries of spatial_correlation() (include/xmhw_amd.h) ------------------------------------------------------
namespace {

using namespace xmhw::entry;

static std::atomic<int> g_spatial_corr_block{0};   // steps a workgroup takes per block, 0 = automatic (xmhw_set_spatial_corr_block)
static std::atomic<int> g_spatial_corr_tile{0};    // grid rows of a tile, 0 = the default (xmhw_set_spatial_corr_tile)

static_assert(XMHW_SPATIAL_CORR_MAX_OFFSETS == xmhw::kSpatialCorrMaxOffsets && XMHW_SPATIAL_CORR_REACH == xmhw::kSpatialCorrReach &&
                  XMHW_SPATIAL_CORR_MAX_CLASSES == xmhw::kSpatialCorrMaxClasses &&
                  XMHW_SPATIAL_CORR_MAX_STEPS == xmhw::kSpatialCorrMaxSteps &&
                  XMHW_SPATIAL_CORR_MAX_AXIS == xmhw::kSpatialCorrMaxAxis && XMHW_SPATIAL_CORR_BITS == xmhw::kSpatialCorrBits &&
                  XMHW_SPATIAL_CORR_RANGE_BITS == xmhw::kSpatialCorrRangeBits &&
                  XMHW_SPATIAL_CORR_MAX_SHIFT == xmhw::kSpatialCorrMaxShift,
              "the public limits of spatial_correlation() are the kernel's");

static int spatial_corr_check_shape(int32_t K, int32_t D, int32_t shift, int64_t Tn, int32_t ny, int32_t nx) {
    if (K < 1 || K > xmhw::kSpatialCorrMaxClasses)
        return fail(XMHW_ERR_UNSUPPORTED,
                    "spatial_corr: K must be in [1, " + std::to_string(xmhw::kSpatialCorrMaxClasses) + "]");
    if (D < 1 || D > xmhw::kSpatialCorrMaxOffsets)
        return fail(XMHW_ERR_UNSUPPORTED,
                    "spatial_corr: D must be in [1, " + std::to_string(xmhw::kSpatialCorrMaxOffsets) + "]");
    if (shift < 0 || shift > xmhw::kSpatialCorrMaxShift)
        return fail(XMHW_ERR_UNSUPPORTED,
                    "spatial_corr: shift must be in [0, " + std::to_string(xmhw::kSpatialCorrMaxShift) + "]");
    if (Tn >= xmhw::kSpatialCorrMaxSteps) return fail(XMHW_ERR_UNSUPPORTED, "spatial_corr: 2^17 steps and more");
    if (ny > xmhw::kSpatialCorrMaxAxis || nx > xmhw::kSpatialCorrMaxAxis)
        return fail(XMHW_ERR_UNSUPPORTED, "spatial_corr: a grid axis of 2^15 points and more");
    return XMHW_OK;
}

template <typename T>
int spatial_corr_accumulate(const T* ts, int64_t ld, int64_t t0, int64_t nt, int64_t Tn, int32_t ny, int32_t nx,
                            int32_t periodic, const double* base, int64_t ldb, int64_t Dr, const int32_t* row_of_t,
                            int32_t shift, const int32_t* class_of_t, int32_t K, const int32_t* offsets, int32_t D, int32_t* n,
                            int64_t* sx, int64_t* sy, int64_t* sxx, int64_t* syy, int64_t* sxy, int64_t ldo, int64_t* n_range,
                            void* stream) {
    if (spatial_corr_check_shape(K, D, shift, Tn, ny, nx) != XMHW_OK) return XMHW_ERR_UNSUPPORTED;
    if (offsets)
        for (int32_t e = 0; e < 2 * D; ++e)
            if (offsets[e] < -xmhw::kSpatialCorrReach || offsets[e] > xmhw::kSpatialCorrReach)
                return fail(XMHW_ERR_UNSUPPORTED,
                            "spatial_corr: offsets reach at most " + std::to_string(xmhw::kSpatialCorrReach) + " points");
    if (ny < 0 || nx < 0) return fail(XMHW_ERR_INVALID, "bad ny/nx");
    const int64_t N = static_cast<int64_t>(ny) * nx;
    if (Tn < 0 || t0 < 0 || nt < 0 || nt > Tn - t0) return fail(XMHW_ERR_INVALID, "bad T/t0/nt");
    if (ld < N || ldb < N || ldo < N || Dr < 1) return fail(XMHW_ERR_INVALID, "bad ld/ldb/ldo/Dr");
    if (!offsets || (Tn > 0 && (!class_of_t || !row_of_t))) return fail(XMHW_ERR_INVALID, "NULL host table");
    if (periodic)
        for (int32_t e = 0; e < D; ++e)
            if (nx > 0 && std::abs(offsets[2 * e + 1]) >= nx)
                return fail(XMHW_ERR_INVALID, "spatial_corr: |di| must be below nx on a periodic grid");
    if (int rc = check_labels(class_of_t, Tn, -1, K, kClassesOutside)) return rc;
    if (int rc = check_labels(row_of_t, Tn, 0, Dr, kRowsOutside)) return rc;
    if (nt == 0 || N == 0) return XMHW_OK;
    if (!ts || !base || !n || !sx || !sy || !sxx || !syy || !sxy || !n_range) return fail(XMHW_ERR_INVALID, "NULL buffer");
    RowsRef rows;
    if (int rc = upload_table(row_of_t, Tn, "row table upload", &rows)) return rc;
    RowsRef classes;                                   // the same content-keyed cache: one more int32[T] table
    if (int rc = upload_table(class_of_t, Tn, "class table upload", &classes)) return rc;
    // ... and the offsets, padded with (0, 0) to whole groups: int32[groups * G][2]
    const int64_t padded_n = xmhw::spatial_corr_groups(D) * xmhw::spatial_corr_group(D);
    std::vector<int32_t> padded(static_cast<size_t>(2 * padded_n), 0);
    std::copy(offsets, offsets + 2 * D, padded.begin());
    RowsRef table;
    if (int rc = upload_table(padded.data(), 2 * padded_n, "offset table upload", &table)) return rc;
    const int32_t tile = g_spatial_corr_tile.load();
    return status_of(xmhw::launch_spatial_corr_accumulate<T>(ts, ld, t0, nt, ny, nx, periodic != 0, base, ldb, Dr, rows->d_rows,
                                                             shift, classes->d_rows, K, table->d_rows, padded.data(), D,
                                                             tile ? tile : xmhw::kSpatialCorrRows, g_spatial_corr_block.load(),
                                                             n, sx, sy, sxx, syy, sxy, ldo, n_range,
                                                             static_cast<hipStream_t>(stream)),
                     "spatial_corr_accumulate launch");
}

}  // namespace

extern "C" {

int xmhw_set_spatial_corr_block(int32_t steps) { return set_knob(g_spatial_corr_block, steps, "steps must be >= 0"); }
int xmhw_set_spatial_corr_tile(int32_t rows) {
    if (rows != 0 && rows != xmhw::kSpatialCorrRows && rows != xmhw::kSpatialCorrShortRows)
        return fail(XMHW_ERR_INVALID, "rows must be 0, 4 or 8");
    g_spatial_corr_tile = rows;
    return XMHW_OK;
}
int xmhw_spatial_corr_init(int32_t K, int32_t D, int32_t ny, int32_t nx, int32_t* n, int64_t* sx, int64_t* sy, int64_t* sxx,
                           int64_t* syy, int64_t* sxy, int64_t ldo, int64_t* n_range, void* stream) {
    if (spatial_corr_check_shape(K, D, 0, 1, ny, nx) != XMHW_OK) return XMHW_ERR_UNSUPPORTED;
    if (ny < 0 || nx < 0 || ldo < static_cast<int64_t>(ny) * nx) return fail(XMHW_ERR_INVALID, "bad ny/nx/ldo");
    if (!n_range || (ny > 0 && nx > 0 && (!n || !sx || !sy || !sxx || !syy || !sxy)))
        return fail(XMHW_ERR_INVALID, "NULL output buffer");
    return status_of(xmhw::launch_spatial_corr_init(K, D, static_cast<int64_t>(ny) * nx, n, sx, sy, sxx, syy, sxy, ldo, n_range,
                                                    static_cast<hipStream_t>(stream)),
                     "spatial_corr_init");
}
int xmhw_spatial_corr_accumulate_f32(const float* ts, int64_t ld, int64_t t0, int64_t nt, int64_t T, int32_t ny, int32_t nx,
                                     int32_t periodic, const double* base, int64_t ldb, int64_t Dr, const int32_t* row_of_t,
                                     int32_t shift, const int32_t* class_of_t, int32_t K, const int32_t* offsets, int32_t D,
                                     int32_t* n, int64_t* sx, int64_t* sy, int64_t* sxx, int64_t* syy, int64_t* sxy,
                                     int64_t ldo, int64_t* n_range, void* stream) {
    return spatial_corr_accumulate<float>(ts, ld, t0, nt, T, ny, nx, periodic, base, ldb, Dr, row_of_t, shift, class_of_t, K,
                                          offsets, D, n, sx, sy, sxx, syy, sxy, ldo, n_range, stream);
}
int xmhw_spatial_corr_accumulate_f64(const double* ts, int64_t ld, int64_t t0, int64_t nt, int64_t T, int32_t ny, int32_t nx,
                                     int32_t periodic, const double* base, int64_t ldb, int64_t Dr, const int32_t* row_of_t,
                                     int32_t shift, const int32_t* class_of_t, int32_t K, const int32_t* offsets, int32_t D,
                                     int32_t* n, int64_t* sx, int64_t* sy, int64_t* sxx, int64_t* syy, int64_t* sxy,
                                     int64_t ldo, int64_t* n_range, void* stream) {
    return spatial_corr_accumulate<double>(ts, ld, t0, nt, T, ny, nx, periodic, base, ldb, Dr, row_of_t, shift, class_of_t, K,
                                           offsets, D, n, sx, sy, sxx, syy, sxy, ldo, n_range, stream);
}

}  // extern "C"
