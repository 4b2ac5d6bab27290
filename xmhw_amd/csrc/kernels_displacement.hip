// kernels_displacement.hip -- mhw_displacement(): the thermal displacement (Jacox et al. 2020) of every MHW cell-day:
// the distance from a grid point in an event to the nearest grid point whose sample of that day is no warmer than the
// event point's own climatology.  The first stage whose cells look at the field around them: a data-dependent search
// over the resident grid, one day at a time.
//
// The grid is (ny, nx), longitude the fast axis, point p = j * nx + i.  A SOURCE is a point-day (p, t) whose compact cell
// c = cell_of_point[p] is >= 0, whose basin label is not negative and whose bit t is set in the in-event bitmap inev
// (event_table_bits: some table row of c has start <= t <= end).  Its target is g = seas[row_of_t[t]][c].  Row j has a
// candidate list, entries list_off[j] .. list_off[j + 1] - 1 of the packed (dj, di) stream (dj in the high 16 bits, di in
// the low 16, both signed) with dist_m, north_m, east_m beside it, sorted ascending by (dist_m, dj, di) on the host.  The
// point (j + dj, i + di) -- i + di wrapped once into [0, nx) when the grid is periodic, otherwise outside the grid when
// not in [0, nx) -- QUALIFIES iff its sample x of day t (as float64, negated for cold spells) is not NaN, x <= g and,
// with a basin map, its label equals the source's.  The source's result is the FIRST qualifying entry of the list; a
// source with NaN g, or none qualifying, is unreached.  Per class k = class_of_t[t] (>= 0) and cell c:
//   n_days[k][c]  int32   sources                       n_found[k][c]  int32   sources that found an entry
//   sum_m, sum_north_m, sum_east_m [k][c]  int64   sums of the entry's dist_m, north_m, east_m over the found sources
//   max_m[k][c]   int32   the largest dist_m found, 0 if none
//   *n_visited    int64   over all sources, the entries the source alone had to look at: the position found plus one,
//                         or the whole list length (entries outside the grid included; a NaN target counts the list)
//
//   displacement_accumulate  lane = grid point, a wave = 64 consecutive longitudes of ONE grid row, so the wave shares
//                     one candidate list and for a fixed entry its lanes read 64 consecutive samples of one day (one
//                     wrap seam at most).  A workgroup is four independent waves; grid.y splits the steps of the block.
//                     class_of_t[t], row_of_t[t], the list bounds and every list entry are uniform over the wave.  The
//                     wave walks its in-event words step by step; a step on which no lane is a source reads nothing.
//                     The list arrives 64 entries at a time: one coalesced load, lane s holding entry s, handed round
//                     with v_readlane -- no dependent scalar load per entry.  The lanes still searching (a ballot) walk
//                     the list together and drop out as they find; the walk ends when none is left or the list is
//                     exhausted.  The addends of the current class stay in registers and leave as in the frame of a
//                     class reduction (kernels.h), whose lane = cell is a lane = grid point here.  Every loop is
//                     bounded by a list length or the block's steps: nothing spins, nothing waits for another wave.
//                     No LDS, no scratch.
//                     Every index is checked where it is formed: an entry whose row leaves the grid is skipped, list
//                     bounds are clamped to the stream's length, a cell id outside [0, C) is no source -- whatever the
//                     tables hold, no access leaves its buffer.
#include "../../include/xmhw_amd.h"
#include "entry_common.h"
#include "stage_reduce.h"

namespace xmhw {

// What the stage computes: the thermal displacement of every MHW cell-day.  The series is the
// UNCOMPACTED block ts[nt][ld] of the steps t0 .. t0 + nt - 1 on the (ny, nx) grid, longitude fastest; inev is the
// in-event bitmap of launch_event_table_bits over the C compact cells and ALL steps; cell_of_point[ny * nx] maps a grid
// point to its compact cell (-1: land), basin[ny * nx] (or NULL) holds its basin label (negative: no source).  Row j's
// candidates are the entries list_off[j] .. list_off[j + 1] - 1 of djdi[] (dj << 16 | di & 0xFFFF), dist_m[], north_m[],
// east_m[], sorted by (dist_m, dj, di).  launch_displacement_accumulate ADDS, per class k of the step and compact cell c,
// the sources to n_days[k][c], those that found a qualifying entry to n_found[k][c], the entry's dist_m, north_m, east_m
// to sum_m, sum_north_m, sum_east_m[k][c], raises max_m[k][c] to its dist_m and adds the entries every source looked at
// to *n_visited (launch_displacement_init zeroes all of them).  row_of_t and class_of_t are DEVICE arrays over all steps
// here.  block_steps: the steps a workgroup takes per block, 0 = automatic; same results for every value.
constexpr int kDisplacementMaxClasses = 1024;
constexpr int kDisplacementMaxAxis = 32767;          // dj and di are packed as int16

namespace {

constexpr int kDpThreads = 256;
constexpr int kDpWaves = kDpThreads / 64;
using u64 = unsigned long long;

struct DpShape {
    int64_t ld, ldc, ldi, ldo;                       // series block, seas, bitmap, outputs
    int64_t t0, nt, tb, C, n_entries;                // the block's steps [t0, t0 + nt), tb steps per grid.y block
    int32_t ny, nx, periodic, negate, K;
};

struct DpOut {
    int32_t *n_days, *n_found, *max_m;               // [K][ldo]
    u64 *sum_m, *sum_n, *sum_e;                      // [K][ldo]
    u64* n_visited;
};

// the addends of one lane for the current class
struct DpAcc {
    int32_t n_days, n_found, max_m;
    u64 sum_m, sum_n, sum_e;
    __device__ __forceinline__ void clear() {
        n_days = n_found = max_m = 0;
        sum_m = sum_n = sum_e = 0;
    }
};

__device__ __forceinline__ void flush(const DpOut& o, int64_t ldo, int32_t k, int64_t c, DpAcc& v) {
    if (v.n_days == 0) return;                       // every addend belongs to a source
    const int64_t p = static_cast<int64_t>(k) * ldo + c;
    atomicAdd(o.n_days + p, v.n_days);
    if (v.n_found) {
        atomicAdd(o.n_found + p, v.n_found);
        if (v.sum_m) atomicAdd(o.sum_m + p, v.sum_m);
        if (v.sum_n) atomicAdd(o.sum_n + p, v.sum_n);
        if (v.sum_e) atomicAdd(o.sum_e + p, v.sum_e);
        if (v.max_m) atomicMax(o.max_m + p, v.max_m);
    }
    v.clear();
}

template <typename T>
__global__ __launch_bounds__(kDpThreads) void displacement_accumulate(
    const T* __restrict__ ts, const double* __restrict__ seas, const int32_t* __restrict__ row_of_t,
    const int32_t* __restrict__ class_of_t, const uint64_t* __restrict__ inev, const int32_t* __restrict__ cell_of_point,
    const int32_t* __restrict__ basin, const int64_t* __restrict__ list_off, const int32_t* __restrict__ djdi,
    const int32_t* __restrict__ dist_m, const int32_t* __restrict__ north_m, const int32_t* __restrict__ east_m, DpShape g,
    DpOut out) {
    const int lane = threadIdx.x & 63;
    const int64_t nxc = (static_cast<int64_t>(g.nx) + 63) / 64;             // waves per grid row
    const int64_t gw = __builtin_amdgcn_readfirstlane(
        static_cast<int32_t>(static_cast<int64_t>(blockIdx.x) * kDpWaves + (threadIdx.x >> 6)));
    if (gw >= nxc * g.ny) return;                    // the whole wave: nothing below synchronises a workgroup
    const int32_t j = static_cast<int32_t>(gw / nxc);
    const int32_t i = static_cast<int32_t>(gw % nxc) * 64 + lane;
    const bool live = i < g.nx;
    const int64_t p = static_cast<int64_t>(j) * g.nx + i;
    int64_t c = live ? cell_of_point[p] : -1;
    if (c >= g.C) c = -1;
    const int32_t b = (live && basin) ? basin[p] : 0;
    const bool src = c >= 0 && b >= 0;
    int64_t e0 = list_off[j], e1 = list_off[j + 1];
    e0 = e0 < 0 ? 0 : (e0 > g.n_entries ? g.n_entries : e0);
    e1 = e1 < e0 ? e0 : (e1 > g.n_entries ? g.n_entries : e1);
    const u64 len = static_cast<u64>(e1 - e0);
    const int64_t nblk = (g.nt + g.tb - 1) / g.tb;
    DpAcc v;
    v.clear();
    u64 visited = 0;
    for (int64_t blk = blockIdx.y; blk < nblk; blk += gridDim.y) {
        const auto [ta, tz] = block_range(blk, g.tb, g.nt, g.t0);
        int32_t kcur = -1;                           // the class the addends belong to (uniform over the wave)
        EventBits bits;
        for (int64_t t = ta; t < tz; ++t) {
            const int32_t k = class_of_t[t];
            if (k < 0 || k >= g.K) continue;         // counts nowhere (labels are checked on the host): reads nothing
            const bool ev = bits.at(inev, g.ldi, c, src, t);
            if (__ballot(ev) == 0) continue;         // uniform over the wave: no source on this step
            if (k != kcur) {
                if (kcur >= 0) flush(out, g.ldo, kcur, c, v);
                kcur = k;
            }
            double target = make_nan();
            if (ev) {
                target = seas[static_cast<int64_t>(row_of_t[t]) * g.ldc + c];
                v.n_days += 1;
            }
            bool active = ev && target == target;    // a NaN target finds nothing: it has looked at the whole list
            if (ev && !active) visited += len;
            const T* __restrict__ day = ts + (t - g.t0) * g.ld;
            for (int64_t eb = e0; eb < e1; eb += 64) {
                if (__ballot(active) == 0) break;
                const int64_t el = eb + lane;
                const int32_t mine = el < e1 ? djdi[el] : 0;               // every lane of the wave is here: entry s in lane s
                const int n = e1 - eb < 64 ? static_cast<int>(e1 - eb) : 64;
                for (int s = 0; s < n; ++s) {
                    if (__ballot(active) == 0) break;
                    const int32_t pk = __builtin_amdgcn_readlane(mine, s);
                    const int32_t jj = j + (pk >> 16);
                    if (jj < 0 || jj >= g.ny) continue;                    // uniform; the host lists no such entry
                    int32_t ii = i + static_cast<int16_t>(pk & 0xFFFF);
                    if (g.periodic) {
                        ii += ii < 0 ? g.nx : 0;
                        ii -= ii >= g.nx ? g.nx : 0;
                    }
                    bool q = false;
                    if (active && ii >= 0 && ii < g.nx) {
                        const int64_t pp = static_cast<int64_t>(jj) * g.nx + ii;
                        double x = static_cast<double>(day[pp]);
                        if (g.negate) x = -x;
                        q = x <= target;             // NaN compares false: land and holes never qualify
                        if (q && basin) q = basin[pp] == b;
                    }
                    if (q) {
                        const int64_t e = eb + s;
                        const int32_t d = dist_m[e];
                        v.n_found += 1;
                        v.sum_m += static_cast<u64>(static_cast<int64_t>(d));
                        v.sum_n += static_cast<u64>(static_cast<int64_t>(north_m[e]));
                        v.sum_e += static_cast<u64>(static_cast<int64_t>(east_m[e]));
                        v.max_m = d > v.max_m ? d : v.max_m;
                        visited += static_cast<u64>(e - e0) + 1;
                        active = false;
                    }
                }
            }
            if (active) visited += len;              // the list is exhausted
        }
        if (kcur >= 0) flush(out, g.ldo, kcur, c, v);
    }
    // one atomic per wave for the visit counter
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) visited += __shfl_down(visited, off, 64);
    if (lane == 0 && visited) atomicAdd(out.n_visited, visited);
}

hipError_t launch_displacement_init(int32_t K, int64_t C, int32_t* n_days, int32_t* n_found, int64_t* sum_m,
                                    int64_t* sum_north_m, int64_t* sum_east_m, int32_t* max_m, int64_t ldo,
                                    int64_t* n_visited, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(n_visited, 0, sizeof(int64_t), stream);
    for (int32_t* p : {n_days, n_found, max_m})
        if (e == hipSuccess) e = zero_rows(p, sizeof(int32_t), K, C, ldo, stream);
    for (int64_t* p : {sum_m, sum_north_m, sum_east_m})
        if (e == hipSuccess) e = zero_rows(p, sizeof(int64_t), K, C, ldo, stream);
    return e;
}

template <typename T>
hipError_t launch_displacement_accumulate(const T* ts, int64_t ld, int64_t t0, int64_t nt, int32_t ny, int32_t nx,
                                          int32_t periodic, const double* seas, int64_t ldc, const int32_t* row_of_t,
                                          int32_t negate, const uint64_t* inev, int64_t ldi, const int32_t* cell_of_point,
                                          int64_t C, const int32_t* basin, const int64_t* list_off, const int32_t* djdi,
                                          const int32_t* dist_m, const int32_t* north_m, const int32_t* east_m,
                                          int64_t n_entries, const int32_t* class_of_t, int32_t K, int64_t block_steps,
                                          int32_t* n_days, int32_t* n_found, int64_t* sum_m, int64_t* sum_north_m,
                                          int64_t* sum_east_m, int32_t* max_m, int64_t ldo, int64_t* n_visited,
                                          hipStream_t stream) {
    if (C <= 0 || nt <= 0 || K <= 0 || ny <= 0 || nx <= 0) return hipSuccess;
    int64_t tb = block_steps > 0 ? block_steps : displacement_auto_block(nt, ny, nx);
    if (tb > nt) tb = nt;
    const DpShape g{ld, ldc, ldi, ldo, t0, nt, tb, C, n_entries, ny, nx, periodic, negate, K};
    const DpOut out{n_days, n_found, max_m, reinterpret_cast<u64*>(sum_m), reinterpret_cast<u64*>(sum_north_m),
                    reinterpret_cast<u64*>(sum_east_m), reinterpret_cast<u64*>(n_visited)};
    const int64_t waves = static_cast<int64_t>(ny) * ((static_cast<int64_t>(nx) + 63) / 64);
    hipLaunchKernelGGL(displacement_accumulate<T>, stage_grid(waves, kDpWaves, nt, tb), dim3(kDpThreads), 0, stream, ts, seas,
                       row_of_t, class_of_t, inev, cell_of_point, basin, list_off, djdi, dist_m, north_m, east_m, g, out);
    return hipGetLastError();
}

}  // namespace

}  // namespace xmhw

// ---- the C entries of mhw_displacement() (include/xmhw_amd.h) ---------------------------------------------------------
namespace {

using namespace xmhw::entry;

static std::atomic<int> g_displacement_block{0};  // steps a workgroup takes per block, 0 = automatic (xmhw_set_displacement_block)

static int displacement_check_shape(int32_t K, int64_t C) {
    if (K < 1 || K > xmhw::kDisplacementMaxClasses)
        return fail(XMHW_ERR_UNSUPPORTED,
                    "displacement: K must be in [1, " + std::to_string(xmhw::kDisplacementMaxClasses) + "]");
    if (C > 0x7FFFFFFFll) return fail(XMHW_ERR_UNSUPPORTED, "displacement: 2^31 cells and more");
    return XMHW_OK;
}

template <typename T>
int displacement_accumulate(const T* ts, int64_t ld, int64_t t0, int64_t nt, int64_t Tn, int32_t ny, int32_t nx,
                            int32_t periodic, const double* seas, int64_t ldc, int64_t D, const int32_t* row_of_t,
                            int32_t negate, const uint64_t* bits, int64_t ldb, const int32_t* cell_of_point, int64_t C,
                            const int32_t* basin, const int64_t* list_off, const int32_t* djdi, const int32_t* dist_m,
                            const int32_t* north_m, const int32_t* east_m, int64_t n_entries, const int32_t* class_of_t,
                            int32_t K, int32_t* n_days, int32_t* n_found, int64_t* sum_m, int64_t* sum_north_m,
                            int64_t* sum_east_m, int32_t* max_m, int64_t ldo, int64_t* n_visited, void* stream) {
    if (displacement_check_shape(K, C) != XMHW_OK) return XMHW_ERR_UNSUPPORTED;
    if (Tn > 0x7FFFFFFFll) return fail(XMHW_ERR_UNSUPPORTED, "displacement: 2^31 steps and more");
    if (ny > xmhw::kDisplacementMaxAxis || nx > xmhw::kDisplacementMaxAxis)
        return fail(XMHW_ERR_UNSUPPORTED, "displacement: a grid axis of 2^15 points and more");
    if (ny < 1 || nx < 1) return fail(XMHW_ERR_INVALID, "bad ny/nx");
    const int64_t N = static_cast<int64_t>(ny) * nx;
    if (Tn <= 0 || t0 < 0 || nt < 1 || nt > Tn - t0) return fail(XMHW_ERR_INVALID, "bad T/t0/nt");
    if (C < 0 || C > N || ld < N || ldc < C || ldb < C || ldo < C || D < 1 || n_entries < 0)
        return fail(XMHW_ERR_INVALID, "bad C/ld/ldc/ldb/ldo/D/n_entries");
    if (!class_of_t || !row_of_t) return fail(XMHW_ERR_INVALID, "NULL class_of_t or row_of_t");
    // the two tables are judged step by step: the one with the earlier bad label is named, class_of_t where both are bad
    // at one step
    const int64_t bad_class = first_outside(class_of_t, Tn, -1, K);
    if (int rc = check_labels(row_of_t, bad_class, 0, D, kRowsOutside)) return rc;
    if (bad_class < Tn) return fail(XMHW_ERR_INVALID, kClassesOutside);
    if (C == 0) return XMHW_OK;
    if (!ts || !seas || !bits || !cell_of_point || !list_off) return fail(XMHW_ERR_INVALID, "NULL buffer");
    if (n_entries > 0 && (!djdi || !dist_m || !north_m || !east_m)) return fail(XMHW_ERR_INVALID, "NULL list buffer");
    if (!n_days || !n_found || !sum_m || !sum_north_m || !sum_east_m || !max_m || !n_visited)
        return fail(XMHW_ERR_INVALID, "NULL output buffer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    RowsRef rows;
    if (int rc = upload_table(row_of_t, Tn, "row table upload", &rows)) return rc;
    RowsRef classes;                                   // the same content-keyed cache: one more int32[T] table
    if (int rc = upload_table(class_of_t, Tn, "class table upload", &classes)) return rc;
    return status_of(xmhw::launch_displacement_accumulate<T>(ts, ld, t0, nt, ny, nx, periodic != 0, seas, ldc, rows->d_rows,
                                                             negate != 0, bits, ldb, cell_of_point, C, basin, list_off, djdi,
                                                             dist_m, north_m, east_m, n_entries, classes->d_rows, K,
                                                             g_displacement_block.load(), n_days, n_found, sum_m,
                                                             sum_north_m, sum_east_m, max_m, ldo, n_visited, st),
                     "displacement_accumulate launch");
}

}  // namespace

extern "C" {

int xmhw_set_displacement_block(int32_t steps) { return set_knob(g_displacement_block, steps, "steps must be >= 0"); }
int xmhw_displacement_init(int32_t K, int64_t C, int32_t* n_days, int32_t* n_found, int64_t* sum_m, int64_t* sum_north_m,
                           int64_t* sum_east_m, int32_t* max_m, int64_t ldo, int64_t* n_visited, void* stream) {
    if (displacement_check_shape(K, C) != XMHW_OK) return XMHW_ERR_UNSUPPORTED;
    if (C < 0 || ldo < C) return fail(XMHW_ERR_INVALID, "bad C/ldo");
    if (!n_visited || (C > 0 && (!n_days || !n_found || !sum_m || !sum_north_m || !sum_east_m || !max_m)))
        return fail(XMHW_ERR_INVALID, "NULL output buffer");
    return status_of(xmhw::launch_displacement_init(K, C, n_days, n_found, sum_m, sum_north_m, sum_east_m, max_m, ldo,
                                                    n_visited, static_cast<hipStream_t>(stream)),
                     "displacement_init");
}
int xmhw_displacement_accumulate_f32(const float* ts, int64_t ld, int64_t t0, int64_t nt, int64_t T, int32_t ny, int32_t nx,
                                     int32_t periodic, const double* seas, int64_t ldc, int64_t D, const int32_t* row_of_t,
                                     int32_t negate, const uint64_t* bits, int64_t ldb, const int32_t* cell_of_point,
                                     int64_t C, const int32_t* basin, const int64_t* list_off, const int32_t* djdi,
                                     const int32_t* dist_m, const int32_t* north_m, const int32_t* east_m, int64_t n_entries,
                                     const int32_t* class_of_t, int32_t K, int32_t* n_days, int32_t* n_found, int64_t* sum_m,
                                     int64_t* sum_north_m, int64_t* sum_east_m, int32_t* max_m, int64_t ldo,
                                     int64_t* n_visited, void* stream) {
    return displacement_accumulate<float>(ts, ld, t0, nt, T, ny, nx, periodic, seas, ldc, D, row_of_t, negate, bits, ldb,
                                          cell_of_point, C, basin, list_off, djdi, dist_m, north_m, east_m, n_entries,
                                          class_of_t, K, n_days, n_found, sum_m, sum_north_m, sum_east_m, max_m, ldo,
                                          n_visited, stream);
}
int xmhw_displacement_accumulate_f64(const double* ts, int64_t ld, int64_t t0, int64_t nt, int64_t T, int32_t ny, int32_t nx,
                                     int32_t periodic, const double* seas, int64_t ldc, int64_t D, const int32_t* row_of_t,
                                     int32_t negate, const uint64_t* bits, int64_t ldb, const int32_t* cell_of_point,
                                     int64_t C, const int32_t* basin, const int64_t* list_off, const int32_t* djdi,
                                     const int32_t* dist_m, const int32_t* north_m, const int32_t* east_m, int64_t n_entries,
                                     const int32_t* class_of_t, int32_t K, int32_t* n_days, int32_t* n_found, int64_t* sum_m,
                                     int64_t* sum_north_m, int64_t* sum_east_m, int32_t* max_m, int64_t ldo,
                                     int64_t* n_visited, void* stream) {
    return displacement_accumulate<double>(ts, ld, t0, nt, T, ny, nx, periodic, seas, ldc, D, row_of_t, negate, bits, ldb,
                                           cell_of_point, C, basin, list_off, djdi, dist_m, north_m, east_m, n_entries,
                                           class_of_t, K, n_days, n_found, sum_m, sum_north_m, sum_east_m, max_m, ldo,
                                           n_visited, stream);
}

}  // extern "C"
