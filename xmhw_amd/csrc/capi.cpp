// capi.cpp -- the C ABI declared in include/xmhw_amd.h.
#include "../../include/xmhw_amd.h"

#include <hip/hip_runtime.h>
#include <unistd.h>

#include <cerrno>
#include <cmath>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <atomic>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "entry_common.h"
#include "kernels.h"
#include "plan.h"
#include "route.h"

using namespace xmhw::entry;

namespace {
thread_local std::string g_err;
}  // namespace

int xmhw::entry::fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}
int xmhw::entry::hip_fail(hipError_t e, const char* what) {
    // out of device memory is reported as such wherever it happens (callers that cache device
    // buffers release them and retry on XMHW_ERR_NOMEM)
    if (e == hipErrorOutOfMemory) {
        (void)hipGetLastError();
        return fail(XMHW_ERR_NOMEM, std::string(what) + ": out of device memory");
    }
    return fail(XMHW_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}
// shared with comm.cpp
int xmhw_set_error_(int code, const std::string& msg) { return fail(code, msg); }
namespace {
#define HIP_TRY(expr)                                        \
    do {                                                     \
        hipError_t _e = (expr);                              \
        if (_e != hipSuccess) return hip_fail(_e, #expr);    \
    } while (0)

constexpr int kSubs = 8;

}  // namespace

// the plan's device arrays apart from the ring step tables: changed under the plan's mutex only; a call works on the copy
// it took there
struct PlanDevice {
    int32_t* row_ptr = nullptr;             // generic kernel: CSR of centres per row
    int32_t* centres = nullptr;
    uint32_t* sflags = nullptr;             // host.step_flags()
    xmhw::DevChunk* chunks = nullptr;       // ring chunks: one array, re-cut when the chunk count changes
    int32_t nchunks = 0;
    unsigned long long* stats = nullptr;    // debug: ring kernel pass counters (xmhw_plan_debug_stats)
    uint32_t* narrow_flag = nullptr;        // float64 input: set when a sample is not float32-representable
    // sorted-list kernel (kernels_sorted.hip): its table (2 lanes per cell), flags and chunks, which depend on the pieces
    uint32_t* table_s = nullptr;
    uint32_t* sflags_s = nullptr;
    xmhw::DevSortedChunk* chunks_s = nullptr;
    int32_t nchunks_s = 0;
    int32_t ndirect_s = 0;                  // how many of them are settled directly (their pooled tracks set)
};

struct xmhw_plan {
    xmhw::Plan host;
    xmhw::RouteSettings settings = xmhw::route_defaults();
    // device state (lazy, per current device at first use)
    std::mutex mu;
    bool uploaded = false;
    PlanDevice dev;
    // ring step tables: (lanes per cell, tracks per lane) -> host.ring_table() on the device.  Filled on first use, kept
    // until the plan is destroyed: a launch in flight never loses its table.
    std::map<std::pair<int32_t, int32_t>, uint32_t*> tables;
    int32_t chunks_cut = 0;                 // the chunk count dev.chunks were cut for
    int32_t yps_s = 0;                      // sorted-list kernel: the tracks per lane and pieces its arrays were built for
    int64_t sorted_pieces = -1;
    // optional timing of the main kernel of every raw-climatology call (xmhw_plan_set_timing): a ring of event pairs
    bool timing = false;
    hipEvent_t tev[32] = {};
    uint64_t tcalls = 0;

    ~xmhw_plan() {
        for (hipEvent_t e : tev) if (e) (void)hipEventDestroy(e);
        for (auto& kv : tables) if (kv.second) (void)hipFree(kv.second);
        for (void* p : std::initializer_list<void*>{dev.row_ptr, dev.centres, dev.sflags, dev.chunks, dev.stats,
                                                    dev.narrow_flag, dev.table_s, dev.sflags_s, dev.chunks_s})
            if (p) (void)hipFree(p);
    }
};

namespace {

// The sorted-list kernel's lists rely on LDS reads outside the workgroup's allocation returning 0 (kernels_sorted.hip).
// Checked once per device of this process before the kernel is used there; a device that answers otherwise keeps the ring
// kernels.  -1 = not probed yet, 1 = holds, 0 = does not.
int sorted_device_ok() {
    static std::mutex mu;
    static int state[64];
    static bool init = false;
    std::lock_guard<std::mutex> lock(mu);
    if (!init) { for (int& v : state) v = -1; init = true; }
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 0;
    if (state[dev] >= 0) return state[dev];
    uint32_t* d_bad = nullptr;
    uint32_t bad = 1;
    if (hipMalloc(&d_bad, sizeof(uint32_t)) != hipSuccess) return 0;
    const bool ran = xmhw::sorted_lds_probe(d_bad, nullptr) == hipSuccess &&
                     hipMemcpy(&bad, d_bad, sizeof(uint32_t), hipMemcpyDeviceToHost) == hipSuccess;
    (void)hipFree(d_bad);
    if (!ran) return 0;          // (not cached: a transient failure is probed again)
    state[dev] = bad == 0 ? 1 : 0;
    return state[dev];
}

// the route of a call on the current device (the device is probed only where the sorted-list kernel would run) ...
xmhw::Route call_route(const xmhw_plan* p, int elem_bytes, double q) {
    xmhw::Route r = xmhw::resolve_route(p->host, p->settings, elem_bytes, q, true);
    if (r.n && r.launch[0].family == xmhw::Family::Sorted && sorted_device_ok() != 1)
        r = xmhw::resolve_route(p->host, p->settings, elem_bytes, q, false);
    return r;
}
// ... and what the introspection entries report from: no device needed, one that passes the probe assumed; float32 at a
// quantile the sorted-list kernel serves, so that the first launch names the plan's float32 kernel
xmhw::Route plan_route(const xmhw_plan* p, int elem_bytes, double q = 1.0) {
    return xmhw::resolve_route(p->host, p->settings, elem_bytes, q, true);
}

// a vector -> device memory, allocated at most once: a failed upload can be retried without leaking
template <typename E>
hipError_t put(E** dst, const std::vector<E>& v) {
    const bool fresh = *dst == nullptr;
    hipError_t e = fresh ? hipMalloc(reinterpret_cast<void**>(dst), sizeof(E) * v.size()) : hipSuccess;
    if (e != hipSuccess) { *dst = nullptr; return e; }
    e = hipMemcpy(*dst, v.data(), sizeof(E) * v.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess && fresh) { (void)hipFree(*dst); *dst = nullptr; }
    return e;
}

// what the launches of one call take: copied out under the plan's lock, used after it is released
struct Ready {
    PlanDevice dev;
    const uint32_t* table[3] = {};          // the step table of every launch (NULL: the generic kernel)
    hipEvent_t t0 = nullptr, t1 = nullptr;  // the call's timing events (NULL: not timed)
};

// XMHW_SORTED_ONEROW=0 (process-wide, read once): no chunk of the sorted-list kernel is settled directly -- every chunk
// walks its table rows.  Not part of the route: the launches, chunks and tables are the same either way.
bool sorted_onerow_enabled() {
    static const bool on = [] {
        const char* v = std::getenv("XMHW_SORTED_ONEROW");
        return !(v && v[0] == '0' && v[1] == '\0');
    }();
    return on;
}

// tables and chunks of the sorted-list kernel (under the plan's lock)
int ensure_sorted(xmhw_plan* p, const xmhw::Launch& l, int64_t pieces) {
    PlanDevice& d = p->dev;
    if (d.table_s && p->yps_s == l.tpl && p->sorted_pieces == pieces) return XMHW_OK;
    HIP_TRY(hipDeviceSynchronize());
    for (void** q : {reinterpret_cast<void**>(&d.table_s), reinterpret_cast<void**>(&d.sflags_s),
                     reinterpret_cast<void**>(&d.chunks_s)})
        if (*q) { HIP_TRY(hipFree(*q)); *q = nullptr; }
    // the kernel's own chunks and table rows (plan.h: sorted_plan).  The tables depend on (tracks per lane, pieces) only:
    // the slabs of one threshold() call -- a different cell count each -- share them.
    const xmhw::Plan::SortedPlan sp = p->host.sorted_plan(l.lanes * l.tpl, 24, pieces);
    if (sp.chunks.empty()) return fail(XMHW_ERR_UNSUPPORTED, "the sorted-list kernel has no chunks for this plan");
    // longest chunk first: workgroups start in the order of their index, blockIdx.y = the chunk, so the launch ends
    // with the short chunks (a 40-year daily plan: rows [60, 366), then [0, 59), then the Feb-29 row) instead of a
    // tail of 316-row waves
    std::vector<xmhw::DevSortedChunk> cs(sp.chunks.size());
    // (a directly settled chunk -- one output row: the shortest there is -- carries its pooled tracks and sorts last)
    const bool onerow = sorted_onerow_enabled();
    d.ndirect_s = 0;
    for (size_t i = 0; i < cs.size(); ++i) {
        const uint64_t set = onerow && sp.direct(i, xmhw::sorted_direct_tracks(l.tpl)) ? sp.pooled[i] : 0;
        d.ndirect_s += set != 0 ? 1 : 0;
        cs[i] = {sp.chunks[i].warm_start, sp.chunks[i].begin, sp.chunks[i].end, sp.chunks[i].trow0,
                 static_cast<uint32_t>(set), static_cast<uint32_t>(set >> 32)};
    }
    std::stable_sort(cs.begin(), cs.end(), [](const xmhw::DevSortedChunk& a, const xmhw::DevSortedChunk& b) {
        return a.end - a.warm_start > b.end - b.warm_start;
    });
    p->sorted_pieces = -1;
    HIP_TRY(put(&d.table_s, sp.table));
    HIP_TRY(put(&d.sflags_s, sp.flags));
    HIP_TRY(put(&d.chunks_s, cs));
    d.nchunks_s = static_cast<int32_t>(cs.size());
    p->yps_s = l.tpl;
    p->sorted_pieces = pieces;
    return XMHW_OK;
}

// everything on the device that the route's launches over C cells need, uploaded or re-cut where it is missing
int ensure(xmhw_plan* p, const xmhw::Route& route, int64_t C, bool timed, Ready* out) {
    std::lock_guard<std::mutex> lock(p->mu);
    const xmhw::Plan& h = p->host;
    PlanDevice& d = p->dev;
    if (!p->uploaded) {
        HIP_TRY(put(&d.row_ptr, h.row_ptr));
        HIP_TRY(put(&d.centres, h.centres));
        HIP_TRY(put(&d.sflags, h.step_flags()));
        p->uploaded = true;
    }
    bool ring = false;
    for (int32_t i = 0; i < route.n; ++i) {
        const xmhw::Launch& l = route.launch[i];
        if (l.family == xmhw::Family::Generic) continue;
        if (l.narrows && !d.narrow_flag) HIP_TRY(hipMalloc(&d.narrow_flag, sizeof(uint32_t)));
        if (l.family == xmhw::Family::Sorted) {
            const int rc = ensure_sorted(p, l, xmhw::sorted_pieces(h, route, C));
            if (rc != XMHW_OK) return rc;
            out->table[i] = d.table_s;
            continue;
        }
        ring = true;
        uint32_t*& table = p->tables[{l.lanes, l.tpl}];
        if (!table) HIP_TRY(put(&table, h.ring_table(l.lanes, l.tpl)));
        out->table[i] = table;
    }
    const int32_t cut = xmhw::ring_chunks(h, route, C);
    if (ring && (!d.chunks || cut != p->chunks_cut)) {
        const std::vector<xmhw::Chunk> ch = h.make_chunks(cut);
        std::vector<xmhw::DevChunk> dch(ch.size());
        for (size_t i = 0; i < ch.size(); ++i) dch[i] = {ch[i].warm_start, ch[i].begin, ch[i].end};
        if (d.chunks) { HIP_TRY(hipFree(d.chunks)); d.chunks = nullptr; }
        HIP_TRY(put(&d.chunks, dch));
        p->chunks_cut = cut;
        d.nchunks = static_cast<int32_t>(dch.size());
    }
    if (timed && p->timing) {
        const int slot = static_cast<int>(p->tcalls % 16);
        for (int i = 0; i < 2; ++i)
            if (!p->tev[2 * slot + i]) HIP_TRY(hipEventCreate(&p->tev[2 * slot + i]));
        out->t0 = p->tev[2 * slot];
        out->t1 = p->tev[2 * slot + 1];
        p->tcalls++;
    }
    out->dev = d;
    return XMHW_OK;
}

// the call's main kernel between its two timing events (xmhw_plan_set_timing)
template <typename F>
hipError_t timed_launch(const Ready& rd, hipStream_t st, F launch) {
    hipError_t e = rd.t0 ? hipEventRecord(rd.t0, st) : hipSuccess;
    if (e == hipSuccess) e = launch();
    if (e == hipSuccess && rd.t1) e = hipEventRecord(rd.t1, st);
    return e;
}

// float64 input through a float32 ring kernel: the probe clears and sets the narrow flag, the kernel reads the samples
// narrowed and leaves at the first lossy one (the round-1 launcher queues its own probe)
hipError_t launch_narrowing(const xmhw::Plan& h, const xmhw::Launch& l, const PlanDevice& rd, const uint32_t* table,
                            const double* ts, int64_t C, int64_t ld, double q, int negate, double* thresh, double* seas,
                            int64_t ldo, hipStream_t st) {
    if (l.family == xmhw::Family::Ring1)
        return xmhw::launch_ring_f32_narrowing(ts, h.T, C, ld, table, h.step_min, rd.chunks, rd.nchunks, h.w, l.tpl, l.lanes,
                                               q, negate, thresh, seas, ldo, st, rd.stats, rd.narrow_flag);
    const hipError_t e = xmhw::launch_narrow_probe(ts, h.T, C, ld, rd.narrow_flag, st);
    if (e != hipSuccess) return e;
    if (l.family == xmhw::Family::Ring2)
        return xmhw::launch_ring2_f32_narrowing(ts, C, ld, h.T, table, rd.sflags, h.step_min, rd.chunks, rd.nchunks, h.w,
                                                l.tpl, h.ntracks, l.layout, q, negate, thresh, seas, ldo, st, rd.narrow_flag);
    if (l.family == xmhw::Family::Ring3)
        return xmhw::launch_ring3_f32_narrowing(ts, C, ld, h.T, table, rd.sflags, h.step_min, rd.chunks, rd.nchunks, h.w,
                                                l.tpl, l.lanes, h.ntracks, q, negate, thresh, seas, ldo, st, rd.narrow_flag);
    return hipErrorInvalidValue;
}

template <typename T>
hipError_t launch_one(const xmhw::Plan& h, const xmhw::Launch& l, const PlanDevice& rd, const uint32_t* table, const T* ts,
                      int64_t C, int64_t ld, double q, int negate, double* thresh, double* seas, int64_t ldo,
                      hipStream_t st) {
    using xmhw::Family;
    const uint32_t* run_flag = l.gated ? rd.narrow_flag : nullptr;
    unsigned long long* stats = l.counters ? rd.stats : nullptr;
    if (l.family == Family::Generic)
        return xmhw::launch_generic<T>(ts, h.T, C, ld, rd.row_ptr, rd.centres, h.D, h.w, q, negate, thresh, seas, ldo, st,
                                       run_flag);
    if constexpr (sizeof(T) == 4) {
        switch (l.family) {
            case Family::Sorted:
                return xmhw::launch_sorted_f32(ts, C, ld, h.T, table, rd.sflags_s, rd.chunks_s, rd.nchunks_s, h.w, l.tpl,
                                               h.ntracks, q, negate, thresh, seas, ldo, st, stats, rd.ndirect_s);
            case Family::Ring1:
                return xmhw::launch_ring_f32(ts, C, ld, table, h.step_min, rd.chunks, rd.nchunks, h.w, l.tpl, l.lanes, q,
                                             negate, thresh, seas, ldo, st, stats);
            case Family::Ring2:
                return xmhw::launch_ring2_f32(ts, C, ld, h.T, table, rd.sflags, h.step_min, rd.chunks, rd.nchunks, h.w, l.tpl,
                                              h.ntracks, l.layout, q, negate, thresh, seas, ldo, st, stats);
            case Family::Ring3:
                return xmhw::launch_ring3_f32(ts, C, ld, h.T, table, rd.sflags, h.step_min, rd.chunks, rd.nchunks, h.w, l.tpl,
                                              l.lanes, h.ntracks, q, negate, thresh, seas, ldo, st, stats);
#ifdef XMHW_RING4
            case Family::Ring4:
                return xmhw::launch_ring4_f32(ts, C, ld, h.T, table, rd.sflags, h.step_min, rd.chunks, rd.nchunks, h.w, l.tpl,
                                              l.lanes, h.ntracks, q, negate, thresh, seas, ldo, st, stats);
#endif
            default: return hipErrorInvalidValue;
        }
    } else {
        if (l.narrows) return launch_narrowing(h, l, rd, table, ts, C, ld, q, negate, thresh, seas, ldo, st);
        // genuinely float64 samples: the 64-bit mode (runs only if the narrowing launch before it flagged a sample)
        if (l.family == Family::Ring2)
            return xmhw::launch_ring2_f64(ts, C, ld, h.T, table, rd.sflags, h.step_min, rd.chunks, rd.nchunks, h.w, l.tpl,
                                          h.ntracks, l.layout, q, negate, thresh, seas, ldo, st, run_flag);
        if (l.family == Family::Ring3)
            return xmhw::launch_ring3_f64(ts, C, ld, h.T, table, rd.sflags, h.step_min, rd.chunks, rd.nchunks, h.w, l.tpl,
                                          l.lanes, h.ntracks, q, negate, thresh, seas, ldo, st, run_flag);
        return hipErrorInvalidValue;
    }
}

// resolve -> ensure -> launch
template <typename T>
int clim_raw(xmhw_plan* plan, const T* ts, int64_t C, int64_t ld, double q, int negate,
             double* thresh, double* seas, int64_t ldo, void* stream) {
    if (!plan) return fail(XMHW_ERR_INVALID, "plan is NULL");
    if (C < 0 || ld < C || ldo < C) return fail(XMHW_ERR_INVALID, "bad C/ld/ldo");
    if (!(q >= 0.0 && q <= 1.0)) return fail(XMHW_ERR_INVALID, "quantile must be in [0, 1]");
    if (C == 0) return XMHW_OK;
    if (!ts || !thresh || !seas) return fail(XMHW_ERR_INVALID, "NULL device buffer");
    const xmhw::Route route = call_route(plan, sizeof(T), q);
    if (route.unsupported) return fail(XMHW_ERR_UNSUPPORTED, route.unsupported);
    // (timed: the main kernel of a float32 call -- the sorted-list or the ring kernel)
    Ready rd;
    const int rc = ensure(plan, route, C, sizeof(T) == 4 && route.launch[0].family != xmhw::Family::Generic, &rd);
    if (rc != XMHW_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipError_t e = hipSuccess;
    for (int32_t i = 0; i < route.n && e == hipSuccess; ++i)
        e = timed_launch(rd, st, [&] {
            return launch_one<T>(plan->host, route.launch[i], rd.dev, rd.table[i], ts, C, ld, q, negate, thresh, seas, ldo, st);
        });
    if (e != hipSuccess) return hip_fail(e, "kernel launch");
    return XMHW_OK;
}

int row_index(const xmhw::Plan& h, int32_t label) {
    auto it = std::lower_bound(h.doys.begin(), h.doys.end(), label);
    if (it == h.doys.end() || *it != label) return -1;
    return static_cast<int>(it - h.doys.begin());
}

template <typename T>
int clim_oneshot(const T* ts, const int32_t* doy, int64_t Tn, int64_t C, int32_t D, int32_t w,
                 double q, int smooth, int smooth_w, int feb29_fix, int negate, double* thresh,
                 double* seas, void* stream) {
    if (smooth && (smooth_w <= 0 || smooth_w % 2 == 0))
        return fail(XMHW_ERR_INVALID, "smoothPercentileWidth should be odd");
    xmhw_plan* plan = nullptr;
    int rc = xmhw_plan_create(doy, Tn, w, &plan);
    if (rc != XMHW_OK) return rc;
    if (plan->host.D != D) {
        xmhw_plan_destroy(plan);
        return fail(XMHW_ERR_INVALID, "D does not match the number of distinct doy labels");
    }
    double *rt = nullptr, *rs = nullptr;
    const size_t bytes = sizeof(double) * static_cast<size_t>(D) * static_cast<size_t>(C);
    hipStream_t st = static_cast<hipStream_t>(stream);
    auto cleanup = [&]() {
        if (rt) (void)hipFree(rt);
        if (rs) (void)hipFree(rs);
        xmhw_plan_destroy(plan);
    };
    if (C == 0) { cleanup(); return XMHW_OK; }
    const bool need_finish = smooth || feb29_fix;
    if (need_finish) {
        if (hipMalloc(&rt, bytes) != hipSuccess || hipMalloc(&rs, bytes) != hipSuccess) {
            cleanup();
            return fail(XMHW_ERR_NOMEM, "hipMalloc of the raw climatology failed");
        }
    }
    rc = clim_raw<T>(plan, ts, C, C, q, negate, need_finish ? rt : thresh, need_finish ? rs : seas, C,
                     stream);
    if (rc == XMHW_OK && need_finish)
        rc = xmhw_clim_finish(plan, rt, rs, C, C, feb29_fix, smooth, smooth_w, thresh, seas, stream);
    hipError_t e = hipStreamSynchronize(st);
    cleanup();
    if (rc != XMHW_OK) return rc;
    if (e != hipSuccess) return hip_fail(e, "hipStreamSynchronize");
    return XMHW_OK;
}

// ---- per-call tables kept on the device between calls ------------------------------------------
// Every detect-side entry needs row_of_t (and the tiled exceedance kernel its chunk tables) on the
// device.  Round 1 allocated, uploaded, synchronised and freed them on every call, which made the
// "asynchronous" stream argument a fiction.  Now a small cache keyed by the table's content keeps them
// (uploaded once, with a blocking copy, at the first call that sees them), and scratch buffers are
// kept per stream and grow on demand: steady-state calls neither allocate nor synchronise.
// (RowsEntry, RowsRef and ScratchRef are declared in entry_common.h: the stage entries in the kernel files hold them too)
}  // namespace
xmhw::entry::RowsEntry::~RowsEntry() {
    if (d_rows) (void)hipFree(d_rows);
    if (d_segs) (void)hipFree(d_segs);
    for (auto& kv : chunks)
        for (int32_t* p : {kv.second.tile_begin, kv.second.t0, kv.second.i0, kv.second.n})
            if (p) (void)hipFree(p);
}
namespace {
std::mutex g_cache_mu;
std::vector<std::shared_ptr<RowsEntry>> g_rows_cache;
uint64_t g_stamp = 0;
constexpr size_t kRowsCacheSlots = 8;

// returns nullptr and sets *err on failure.  The caller HOLDS the returned pointer until its launches are queued: an
// entry another thread evicts meanwhile is destroyed (hipFree, which waits for the device) only when the last holder
// lets go of it.
RowsRef cached_rows(const int32_t* row_of_t, int64_t Tn, hipError_t* err) {
    std::lock_guard<std::mutex> lock(g_cache_mu);
    int dev = 0;
    *err = hipGetDevice(&dev);
    if (*err != hipSuccess) return nullptr;
    for (auto& e : g_rows_cache)
        if (e->device == dev && static_cast<int64_t>(e->host.size()) == Tn &&
            std::memcmp(e->host.data(), row_of_t, sizeof(int32_t) * static_cast<size_t>(Tn)) == 0) {
            e->stamp = ++g_stamp;
            return e;
        }
    auto e = std::make_shared<RowsEntry>();
    e->host.assign(row_of_t, row_of_t + Tn);
    e->device = dev;
    *err = hipMalloc(&e->d_rows, sizeof(int32_t) * static_cast<size_t>(Tn));
    if (*err != hipSuccess) { e->d_rows = nullptr; return nullptr; }
    *err = hipMemcpy(e->d_rows, row_of_t, sizeof(int32_t) * static_cast<size_t>(Tn), hipMemcpyHostToDevice);
    if (*err != hipSuccess) return nullptr;
    if (g_rows_cache.size() >= kRowsCacheSlots) {
        size_t oldest = 0;
        for (size_t i = 1; i < g_rows_cache.size(); ++i)
            if (g_rows_cache[i]->stamp < g_rows_cache[oldest]->stamp) oldest = i;
        (void)hipDeviceSynchronize();          // nothing in flight may still read the evicted tables
        g_rows_cache.erase(g_rows_cache.begin() + static_cast<long>(oldest));
    }
    e->stamp = ++g_stamp;
    g_rows_cache.push_back(e);
    return e;
}

// scratch memory per (device, stream): grows on demand (the only synchronising moment), never shrinks.  A caller
// keeps the ScratchRef for the length of its call -- scratch->get() is its buffer: a buffer that another thread on the
// same stream outgrows meanwhile is freed only when its last holder is done.
struct Scratch { ScratchRef ptr; size_t cap = 0; };
std::map<std::pair<int, void*>, Scratch> g_scratch;
hipError_t scratch_get(hipStream_t st, size_t bytes, ScratchRef* keep) {
    std::lock_guard<std::mutex> lock(g_cache_mu);
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    Scratch& sc = g_scratch[{dev, static_cast<void*>(st)}];
    if (sc.cap < bytes) {
        if (sc.ptr) {
            e = hipStreamSynchronize(st);
            if (e != hipSuccess) return e;
            sc.ptr.reset();
            sc.cap = 0;
        }
        void* p = nullptr;
        e = hipMalloc(&p, bytes);
        if (e != hipSuccess) return e;
        sc.ptr = ScratchRef(p, [](void* q) { (void)hipFree(q); });
        sc.cap = bytes;
    }
    *keep = sc.ptr;
    return hipSuccess;
}
void release_cached_tables() {
    std::lock_guard<std::mutex> lock(g_cache_mu);
    (void)hipDeviceSynchronize();
    g_rows_cache.clear();
    g_scratch.clear();
}

}  // namespace

// ---- the steps the stage entries share (declared in entry_common.h) ------------------------------
namespace xmhw {
namespace entry {

int status_of(hipError_t e, const char* what) { return e == hipSuccess ? XMHW_OK : hip_fail(e, what); }

int set_knob(std::atomic<int>& knob, int32_t value, const char* message) {
    if (value < 0) return fail(XMHW_ERR_INVALID, message);
    knob = value;
    return XMHW_OK;
}

// (cached_rows)
int upload_table(const int32_t* host, int64_t n, const char* what, RowsRef* table) {
    hipError_t e = hipSuccess;
    *table = cached_rows(host, n, &e);
    return *table ? XMHW_OK : hip_fail(e, what);
}

int claim_scratch(hipStream_t st, size_t bytes, ScratchRef* scratch) {
    return status_of(scratch_get(st, bytes, scratch), "scratch allocation");
}

int64_t first_outside(const int32_t* labels, int64_t n, int64_t lo, int64_t hi) {
    int64_t t = 0;
    while (t < n && labels[t] >= lo && labels[t] < hi) ++t;
    return t;
}
int check_labels(const int32_t* labels, int64_t n, int64_t lo, int64_t hi, const char* message) {
    return first_outside(labels, n, lo, hi) < n ? fail(XMHW_ERR_INVALID, message) : XMHW_OK;
}

int event_day_bitmap(const uint64_t* bits, int64_t Tn, int64_t C, int64_t ldb, int32_t min_duration, int32_t join_gaps,
                     int32_t max_gap, hipStream_t st, ScratchRef* scratch, const uint64_t** inev) {
    const int64_t W = (Tn + 63) / 64;
    if (int rc = claim_scratch(st, sizeof(uint64_t) * static_cast<size_t>(W) * static_cast<size_t>(C), scratch)) return rc;
    uint64_t* words = static_cast<uint64_t*>(scratch->get());
    *inev = words;
    return status_of(xmhw::launch_event_day_bits(bits, Tn, C, ldb, min_duration, join_gaps, max_gap, words, C, st),
                     "event_day_bits launch");
}

// One allocation: masks, offsets, classes.
hipError_t cooccur_segments(const RowsRef& classes, int64_t Tn) {
    std::lock_guard<std::mutex> lock(g_cache_mu);
    if (classes->d_segs) return hipSuccess;
    const std::vector<int32_t>& k = classes->host;
    const int64_t W = (Tn + 63) / 64;
    std::vector<int32_t> off(static_cast<size_t>(W) + 1, 0), cls;
    std::vector<uint64_t> mask;
    for (int64_t w = 0; w < W; ++w) {
        const int64_t t1 = std::min<int64_t>(Tn, w * 64 + 64);
        for (int64_t t = w * 64; t < t1;) {
            if (k[t] < 0) { ++t; continue; }
            uint64_t m = 0;
            const int32_t c = k[t];
            for (; t < t1 && k[t] == c; ++t) m |= uint64_t{1} << (t & 63);
            cls.push_back(c);
            mask.push_back(m);
        }
        off[static_cast<size_t>(w) + 1] = static_cast<int32_t>(cls.size());
    }
    const size_t n = cls.size();
    const size_t b_mask = sizeof(uint64_t) * n, b_off = sizeof(int32_t) * off.size(), b_cls = sizeof(int32_t) * n;
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, b_mask + b_off + b_cls + 8);
    if (e != hipSuccess) return e;
    char* base = static_cast<char*>(p);
    if (n) e = hipMemcpy(base, mask.data(), b_mask, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(base + b_mask, off.data(), b_off, hipMemcpyHostToDevice);
    if (e == hipSuccess && n) e = hipMemcpy(base + b_mask + b_off, cls.data(), b_cls, hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(p); return e; }
    classes->d_segs = p;
    classes->seg_mask = reinterpret_cast<uint64_t*>(base);
    classes->seg_off = reinterpret_cast<int32_t*>(base + b_mask);
    classes->seg_class = reinterpret_cast<int32_t*>(base + b_mask + b_off);
    return hipSuccess;
}

}  // namespace entry
}  // namespace xmhw

namespace {

template <typename T>
int detect_events(const T* ts, int64_t Tn, int64_t C, int64_t ld, const double* thresh, int64_t ldt,
                  const int32_t* row_of_t, int32_t min_duration, int32_t join_gaps, int32_t max_gap,
                  int32_t negate, int32_t* events, int32_t* start, int32_t* end, uint8_t* bthresh,
                  int64_t ldo, int32_t* nevents, void* stream) {
    if (Tn <= 0 || C < 0 || ld < C || ldt < C || ldo < C) return fail(XMHW_ERR_INVALID, "bad T/C/ld/ldt/ldo");
    if (min_duration < 1 || max_gap < 0) return fail(XMHW_ERR_INVALID, "minDuration must be >= 1 and maxGap >= 0");
    if (C == 0) return XMHW_OK;
    if (!ts || !thresh || !row_of_t || !events || !start || !end)
        return fail(XMHW_ERR_INVALID, "NULL buffer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    RowsRef rows;
    if (int rc = upload_table(row_of_t, Tn, "row table upload", &rows)) return rc;
    return status_of(xmhw::launch_detect<T>(ts, Tn, C, ld, thresh, ldt, rows->d_rows, min_duration, join_gaps, max_gap,
                                            negate, events, start, end, bthresh, ldo, nevents, st),
                     "detect_events launch");
}

template <typename T>
int event_stats(const T* ts, int64_t Tn, int64_t C, int64_t ld, const double* seas, const double* thresh,
                int64_t ldc, const int32_t* row_of_t, int32_t negate, const int32_t* events, int64_t ldo,
                const int64_t* offsets, double* table, void* stream) {
    if (Tn <= 0 || C < 0 || ld < C || ldc < C || ldo < C) return fail(XMHW_ERR_INVALID, "bad T/C/ld/ldc/ldo");
    if (C == 0) return XMHW_OK;
    if (!ts || !seas || !thresh || !row_of_t || !events || !offsets)
        return fail(XMHW_ERR_INVALID, "NULL buffer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    RowsRef rows;
    if (int rc = upload_table(row_of_t, Tn, "row table upload", &rows)) return rc;
    return status_of(xmhw::launch_event_stats<T>(ts, Tn, C, ld, seas, thresh, ldc, rows->d_rows, negate, events, ldo,
                                                 offsets, table, st),
                     "event_stats launch");
}

static std::atomic<int> g_exceed_kernel{0};   // 0 auto, 1 per-step kernel, 2 tiled kernel (xmhw_set_exceed_kernel)

// Chunks for exceed_bits_tiled: maximal segments of consecutive steps with consecutive rows inside one
// tile of `tile` rows, grouped by tile (time order kept inside a tile).
struct ExceedChunks {
    std::vector<int32_t> tile_begin, t0, i0, n;
    int32_t ntiles = 0;
    ExceedChunks(const int32_t* row_of_t, int64_t Tn, int64_t D, int tile) {
        ntiles = static_cast<int32_t>((D + tile - 1) / tile);
        std::vector<std::vector<int32_t>> per(ntiles);          // chunk start steps per tile
        std::vector<int32_t> len;                                 // by start step (sparse via map below)
        std::vector<int32_t> start, count;
        for (int64_t t = 0; t < Tn;) {
            const int32_t r = row_of_t[t];
            const int32_t k = r / tile;
            int64_t e = t + 1;
            while (e < Tn && row_of_t[e] == row_of_t[e - 1] + 1 && row_of_t[e] / tile == k) ++e;
            per[k].push_back(static_cast<int32_t>(start.size()));
            start.push_back(static_cast<int32_t>(t));
            count.push_back(static_cast<int32_t>(e - t));
            t = e;
        }
        tile_begin.assign(ntiles + 1, 0);
        for (int32_t k = 0; k < ntiles; ++k) {
            tile_begin[k + 1] = tile_begin[k] + static_cast<int32_t>(per[k].size());
            for (int32_t id : per[k]) {
                t0.push_back(start[id]);
                i0.push_back(row_of_t[start[id]] - k * tile);
                n.push_back(count[id]);
            }
        }
    }
};

template <typename T>
int exceed_bits(const T* ts, int64_t Tn, int64_t C, int64_t ld, const double* thresh, int64_t ldt, int64_t D,
                const int32_t* row_of_t, int32_t negate, uint64_t* bits, int64_t ldb, void* stream) {
    if (Tn <= 0 || C < 0 || ld < C || ldt < C || ldb < C || D <= 0) return fail(XMHW_ERR_INVALID, "bad T/C/ld/ldt/ldb/D");
    if (Tn >= (int64_t{1} << 31)) return fail(XMHW_ERR_INVALID, "T too large");
    if (C == 0) return XMHW_OK;
    if (!ts || !thresh || !row_of_t || !bits) return fail(XMHW_ERR_INVALID, "NULL buffer");
    if (int rc = check_labels(row_of_t, Tn, 0, D, kRowsOutside)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    constexpr int kTile = sizeof(T) == 4 ? 64 : 32;
    RowsRef rows;
    if (int rc = upload_table(row_of_t, Tn, "row table upload", &rows)) return rc;
    // chunk tables of the tiled kernel: built and uploaded once per (row table, D, tile)
    ChunkTables* ct = nullptr;
    {
        std::lock_guard<std::mutex> lock(g_cache_mu);
        auto key = std::make_pair(D, kTile);
        auto it = rows->chunks.find(key);
        if (it == rows->chunks.end()) {
            const ExceedChunks ch(row_of_t, Tn, D, kTile);
            ChunkTables t;
            t.ntiles = ch.ntiles;
            t.nchunks = static_cast<int64_t>(ch.t0.size());
            auto put = [&](int32_t** dst, const std::vector<int32_t>& v) -> hipError_t {
                const size_t bytes = sizeof(int32_t) * (v.empty() ? 1 : v.size());
                hipError_t err = hipMalloc(dst, bytes);
                if (err == hipSuccess && !v.empty()) err = hipMemcpy(*dst, v.data(), sizeof(int32_t) * v.size(), hipMemcpyHostToDevice);
                return err;
            };
            hipError_t e = hipSuccess;
            for (auto pr : {std::make_pair(&t.tile_begin, &ch.tile_begin), std::make_pair(&t.t0, &ch.t0),
                            std::make_pair(&t.i0, &ch.i0), std::make_pair(&t.n, &ch.n)})
                if (e == hipSuccess) e = put(pr.first, *pr.second);
            if (e != hipSuccess) return hip_fail(e, "chunk table upload");
            it = rows->chunks.emplace(key, t).first;
        }
        ct = &it->second;
    }
    // The tiled kernel pays one pass over its unrolled tile per chunk: worth it when chunks are long
    // (calendar-like labels); an arbitrary label sequence falls back to the per-step kernel.
    // One thread walks all tiles of a cell, so small grids (too few workgroups to fill 256 CUs) keep the
    // per-step kernel, which also splits the time axis over blocks.
    const int mode = g_exceed_kernel.load();
    const bool tiled = mode == 2 || (mode == 0 && ct->nchunks * kTile <= 4 * Tn && C >= 131072);
    const int64_t W = (Tn + 63) / 64;
    float* thf = nullptr;
    ScratchRef scratch;
    if constexpr (sizeof(T) == 4) {
        // float32 series: compare against the float32 floor of the thresholds (same results, see
        // kernels_events.hip), 4 instead of 8 bytes per threshold.  Only the addressed (D, C) region is
        // converted: `thresh` may point into a wider array (column block k0 of a (D, ldt) climatology),
        // where D * ldt elements would overrun it.  The copy lives in this stream's scratch buffer.
        if (int rc = claim_scratch(st, sizeof(float) * static_cast<size_t>(D) * static_cast<size_t>(C), &scratch)) return rc;
        thf = static_cast<float*>(scratch.get());
        if (int rc = status_of(xmhw::launch_floor_to_f32(thresh, D, C, ldt, thf, C, st), "floor_to_f32 launch")) return rc;
    }
    const int64_t ldtf = sizeof(T) == 4 ? C : ldt;   // leading dimension of the thresholds the kernels read
    if (tiled) {
        hipError_t e =
            ldb == C ? hipMemsetAsync(bits, 0, sizeof(uint64_t) * static_cast<size_t>(W) * static_cast<size_t>(C), st)
                     : hipMemset2DAsync(bits, sizeof(uint64_t) * static_cast<size_t>(ldb), 0,
                                        sizeof(uint64_t) * static_cast<size_t>(C), static_cast<size_t>(W), st);
        if (e == hipSuccess) {
            if constexpr (sizeof(T) == 4)
                e = xmhw::launch_exceed_bits_tiled<float, float, 64>(ts, C, ld, thf, ldtf, D, ct->tile_begin, ct->ntiles,
                                                                     ct->t0, ct->i0, ct->n, negate, bits, ldb, st);
            else
                e = xmhw::launch_exceed_bits_tiled<double, double, 32>(ts, C, ld, thresh, ldt, D, ct->tile_begin, ct->ntiles,
                                                                       ct->t0, ct->i0, ct->n, negate, bits, ldb, st);
        }
        return status_of(e, "exceed_bits_tiled launch");
    }
    if constexpr (sizeof(T) == 4)
        return status_of(xmhw::launch_exceed_bits<float, float>(ts, Tn, C, ld, thf, ldtf, rows->d_rows, negate, bits, ldb,
                                                                st),
                         "exceed_bits launch");
    else
        return status_of(xmhw::launch_exceed_bits<double, double>(ts, Tn, C, ld, thresh, ldt, rows->d_rows, negate, bits,
                                                                  ldb, st),
                         "exceed_bits launch");
}

template <typename T>
int event_stats_sparse(const T* ts, int64_t Tn, int64_t C, int64_t ld, const double* seas, const double* thresh,
                       int64_t ldc, const int32_t* row_of_t, int32_t negate, int64_t n_events, double* table,
                       void* stream) {
    if (Tn <= 0 || C < 0 || ld < C || ldc < C || n_events < 0) return fail(XMHW_ERR_INVALID, "bad T/C/ld/ldc/n_events");
    if (n_events == 0) return XMHW_OK;
    if (!ts || !seas || !thresh || !row_of_t || !table) return fail(XMHW_ERR_INVALID, "NULL buffer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    RowsRef rows;
    if (int rc = upload_table(row_of_t, Tn, "row table upload", &rows)) return rc;
    return status_of(xmhw::launch_event_stats_sparse<T>(ts, Tn, ld, seas, thresh, ldc, rows->d_rows, negate, n_events, table,
                                                        st),
                     "event_stats_sparse launch");
}

template <typename T>
int event_intermediate(const T* ts, int64_t Tn, int64_t C, int64_t ld, const double* seas, const double* thresh,
                       int64_t ldc, const int32_t* row_of_t, int32_t negate, const int32_t* events, int64_t ldo,
                       double* out, int64_t ldv, uint8_t* dur, void* stream) {
    if (Tn <= 0 || C < 0 || ld < C || ldc < C || ldo < C || ldv < C)
        return fail(XMHW_ERR_INVALID, "bad T/C/ld/ldc/ldo/ldv");
    if (C == 0) return XMHW_OK;
    if (!ts || !seas || !thresh || !row_of_t || !events || !out || !dur) return fail(XMHW_ERR_INVALID, "NULL buffer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    RowsRef rows;
    if (int rc = upload_table(row_of_t, Tn, "row table upload", &rows)) return rc;
    return status_of(xmhw::launch_event_intermediate<T>(ts, Tn, C, ld, seas, thresh, ldc, rows->d_rows, negate, events, ldo,
                                                        out, ldv, dur, st),
                     "event_intermediate launch");
}

template <typename T>
int clim_host(const T* ts, const int32_t* doy, int64_t Tn, int64_t C, int32_t D, int32_t w, double q,
              int smooth, int smooth_w, int feb29_fix, int negate, double* thresh, double* seas) {
    if (C == 0) return XMHW_OK;
    if (!ts || !thresh || !seas) return fail(XMHW_ERR_INVALID, "NULL host buffer");
    T* d_ts = nullptr;
    double *d_th = nullptr, *d_se = nullptr;
    const size_t in_bytes = sizeof(T) * static_cast<size_t>(Tn) * static_cast<size_t>(C);
    const size_t out_bytes = sizeof(double) * static_cast<size_t>(D) * static_cast<size_t>(C);
    auto cleanup = [&]() {
        if (d_ts) (void)hipFree(d_ts);
        if (d_th) (void)hipFree(d_th);
        if (d_se) (void)hipFree(d_se);
    };
    if (hipMalloc(&d_ts, in_bytes) != hipSuccess || hipMalloc(&d_th, out_bytes) != hipSuccess ||
        hipMalloc(&d_se, out_bytes) != hipSuccess) {
        cleanup();
        return fail(XMHW_ERR_NOMEM, "hipMalloc failed");
    }
    hipError_t e = hipMemcpy(d_ts, ts, in_bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) { cleanup(); return hip_fail(e, "hipMemcpy H2D"); }
    int rc = clim_oneshot<T>(d_ts, doy, Tn, C, D, w, q, smooth, smooth_w, feb29_fix, negate, d_th, d_se,
                             nullptr);
    if (rc == XMHW_OK) {
        e = hipMemcpy(thresh, d_th, out_bytes, hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(seas, d_se, out_bytes, hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = hip_fail(e, "hipMemcpy D2H");
    }
    cleanup();
    return rc;
}

template <typename T>
int block_time(const T* ts, int64_t Tn, int64_t C, int64_t ld, const double* cats, int64_t ldcat,
               const int32_t* bin_of_t, int32_t nbins, double* out, int64_t ldo, void* stream) {
    if (C < 0 || Tn <= 0 || nbins <= 0 || ldo < C || ld < C || (cats && ldcat < C)) return fail(XMHW_ERR_INVALID, "bad C/T/nbins/ld");
    if (C == 0) return XMHW_OK;
    if (!ts || !bin_of_t || !out) return fail(XMHW_ERR_INVALID, "NULL buffer");
    return status_of(xmhw::launch_block_time<T>(ts, Tn, C, ld, cats, ldcat, bin_of_t, nbins, out, ldo,
                                                static_cast<hipStream_t>(stream)),
                     "block_time launch");
}

int fit_args(const void* ts, int64_t Tn, int64_t C, int64_t ld, const double* basis, int32_t P, const double* coef,
             int64_t ldc) {
    if (Tn < 0 || C < 0) return fail(XMHW_ERR_INVALID, "bad T/C");
    if (P < 1) return fail(XMHW_ERR_INVALID, "P must be >= 1");
    if (P > XMHW_FIT_MAX_TERMS)
        return fail(XMHW_ERR_UNSUPPORTED, "series fit: more than " + std::to_string(XMHW_FIT_MAX_TERMS) + " terms");
    if (ld < C) return fail(XMHW_ERR_INVALID, "ld must be >= C");
    if (ldc < C) return fail(XMHW_ERR_INVALID, "ldc must be >= C");
    if (C == 0 || Tn == 0) return XMHW_OK;
    if (!ts || !basis || !coef) return fail(XMHW_ERR_INVALID, "NULL buffer");
    if ((C + 63) / 64 > 0x7FFFFFFFll) return fail(XMHW_ERR_UNSUPPORTED, "C too large for one launch");
    return XMHW_OK;
}

template <typename T>
int series_fit(const T* ts, int64_t Tn, int64_t C, int64_t ld, const double* basis, int32_t P, const uint8_t* weight,
               int32_t min_valid, double* coef, int64_t ldc, int32_t* nvalid, void* stream) {
    if (int rc = fit_args(ts, Tn, C, ld, basis, P, coef, ldc)) return rc;
    if (C == 0 || Tn == 0) return XMHW_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t gram_bytes = sizeof(double) * xmhw::kFitGramWords;      // then one flag byte per cell
    ScratchRef scratch;
    if (int rc = claim_scratch(st, gram_bytes + static_cast<size_t>(C), &scratch)) return rc;
    void* sp = scratch.get();
    return status_of(xmhw::launch_series_fit<T>(ts, Tn, C, ld, basis, P, weight, min_valid > P ? min_valid : P,
                                                static_cast<double*>(sp), static_cast<uint8_t*>(sp) + gram_bytes, coef, ldc,
                                                nvalid, st),
                     "series_fit launch");
}

template <typename T>
int series_remove(T* ts, int64_t Tn, int64_t C, int64_t ld, const double* basis, int32_t P, int32_t R,
                  const double* coef, int64_t ldc, void* stream) {
    if (int rc = fit_args(ts, Tn, C, ld, basis, P, coef, ldc)) return rc;
    if (R < 1 || R > P) return fail(XMHW_ERR_INVALID, "R must be in [1, P]");
    if (C == 0 || Tn == 0) return XMHW_OK;
    if ((Tn + 63) / 64 > 65535) return fail(XMHW_ERR_UNSUPPORTED, "T too large for one launch");
    return status_of(xmhw::launch_series_remove<T>(ts, Tn, C, ld, basis, P, R, coef, ldc, static_cast<hipStream_t>(stream)),
                     "series_remove launch");
}

}  // namespace

extern "C" {

int xmhw_version(void) { return 1000 * 0 + 1; }
const char* xmhw_arch(void) { return "gfx950"; }
const char* xmhw_last_error(void) { return g_err.c_str(); }

int xmhw_device_count(int* count) {
    if (!count) return fail(XMHW_ERR_INVALID, "count is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { *count = 0; return hip_fail(e, "hipGetDeviceCount"); }
    *count = n;
    return XMHW_OK;
}
int xmhw_set_device(int device) {
    HIP_TRY(hipSetDevice(device));
    return XMHW_OK;
}
int xmhw_get_device(int* device) {
    if (!device) return fail(XMHW_ERR_INVALID, "device is NULL");
    HIP_TRY(hipGetDevice(device));
    return XMHW_OK;
}
int xmhw_device_info(int device, char* name, int name_len, int* compute_units, uint64_t* hbm_bytes) {
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (name && name_len > 0) {
        std::snprintf(name, static_cast<size_t>(name_len), "%s (%s)", prop.name, prop.gcnArchName);
    }
    if (compute_units) *compute_units = prop.multiProcessorCount;
    if (hbm_bytes) *hbm_bytes = prop.totalGlobalMem;
    return XMHW_OK;
}

int xmhw_malloc(void** dev_ptr, size_t bytes) {
    if (!dev_ptr) return fail(XMHW_ERR_INVALID, "dev_ptr is NULL");
    *dev_ptr = nullptr;
    if (bytes == 0) return XMHW_OK;
    hipError_t e = hipMalloc(dev_ptr, bytes);
    if (e == hipErrorOutOfMemory) return fail(XMHW_ERR_NOMEM, "hipMalloc: out of memory");
    if (e != hipSuccess) return hip_fail(e, "hipMalloc");
    return XMHW_OK;
}
int xmhw_free(void* dev_ptr) {
    if (dev_ptr) HIP_TRY(hipFree(dev_ptr));
    return XMHW_OK;
}
int xmhw_memcpy_h2d(void* dst, const void* src, size_t bytes, void* stream) {
    if (bytes == 0) return XMHW_OK;
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, static_cast<hipStream_t>(stream)));
    HIP_TRY(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    return XMHW_OK;
}
int xmhw_memcpy_d2h(void* dst, const void* src, size_t bytes, void* stream) {
    if (bytes == 0) return XMHW_OK;
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, static_cast<hipStream_t>(stream)));
    HIP_TRY(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    return XMHW_OK;
}
int xmhw_memcpy2d_h2d(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t height,
                      void* stream) {
    if (width == 0 || height == 0) return XMHW_OK;
    if (!dst || !src || dpitch < width || spitch < width) return fail(XMHW_ERR_INVALID, "bad pointer/pitch");
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIP_TRY(hipMemcpy2DAsync(dst, dpitch, src, spitch, width, height, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    return XMHW_OK;
}
int xmhw_host_alloc(void** host_ptr, size_t bytes) {
    if (!host_ptr) return fail(XMHW_ERR_INVALID, "host_ptr is NULL");
    *host_ptr = nullptr;
    if (bytes == 0) return XMHW_OK;
    hipError_t e = hipHostMalloc(host_ptr, bytes, hipHostMallocDefault);
    if (e == hipErrorOutOfMemory) return fail(XMHW_ERR_NOMEM, "hipHostMalloc: out of memory");
    if (e != hipSuccess) return hip_fail(e, "hipHostMalloc");
    return XMHW_OK;
}
int xmhw_host_free(void* host_ptr) {
    if (host_ptr) HIP_TRY(hipHostFree(host_ptr));
    return XMHW_OK;
}
int xmhw_memcpy2d_h2d_async(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t height,
                            void* stream) {
    if (width == 0 || height == 0) return XMHW_OK;
    if (!dst || !src || dpitch < width || spitch < width) return fail(XMHW_ERR_INVALID, "bad pointer/pitch");
    HIP_TRY(hipMemcpy2DAsync(dst, dpitch, src, spitch, width, height, hipMemcpyHostToDevice, static_cast<hipStream_t>(stream)));
    return XMHW_OK;
}
int xmhw_memcpy_h2d_async(void* dst, const void* src, size_t bytes, void* stream) {
    if (bytes == 0) return XMHW_OK;
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, static_cast<hipStream_t>(stream)));
    return XMHW_OK;
}
int xmhw_event_sync(void* event) {
    HIP_TRY(hipEventSynchronize(static_cast<hipEvent_t>(event)));
    return XMHW_OK;
}
int xmhw_memcpy_d2h_async(void* dst, const void* src, size_t bytes, void* stream) {
    if (bytes == 0) return XMHW_OK;
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, static_cast<hipStream_t>(stream)));
    return XMHW_OK;
}
int xmhw_decode(const void* raw_dev, int raw_itemsize, int big_endian, int64_t rows, int64_t cols, int64_t ld_raw,
                void* out_dev, int out_itemsize, int64_t ld_out, int has_scale, double scale_factor, double add_offset,
                int has_fill, double fill_value, void* stream) {
    if (rows < 0 || cols < 0 || ld_raw < cols || ld_out < cols) return fail(XMHW_ERR_INVALID, "bad rows/cols/ld");
    if (rows == 0 || cols == 0) return XMHW_OK;
    if (!raw_dev || !out_dev) return fail(XMHW_ERR_INVALID, "NULL device buffer");
    hipError_t e = xmhw::launch_decode(raw_dev, raw_itemsize, big_endian, rows, cols, ld_raw, out_dev, out_itemsize, ld_out,
                                       scale_factor, add_offset, has_scale, has_fill, fill_value,
                                       static_cast<hipStream_t>(stream));
    if (e == hipErrorInvalidValue)
        return fail(XMHW_ERR_UNSUPPORTED, "decode: stored/decoded type pair not supported (int16->f32/f64, f32->f32, f64->f64)");
    if (e != hipSuccess) return hip_fail(e, "decode launch");
    return XMHW_OK;
}
int xmhw_encode_i16(const float* in_dev, int64_t rows, int64_t cols, int64_t ld_in, int16_t* out_dev, int64_t ld_out,
                    double scale_factor, double add_offset, int32_t fill_code, void* stream) {
    if (rows < 0 || cols < 0 || ld_in < cols || ld_out < cols) return fail(XMHW_ERR_INVALID, "bad rows/cols/ld");
    if (!(scale_factor == scale_factor) || scale_factor == 0.0 || !(add_offset == add_offset))
        return fail(XMHW_ERR_INVALID, "scale_factor must be a non-zero number, add_offset a number");
    if (fill_code < -32768 || fill_code > 32767) return fail(XMHW_ERR_INVALID, "fill_code is not an int16");
    if (rows == 0 || cols == 0) return XMHW_OK;
    if (!in_dev || !out_dev) return fail(XMHW_ERR_INVALID, "NULL device buffer");
    return status_of(xmhw::launch_encode_i16(in_dev, rows, cols, ld_in, out_dev, ld_out, scale_factor, add_offset, fill_code,
                                             static_cast<hipStream_t>(stream)),
                     "encode launch");
}
int xmhw_read_rows(int fd, int64_t file_offset, int64_t row_pitch, int64_t row_bytes, int64_t rows, void* dst_host) {
    // pread() copies from the page cache (or the disk) straight into the caller's buffer -- for the ingest
    // path a page-locked staging buffer: no page of the file is ever mapped into this process, so many
    // threads calling this at once do not queue up on the address space's page-fault path the way
    // copies out of an mmap() do
    if (fd < 0 || file_offset < 0 || row_pitch < row_bytes || row_bytes < 0 || rows < 0)
        return fail(XMHW_ERR_INVALID, "bad fd/offset/pitch/row_bytes/rows");
    if (rows == 0 || row_bytes == 0) return XMHW_OK;
    if (!dst_host) return fail(XMHW_ERR_INVALID, "NULL destination");
    char* dst = static_cast<char*>(dst_host);
    for (int64_t r = 0; r < rows; ++r) {
        int64_t done = 0;
        while (done < row_bytes) {
            const ssize_t got = ::pread(fd, dst + r * row_bytes + done, static_cast<size_t>(row_bytes - done),
                                        static_cast<off_t>(file_offset + r * row_pitch + done));
            if (got < 0) {
                if (errno == EINTR) continue;
                return fail(XMHW_ERR_INVALID, std::string("pread: ") + std::strerror(errno));
            }
            if (got == 0) return fail(XMHW_ERR_INVALID, "pread: unexpected end of file");
            done += got;
        }
    }
    return XMHW_OK;
}
int xmhw_pad_gaps(void* ts_dev, int itemsize, int64_t T, int64_t C, int64_t ld, const double* x_dev, double max_gap,
                  void* stream) {
    if (T < 0 || C < 0 || ld < C) return fail(XMHW_ERR_INVALID, "bad T/C/ld");
    if (itemsize != 4 && itemsize != 8) return fail(XMHW_ERR_INVALID, "itemsize must be 4 or 8");
    if (!(max_gap == max_gap)) return fail(XMHW_ERR_INVALID, "max_gap is NaN");
    if (T == 0 || C == 0) return XMHW_OK;
    if (!ts_dev || !x_dev) return fail(XMHW_ERR_INVALID, "NULL device buffer");
    return status_of(xmhw::launch_pad_gaps(ts_dev, itemsize, T, C, ld, x_dev, max_gap, static_cast<hipStream_t>(stream)),
                     "pad_gaps launch");
}
int xmhw_memset(void* dst, int value, size_t bytes, void* stream) {
    if (bytes == 0) return XMHW_OK;
    HIP_TRY(hipMemsetAsync(dst, value, bytes, static_cast<hipStream_t>(stream)));
    return XMHW_OK;
}
int xmhw_stream_create(void** stream) {
    if (!stream) return fail(XMHW_ERR_INVALID, "stream is NULL");
    hipStream_t s;
    HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    *stream = s;
    return XMHW_OK;
}
int xmhw_stream_destroy(void* stream) {
    if (stream) HIP_TRY(hipStreamDestroy(static_cast<hipStream_t>(stream)));
    return XMHW_OK;
}
int xmhw_stream_sync(void* stream) {
    HIP_TRY(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    return XMHW_OK;
}
int xmhw_event_create(void** event) {
    if (!event) return fail(XMHW_ERR_INVALID, "event is NULL");
    hipEvent_t ev;
    HIP_TRY(hipEventCreate(&ev));
    *event = ev;
    return XMHW_OK;
}
int xmhw_event_destroy(void* event) {
    if (event) HIP_TRY(hipEventDestroy(static_cast<hipEvent_t>(event)));
    return XMHW_OK;
}
int xmhw_event_record(void* event, void* stream) {
    HIP_TRY(hipEventRecord(static_cast<hipEvent_t>(event), static_cast<hipStream_t>(stream)));
    return XMHW_OK;
}
int xmhw_stream_wait_event(void* stream, void* event) {
    HIP_TRY(hipStreamWaitEvent(static_cast<hipStream_t>(stream), static_cast<hipEvent_t>(event), 0));
    return XMHW_OK;
}
int xmhw_event_elapsed_ms(void* start, void* stop, float* ms) {
    if (!ms) return fail(XMHW_ERR_INVALID, "ms is NULL");
    HIP_TRY(hipEventSynchronize(static_cast<hipEvent_t>(stop)));
    HIP_TRY(hipEventElapsedTime(ms, static_cast<hipEvent_t>(start), static_cast<hipEvent_t>(stop)));
    return XMHW_OK;
}

int xmhw_plan_create(const int32_t* doy_host, int64_t T, int32_t window_half_width, xmhw_plan** plan) {
    if (!plan) return fail(XMHW_ERR_INVALID, "plan is NULL");
    *plan = nullptr;
    if (!doy_host) return fail(XMHW_ERR_INVALID, "doy is NULL");
    xmhw_plan* p = new (std::nothrow) xmhw_plan();
    if (!p) return fail(XMHW_ERR_NOMEM, "out of host memory");
    if (!p->host.build(doy_host, T, window_half_width)) {
        std::string msg = p->host.error;
        delete p;
        return fail(XMHW_ERR_INVALID, msg);
    }
    // (the environment sets the default layout of new plans; a number this build does not have is ignored)
    if (const char* v = std::getenv("XMHW_RING2")) {
        const int32_t lay = std::atoi(v);
        if (xmhw::layout_compiled(lay) && (lay != XMHW_LAYOUT_SORTED || xmhw::sorted_pick_yps(p->host.w, p->host.ntracks) != 0))
            p->settings.layout = lay;
    }
    *plan = p;
    return XMHW_OK;
}
int xmhw_plan_set_layout(xmhw_plan* plan, int32_t layout) {
    if (!plan) return fail(XMHW_ERR_INVALID, "plan is NULL");
    if (!xmhw::layout_compiled(layout))
        return fail(XMHW_ERR_UNSUPPORTED,
                    "layout must be one of the XMHW_LAYOUT_* constants this library was built with: -2 (auto), -1, 8, 10, 12, "
                    "20, 21, 22, 40 (the plain second-generation layouts 0..7, 9, 11 left the build in round 4; 30..32 need "
                    "make RING4=1)");
    if (layout == XMHW_LAYOUT_SORTED && xmhw::sorted_pick_yps(plan->host.w, plan->host.ntracks) == 0)
        return fail(XMHW_ERR_UNSUPPORTED, "the sorted-list kernel is not instantiated for this window / record length");
    plan->settings.layout = layout;
    return XMHW_OK;
}
int xmhw_sorted_device_ok(int32_t* holds) {
    if (!holds) return fail(XMHW_ERR_INVALID, "NULL argument");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n < 1) return fail(XMHW_ERR_HIP, "no HIP device");
    *holds = sorted_device_ok() == 1 ? 1 : 0;
    return XMHW_OK;
}
int xmhw_plan_layout_in_use(const xmhw_plan* plan, int32_t* layout) {
    if (!plan || !layout) return fail(XMHW_ERR_INVALID, "NULL argument");
    const xmhw::Route r = plan_route(plan, 4);
    *layout = r.n ? r.launch[0].layout : -1;
    return XMHW_OK;
}
// deprecated aliases (rounds 2 and 3)
int xmhw_plan_set_ring2(xmhw_plan* plan, int32_t variant) { return xmhw_plan_set_layout(plan, variant); }
int xmhw_plan_ring2_in_use(const xmhw_plan* plan, int32_t* variant) { return xmhw_plan_layout_in_use(plan, variant); }
int xmhw_plan_f64_mode(const xmhw_plan* plan, int32_t* variant) {
    if (!plan || !variant) return fail(XMHW_ERR_INVALID, "NULL argument");
    const xmhw::Route r = plan_route(plan, 8);      // (the last launch: the 64-bit mode, or the generic kernel)
    *variant = r.n ? r.launch[r.n - 1].layout : -1;
    return XMHW_OK;
}
int xmhw_plan_destroy(xmhw_plan* plan) {
    delete plan;
    return XMHW_OK;
}
int xmhw_plan_info(const xmhw_plan* plan, int32_t* D, int32_t* ntracks, int32_t* kernel, int32_t* nsteps,
                   int32_t* step_min) {
    if (!plan) return fail(XMHW_ERR_INVALID, "plan is NULL");
    if (D) *D = plan->host.D;
    if (ntracks) *ntracks = plan->host.ntracks;
    if (kernel) {
        const xmhw::Route r = plan_route(plan, 4);
        *kernel = !r.n ? -1 : r.launch[0].family == xmhw::Family::Generic ? XMHW_KERNEL_GENERIC : XMHW_KERNEL_RING;
    }
    if (nsteps) *nsteps = plan->host.nsteps;
    if (step_min) *step_min = plan->host.step_min;
    return XMHW_OK;
}
int xmhw_plan_doys(const xmhw_plan* plan, int32_t* doys_out) {
    if (!plan || !doys_out) return fail(XMHW_ERR_INVALID, "NULL argument");
    std::memcpy(doys_out, plan->host.doys.data(), sizeof(int32_t) * plan->host.doys.size());
    return XMHW_OK;
}
int xmhw_plan_set_kernel(xmhw_plan* plan, int32_t kernel) {
    if (!plan) return fail(XMHW_ERR_INVALID, "plan is NULL");
    if (kernel < XMHW_KERNEL_AUTO || kernel > XMHW_KERNEL_GENERIC)
        return fail(XMHW_ERR_INVALID, "unknown kernel selector");
    plan->settings.kernel_choice = kernel;
    return XMHW_OK;
}
int xmhw_plan_set_timing(xmhw_plan* plan, int32_t enable) {
    if (!plan) return fail(XMHW_ERR_INVALID, "plan is NULL");
    plan->timing = enable != 0;
    return XMHW_OK;
}
int xmhw_plan_kernel_ms(xmhw_plan* plan, int32_t calls_back, float* ms) {
    if (!plan || !ms) return fail(XMHW_ERR_INVALID, "NULL argument");
    if (calls_back < 0 || calls_back >= 16 || static_cast<uint64_t>(calls_back) >= plan->tcalls)
        return fail(XMHW_ERR_INVALID, "no such timed call");
    const int slot = static_cast<int>((plan->tcalls - 1 - static_cast<uint64_t>(calls_back)) % 16);
    if (!plan->tev[2 * slot] || !plan->tev[2 * slot + 1]) return fail(XMHW_ERR_INVALID, "no such timed call");
    HIP_TRY(hipEventSynchronize(plan->tev[2 * slot + 1]));
    HIP_TRY(hipEventElapsedTime(ms, plan->tev[2 * slot], plan->tev[2 * slot + 1]));
    return XMHW_OK;
}
int xmhw_plan_set_narrowing(xmhw_plan* plan, int32_t enable) {
    if (!plan) return fail(XMHW_ERR_INVALID, "plan is NULL");
    plan->settings.narrowing = enable != 0;
    return XMHW_OK;
}
int xmhw_plan_narrowed(xmhw_plan* plan, int32_t* narrowed_out) {
    if (!plan || !narrowed_out) return fail(XMHW_ERR_INVALID, "NULL argument");
    *narrowed_out = 0;
    if (!plan->dev.narrow_flag) return XMHW_OK;
    uint32_t flag = 1;
    HIP_TRY(hipMemcpy(&flag, plan->dev.narrow_flag, sizeof(uint32_t), hipMemcpyDeviceToHost));
    *narrowed_out = flag == 0 ? 1 : 0;
    return XMHW_OK;
}
int xmhw_plan_set_chunks(xmhw_plan* plan, int32_t nchunks) {
    if (!plan) return fail(XMHW_ERR_INVALID, "plan is NULL");
    if (nchunks < 0) return fail(XMHW_ERR_INVALID, "nchunks must be >= 0");
    plan->host.nchunks_req = nchunks;
    return XMHW_OK;
}
int xmhw_plan_chunks_in_use(const xmhw_plan* plan, int64_t C, int32_t* nchunks) {
    if (!plan || !nchunks) return fail(XMHW_ERR_INVALID, "NULL argument");
    if (C < 0) return fail(XMHW_ERR_INVALID, "bad C");
    *nchunks = xmhw::ring_chunks(plan->host, plan_route(plan, 4), std::max<int64_t>(C, 1));
    return XMHW_OK;
}
int xmhw_plan_route(const xmhw_plan* plan, int32_t elem_bytes, double q, int64_t C, int32_t* out, int32_t n) {
    if (!plan || !out) return fail(XMHW_ERR_INVALID, "NULL argument");
    if (elem_bytes != 4 && elem_bytes != 8) return fail(XMHW_ERR_INVALID, "elem_bytes must be 4 or 8");
    if (C < 0) return fail(XMHW_ERR_INVALID, "bad C");
    if (n < XMHW_ROUTE_WORDS) return fail(XMHW_ERR_INVALID, "out holds fewer than XMHW_ROUTE_WORDS values");
    const xmhw::Route r = plan_route(plan, elem_bytes, q);
    std::fill(out, out + XMHW_ROUTE_WORDS, 0);
    out[0] = r.unsupported ? XMHW_ERR_UNSUPPORTED : XMHW_OK;
    out[1] = r.n;
    for (int32_t i = 0; i < r.n; ++i) {
        const xmhw::Launch& l = r.launch[i];
        const int32_t v[7] = {static_cast<int32_t>(l.family), l.layout, l.lanes, l.tpl, l.narrows, l.gated, l.counters};
        std::copy(v, v + 7, out + 2 + 7 * i);
    }
    out[23] = xmhw::ring_chunks(plan->host, r, std::max<int64_t>(C, 1));
    out[24] = xmhw::sorted_pick_yps(plan->host.w, plan->host.ntracks) == 0
                  ? 0 : static_cast<int32_t>(xmhw::sorted_pieces(plan->host, r, C));
    return XMHW_OK;
}
int xmhw_debug_stats_available(void) { return xmhw::ring_stats_built() ? 1 : 0; }
int xmhw_plan_debug_stats_n(xmhw_plan* plan, int enable, uint64_t* out, int32_t n) {
    if (!plan) return fail(XMHW_ERR_INVALID, "plan is NULL");
    if (out && n <= 0) return fail(XMHW_ERR_INVALID, "n must be > 0");
    if (enable && !plan->dev.stats) {
        HIP_TRY(hipMalloc(&plan->dev.stats, 16 * sizeof(unsigned long long)));
        HIP_TRY(hipMemset(plan->dev.stats, 0, 16 * sizeof(unsigned long long)));
    }
    if (out) {
        if (!plan->dev.stats) return fail(XMHW_ERR_INVALID, "stats not enabled");
        unsigned long long all[16];
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipMemcpy(all, plan->dev.stats, sizeof(all), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemset(plan->dev.stats, 0, sizeof(all)));
        for (int32_t i = 0; i < std::min<int32_t>(n, 16); ++i) out[i] = all[i];
    }
    return XMHW_OK;
}
// (the round-1 contract: 8 values)
int xmhw_plan_debug_stats(xmhw_plan* plan, int enable, uint64_t* out8) {
    return xmhw_plan_debug_stats_n(plan, enable, out8, 8);
}
int xmhw_plan_table(const xmhw_plan* plan, int32_t years_per_lane, uint32_t* table_out,
                    int32_t* ntracks_padded) {
    if (!plan) return fail(XMHW_ERR_INVALID, "plan is NULL");
    if (years_per_lane <= 0) return fail(XMHW_ERR_INVALID, "years_per_lane must be > 0");
    if (plan->host.ntracks > kSubs * years_per_lane)
        return fail(XMHW_ERR_INVALID, "years_per_lane too small for the number of tracks");
    if (ntracks_padded) *ntracks_padded = kSubs * years_per_lane;
    if (table_out) {
        std::vector<uint32_t> tab = plan->host.ring_table(kSubs, years_per_lane);
        std::memcpy(table_out, tab.data(), sizeof(uint32_t) * tab.size());
    }
    return XMHW_OK;
}

int xmhw_plan_sorted_info(const xmhw_plan* plan, int64_t C, int32_t* keys_per_list, int32_t* lds_bytes_per_wave,
                          int32_t* pieces) {
    if (!plan) return fail(XMHW_ERR_INVALID, "plan is NULL");
    const int32_t k = xmhw::sorted_pick_k(plan->host.w, plan->host.ntracks);
    if (k == 0) return fail(XMHW_ERR_UNSUPPORTED, "the sorted-list kernel is not instantiated for this window / record length");
    if (keys_per_list) *keys_per_list = k;
    if (lds_bytes_per_wave) *lds_bytes_per_wave = xmhw::sorted_lds_bytes(plan->host.w, plan->host.ntracks);
    if (pieces) *pieces = static_cast<int32_t>(xmhw::sorted_pieces(plan->host, plan_route(plan, 4), C));
    return XMHW_OK;
}

int xmhw_plan_sorted_table(const xmhw_plan* plan, int32_t pieces, int32_t* nchunks, int32_t* nrows, int32_t* ntp,
                           int32_t* chunks_out, uint32_t* table_out, uint32_t* flags_out) {
    if (!plan) return fail(XMHW_ERR_INVALID, "plan is NULL");
    const int32_t yps = xmhw::sorted_pick_yps(plan->host.w, plan->host.ntracks);
    if (yps == 0) return fail(XMHW_ERR_UNSUPPORTED, "the sorted-list kernel is not instantiated for this window / record length");
    const xmhw::Plan::SortedPlan sp = plan->host.sorted_plan(2 * yps, 24, std::max(pieces, 1));
    if (nchunks) *nchunks = static_cast<int32_t>(sp.chunks.size());
    if (nrows) *nrows = static_cast<int32_t>(sp.flags.size());
    if (ntp) *ntp = 2 * yps;
    if (chunks_out)
        for (size_t i = 0; i < sp.chunks.size(); ++i) {
            chunks_out[4 * i + 0] = sp.chunks[i].warm_start;
            chunks_out[4 * i + 1] = sp.chunks[i].begin;
            chunks_out[4 * i + 2] = sp.chunks[i].end;
            chunks_out[4 * i + 3] = sp.chunks[i].trow0;
        }
    if (table_out) std::memcpy(table_out, sp.table.data(), sizeof(uint32_t) * sp.table.size());
    if (flags_out) std::memcpy(flags_out, sp.flags.data(), sizeof(uint32_t) * sp.flags.size());
    return XMHW_OK;
}

int xmhw_plan_sorted_direct(const xmhw_plan* plan, int64_t C, int32_t* count) {
    if (!plan || !count) return fail(XMHW_ERR_INVALID, "NULL argument");
    if (C < 0) return fail(XMHW_ERR_INVALID, "bad C");
    const int32_t yps = xmhw::sorted_pick_yps(plan->host.w, plan->host.ntracks);
    if (yps == 0) return fail(XMHW_ERR_UNSUPPORTED, "the sorted-list kernel is not instantiated for this window / record length");
    const xmhw::Plan::SortedPlan sp = plan->host.sorted_plan(2 * yps, 24, xmhw::sorted_pieces(plan->host, plan_route(plan, 4), C));
    int32_t n = 0;
    for (size_t i = 0; i < sp.chunks.size(); ++i) n += sorted_onerow_enabled() && sp.direct(i, xmhw::sorted_direct_tracks(yps)) ? 1 : 0;
    *count = n;
    return XMHW_OK;
}

int xmhw_clim_raw_f32(xmhw_plan* plan, const float* ts, int64_t C, int64_t ld, double q, int negate,
                      double* thresh, double* seas, int64_t ldo, void* stream) {
    return clim_raw<float>(plan, ts, C, ld, q, negate, thresh, seas, ldo, stream);
}
int xmhw_clim_raw_f64(xmhw_plan* plan, const double* ts, int64_t C, int64_t ld, double q, int negate,
                      double* thresh, double* seas, int64_t ldo, void* stream) {
    return clim_raw<double>(plan, ts, C, ld, q, negate, thresh, seas, ldo, stream);
}

int xmhw_clim_raw_i16(xmhw_plan* plan, const int16_t* codes, int64_t C, int64_t ld, int big_endian, int has_scale,
                      double scale_factor, double add_offset, int has_fill, int32_t fill_code, int decoded_itemsize, double q,
                      int negate, double* thresh, double* seas, int64_t ldo, void* stream) {
    if (!plan) return fail(XMHW_ERR_INVALID, "plan is NULL");
    if (C < 0 || ld < C || ldo < C) return fail(XMHW_ERR_INVALID, "bad C/ld/ldo");
    if (!(q >= 0.0 && q <= 1.0)) return fail(XMHW_ERR_INVALID, "quantile must be in [0, 1]");
    if (decoded_itemsize != 4 && decoded_itemsize != 8) return fail(XMHW_ERR_INVALID, "decoded_itemsize must be 4 or 8");
    if (has_scale && !(scale_factor == scale_factor && add_offset == add_offset && scale_factor != 0.0))
        return fail(XMHW_ERR_INVALID, "scale_factor must be a non-zero number, add_offset a number");
    if (C == 0) return XMHW_OK;
    if (!codes || !thresh || !seas) return fail(XMHW_ERR_INVALID, "NULL device buffer");
    // the codes are read in place by the sorted-list kernel and its recomputation only: the plans and quantiles those
    // serve (w = 5, 9..48 tracks, quantile >= 0.85 or <= 0.15).  Anything else: xmhw_decode() + xmhw_clim_raw_f32 / _f64.
    const xmhw::Route route = call_route(plan, 4, q);
    if (!route.n || route.launch[0].family != xmhw::Family::Sorted)
        return fail(XMHW_ERR_UNSUPPORTED, "packed input runs on the sorted-list kernel only (w = 5, 9..48 tracks, quantile >= 0.85 or <= 0.15): "
                                         "decode the series (xmhw_decode) and call xmhw_clim_raw_f32 / _f64");
    xmhw::PackedI16 pk;
    pk.swap = big_endian ? 1 : 0;
    pk.fill = has_fill ? fill_code : 0x7FFFFFFF;
    int kneg = negate ? 1 : 0;
    if (!has_scale) {
        pk.mode = 3;
    } else if (decoded_itemsize == 4) {
        // float32 decode: the kernels key and sum float(code) * sf + of, exactly the series xmhw_decode() would write
        pk.mode = 1;
        pk.sf = static_cast<float>(scale_factor);
        pk.of = static_cast<float>(add_offset);
    } else {
        // float64 decode: code -> value is monotone (decreasing for a negative scale_factor: the kernels then key the
        // negated codes); the two selected codes and the mean of the codes are decoded in float64
        pk.mode = 2;
        pk.s = scale_factor;
        pk.o = add_offset;
        pk.val_neg = negate ? 1 : 0;
        kneg = (negate ? 1 : 0) ^ (scale_factor < 0.0 ? 1 : 0);
    }
    pk.key_neg = kneg;
    Ready rd;
    const int rc = ensure(plan, route, C, true, &rd);
    if (rc != XMHW_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const xmhw::Plan& h = plan->host;
    const hipError_t e = timed_launch(rd, st, [&] {
        return xmhw::launch_sorted_i16(codes, pk, C, ld, h.T, rd.table[0], rd.dev.sflags_s, rd.dev.chunks_s, rd.dev.nchunks_s, h.w,
                                       route.launch[0].tpl, h.ntracks, q, kneg, thresh, seas, ldo, st);
    });
    if (e != hipSuccess) return hip_fail(e, "packed climatology launch");
    return XMHW_OK;
}

int xmhw_clim_finish(const xmhw_plan* plan, const double* thresh_in, const double* seas_in, int64_t C,
                     int64_t ldo, int feb29_fix, int smooth, int smooth_width, double* thresh_out,
                     double* seas_out, void* stream) {
    if (!plan) return fail(XMHW_ERR_INVALID, "plan is NULL");
    if (smooth && (smooth_width <= 0 || smooth_width % 2 == 0))
        return fail(XMHW_ERR_INVALID, "Running average window should be odd");
    if (C < 0 || ldo < C) return fail(XMHW_ERR_INVALID, "bad C/ldo");
    if (C == 0) return XMHW_OK;
    if (!thresh_in || !seas_in || !thresh_out || !seas_out)
        return fail(XMHW_ERR_INVALID, "NULL device buffer");
    if (thresh_in == thresh_out || seas_in == seas_out)
        return fail(XMHW_ERR_INVALID, "in and out may not alias");
    const xmhw::Plan& h = plan->host;
    ScratchRef flags;           // per-column "has an absent group" flags of the one-pass finish kernel
    if (smooth && smooth_width == 31)
        if (int rc = claim_scratch(static_cast<hipStream_t>(stream), static_cast<size_t>(C), &flags)) return rc;
    return status_of(xmhw::launch_finish(thresh_in, seas_in, C, ldo, h.D, row_index(h, 59), row_index(h, 60),
                                         row_index(h, 61), feb29_fix, smooth, smooth ? smooth_width : 1, thresh_out,
                                         seas_out, static_cast<hipStream_t>(stream), static_cast<uint8_t*>(flags.get())),
                     "clim_finish launch");
}

int xmhw_clim_f32(const float* ts, const int32_t* doy, int64_t T, int64_t C, int32_t D, int32_t w,
                  double q, int smooth, int smooth_w, int feb29_fix, int negate, double* thresh,
                  double* seas, void* stream) {
    return clim_oneshot<float>(ts, doy, T, C, D, w, q, smooth, smooth_w, feb29_fix, negate, thresh, seas,
                               stream);
}
int xmhw_clim_f64(const double* ts, const int32_t* doy, int64_t T, int64_t C, int32_t D, int32_t w,
                  double q, int smooth, int smooth_w, int feb29_fix, int negate, double* thresh,
                  double* seas, void* stream) {
    return clim_oneshot<double>(ts, doy, T, C, D, w, q, smooth, smooth_w, feb29_fix, negate, thresh, seas,
                                stream);
}
int xmhw_clim_host_f32(const float* ts, const int32_t* doy, int64_t T, int64_t C, int32_t D, int32_t w,
                       double q, int smooth, int smooth_w, int feb29_fix, int negate, double* thresh,
                       double* seas) {
    return clim_host<float>(ts, doy, T, C, D, w, q, smooth, smooth_w, feb29_fix, negate, thresh, seas);
}
int xmhw_clim_host_f64(const double* ts, const int32_t* doy, int64_t T, int64_t C, int32_t D, int32_t w,
                       double q, int smooth, int smooth_w, int feb29_fix, int negate, double* thresh,
                       double* seas) {
    return clim_host<double>(ts, doy, T, C, D, w, q, smooth, smooth_w, feb29_fix, negate, thresh, seas);
}

int xmhw_land_mask_f32(const float* ts, int64_t T, int64_t C, int64_t ld, int anynans, uint8_t* keep,
                       void* stream) {
    if (C < 0 || ld < C || T <= 0) return fail(XMHW_ERR_INVALID, "bad T/C/ld");
    return status_of(xmhw::launch_land_mask<float>(ts, T, C, ld, anynans, keep, static_cast<hipStream_t>(stream)),
                     "land_mask launch");
}
int xmhw_land_mask_f64(const double* ts, int64_t T, int64_t C, int64_t ld, int anynans, uint8_t* keep,
                       void* stream) {
    if (C < 0 || ld < C || T <= 0) return fail(XMHW_ERR_INVALID, "bad T/C/ld");
    return status_of(xmhw::launch_land_mask<double>(ts, T, C, ld, anynans, keep, static_cast<hipStream_t>(stream)),
                     "land_mask launch");
}

int xmhw_land_mask_i16(const int16_t* codes, int64_t T, int64_t C, int64_t ld, int big_endian, int has_fill,
                       int32_t fill_code, int anynans, uint8_t* keep, void* stream) {
    if (C < 0 || ld < C || T <= 0) return fail(XMHW_ERR_INVALID, "bad T/C/ld");
    if (has_fill && (fill_code < -32768 || fill_code > 32767)) return fail(XMHW_ERR_INVALID, "fill_code is not an int16");
    if (C == 0) return XMHW_OK;
    if (!codes || !keep) return fail(XMHW_ERR_INVALID, "NULL device buffer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (!has_fill) {           // no code means "missing": every cell stays
        return status_of(hipMemsetAsync(keep, 1, static_cast<size_t>(C), st), "land_mask memset");
    }
    uint16_t raw = static_cast<uint16_t>(static_cast<int16_t>(fill_code));
    if (big_endian) raw = static_cast<uint16_t>((raw >> 8) | (raw << 8));
    return status_of(xmhw::launch_land_mask_i16(codes, T, C, ld, static_cast<int16_t>(raw), anynans, keep, st),
                     "land_mask launch");
}
int xmhw_gather_cells_i16(const int16_t* in, int64_t rows, int64_t ld_in, const int64_t* index, int64_t n,
                          int16_t* out, int64_t ld_out, void* stream) {
    if (rows < 0 || n < 0 || ld_out < n) return fail(XMHW_ERR_INVALID, "bad rows/n/ld_out");
    return status_of(xmhw::launch_gather_cells<int16_t>(in, rows, ld_in, index, n, out, ld_out,
                                                        static_cast<hipStream_t>(stream)),
                     "gather_cells launch");
}
int xmhw_gather_cells_f32(const float* in, int64_t rows, int64_t ld_in, const int64_t* index, int64_t n,
                          float* out, int64_t ld_out, void* stream) {
    if (rows < 0 || n < 0 || ld_out < n) return fail(XMHW_ERR_INVALID, "bad rows/n/ld_out");
    return status_of(xmhw::launch_gather_cells<float>(in, rows, ld_in, index, n, out, ld_out,
                                                      static_cast<hipStream_t>(stream)),
                     "gather_cells launch");
}
int xmhw_gather_cells_f64(const double* in, int64_t rows, int64_t ld_in, const int64_t* index, int64_t n,
                          double* out, int64_t ld_out, void* stream) {
    if (rows < 0 || n < 0 || ld_out < n) return fail(XMHW_ERR_INVALID, "bad rows/n/ld_out");
    return status_of(xmhw::launch_gather_cells<double>(in, rows, ld_in, index, n, out, ld_out,
                                                       static_cast<hipStream_t>(stream)),
                     "gather_cells launch");
}
int xmhw_scatter_cells_f64(const double* in, int64_t rows, int64_t ld_in, const int64_t* index, int64_t n,
                           double* out, int64_t ld_out, void* stream) {
    if (rows < 0 || n < 0 || ld_in < n) return fail(XMHW_ERR_INVALID, "bad rows/n/ld_in");
    return status_of(xmhw::launch_scatter_cells(in, rows, ld_in, index, n, out, ld_out, ld_out,
                                                static_cast<hipStream_t>(stream)),
                     "scatter_cells launch");
}

int xmhw_detect_events_f32(const float* ts, int64_t T, int64_t C, int64_t ld, const double* thresh, int64_t ldt,
                           const int32_t* row_of_t, int32_t min_duration, int32_t join_gaps, int32_t max_gap,
                           int32_t negate, int32_t* events, int32_t* start, int32_t* end, uint8_t* bthresh,
                           int64_t ldo, int32_t* nevents, void* stream) {
    return detect_events<float>(ts, T, C, ld, thresh, ldt, row_of_t, min_duration, join_gaps, max_gap, negate,
                                events, start, end, bthresh, ldo, nevents, stream);
}
int xmhw_detect_events_f64(const double* ts, int64_t T, int64_t C, int64_t ld, const double* thresh, int64_t ldt,
                           const int32_t* row_of_t, int32_t min_duration, int32_t join_gaps, int32_t max_gap,
                           int32_t negate, int32_t* events, int32_t* start, int32_t* end, uint8_t* bthresh,
                           int64_t ldo, int32_t* nevents, void* stream) {
    return detect_events<double>(ts, T, C, ld, thresh, ldt, row_of_t, min_duration, join_gaps, max_gap, negate,
                                 events, start, end, bthresh, ldo, nevents, stream);
}

int xmhw_count_events(const int32_t* start, int64_t T, int64_t C, int64_t ldo, int32_t* nevents, void* stream) {
    if (T <= 0 || C < 0 || ldo < C) return fail(XMHW_ERR_INVALID, "bad T/C/ldo");
    if (C == 0) return XMHW_OK;
    if (!start || !nevents) return fail(XMHW_ERR_INVALID, "NULL buffer");
    return status_of(xmhw::launch_count_events(start, T, C, ldo, nevents, static_cast<hipStream_t>(stream)),
                     "count_events launch");
}
int xmhw_event_stats_f32(const float* ts, int64_t T, int64_t C, int64_t ld, const double* seas,
                         const double* thresh, int64_t ldc, const int32_t* row_of_t, int32_t negate,
                         const int32_t* events, int64_t ldo, const int64_t* offsets, double* table, void* stream) {
    return event_stats<float>(ts, T, C, ld, seas, thresh, ldc, row_of_t, negate, events, ldo, offsets, table, stream);
}
int xmhw_event_stats_f64(const double* ts, int64_t T, int64_t C, int64_t ld, const double* seas,
                         const double* thresh, int64_t ldc, const int32_t* row_of_t, int32_t negate,
                         const int32_t* events, int64_t ldo, const int64_t* offsets, double* table, void* stream) {
    return event_stats<double>(ts, T, C, ld, seas, thresh, ldc, row_of_t, negate, events, ldo, offsets, table, stream);
}
int xmhw_set_exceed_kernel(int32_t mode) {
    if (mode < 0 || mode > 2) return fail(XMHW_ERR_INVALID, "mode must be 0 (auto), 1 (per-step) or 2 (tiled)");
    g_exceed_kernel = mode;
    return XMHW_OK;
}
int xmhw_exceed_bits_f32(const float* ts, int64_t T, int64_t C, int64_t ld, const double* thresh, int64_t ldt,
                         int64_t D, const int32_t* row_of_t, int32_t negate, uint64_t* bits, int64_t ldb,
                         void* stream) {
    return exceed_bits<float>(ts, T, C, ld, thresh, ldt, D, row_of_t, negate, bits, ldb, stream);
}
int xmhw_exceed_bits_f64(const double* ts, int64_t T, int64_t C, int64_t ld, const double* thresh, int64_t ldt,
                         int64_t D, const int32_t* row_of_t, int32_t negate, uint64_t* bits, int64_t ldb,
                         void* stream) {
    return exceed_bits<double>(ts, T, C, ld, thresh, ldt, D, row_of_t, negate, bits, ldb, stream);
}
int xmhw_events_from_bits(const uint64_t* bits, int64_t T, int64_t C, int64_t ldb, int32_t min_duration,
                          int32_t join_gaps, int32_t max_gap, const int64_t* offsets, int32_t* nevents,
                          double* table, void* stream) {
    if (T <= 0 || C < 0 || ldb < C) return fail(XMHW_ERR_INVALID, "bad T/C/ldb");
    if (C == 0) return XMHW_OK;
    if (!bits || (!offsets && !nevents) || (offsets && !table)) return fail(XMHW_ERR_INVALID, "NULL buffer");
    if (min_duration < 1 || max_gap < 0) return fail(XMHW_ERR_INVALID, "bad minDuration/maxGap");
    return status_of(xmhw::launch_events_from_bits(bits, T, C, ldb, min_duration, join_gaps, max_gap, offsets, nevents,
                                                   table, static_cast<hipStream_t>(stream)),
                     "events_from_bits launch");
}
int xmhw_event_stats_sparse_f32(const float* ts, int64_t T, int64_t C, int64_t ld, const double* seas,
                                const double* thresh, int64_t ldc, const int32_t* row_of_t, int32_t negate,
                                int64_t n_events, double* table, void* stream) {
    return event_stats_sparse<float>(ts, T, C, ld, seas, thresh, ldc, row_of_t, negate, n_events, table, stream);
}
int xmhw_event_stats_sparse_f64(const double* ts, int64_t T, int64_t C, int64_t ld, const double* seas,
                                const double* thresh, int64_t ldc, const int32_t* row_of_t, int32_t negate,
                                int64_t n_events, double* table, void* stream) {
    return event_stats_sparse<double>(ts, T, C, ld, seas, thresh, ldc, row_of_t, negate, n_events, table, stream);
}
int xmhw_event_intermediate_f32(const float* ts, int64_t T, int64_t C, int64_t ld, const double* seas,
                                const double* thresh, int64_t ldc, const int32_t* row_of_t, int32_t negate,
                                const int32_t* events, int64_t ldo, double* out, int64_t ldv, uint8_t* dur,
                                void* stream) {
    return event_intermediate<float>(ts, T, C, ld, seas, thresh, ldc, row_of_t, negate, events, ldo, out, ldv, dur,
                                     stream);
}
int xmhw_event_intermediate_f64(const double* ts, int64_t T, int64_t C, int64_t ld, const double* seas,
                                const double* thresh, int64_t ldc, const int32_t* row_of_t, int32_t negate,
                                const int32_t* events, int64_t ldo, double* out, int64_t ldv, uint8_t* dur,
                                void* stream) {
    return event_intermediate<double>(ts, T, C, ld, seas, thresh, ldc, row_of_t, negate, events, ldo, out, ldv, dur,
                                      stream);
}
int xmhw_release_cached_tables(void) {
    release_cached_tables();
    return XMHW_OK;
}
int xmhw_offsets_from_counts(const int32_t* counts_dev, int64_t n, int64_t* offsets_dev, void* stream) {
    if (n < 0) return fail(XMHW_ERR_INVALID, "n must be >= 0");
    if (!offsets_dev || (n > 0 && !counts_dev)) return fail(XMHW_ERR_INVALID, "NULL buffer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t nblocks = (n + 1023) / 1024;
    ScratchRef scratch;
    if (int rc = claim_scratch(st, sizeof(int64_t) * static_cast<size_t>(nblocks + 1), &scratch)) return rc;
    return status_of(xmhw::launch_offsets_from_counts(counts_dev, n, offsets_dev, static_cast<int64_t*>(scratch.get()), st),
                     "offsets_from_counts launch");
}

int xmhw_block_events(const double* table, const int64_t* offsets, int64_t C, const int32_t* bin_of_t, int64_t T,
                      int32_t nbins, int32_t mtime_column, double* out, int64_t ldo, void* stream) {
    if (C < 0 || T <= 0 || nbins <= 0 || ldo < C) return fail(XMHW_ERR_INVALID, "bad C/T/nbins/ldo");
    if (mtime_column < 0 || mtime_column >= xmhw::kEventColumns) return fail(XMHW_ERR_INVALID, "bad mtime column");
    if (C == 0) return XMHW_OK;
    if (!table || !offsets || !bin_of_t || !out) return fail(XMHW_ERR_INVALID, "NULL buffer");
    return status_of(xmhw::launch_block_events(table, offsets, C, bin_of_t, T, nbins, mtime_column, out, ldo,
                                               static_cast<hipStream_t>(stream)),
                     "block_events launch");
}
int xmhw_block_time_f32(const float* ts, int64_t T, int64_t C, int64_t ld, const double* cats, int64_t ldcat,
                        const int32_t* bin_of_t, int32_t nbins, double* out, int64_t ldo, void* stream) {
    return block_time<float>(ts, T, C, ld, cats, ldcat, bin_of_t, nbins, out, ldo, stream);
}
int xmhw_block_time_f64(const double* ts, int64_t T, int64_t C, int64_t ld, const double* cats, int64_t ldcat,
                        const int32_t* bin_of_t, int32_t nbins, double* out, int64_t ldo, void* stream) {
    return block_time<double>(ts, T, C, ld, cats, ldcat, bin_of_t, nbins, out, ldo, stream);
}

int xmhw_event_rank(const double* table, int64_t ld_table, const int64_t* offsets, int64_t C, const int32_t* columns,
                    int32_t ncols, double n_years, double* rank, double* rp, int64_t ld_out, void* stream) {
    if (C < 0 || ld_table < 1) return fail(XMHW_ERR_INVALID, "bad C/ld_table");
    if (ncols < 1 || ncols > xmhw::kEventColumns) return fail(XMHW_ERR_INVALID, "ncols must be in 1..31");
    if (!columns) return fail(XMHW_ERR_INVALID, "NULL column list");
    for (int32_t k = 0; k < ncols; ++k)
        if (columns[k] < 0 || columns[k] >= ld_table) return fail(XMHW_ERR_INVALID, "column outside the table row (ld_table)");
    if (ld_out < ncols) return fail(XMHW_ERR_INVALID, "ld_out must be >= ncols");
    if (!(n_years > 0.0) || !std::isfinite(n_years)) return fail(XMHW_ERR_INVALID, "n_years must be finite and > 0");
    if (C == 0) return XMHW_OK;
    if (!table || !offsets || !rank || !rp) return fail(XMHW_ERR_INVALID, "NULL buffer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    // scratch: item counts (int32, C), item offsets (int64, C + 1), the scan's block sums, the item counter
    const size_t n_counts = static_cast<size_t>(C + 1) & ~size_t{1};
    const size_t n_sums = static_cast<size_t>((C + 1023) / 1024 + 1);
    ScratchRef scratch;
    const size_t bytes = sizeof(int32_t) * n_counts + sizeof(int64_t) * (static_cast<size_t>(C) + 2 + n_sums);
    if (int rc = claim_scratch(st, bytes, &scratch)) return rc;
    void* sp = scratch.get();
    int32_t* counts = static_cast<int32_t*>(sp);
    int64_t* item_off = reinterpret_cast<int64_t*>(counts + n_counts);
    int64_t* sums = item_off + C + 1;
    unsigned long long* next_item = reinterpret_cast<unsigned long long*>(sums + n_sums);
    // one launch per window of at most kRankWindow table columns (the ranked columns of detect(): two)
    std::vector<std::pair<int32_t, int32_t>> cols;             // (table column, output column)
    for (int32_t k = 0; k < ncols; ++k) cols.push_back({columns[k], k});
    std::sort(cols.begin(), cols.end());
    for (size_t a = 0; a < cols.size();) {
        xmhw::RankColumns rc{};
        rc.cmin = cols[a].first;
        size_t b = a;
        while (b < cols.size() && b - a < xmhw::kRankWindow && cols[b].first - rc.cmin < xmhw::kRankWindow) {
            rc.col[b - a] = cols[b].first;
            rc.out[b - a] = cols[b].second;
            ++b;
        }
        rc.ncols = static_cast<int32_t>(b - a);
        rc.span = cols[b - 1].first - rc.cmin + 1;
        const hipError_t e = xmhw::launch_event_rank(table, ld_table, offsets, C, rc, n_years, rank, rp, ld_out, counts, item_off,
                                                     sums, next_item, st);
        if (int err = status_of(e, "event_rank launch")) return err;
        a = b;
    }
    return XMHW_OK;
}

static int trend_args(const double* y, int32_t nstat, int32_t nb, int64_t C, int64_t ld, const double* x, const double* out,
               int64_t ldo) {
    if (nstat < 0 || nb < 0 || C < 0) return fail(XMHW_ERR_INVALID, "bad nstat/nb/C");
    if (ld < C) return fail(XMHW_ERR_INVALID, "ld must be >= C");
    if (ldo < C) return fail(XMHW_ERR_INVALID, "ldo must be >= C");
    if (nstat == 0 || C == 0) return XMHW_OK;
    if (!out) return fail(XMHW_ERR_INVALID, "NULL output buffer");
    if (nb > 0 && (!y || !x)) return fail(XMHW_ERR_INVALID, "NULL buffer");
    return XMHW_OK;
}

int xmhw_block_trend_ols(const double* y, int32_t nstat, int32_t nb, int64_t C, int64_t ld, const double* x,
                         const double* tcrit, double* out, int64_t ldo, void* stream) {
    if (int rc = trend_args(y, nstat, nb, C, ld, x, out, ldo)) return rc;
    if (nstat == 0 || C == 0) return XMHW_OK;
    if (nb >= 3 && !tcrit) return fail(XMHW_ERR_INVALID, "NULL tcrit table");
    if (static_cast<int64_t>(nstat) * ((C + 63) / 64) > 0x7FFFFFFFll) return fail(XMHW_ERR_UNSUPPORTED, "nstat * C too large for one launch");
    return status_of(xmhw::launch_trend_ols(y, nstat, nb, C, ld, x, tcrit, out, ldo, static_cast<hipStream_t>(stream)),
                     "trend_ols launch");
}

int xmhw_block_trend_theil_sen(const double* y, int32_t nstat, int32_t nb, int64_t C, int64_t ld, const double* x,
                               double* out, int64_t ldo, void* stream) {
    if (int rc = trend_args(y, nstat, nb, C, ld, x, out, ldo)) return rc;
    if (nb > xmhw::kTrendMaxBlocks)
        return fail(XMHW_ERR_UNSUPPORTED, "Theil-Sen trend: nb above the cap of " + std::to_string(xmhw::kTrendMaxBlocks) + " blocks");
    if (nstat == 0 || C == 0) return XMHW_OK;
    if (static_cast<int64_t>(nstat) * ((C + 15) / 16) > 0x7FFFFFFFll) return fail(XMHW_ERR_UNSUPPORTED, "nstat * C too large for one launch");
    return status_of(xmhw::launch_trend_theil_sen(y, nstat, nb, C, ld, x, out, ldo, static_cast<hipStream_t>(stream)),
                     "trend_theil_sen launch");
}

int xmhw_series_fit_f32(const float* ts, int64_t T, int64_t C, int64_t ld, const double* basis, int32_t P,
                        const uint8_t* weight, int32_t min_valid, double* coef, int64_t ldc, int32_t* nvalid, void* stream) {
    return series_fit<float>(ts, T, C, ld, basis, P, weight, min_valid, coef, ldc, nvalid, stream);
}
int xmhw_series_fit_f64(const double* ts, int64_t T, int64_t C, int64_t ld, const double* basis, int32_t P,
                        const uint8_t* weight, int32_t min_valid, double* coef, int64_t ldc, int32_t* nvalid, void* stream) {
    return series_fit<double>(ts, T, C, ld, basis, P, weight, min_valid, coef, ldc, nvalid, stream);
}
int xmhw_series_remove_f32(float* ts, int64_t T, int64_t C, int64_t ld, const double* basis, int32_t P, int32_t R,
                           const double* coef, int64_t ldc, void* stream) {
    return series_remove<float>(ts, T, C, ld, basis, P, R, coef, ldc, stream);
}
int xmhw_series_remove_f64(double* ts, int64_t T, int64_t C, int64_t ld, const double* basis, int32_t P, int32_t R,
                           const double* coef, int64_t ldc, void* stream) {
    return series_remove<double>(ts, T, C, ld, basis, P, R, coef, ldc, stream);
}

int xmhw_event_objects(const int32_t* start, const int32_t* end, int64_t n, const int64_t* offsets, int64_t C,
                       const int32_t* nbr, int32_t K, int32_t gap, int32_t* cell_of_row, int32_t* root, void* stream) {
    if (n < 0 || C < 0) return fail(XMHW_ERR_INVALID, "bad n/C");
    if (K < 1 || gap < 0) return fail(XMHW_ERR_INVALID, "K must be >= 1 and gap >= 0");
    if (n > 0x7FFFFFFFll || C > 0x7FFFFFFFll) return fail(XMHW_ERR_UNSUPPORTED, "event_objects: 2^31 rows or cells and more");
    if (n == 0) return XMHW_OK;
    if (C == 0) return fail(XMHW_ERR_INVALID, "rows without cells");
    if (!start || !end || !offsets || !nbr || !cell_of_row || !root) return fail(XMHW_ERR_INVALID, "NULL buffer");
    return status_of(xmhw::launch_event_objects(start, end, n, offsets, C, nbr, K, gap, cell_of_row, root,
                                                static_cast<hipStream_t>(stream)),
                     "event_objects launch");
}

int xmhw_object_reduce(const int32_t* start, const int32_t* end, const double* imax, int64_t n, const int32_t* cell_of_row,
                       const int64_t* offsets, const int64_t* wq, const int32_t* slot, int64_t n_slots, int32_t* n_events,
                       int32_t* n_cells, int32_t* time_start, int32_t* time_end, int64_t* cell_days, int64_t* area_days_q,
                       double* intensity_max, int32_t* peak_row, void* stream) {
    if (n < 0 || n_slots < 0) return fail(XMHW_ERR_INVALID, "bad n/n_slots");
    if (n > 0x7FFFFFFFll || n_slots > 0x7FFFFFFFll) return fail(XMHW_ERR_UNSUPPORTED, "object_reduce: 2^31 rows or slots and more");
    if (n_slots == 0) return XMHW_OK;
    if (!n_events || !n_cells || !time_start || !time_end || !cell_days || !area_days_q || !intensity_max || !peak_row)
        return fail(XMHW_ERR_INVALID, "NULL output buffer");
    if (n > 0 && (!start || !end || !imax || !cell_of_row || !offsets || !wq || !slot)) return fail(XMHW_ERR_INVALID, "NULL buffer");
    return status_of(xmhw::launch_object_reduce(start, end, imax, n, cell_of_row, offsets, wq, slot, n_slots, n_events,
                                                n_cells, time_start, time_end, cell_days, area_days_q, intensity_max,
                                                peak_row, static_cast<hipStream_t>(stream)),
                     "object_reduce launch");
}

int xmhw_object_tracks(const int32_t* start, const int32_t* end, int64_t n, const int32_t* slot, const int32_t* cell_of_row,
                       int64_t C, const int64_t* vec, int64_t ldv, const int32_t* time_start, const int64_t* offsets,
                       int64_t n_slots, int64_t L, int32_t* n_cells, int64_t* sums, int64_t ld, int32_t* n_bad, void* stream) {
    if (n < 0 || C < 0 || n_slots < 0 || L < 0) return fail(XMHW_ERR_INVALID, "bad n/C/n_slots/L");
    if (n > 0x7FFFFFFFll || n_slots > 0x7FFFFFFFll || L >= 0x7FFFFFFFll)
        return fail(XMHW_ERR_UNSUPPORTED, "object_tracks: 2^31 rows, slots or series entries (L + 1) and more");
    if (ld < L + 1 || ldv < C) return fail(XMHW_ERR_INVALID, "ld must be >= L + 1 and ldv >= C");
    if (!n_cells || !sums || !n_bad) return fail(XMHW_ERR_INVALID, "NULL output buffer");
    if (n > 0 && n_slots > 0 && L > 0 && (!start || !end || !slot || !cell_of_row || !vec || !time_start || !offsets))
        return fail(XMHW_ERR_INVALID, "NULL buffer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    // the levels of tile sums live in this stream's scratch buffer
    ScratchRef scratch;
    if (int rc = claim_scratch(st, xmhw::object_tracks_scratch_bytes(L + 1), &scratch)) return rc;
    return status_of(xmhw::launch_object_tracks(start, end, n, slot, cell_of_row, C, vec, ldv, time_start, offsets, n_slots,
                                                L, n_cells, sums, ld, n_bad, static_cast<int64_t*>(scratch.get()), st),
                     "object_tracks launch");
}

int xmhw_object_parts(const int32_t* start, const int32_t* end, const int32_t* slot, const int32_t* cell_of_row, int64_t n,
                      const int64_t* row_offsets, int64_t C, const int32_t* nbr, int32_t K, const int64_t* wq,
                      const int64_t* vox_off, int64_t V, const int32_t* time_start, const int64_t* offsets, int64_t n_slots,
                      int64_t L, int32_t* n_parts, int32_t* cells_largest, int64_t* area_largest_q, int32_t* n_bad,
                      void* stream) {
    if (n < 0 || C < 0 || n_slots < 0 || L < 0 || V < 0) return fail(XMHW_ERR_INVALID, "bad n/C/n_slots/L/V");
    if (K < 1) return fail(XMHW_ERR_INVALID, "K must be >= 1");
    if (n > 0x7FFFFFFFll || C > 0x7FFFFFFFll || n_slots > 0x7FFFFFFFll || L > 0x7FFFFFFFll || V > 0x7FFFFFFFll)
        return fail(XMHW_ERR_UNSUPPORTED, "object_parts: 2^31 rows, cells, slots, series entries or voxels and more");
    if (!n_bad || (L > 0 && (!n_parts || !cells_largest || !area_largest_q))) return fail(XMHW_ERR_INVALID, "NULL output buffer");
    if (n > 0 && n_slots > 0 && L > 0 &&
        (!start || !end || !slot || !cell_of_row || !row_offsets || !nbr || !wq || !vox_off || !time_start || !offsets))
        return fail(XMHW_ERR_INVALID, "NULL buffer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    // parent, cells and area of every voxel live in this stream's scratch buffer
    ScratchRef scratch;
    if (int rc = claim_scratch(st, xmhw::object_parts_scratch_bytes(V), &scratch)) return rc;
    return status_of(xmhw::launch_object_parts(start, end, slot, cell_of_row, n, row_offsets, C, nbr, K, wq, vox_off, V,
                                               time_start, offsets, n_slots, L, n_parts, cells_largest, area_largest_q,
                                               n_bad, scratch.get(), st),
                     "object_parts launch");
}

static_assert(xmhw::kGenealogyVoxelBytes == XMHW_GENEALOGY_VOXEL_BYTES && xmhw::kGenealogySlotBytes == XMHW_GENEALOGY_SLOT_BYTES &&
                  xmhw::kGenealogyFields == XMHW_GENEALOGY_FIELDS && xmhw::kGenealogyParts == XMHW_GENEALOGY_PARTS &&
                  xmhw::kGenealogyLinks == XMHW_GENEALOGY_LINKS && xmhw::kGenealogyBorn == XMHW_GENEALOGY_BORN &&
                  xmhw::kGenealogyMerged == XMHW_GENEALOGY_MERGED && xmhw::kGenealogyEnded == XMHW_GENEALOGY_ENDED &&
                  xmhw::kGenealogySplit == XMHW_GENEALOGY_SPLIT,
              "the genealogy constants of include/xmhw_amd.h and kernels.h differ");

int xmhw_object_genealogy(const int32_t* start, const int32_t* end, const int32_t* slot, const int32_t* cell_of_row, int64_t n,
                          const int64_t* row_offsets, int64_t C, const int32_t* nbr, int32_t K, const int64_t* vox_off,
                          int64_t V, const int32_t* time_start, const int64_t* offsets, int64_t n_slots, int64_t L,
                          int32_t* counts, uint64_t* edges, int64_t edge_capacity, int64_t* n_edges, int32_t* n_bad,
                          int32_t* overflow, void* stream) {
    if (n < 0 || C < 0 || n_slots < 0 || L < 0 || V < 0 || edge_capacity < 0)
        return fail(XMHW_ERR_INVALID, "bad n/C/n_slots/L/V/edge_capacity");
    if (K < 1) return fail(XMHW_ERR_INVALID, "K must be >= 1");
    if (n > 0x7FFFFFFFll || C > 0x7FFFFFFFll || n_slots > 0x7FFFFFFFll || L > 0x7FFFFFFFll || V > 0x7FFFFFFFll ||
        edge_capacity > 0x7FFFFFFFll)
        return fail(XMHW_ERR_UNSUPPORTED, "object_genealogy: 2^31 rows, cells, slots, series entries, voxels or edges and more");
    if (!n_bad || !overflow || !n_edges || (L > 0 && !counts) || (edge_capacity > 0 && !edges))
        return fail(XMHW_ERR_INVALID, "NULL output buffer");
    if (n > 0 && n_slots > 0 && L > 0 &&
        (!start || !end || !slot || !cell_of_row || !row_offsets || !nbr || !vox_off || !time_start || !offsets))
        return fail(XMHW_ERR_INVALID, "NULL buffer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    // the hash set and parent, indeg, outdeg of every voxel: this stream's scratch
    ScratchRef scratch;
    if (int rc = claim_scratch(st, xmhw::object_genealogy_scratch_bytes(V, edge_capacity), &scratch)) return rc;
    return status_of(xmhw::launch_object_genealogy(start, end, slot, cell_of_row, n, row_offsets, C, nbr, K, vox_off, V,
                                                   time_start, offsets, n_slots, L, counts, edges, edge_capacity, n_edges,
                                                   n_bad, overflow, scratch.get(), st),
                     "object_genealogy launch");
}

static_assert(xmhw::kShapeClasses == XMHW_SHAPE_CLASSES && xmhw::kShapeOpen == XMHW_SHAPE_OPEN &&
                  xmhw::kShapeCoast == XMHW_SHAPE_COAST && xmhw::kShapeBorder == XMHW_SHAPE_BORDER &&
                  xmhw::kShapeFaceCoast == XMHW_SHAPE_FACE_COAST && xmhw::kShapeFaceBorder == XMHW_SHAPE_FACE_BORDER &&
                  xmhw::kShapeFaceFolded == XMHW_SHAPE_FACE_FOLDED,
              "the shape constants of include/xmhw_amd.h and kernels.h differ");

int xmhw_object_shape(const int32_t* start, const int32_t* end, const int32_t* slot, const int32_t* cell_of_row, int64_t n,
                      const int64_t* row_offsets, int64_t C, const int32_t* faces, int32_t K, const int64_t* lq,
                      const int32_t* time_start, const int64_t* offsets, int64_t n_slots, int64_t L, int32_t* edges,
                      int64_t* perimeter_q, int32_t* cells_edge, int32_t* n_bad, void* stream) {
    if (n < 0 || C < 0 || n_slots < 0 || L < 0) return fail(XMHW_ERR_INVALID, "bad n/C/n_slots/L");
    if (K != 4) return fail(XMHW_ERR_UNSUPPORTED, "object_shape: a cell has K = 4 faces");
    if (n > 0x7FFFFFFFll || C > 0x7FFFFFFFll || n_slots > 0x7FFFFFFFll || L > 0x7FFFFFFFll)
        return fail(XMHW_ERR_UNSUPPORTED, "object_shape: 2^31 rows, cells, slots or series entries and more");
    if (!n_bad || (L > 0 && (!edges || !perimeter_q || !cells_edge))) return fail(XMHW_ERR_INVALID, "NULL output buffer");
    if (n > 0 && n_slots > 0 && L > 0 &&
        (!start || !end || !slot || !cell_of_row || !row_offsets || !faces || !lq || !time_start || !offsets))
        return fail(XMHW_ERR_INVALID, "NULL buffer");
    return status_of(xmhw::launch_object_shape(start, end, slot, cell_of_row, n, row_offsets, C, faces, lq, time_start,
                                               offsets, n_slots, L, edges, perimeter_q, cells_edge, n_bad,
                                               static_cast<hipStream_t>(stream)),
                     "object_shape launch");
}

int xmhw_synth_sst_f32(float* ts, int64_t T, int64_t C, int64_t ld, int64_t cell0, uint64_t seed,
                       double nan_frac, void* stream) {
    if (C < 0 || ld < C || T <= 0) return fail(XMHW_ERR_INVALID, "bad T/C/ld");
    return status_of(xmhw::launch_synth<float>(ts, T, C, ld, cell0, seed, nan_frac, static_cast<hipStream_t>(stream)),
                     "synth launch");
}
int xmhw_synth_sst_ex_f32(float* ts, int64_t T, int64_t C, int64_t ld, int64_t cell0, uint64_t seed, double nan_frac,
                          double quant, double ice_frac, double rho, int64_t ice_patch, void* stream) {
    if (!ts || T < 0 || C < 0 || ld < C) return fail(XMHW_ERR_INVALID, "bad argument");
    if (!(rho >= 0.0 && rho < 1.0) || quant < 0.0 || ice_frac < 0.0 || ice_frac > 1.0)
        return fail(XMHW_ERR_INVALID, "rho must be in [0, 1), quant >= 0, ice_frac in [0, 1]");
    return status_of(xmhw::launch_synth_ex<float>(ts, T, C, ld, cell0, seed, nan_frac, quant, ice_frac, rho, ice_patch,
                                                  static_cast<hipStream_t>(stream)),
                     "synth launch");
}
int xmhw_synth_sst_f64(double* ts, int64_t T, int64_t C, int64_t ld, int64_t cell0, uint64_t seed,
                       double nan_frac, void* stream) {
    if (C < 0 || ld < C || T <= 0) return fail(XMHW_ERR_INVALID, "bad T/C/ld");
    return status_of(xmhw::launch_synth<double>(ts, T, C, ld, cell0, seed, nan_frac, static_cast<hipStream_t>(stream)),
                     "synth launch");
}

}  // extern "C"
