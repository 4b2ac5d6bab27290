// route.cpp -- see route.h.
#include "route.h"

#include <algorithm>
#include <cstdlib>

#include "../../include/xmhw_amd.h"
#include "kernels.h"

namespace xmhw {
namespace {

static_assert(int(Family::Generic) == XMHW_ROUTE_GENERIC && int(Family::Ring1) == XMHW_ROUTE_RING1 &&
              int(Family::Ring2) == XMHW_ROUTE_RING2 && int(Family::Ring3) == XMHW_ROUTE_RING3 &&
              int(Family::Ring4) == XMHW_ROUTE_RING4 && int(Family::Sorted) == XMHW_ROUTE_SORTED, "XMHW_ROUTE_*");

// layout number -> kernel generation and lanes per cell.  8 / 10 / 12: the second-generation kernel (kernels_ring2.hip);
// 20 / 21 / 22: the third (kernels_ring3.hip); 30 / 31 / 32: the round-4 key-store experiment (kernels_ring4.hip, built
// with `make RING4=1` only: profiles/r4_store_experiment.txt).
struct LayoutDef { int32_t layout; Family family; int32_t lanes; };
constexpr LayoutDef kLayouts[] = {
    {8, Family::Ring2, 8},  {10, Family::Ring2, 4}, {12, Family::Ring2, 16},
    {20, Family::Ring3, 8}, {21, Family::Ring3, 4}, {22, Family::Ring3, 2},
#ifdef XMHW_RING4
    {30, Family::Ring4, 8}, {31, Family::Ring4, 4}, {32, Family::Ring4, 2},
#endif
};
const LayoutDef* find_layout(int32_t layout) {
    for (const LayoutDef& d : kLayouts)
        if (d.layout == layout) return &d;
    return nullptr;
}

// tracks per lane of the layout on this plan, 0 if it is not instantiated
int32_t pick_tpl(const LayoutDef& d, const Plan& h) {
    switch (d.family) {
        case Family::Ring2: return ring2_pick_yps(h.w, h.ntracks, d.layout);
        case Family::Ring3: return ring3_pick_yps(h.w, h.ntracks, d.lanes);
#ifdef XMHW_RING4
        case Family::Ring4: return ring4_pick_yps(h.w, h.ntracks, d.lanes);
#endif
        default: return 0;
    }
}
// the float32 kernel of the layout, or its narrowing twin (float64 input read as float32), exists
bool instantiated(const LayoutDef& d, int32_t w, int32_t tpl, bool narrowing) {
    switch (d.family) {
        case Family::Ring2: return narrowing ? ring2_narrowing_supported(w, tpl, d.layout) : ring2_f32_supported(w, tpl, d.layout);
        case Family::Ring3: return narrowing ? ring3_narrowing_supported(w, tpl, d.lanes) : ring3_supported(w, tpl, d.lanes);
#ifdef XMHW_RING4
        case Family::Ring4: return !narrowing && ring4_supported(w, tpl, d.lanes);
#endif
        default: return false;
    }
}
Launch ring_launch(int32_t layout, int32_t tpl) {
    const LayoutDef* d = find_layout(layout);
    return Launch{d->family, layout, d->lanes, tpl};
}

// the sorted-list kernel keeps the K largest keys of a row-list, K sized for the top tenth of the pool (four times a list's
// average share): quantiles from here up -- and, mirrored (the K smallest keys: round 6), from 1 - that down.  In between a
// list's share outgrows K and too many cell-rows would be recomputed: those calls run on the ring layout.
constexpr double kSortedMinQ = 0.85;
bool sorted_serves(double q) { return q >= kSortedMinQ || q <= 1.0 - kSortedMinQ; }

// the second-generation layout float32 input runs on: 8 lanes per cell unless the 4-lane layout pads fewer tracks
// (20 tracks: 4 x 5 exactly against 8 x 3 = 24) and does not spill; both with the lanes' lists merged into a wider
// window (layouts 8 and 10: measured 3-4 % faster than the plain ones); 16 lanes for records neither holds
int32_t legacy_layout(const Plan& h) {
    const int32_t y8 = ring2_pick_yps(h.w, h.ntracks, 8);
    const int32_t y4 = ring2_pick_yps(h.w, h.ntracks, 10);
    if (y4 && y4 <= 8 && (!y8 || y4 * 4 < y8 * 8)) return 10;
    if (!y8 && ring2_pick_yps(h.w, h.ntracks, 12) >= 4) return 12;
    return 8;
}

// the ring layout float32 input runs on: the requested one, or (automatic, and behind the sorted-list kernel) ...
int32_t ring_layout(const Plan& h, const RouteSettings& s) {
    if (s.layout != XMHW_LAYOUT_AUTO && s.layout != XMHW_LAYOUT_SORTED) return s.layout;
    // the third-generation kernel (kernels_ring3.hip) on 4 lanes per cell where a lane holds at least 4 tracks
    // (w = 5, 13..48 tracks).  1,036,800 cells, daily (tools/bench_ring2.py --years, counters on): 40 tracks 57.6 ms
    // against 80 ms for the second-generation layouts, 24 tracks 41.8 against 59.8, 20 tracks 38.3 against 44.0,
    // 16 tracks 34.5 against 35.3; 12 tracks 31.0 against 29.7 -- with so few keys per lane its per-row overheads
    // (histogram, walk, sort) outweigh the cheaper selection.  The 6-hourly share of configs[4] (20 tracks): 116 against
    // 130 ms.
    // ... on 2 lanes per cell (32 cells per wave) for records of 9..24 tracks: 518,400 cells daily, counters on: 13
    // tracks 12.4 against 17.7 ms on 4 lanes, 18 tracks 14.6 / 19.5, 22 tracks 17.5 / 21.3, 24 tracks 20.4 / 21.1; the
    // 6-hourly share of configs[4] (20 tracks, 405,000 cells): 48.1 / 58.9
    if (ring3_pick_yps(h.w, h.ntracks, 2) >= 5) return 22;
    if (ring3_pick_yps(h.w, h.ntracks, 4) >= 4) return 21;
    // ... and on 8 lanes per cell for longer records (49..88 tracks, 7..11 per lane) instead of the second-generation
    // kernel's 16-lane layout: 259,200 cells daily, counters on: 50 tracks 24.9 against 36.6 ms, 65 tracks 31.6 / 45.1,
    // 85 tracks 42.8 / 51.0; 96 tracks (12 per lane, 256 registers) 53.5 / 52.0 -- those stay where they were
    const int32_t y8 = ring3_pick_yps(h.w, h.ntracks, 8);
    if (y8 >= 7 && y8 <= 11) return 20;
    return legacy_layout(h);
}

// genuinely float64 samples: the 64-bit mode (64-bit keys as a high and a low word) that serves the plan; tpl == 0: none
Launch x64_launch(const Plan& h, const RouteSettings& s) {
    if (!s.ring2_f64 || s.layout == XMHW_LAYOUT_RING1) return Launch();
    // the third-generation kernel where both rings fit its registers: 13..20 tracks on the 4-lane layout of the float32
    // path, 16 cells per wave (XMHW_RING3_F64_LANES=8 keeps the 8-lane layout) ...
    if (s.ring3_f64 && s.ring3_f64_4lanes) {
        const int32_t y4 = ring3_pick_yps(h.w, h.ntracks, 4);
        if (y4 > 0 && ring3_x64_supported(h.w, y4, 4)) return ring_launch(21, y4);
    }
    // ... up to 5 tracks per lane on 8 lanes = 9..40 tracks (XMHW_RING3_F64=0 keeps the second-generation kernel)
    const int32_t y8 = ring2_pick_yps(h.w, h.ntracks, 8);
    if (s.ring3_f64 && y8 > 0 && ring3_pick_yps(h.w, h.ntracks, 8) == y8 && ring3_x64_supported(h.w, y8, 8))
        return ring_launch(20, y8);
    // the second-generation kernel on 8 lanes per cell: low words in registers up to 4 tracks per lane (9..32 tracks), in
    // LDS at 5 and 6 (33..48; XMHW_RING2_F64_LDS=0 turns those off) ...
    if (y8 > 0 && (y8 <= 4 || s.ring2_f64_lds) && ring2_x64_supported(h.w, y8, 8)) return ring_launch(8, y8);
    // ... 16 lanes per cell for longer and for very short records
    const int32_t y16 = ring2_pick_yps(h.w, h.ntracks, 12);
    if (y16 > 0 && y16 <= 6 && ring2_x64_supported(h.w, y16, 12)) return ring_launch(12, y16);
    return Launch();
}

// float64 input that is really float32 (decoded archives): which ring layout narrows it; tpl == 0: none.  The plan's own
// float32 layout where its narrowing twin exists (the third-generation kernel: 4..12 tracks per lane at 4 lanes per
// cell, ...); any other third- or fourth-generation plan narrows on the second-generation kernel -- on a step table the
// call has anyway: that of the float32 layout when the lanes are the same (4 lanes: layout 10), or that of the 64-bit
// mode on 8 or 4 lanes.
Launch narrowing_launch(const Plan& h, int32_t layout, const Launch& x64) {
    const LayoutDef* d = find_layout(layout);
    if (!d) return Launch();
    const int32_t tpl = pick_tpl(*d, h);
    if (tpl && instantiated(*d, h.w, tpl, true)) return ring_launch(layout, tpl);
    if (d->family == Family::Ring2) return Launch();
    const LayoutDef* l = find_layout(legacy_layout(h));
    const int32_t ltpl = pick_tpl(*l, h);
    if (!ltpl || !instantiated(*l, h.w, ltpl, true)) return Launch();
    const bool own = l->lanes == d->lanes && ltpl == tpl;
    const bool of_x64 = x64.layout != 12 && l->lanes == x64.lanes && ltpl == x64.tpl;
    return own || of_x64 ? ring_launch(l->layout, ltpl) : Launch();
}

}  // namespace

RouteSettings route_defaults() {
    static const RouteSettings env = [] {
        auto is = [](const char* name, char c) { const char* v = std::getenv(name); return v && v[0] == c; };
        RouteSettings s;
        s.sorted_on = !is("XMHW_SORTED", '0');
        s.ring2_f64 = !is("XMHW_RING2_F64", '0');
        s.ring2_f64_lds = !is("XMHW_RING2_F64_LDS", '0');
        s.ring3_f64 = !is("XMHW_RING3_F64", '0');
        s.ring3_f64_4lanes = !is("XMHW_RING3_F64_LANES", '8');
        return s;
    }();
    return env;
}

bool layout_compiled(int32_t layout) {
    return layout == XMHW_LAYOUT_AUTO || layout == XMHW_LAYOUT_RING1 || layout == XMHW_LAYOUT_SORTED || find_layout(layout);
}

Route resolve_route(const Plan& h, const RouteSettings& s, int elem_bytes, double q, bool sorted_device_ok) {
    static const char* const kNoRing = "ring kernel not available for this window/track count/dtype";
    Route r;
    r.ring_layout = ring_layout(h, s);
    auto push = [&r](Launch l) {
        l.gated = r.n > 0;          // (a second launch only ever follows a narrowing one)
        r.launch[r.n++] = l;
    };
    if (s.kernel_choice == XMHW_KERNEL_GENERIC) {
        push(Launch());
        return r;
    }
    const bool must_ring = s.kernel_choice == XMHW_KERNEL_RING;
    Launch ring1{Family::Ring1, -1, 0, 0, false, false, true};
    ring1.tpl = ring_pick(h.w, h.ntracks, 4, &ring1.lanes);
    if (elem_bytes == 4) {
        // float32: the ring kernels wherever the round-1 kernel covers the plan, the generic kernel otherwise
        if (!ring1.tpl) {
            if (must_ring) r.unsupported = kNoRing;
            else push(Launch());
            return r;
        }
        // The sorted-list kernel serves plans with w = 5 whose record it is instantiated for, under the automatic layout
        // choice or XMHW_LAYOUT_SORTED (environment XMHW_SORTED=0 turns it off), on a device that passed its LDS probe
        // (capi.cpp: sorted_device_ok), for the quantiles its lists hold.  It serves every row of the plan.
        const int32_t stpl = sorted_pick_yps(h.w, h.ntracks);
        const bool sorted_layout = s.layout == XMHW_LAYOUT_SORTED || (s.layout == XMHW_LAYOUT_AUTO && s.sorted_on);
        const LayoutDef* d = find_layout(r.ring_layout);
        const int32_t tpl = d ? pick_tpl(*d, h) : 0;
        if (sorted_layout && stpl && sorted_device_ok && sorted_serves(q)) push(Launch{Family::Sorted, XMHW_LAYOUT_SORTED, 2, stpl});
        else if (tpl && instantiated(*d, h.w, tpl, false)) push(ring_launch(r.ring_layout, tpl));
        else push(ring1);
        r.launch[0].counters = true;
        return r;
    }
    // float64: the 64-bit mode where it is instantiated (w = 5, up to 96 tracks), the generic kernel otherwise.  The
    // round-1 float64 ring (kernels_ring64.hip) is gone: round 2's randomised cross-check found it returning wrong rows
    // on clustered doubles and it was never repaired; an explicit XMHW_KERNEL_RING request on a plan the 64-bit mode
    // does not cover is refused instead of being served by a kernel known to be wrong.
    const Launch x64 = x64_launch(h, s);
    if (!x64.tpl && must_ring) {
        r.unsupported = kNoRing;
        return r;
    }
    // If every sample is float32-representable (decoded int16 / float32 archives) the float32 kernel gives the same
    // pools at 2.7x the rate.  All decisions are taken on the device so that the call stays asynchronous: probe ->
    // narrowing float32 kernel (stops at the first lossy sample) -> float64 or generic kernel (runs only if flagged).
    if (s.narrowing) {
        Launch narrow = narrowing_launch(h, r.ring_layout, x64);
        if (!narrow.tpl) narrow = ring1;
        narrow.narrows = true;
        if (narrow.tpl) push(narrow);
    }
    push(x64.tpl ? x64 : Launch());
    return r;
}

int32_t ring_chunks(const Plan& h, const Route& route, int64_t C) {
    if (h.nchunks_req > 0) return std::min(h.nchunks_req, h.D);
    // enough waves to fill 256 CUs x 16 waves a few times over; each chunk
    // re-reads 2w rows per track and cold-starts its bracket, so keep them long
    int64_t waves = (C + 7) / 8;
    int64_t want = (4 * 4096 + waves - 1) / std::max<int64_t>(waves, 1);
    // the third-generation kernel runs two waves per SIMD (2,048 at a time) of 16 or 8 cells: twice that many
    // waves in all is enough, and every further chunk costs its warm-up rows (1 degree grid, 64,800 cells: 3.67 ms
    // with 1 or 2 chunks, 3.87 with 3, 4.16 with 6).
    // The model behind it (round 4): a workgroup is 2 waves, a CU holds 4, the chip 1,024 at a time.  With n chunks
    // a grid is W = n * ceil(C / 32) workgroups of (D / n + 2w) rows each and runs in about
    // ceil(W / 1024) * (D / n + 2w) row-times.  The 1 degree grid (2,025 workgroups per chunk, D = 366): n = 1
    // -> 2 rounds x 376 = 752; n = 2 -> 4 x 193 = 772; n = 3 -> 6 x 132 = 792; n = 6 -> 12 x 71 = 852 --
    // the measured order.  One or two chunks fill the last round to 99 %: there is no tail to remove, and what
    // keeps this grid at 11 % of the roofline against 15 % for the 40-year one is the record, not the grid:
    // 30 tracks pad to 32 (6 % idle ring slots) and the per-row costs that do not depend on the number of
    // tracks (walk, sort, epilogue, row overhead: ~40 % of a row) are spread over 120 bytes of samples per
    // cell-row instead of 160.
    const LayoutDef* d = find_layout(route.ring_layout);
    if (d && d->family >= Family::Ring3) {
        const int64_t cpw = 64 / d->lanes;
        waves = (C + cpw - 1) / cpw;
        want = (4096 + waves - 1) / std::max<int64_t>(waves, 1);
    }
    return static_cast<int32_t>(std::max<int64_t>(1, std::min<int64_t>(want, h.D / 24)));
}

int64_t sorted_pieces(const Plan& h, const Route&, int64_t C) {
    // a small grid is cut into more pieces so that it still fills the chip (7 waves per CU; every piece pays R - 1
    // warm-up rows)
    const int64_t waves = (std::max<int64_t>(C, 1) + 31) / 32;
    return h.nchunks_req > 0 ? h.nchunks_req : (1536 + waves - 1) / waves;
}

}  // namespace xmhw
