// route.h -- which kernels one raw-climatology call launches, on which lane layouts and step tables: resolved once per
// call from the plan, its settings, the element size and the quantile.  Pure host code: no HIP call, no device state.
// capi.cpp launches what the route says, and the introspection entries of the C ABI report from the same answer.
#pragma once
#include <cstdint>

#include "plan.h"

namespace xmhw {

enum class Family : int32_t { Generic = 0, Ring1 = 1, Ring2 = 2, Ring3 = 3, Ring4 = 4, Sorted = 5 };   // XMHW_ROUTE_*

struct RouteSettings {
    int32_t layout = -2;          // XMHW_LAYOUT_* requested (xmhw_plan_set_layout, environment XMHW_RING2); -2: automatic
    int32_t kernel_choice = 0;    // XMHW_KERNEL_* requested (xmhw_plan_set_kernel)
    bool narrowing = true;        // xmhw_plan_set_narrowing
    // the process-wide environment switches, each on unless set to the value named: XMHW_SORTED=0, XMHW_RING2_F64=0,
    // XMHW_RING2_F64_LDS=0, XMHW_RING3_F64=0, XMHW_RING3_F64_LANES=8
    bool sorted_on = true, ring2_f64 = true, ring2_f64_lds = true, ring3_f64 = true, ring3_f64_4lanes = true;
};
// the defaults with the environment switches as this process first saw them (read once)
RouteSettings route_defaults();

struct Launch {
    Family family = Family::Generic;
    int32_t layout = -1;          // the public XMHW_LAYOUT_* number (-1: round-1 and generic kernels)
    int32_t lanes = 0, tpl = 0;   // lanes per cell and tracks per lane: the key of the step table (0: no table)
    bool narrows = false;         // float64 samples read as float32, behind the probe; gives up at the first lossy sample
    bool gated = false;           // runs only if the narrowing launch before it gave up (the narrow flag)
    bool counters = false;        // takes the debug pass counters (xmhw_plan_debug_stats)
};

// Today's sequences: sorted | ring | narrowing ring, then the gated 64-bit ring | narrowing ring, then the gated generic
// kernel | generic.
struct Route {
    const char* unsupported = nullptr;   // non-NULL: the call is refused (XMHW_ERR_UNSUPPORTED) with this message
    int32_t n = 0;
    Launch launch[3];
    int32_t ring_layout = -1;            // the plan's float32 ring layout: what the ring chunks are cut for
};

Route resolve_route(const Plan& host, const RouteSettings& s, int elem_bytes, double q, bool sorted_device_ok);
// chunks of the doy axis of a ring launch over C cells, and the pieces the sorted-list kernel's chunks are cut into
int32_t ring_chunks(const Plan& host, const Route& route, int64_t C);
int64_t sorted_pieces(const Plan& host, const Route& route, int64_t C);
// the layouts xmhw_plan_set_layout accepts in this build
bool layout_compiled(int32_t layout);

}  // namespace xmhw
