"""One leg of tests/f64_mode_cases.py through the kernels, in a process of its own (the switches of a leg are read once
per process).  Not collected by pytest.

    python tests/f64_mode_child.py LEG_INDEX OUT.npz            every case of the leg on the GPU
    python tests/f64_mode_child.py LEG_INDEX OUT.npz routes     no GPU: the routes of the leg's cases and of 1..96 tracks

For every case: the data from its seed, plan.route(float64, q, C) with narrowing off and on, clim_raw with narrowing off,
clim_raw with narrowing on and plan.narrowed() after it; thresh and seas go to OUT.npz with their pitched rows whole.
Nothing is asserted about values here: tests/test_gpu_f64_modes.py does that.  Every call's status is checked (the
bindings raise on any that is not success, the stream is synchronised after every call); the first failure ends the
process with a non-zero status before anything else is started."""
import json
import os
import sys
import traceback

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for _p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import f64_mode_cases as fc          # noqa: E402

MAX_TRACKS = 96


def launches(plan, q, cells):
    """[(family, layout, lanes, tracks per lane, narrows, gated)] of a float64 call"""
    r = plan.route(np.float64, q, cells)
    assert r["supported"], r
    return [[la["family"], la["layout"], la["lanes"], la["tracks_per_lane"], int(la["narrows"]), int(la["gated"])]
            for la in r["launches"]]


def case_routes(dev, case, doy):
    out = {}
    for narrowing in (False, True):
        plan = dev.Plan(doy, fc.W, kernel="auto", narrowing=narrowing, nchunks=case["nchunks"])
        try:
            out["on" if narrowing else "off"] = launches(plan, case["q"], fc.C)
        finally:
            plan.destroy()
    return out


def run_case(dev, case):
    """{route, narrowed, th_off, se_off, th_on, se_on}: the (D, ldo) outputs of the narrowing=False and narrowing=True
    calls, their padding columns included (0xFF bytes before each call)"""
    h = dev.hip()
    doy, x = fc.samples(case)
    T = x.shape[0]
    ld, first, ldo = (fc.PITCH["ld"], fc.PITCH["first"], fc.PITCH["ldo"]) if case["pitched"] else (fc.C, 0, fc.C)
    # the slab inside a wider buffer: sample (t, c) at first + t * ld + c; every other double is one float32 cannot hold
    wide = np.full(first + T * ld, 1e300)
    wide[1::2] = np.pi
    rows = first + np.arange(T)[:, None] * ld + np.arange(fc.C)[None, :]
    wide[rows] = x
    out = {"route": case_routes(dev, case, doy)}
    d_ts = dev.DeviceBuffer.from_array(wide)
    bufs = []
    try:
        for narrowing in (False, True):
            plan = dev.Plan(doy, fc.W, kernel="auto", narrowing=narrowing, nchunks=case["nchunks"])
            th, se = dev.DeviceBuffer(8 * plan.D * ldo), dev.DeviceBuffer(8 * plan.D * ldo)
            bufs += [th, se]
            try:
                for b in (th, se):
                    h.memset(b.ptr, 0xFF, b.nbytes)
                dev.clim_raw(plan, d_ts.ptr + 8 * first, 8, fc.C, case["q"], case["negate"], th, se, ld=ld, ldo=ldo)
                h.stream_sync(0)
                tag = "on" if narrowing else "off"
                out["th_" + tag] = th.to_array((plan.D, ldo), np.float64)
                out["se_" + tag] = se.to_array((plan.D, ldo), np.float64)
                if narrowing:
                    out["narrowed"] = plan.narrowed()
            finally:
                plan.destroy()
    finally:
        for b in [d_ts] + bufs:
            b.free()
    return out


def track_routes(dev):
    """the single launch of a float64 call with narrowing off, for 1 .. MAX_TRACKS tracks"""
    out = []
    for n in range(1, MAX_TRACKS + 1):
        plan = dev.Plan(np.tile(np.arange(1, 40), n), fc.W, kernel="auto", narrowing=False)
        try:
            out.append(launches(plan, 0.9, fc.C))
        finally:
            plan.destroy()
    return out


def main(argv):
    leg, path = int(argv[1]), argv[2]
    routes_only = len(argv) > 3 and argv[3] == "routes"
    import xmhw_amd.device as dev
    saved = {}
    if routes_only:
        saved["tracks"] = np.array(json.dumps(track_routes(dev)))
        for i, case in enumerate(fc.CASES[leg]):
            saved[f"{i}_route"] = np.array(json.dumps(case_routes(dev, case, fc.calendar(case)[1])))
    else:
        from xmhw_amd._lib import require_gpu
        require_gpu()
        for i, case in enumerate(fc.CASES[leg]):
            r = run_case(dev, case)
            saved[f"{i}_route"] = np.array(json.dumps(r["route"]))
            saved[f"{i}_narrowed"] = np.array(bool(r["narrowed"]))
            for k in ("th_off", "se_off", "th_on", "se_on"):
                saved[f"{i}_{k}"] = r[k]
            print(f"case {i + 1} of {len(fc.CASES[leg])} done: {case['id']}", flush=True)
    np.savez(path, **saved)
    return 0


if __name__ == "__main__":
    try:
        status = main(sys.argv)
    except BaseException:
        traceback.print_exc()
        status = 1
    sys.exit(status)
