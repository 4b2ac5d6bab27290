"""The threshold dispatch of every plan in a sweep, as small integers: what xmhw_plan_route, xmhw_plan_layout_in_use,
xmhw_plan_f64_mode, xmhw_plan_info, xmhw_plan_chunks_in_use and xmhw_plan_sorted_info answer.  Pure host code: no GPU.

    python tools/record_routes.py                 writes tests/golden/threshold_routes.npz
    python tools/record_routes.py --leg OUT.npz   one sweep of this process' environment into OUT.npz
                                                  (XMHW_ROUTE_WINDOWS=5: that window only)

tests/test_host_routes.py replays the same sweep and compares.  The environment switches are read once per process,
so the default leg and each switch run in a child process of their own."""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
FIXTURE = os.path.join(ROOT, "tests", "golden", "threshold_routes.npz")

WINDOWS = (1, 2, 3, 4, 5, 7, 10, 15)
TRACKS = tuple(range(1, 201))
LAYOUTS = (None, -1, 8, 10, 12, 20, 21, 22, 40)
KERNELS = (0, 1, 2)                    # XMHW_KERNEL_AUTO, _RING, _GENERIC
ELEM_BYTES = (4, 8)
QUANTILES = (0.0, 0.15, 0.5, 0.85, 0.9)
YEARS = (9, 20, 30, 40, 60, 90)
CELLS = (1, 33, 20000, 64800, 1036800)
CHUNKS = (0, 3)
ROUTE_WORDS = 23                       # status, launches, 3 x 7 launch fields (the counts are in the chunk sweep)
# the legs: the default environment, then each switch on its own (at w = 5)
SWITCHES = ("XMHW_SORTED=0", "XMHW_RING2_F64=0", "XMHW_RING2_F64_LDS=0", "XMHW_RING3_F64=0", "XMHW_RING3_F64_LANES=8",
            "XMHW_RING2=21")
LEGS = ("default",) + SWITCHES


def _code(h, e):
    """the C ABI's error code behind an exception of the bindings"""
    return 3 if isinstance(e, h.Unsupported) else 1 if isinstance(e, h.InvalidArgument) else 2


def _open(h, doy, w, layout):
    """(plan handle or 0, error code)"""
    try:
        p = h.plan_create(doy, w)
    except Exception as e:
        return 0, _code(h, e)
    if layout is not None:
        try:
            h.plan_set_layout(p, layout)
        except Exception as e:
            h.plan_destroy(p)
            return 0, _code(h, e)
    return p, 0


def sweep(windows=WINDOWS):
    for d in (ROOT, os.path.join(ROOT, "oracle")):
        if d not in sys.path:
            sys.path.insert(0, d)
    import xmhw_oracle as ora
    from xmhw_amd._lib import hip
    h = hip()
    nw, nt, nl, nk = len(windows), len(TRACKS), len(LAYOUTS), len(KERNELS)
    refused = np.zeros((nw, nt, nl), np.int8)
    intro = np.zeros((nw, nt, nl, nk, 3), np.int8)       # layout_in_use, f64_mode, the kernel of plan_info
    routes = np.zeros((nw, nt, nl, nk, 2, len(ELEM_BYTES), len(QUANTILES), ROUTE_WORDS), np.int8)
    for iw, w in enumerate(windows):
        for it, n in enumerate(TRACKS):
            doy = np.tile(np.arange(1, 40), n).astype(np.int32)
            for il, layout in enumerate(LAYOUTS):
                p, refused[iw, it, il] = _open(h, doy, w, layout)
                if not p:
                    continue
                for ik, kernel in enumerate(KERNELS):
                    h.plan_set_kernel(p, kernel)
                    intro[iw, it, il, ik] = (h.plan_layout_in_use(p), h.plan_f64_mode(p), h.plan_info(p)["kernel"])
                    for narrowing in (0, 1):
                        h.plan_set_narrowing(p, narrowing)
                        for ie, eb in enumerate(ELEM_BYTES):
                            for iq, q in enumerate(QUANTILES):
                                routes[iw, it, il, ik, narrowing, ie, iq] = h.plan_route(p, eb, q, 1)[:ROUTE_WORDS]
                h.plan_destroy(p)
    # chunk counts and sorted pieces on daily calendars: chunks_in_use, pieces of sorted_info (-1: refused), and the two
    # counts of the route record
    counts = np.zeros((len(YEARS), len(LAYOUTS), len(CHUNKS), len(CELLS), 4), np.int32)
    for iy, years in enumerate(YEARS):
        t = np.arange("1982-01-01", f"{1982 + years}-01-01", dtype="datetime64[D]")
        doy = ora.add_doy(t).astype(np.int32)
        for il, layout in enumerate(LAYOUTS):
            p, err = _open(h, doy, 5, layout)
            if not p:
                counts[iy, il] = -err
                continue
            for ic, req in enumerate(CHUNKS):
                h.plan_set_chunks(p, req)
                for ix, C in enumerate(CELLS):
                    try:
                        pieces = h.plan_sorted_info(p, C)[2]
                    except h.Unsupported:
                        pieces = -1
                    r = h.plan_route(p, 4, 0.9, C)
                    counts[iy, il, ic, ix] = (h.plan_chunks_in_use(p, C), pieces, r[23], r[24])
            h.plan_destroy(p)
    return {"refused": refused, "intro": intro, "routes": routes, "counts": counts}


def run_legs():
    """every leg in a child process of its own -> {leg: arrays}"""
    clean = {k: v for k, v in os.environ.items() if k not in {s.split("=")[0] for s in SWITCHES}}
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        jobs = []
        for i, leg in enumerate(LEGS):
            env = dict(clean)
            if leg != "default":
                name, value = leg.split("=")
                env[name] = value
                env["XMHW_ROUTE_WINDOWS"] = "5"
            path = os.path.join(tmp, f"leg{i}.npz")
            jobs.append((leg, path, subprocess.Popen([sys.executable, os.path.abspath(__file__), "--leg", path], env=env)))
        for leg, path, job in jobs:
            if job.wait() != 0:
                raise RuntimeError(f"the {leg} leg failed")
            with np.load(path) as z:
                out[leg] = {k: z[k] for k in z.files}
    return out


def flatten(legs):
    return {f"{i}_{k}": v for i, leg in enumerate(LEGS) for k, v in legs[leg].items()}


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--leg":
        only = os.environ.get("XMHW_ROUTE_WINDOWS")
        np.savez(sys.argv[2], **sweep(tuple(int(v) for v in only.split(",")) if only else WINDOWS))
    else:
        np.savez_compressed(FIXTURE, legs=np.array(LEGS), **flatten(run_legs()))
        print(FIXTURE, os.path.getsize(FIXTURE), "bytes")
