"""ONE plan object reused across routes: the step tables are cached per (lanes per cell, tracks per lane) and added as
calls need them, the ring chunks and the sorted-list kernel's pieces are re-cut when the cell count or the forced chunk
count changes, the layout is switched and switched back -- and every call still computes what a fresh generic-kernel
plan computes on the same input.  Before every call Plan.route() must name the kernel family and layout the step is
meant to exercise.

The shapes are the smallest at which each table path is taken: 20 tracks (float32 on the sorted-list kernel, layout 22
for mid quantiles; the 64-bit mode on layout 21: 4 lanes next to the 2-lane float32 table) and 40 tracks (sorted, layout
21 on 4 lanes; the 64-bit mode on layout 20: 8 lanes, a second table).  33 cells leave the 32- and 16-cell waves ragged.

Comparisons as in tests/test_gpu_sorted.py (float32 against the generic kernel: thresh bit for bit, seas rtol 1e-12,
atol 1e-300) and tests/test_gpu_parity_f64.py (float64 against the generic kernel: thresh bit for bit, seas rtol 1e-12,
atol 1e-12)."""
import numpy as np
import numpy.testing as npt
import pytest

from test_gpu_parity_f64 import _clustered
from test_gpu_sorted import _daily, _series

pytestmark = pytest.mark.gpu

# years -> (family, layout) of: float32 mid quantiles (and the narrowing launch), the 64-bit mode; tracks per lane on layout 8
EXPECT = {20: (("ring3", 22), ("ring3", 21), 3), 40: (("ring3", 21), ("ring3", 20), 5)}


@pytest.fixture(scope="module")
def dev():
    from xmhw_amd._lib import require_gpu
    require_gpu()
    import xmhw_amd.device as d
    return d


def _run(dev, plan, x, q):
    C = x.shape[1]
    bufs = [dev.DeviceBuffer.from_array(np.ascontiguousarray(x)), dev.DeviceBuffer(8 * plan.D * C),
            dev.DeviceBuffer(8 * plan.D * C)]
    try:
        dev.clim_raw(plan, bufs[0], x.dtype.itemsize, C, q, False, bufs[1], bufs[2])
        dev.hip().stream_sync(0)
        return bufs[1].to_array((plan.D, C), np.float64), bufs[2].to_array((plan.D, C), np.float64)
    finally:
        for b in bufs:
            b.free()


def _fresh(dev, doy, x, q, **kw):
    plan = dev.Plan(doy, 5, **kw)
    try:
        return _run(dev, plan, x, q)
    finally:
        plan.destroy()


@pytest.mark.parametrize("years", [20, 40])
def test_one_plan_across_routes(dev, years):
    (mid, x64, tpl8) = EXPECT[years]
    doy = _daily(1982, 1982 + years - 1)
    T = doy.shape[0]
    x32 = _series(T, 200, 300 + years, nanfrac=0.01)
    xrep = x32.astype(np.float64)                        # float64 holding float32-representable values
    xclu = _clustered(T, 200, 400 + years)               # doubles no float32 holds
    assert not np.array_equal(xclu, xclu.astype(np.float32).astype(np.float64), equal_nan=True)
    # the reference: fresh generic-kernel plans, once, on all 200 cells (cells are independent: the first 33 are a slice)
    ref = {(name, q): _fresh(dev, doy, x, q, kernel="generic")
           for name, x, qs in (("f32", x32, (0.9, 0.5)), ("rep", xrep, (0.9,)), ("clu", xclu, (0.9,))) for q in qs}
    data = {"f32": x32, "rep": xrep, "clu": xclu}
    plan = dev.Plan(doy, 5)
    h = dev.hip()

    def call(name, q, C, first, then=None, chunks=None):
        """one clim_raw on the shared plan, its route checked first: `first` / `then` = (family, layout) of the launches"""
        x = data[name][:, :C]
        r = plan.route(x.dtype, q, C)
        assert r["supported"]
        got = [(la["family"], la["layout"]) for la in r["launches"]]
        assert got == [first] + ([then] if then else []), (name, q, C, r)
        if then:
            assert r["launches"][0]["narrows"] and r["launches"][1]["gated"] and not r["launches"][0]["gated"]
        if chunks is not None:
            assert (r["chunks"], r["sorted_pieces"]) == (chunks, chunks)
        th, se = _run(dev, plan, x, q)
        t0, s0 = (a[:, :C] for a in ref[(name, q)])
        npt.assert_array_equal(th, t0, err_msg=f"{name} q={q} C={C}")
        if name == "f32":
            npt.assert_allclose(se, s0, rtol=1e-12, atol=1e-300, equal_nan=True)
        else:
            npt.assert_allclose(se, s0, rtol=1e-12, atol=1e-12, equal_nan=True)
        return th, se

    try:
        assert plan.layout_in_use() == 40 and plan.f64_mode() == x64[1]
        first = call("f32", 0.9, 33, ("sorted", 40))                                   # 1
        call("f32", 0.5, 33, mid)                                                      # 2
        call("rep", 0.9, 33, mid, x64)                                                 # 3
        assert plan.narrowed()
        call("clu", 0.9, 33, mid, x64)                                                 # 4
        assert not plan.narrowed()
        h.plan_set_layout(plan.handle, 8)                                              # 5
        r = plan.route(np.float32, 0.9, 33)["launches"]
        assert (r[0]["lanes"], r[0]["tracks_per_lane"]) == (8, tpl8)
        call("f32", 0.9, 33, ("ring2", 8))
        call("clu", 0.9, 33, ("ring2", 8), x64)
        assert not plan.narrowed()
        h.plan_set_layout(plan.handle, dev.LAYOUTS["auto"])                            # 6
        again = call("f32", 0.9, 33, ("sorted", 40))
        npt.assert_array_equal(again[0], first[0])
        npt.assert_array_equal(again[1], first[1])
        call("f32", 0.9, 200, ("sorted", 40))                                          # 7
        call("f32", 0.5, 200, mid)
        call("clu", 0.9, 200, mid, x64)
        h.plan_set_chunks(plan.handle, 3)                                              # 8
        call("f32", 0.5, 200, mid, chunks=3)
        call("clu", 0.9, 200, mid, x64, chunks=3)
        last = call("f32", 0.9, 200, ("sorted", 40), chunks=3)                         # 9
        want = _fresh(dev, doy, x32, 0.9, nchunks=3)
        npt.assert_array_equal(last[0], want[0])
        npt.assert_array_equal(last[1], want[1])
    finally:
        plan.destroy()
