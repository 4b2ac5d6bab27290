"""detrend() on the GPU: the fit and removal kernels through the C ABI (pybind) and the public API against the numpy
oracle (tests/detrend_oracle.py: lstsq per cell).

Tolerances (the device solves normal equations, the oracle uses lstsq; they cannot be bit-equal):
* float64 quantities (coefficients, detrended float64 series): |got - want| <= 1e-11 * max|y| of the cell;
* float32 detrended series: within one float32 ulp of the oracle's rounded value everywhere and bit-identical in all
  but at most 1e-4 of the valid samples of a test;
* invariance (a cell alone / in a slab / another ld / a second run) and the threshold_detect() equivalences: exact.
Only cells whose pivot ratio, evaluated by the oracle, is above 1e-3 (accepted) or below 1e-9 in magnitude (must
fail) are used.  Every comparison prints its worst figure before it asserts.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import detrend_oracle as dor  # noqa: E402

pytestmark = pytest.mark.gpu

TOL64 = 1e-11
DIFFER_CAP = 1e-4

AXES = {
    "40y_daily": lambda: np.arange("1982-01-01", "2022-01-01", dtype="datetime64[D]"),
    "12y_daily": lambda: np.arange("2000-01-01", "2012-01-01", dtype="datetime64[D]"),
    "2y_daily": lambda: np.arange("2003-01-01", "2005-01-01", dtype="datetime64[D]"),
    "20y_6hourly": lambda: np.arange("2000-01-01", "2020-01-01", dtype="datetime64[6h]"),
}
FIT_PERIODS = {"40y_daily": [1991, 2020], "12y_daily": [None, None], "2y_daily": [None, None], "20y_6hourly": [2003, 2017]}
PAIRS = [(o, h) for o in (1, 2, 3) for h in (0, 1, 2, 3)]


@pytest.fixture(scope="module")
def gpu():
    from xmhw_amd._lib import hip, require_gpu
    require_gpu()
    return hip()


def days_of(t):
    return (t - t[0]) / np.timedelta64(1, "D")


def make_cells(t, C, rng, dtype):
    """SST-like cells with 0 %, 5 % and 30 % NaN in turn, a 200-day gap in cell 3 and 60 % NaN in cell 4"""
    y = dor.sst_like(days_of(t), C, rng, dtype)
    T = t.shape[0]
    for c in range(C):
        frac = (0.0, 0.05, 0.30)[c % 3]
        if frac:
            y[rng.random(T) < frac, c] = np.nan
    if C > 3:
        per_day = int(round(1.0 / (days_of(t)[1] - days_of(t)[0])))
        g0 = T // 3
        y[g0:g0 + 200 * per_day, 3] = np.nan
    if C > 4:
        y[rng.random(T) < 0.6, 4] = np.nan                    # more missing than valid: the cell sums its own Gram matrix
    return y


def run_device(h, y, spec, ld=None, remove=True):
    """fit (+ remove) through the C ABI: (series after the call, coef (P, C), nvalid (C,))"""
    from xmhw_amd.device import DeviceBuffer
    T, C = y.shape
    ld = C if ld is None else ld
    host = np.full((T, ld), -777.0, dtype=y.dtype)
    host[:, :C] = y
    bufs = []
    try:
        d_ts = DeviceBuffer.from_array(host); bufs.append(d_ts)
        d_b = DeviceBuffer.from_array(spec.basis); bufs.append(d_b)
        d_w = DeviceBuffer.from_array(spec.weight); bufs.append(d_w)
        ldc = C + 3
        d_coef = DeviceBuffer.from_array(np.full((spec.P, ldc), -555.0)); bufs.append(d_coef)
        d_nv = DeviceBuffer.from_array(np.full(C + 2, -9, dtype=np.int32)); bufs.append(d_nv)
        h.series_fit(d_ts.ptr, y.dtype.itemsize, T, C, ld, d_b.ptr, spec.P, d_w.ptr, spec.min_valid, d_coef.ptr, ldc,
                     d_nv.ptr)
        if remove:
            h.series_remove(d_ts.ptr, y.dtype.itemsize, T, C, ld, d_b.ptr, spec.P, spec.R, d_coef.ptr, ldc)
        h.stream_sync(0)
        out = d_ts.to_array((T, ld), y.dtype)
        coef = d_coef.to_array((spec.P, ldc), np.float64)
        nv = d_nv.to_array((C + 2,), np.int32)
    finally:
        for b in bufs:
            b.free()
    assert (out[:, C:] == -777.0).all(), "columns >= C of the series were touched"
    assert (coef[:, C:] == -555.0).all(), "columns >= C of the coefficients were touched"
    assert (nv[C:] == -9).all()
    return out[:, :C], coef[:, :C], nv[:C]


def ulp_steps32(a, b):
    """distance in float32 representable values"""
    ka = a.view(np.int32).astype(np.int64)
    kb = b.view(np.int32).astype(np.int64)
    ka = np.where(ka < 0, -(ka & 0x7FFFFFFF), ka)
    kb = np.where(kb < 0, -(kb & 0x7FFFFFFF), kb)
    return np.abs(ka - kb)


def compare(y, got, coef, nv, spec, label):
    """the checks of item 1 for one (T, C) case; returns the figures"""
    want, want64, wcoef, wnv, ratio = dor.detrend_cells(y, spec.basis, spec.weight, spec.R, spec.min_valid)
    assert (ratio > 1e-3).all(), f"{label}: the test data holds a cell with pivot ratio {ratio.min():.2e}"
    np.testing.assert_array_equal(nv, wnv)
    scale = np.nanmax(np.abs(y.astype(np.float64)), axis=0)
    cerr = float(np.max(np.abs(coef - wcoef) / scale))
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    fig = {"coef": cerr}
    if y.dtype == np.float64:
        verr = float(np.nanmax(np.abs(got - want64) / scale))
        fig["value"] = verr
        print(f"{label}: coefficient error {cerr:.2e}, value error {verr:.2e} of max|y|")
        assert verr <= TOL64
    else:
        steps = ulp_steps32(got[ok], want[ok])
        differ = int((steps != 0).sum())
        fig["differ"], fig["valid"] = differ, int(ok.sum())
        print(f"{label}: coefficient error {cerr:.2e} of max|y|; {differ} of {int(ok.sum())} float32 samples differ, "
              f"largest distance {int(steps.max())} ulp")
        assert steps.max() <= 1
        assert differ <= DIFFER_CAP * ok.sum()
    assert cerr <= TOL64
    return fig


# ---- 1. against the oracle ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("axis", list(AXES))
@pytest.mark.parametrize("order,harmonics", PAIRS)
def test_fit_and_remove_match_oracle(gpu, order, harmonics, axis, dtype):
    """Measured on the MI355X (96 cases, 12 cells each): coefficients within 3.6e-12 max|y| of the oracle (the largest:
    the x^3 coefficient of a cubic on the two-year axis; 5.1e-14 elsewhere), detrended float64 values within 3.7e-14
    max|y|; float32 series: 0 of 7.73 M valid samples differ from the oracle's rounded value."""
    from xmhw_amd.detrend import DetrendSpec
    t = AXES[axis]()
    spec = DetrendSpec(t, order, harmonics, fitPeriod=FIT_PERIODS[axis])
    rng = np.random.default_rng(1000 * order + 100 * harmonics + len(axis))
    C = 12
    y = make_cells(t, C, rng, dtype)
    got, coef, nv = run_device(gpu, y, spec, ld=C + 5)
    compare(y, got, coef, nv, spec, f"{axis} order {order} harmonics {harmonics} {np.dtype(dtype).name}")


@pytest.mark.parametrize("C", [1, 63, 65, 1000])
def test_ragged_widths(gpu, C):
    from xmhw_amd.detrend import DetrendSpec
    t = AXES["2y_daily"]()
    spec = DetrendSpec(t, 1, 2)
    y = make_cells(t, C, np.random.default_rng(C), np.float32)
    got, coef, nv = run_device(gpu, y, spec)
    compare(y, got, coef, nv, spec, f"C = {C}")


def test_null_weight_and_no_nvalid(gpu):
    """weight NULL = all steps; nvalid NULL is allowed"""
    from xmhw_amd.detrend import DetrendSpec
    from xmhw_amd.device import DeviceBuffer
    t = AXES["2y_daily"]()
    spec = DetrendSpec(t, 2, 1)
    y = make_cells(t, 70, np.random.default_rng(3), np.float64)
    _, coef, _ = run_device(gpu, y, spec)
    d_ts, d_b, d_c = DeviceBuffer.from_array(y), DeviceBuffer.from_array(spec.basis), DeviceBuffer(8 * spec.P * 70)
    try:
        gpu.series_fit(d_ts.ptr, 8, t.shape[0], 70, 70, d_b.ptr, spec.P, 0, spec.min_valid, d_c.ptr, 70, 0)
        gpu.stream_sync(0)
        np.testing.assert_array_equal(d_c.to_array((spec.P, 70), np.float64), coef)
    finally:
        for b in (d_ts, d_b, d_c):
            b.free()


# ---- 2. failing cells ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_failing_cells(gpu, dtype):
    from xmhw_amd.detrend import DetrendSpec
    t = AXES["40y_daily"]()
    T = t.shape[0]
    spec = DetrendSpec(t, 3, 3, fitPeriod=[1985, 2018])
    inside = np.nonzero(spec.weight)[0]
    rng = np.random.default_rng(11)
    C = 64                                                   # one wave: the neighbours share it
    y = make_cells(t, C, rng, dtype)
    clean = y.copy()
    few, ill, inf_in, inf_out = 5, 18, 30, 41                # (18 and 30 are gap-free cells)
    y[:, few] = np.nan
    y[inside[100:109], few] = 15.0                           # 9 samples for 10 terms
    y[:, ill] = np.nan
    y[7000:7012, ill] = clean[7000:7012, ill]                # valid on 12 consecutive days only
    y[inside[4000], inf_in] = np.inf                         # a contributing +Inf
    y[inside[0] - 3, inf_out] = np.inf                       # an Inf outside the fit period
    y[inside[-1] + 5, inf_out] = -np.inf
    _, _, _, _, ratio = dor.detrend_cells(y[:, [ill]], spec.basis, spec.weight, spec.R, spec.min_valid)
    print(f"pivot ratio of the ill-posed cell (oracle): {ratio[0]:.2e}")
    assert abs(ratio[0]) < 1e-9
    got, coef, nv = run_device(gpu, y, spec)
    for c in (few, ill, inf_in):
        assert np.isnan(coef[:, c]).all() and np.isnan(got[:, c]).all(), c
    assert nv[few] == 9 and nv[ill] == 12
    # the Inf outside the fit period does not fail the cell: same coefficients as without it, Inf stays Inf
    others = [c for c in range(C) if c not in (few, ill, inf_in)]
    assert not np.isnan(coef[:, others]).any()
    got0, coef0, _ = run_device(gpu, clean, spec)
    np.testing.assert_array_equal(coef[:, others], coef0[:, others])             # neighbours in the wave untouched
    plain = [c for c in others if c != inf_out]
    np.testing.assert_array_equal(got[:, plain], got0[:, plain])
    assert got[inside[0] - 3, inf_out] == np.inf and got[inside[-1] + 5, inf_out] == -np.inf
    keep = np.ones(T, dtype=bool)
    keep[[inside[0] - 3, inside[-1] + 5]] = False
    np.testing.assert_array_equal(got[keep, inf_out], got0[keep, inf_out])
    compare(clean[:, plain], got[:, plain], coef[:, plain], nv[plain], spec, f"neighbours {np.dtype(dtype).name}")


def test_too_few_by_min_valid(gpu):
    from xmhw_amd.detrend import DetrendSpec
    t = AXES["2y_daily"]()
    y = make_cells(t, 6, np.random.default_rng(5), np.float32)
    y[100:, 0] = np.nan                                       # 100 samples (cell 0 is gap-free)
    _, coef, nv = run_device(gpu, y, DetrendSpec(t, 1, 0, min_valid=101))
    assert np.isnan(coef[:, 0]).all() and nv[0] == 100 and not np.isnan(coef[:, 1:]).any()
    _, coef, nv = run_device(gpu, y, DetrendSpec(t, 1, 0, min_valid=100))
    assert not np.isnan(coef).any()


# ---- 3. a cell's result depends on its own samples only ---------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_cell_alone_in_a_slab_other_ld_and_twice(gpu, dtype):
    from xmhw_amd.detrend import DetrendSpec
    t = AXES["12y_daily"]()
    spec = DetrendSpec(t, 3, 3, fitPeriod=[2001, 2010])
    rng = np.random.default_rng(21)
    C = 4097
    y = make_cells(t, C, rng, dtype)
    y[:, 77] = np.nan
    y[1500:2400, 77] = dor.sst_like(np.arange(900), 1, rng, dtype)[:, 0]     # more missing than valid: the direct sums
    got, coef, nv = run_device(gpu, y, spec)
    got2, coef2, nv2 = run_device(gpu, y, spec)
    np.testing.assert_array_equal(got, got2)
    np.testing.assert_array_equal(coef, coef2)
    got3, coef3, _ = run_device(gpu, y, spec, ld=C + 59)
    np.testing.assert_array_equal(got, got3)
    np.testing.assert_array_equal(coef, coef3)
    assert not np.isnan(coef[:, 77]).any()
    for c in (0, 1, 64, 77, 2048, 4096):
        g1, c1, n1 = run_device(gpu, np.ascontiguousarray(y[:, c:c + 1]), spec)
        np.testing.assert_array_equal(g1[:, 0], got[:, c])
        np.testing.assert_array_equal(c1[:, 0], coef[:, c])
        assert n1[0] == nv[c]
    # the same cell at another lane, among other neighbours
    sub = np.ascontiguousarray(y[:, [5, 77, 9, 1, 4000]])
    g5, c5, _ = run_device(gpu, sub, spec, ld=8)
    np.testing.assert_array_equal(c5, coef[:, [5, 77, 9, 1, 4000]])
    np.testing.assert_array_equal(g5, got[:, [5, 77, 9, 1, 4000]])
    # and against the oracle, the mostly-missing cell (its own Gram matrix, summed by the second kernel) included
    pick = [0, 1, 2, 3, 4, 77, 4096]
    compare(y[:, pick], got[:, pick], coef[:, pick], nv[pick], spec, f"slab cells {np.dtype(dtype).name}")


# ---- 4. threshold_detect(detrend=...) == detrend() then threshold_detect() ---------------------------------------------------
def api_grid(dtype=np.float32, nlat=6, nlon=9, years=6, seed=31):
    from xmhw_amd import GridSeries
    t = np.arange("2000-01-01", f"{2000 + years}-01-01", dtype="datetime64[D]")
    rng = np.random.default_rng(seed)
    y = dor.sst_like(days_of(t), nlat * nlon, rng, np.float64, trend=rng.uniform(1.0, 4.0, nlat * nlon))
    a = np.zeros(nlat * nlon)
    for k in range(t.shape[0]):                               # AR(1) anomalies: events that last
        a = 0.9 * a + rng.normal(size=nlat * nlon)
        y[k] += a
    y = y.astype(dtype).reshape(t.shape[0], nlat, nlon)
    y[:, 2, 3] = np.nan                                       # land
    y[:, :, 7] = np.nan                                       # an all-land meridian
    y[200:203, 1, 1] = np.nan                                 # a short gap (maxPadLength fills it)
    y[900:960, 4, 4] = np.nan                                 # a long one
    y[:, 5, 0] = np.nan
    y[50:54, 5, 0] = 14.0                                     # not land, too few samples: the fit fails
    return GridSeries(y, ("time", "lat", "lon"), {"time": t, "lat": np.arange(nlat) * 1.0, "lon": np.arange(nlon) * 1.0})


def assert_same_result(a, b, intermediate=False):
    np.testing.assert_array_equal(a[0]["thresh"], b[0]["thresh"])
    np.testing.assert_array_equal(a[0]["seas"], b[0]["seas"])
    np.testing.assert_array_equal(a[1].table, b[1].table)
    np.testing.assert_array_equal(a[1].offsets, b[1].offsets)
    np.testing.assert_array_equal(a[1].cell_index, b[1].cell_index)
    if intermediate:
        for k in a[2].data_vars:
            np.testing.assert_array_equal(a[2][k], b[2][k])


@pytest.mark.parametrize("case", ["plain", "pad", "intermediate", "cold", "slabs", "no_resident", "dict"])
def test_threshold_detect_equals_two_steps(gpu, case, monkeypatch):
    import xmhw_amd
    import xmhw_amd.device as dev
    temp = api_grid()
    kw, dkw = {}, {}
    if case == "pad":
        kw["maxPadLength"] = np.timedelta64(5, "D")
    if case == "intermediate":
        kw["intermediate"] = True
    if case == "cold":
        kw["coldSpells"] = True
    if case == "dict":
        dkw = {"order": 2, "harmonics": 1, "reference": "2001-06-01", "min_valid": 400}
    if case in ("slabs", "no_resident"):
        T = temp.values.shape[0]
        monkeypatch.setattr(dev, "device_budget_bytes", lambda fraction=0.6: 20 * T * 16 + 20 * 4 * 366 * 8)
    if case == "no_resident":
        monkeypatch.setenv("XMHW_AMD_RESIDENT_FRACTION", "0")
    fused = xmhw_amd.threshold_detect(temp, detrend=dkw if dkw else True, **kw)
    if case == "pad":
        # the two-step route interpolates first too: detrend() sees what threshold() would see
        import xmhw_amd.padding as padding
        from xmhw_amd.device import DeviceBuffer
        v = np.ascontiguousarray(temp.values.reshape(temp.values.shape[0], -1))
        spec = padding.PadSpec(temp.coords["time"], kw["maxPadLength"])
        d = DeviceBuffer.from_array(v)
        spec.apply(d.ptr, 4, v.shape[0], v.shape[1])
        gpu.stream_sync(0)
        filled = d.to_array(v.shape, np.float32).reshape(temp.values.shape)
        d.free(); spec.free()
        src = xmhw_amd.GridSeries(filled, temp.dims, temp.coords)
    else:
        src = temp
    det, fit = xmhw_amd.detrend(src, **dkw)
    assert fit.n_failed == 1 and np.isnan(det.values[:, 5, 0]).all()
    two = xmhw_amd.threshold_detect(det, **kw)
    assert_same_result(fused, two, intermediate=(case == "intermediate"))
    assert "xmhw_detrend" in fused[0].attrs and "xmhw_detrend" not in two[0].attrs
    print(f"{case}: {fused[1].n_events} events in {fused[1].n_cells} cells")
    assert fused[1].n_events > 50 and fused[1].n_cells == 6 * 8 - 2
    if case in ("slabs", "no_resident"):
        monkeypatch.undo()
        whole = xmhw_amd.threshold_detect(temp, detrend=True)
        assert_same_result(fused, whole)


def test_detrend_none_changes_nothing(gpu):
    import xmhw_amd
    temp = api_grid(seed=32)
    a = xmhw_amd.threshold_detect(temp)
    b = xmhw_amd.threshold_detect(temp, detrend=None)
    assert_same_result(a, b)
    assert "xmhw_detrend" not in b[0].attrs
    c = xmhw_amd.threshold_detect(temp, detrend=True)
    assert not np.array_equal(a[0]["thresh"], c[0]["thresh"], equal_nan=True)


def test_detrend_api_matches_oracle_and_slabs(gpu, monkeypatch):
    import xmhw_amd
    import xmhw_amd.device as dev
    temp = api_grid(dtype=np.float64, seed=33)
    out, fit = xmhw_amd.detrend(temp, order=2, harmonics=2, fitPeriod=[2001, 2004])
    T = temp.values.shape[0]
    monkeypatch.setattr(dev, "device_budget_bytes", lambda fraction=0.6: 7 * T * 32 + 7 * 100)
    out2, fit2 = xmhw_amd.detrend(temp, order=2, harmonics=2, fitPeriod=[2001, 2004])
    np.testing.assert_array_equal(out.values, out2.values)
    np.testing.assert_array_equal(fit.coef, fit2.coef)
    np.testing.assert_array_equal(fit.n_valid, fit2.n_valid)
    assert out.values.shape == temp.values.shape and out.values.dtype == np.float64 and fit.coef.shape == (7, 6, 9)
    from xmhw_amd.detrend import DetrendSpec
    spec = DetrendSpec(temp.coords["time"], 2, 2, fitPeriod=[2001, 2004])
    ref_keep, ref, rcoef, rnv = dor.standin_grid(temp.values.reshape(T, -1), spec, False)
    np.testing.assert_array_equal(fit.n_valid.reshape(-1), rnv)
    np.testing.assert_array_equal(np.isnan(out.values.reshape(T, -1)), np.isnan(ref))
    scale = np.nanmax(np.abs(temp.values.reshape(T, -1)), axis=0, initial=1.0)
    err = np.nanmax(np.abs(out.values.reshape(T, -1) - ref) / scale)
    cerr = np.nanmax(np.abs(fit.coef.reshape(7, -1) - rcoef) / scale)
    print(f"detrend() float64 grid: value error {err:.2e}, coefficient error {cerr:.2e} of max|y|")
    assert err <= TOL64 and cerr <= TOL64
    assert fit.n_failed == 1


# ---- 5. a planted trend -----------------------------------------------------------------------------------------------------
def test_planted_trend(gpu):
    import xmhw_amd
    t = AXES["40y_daily"]()
    T = t.shape[0]
    spec_x = (days_of(t) - (T - 1) / 2.0) / 3652.5
    d = days_of(t)
    y = np.empty((T, 3))
    y[:, 0] = 15 + 0.3 * spec_x
    y[:, 1] = 15 + 0.3 * spec_x + 4 * np.sin(2 * np.pi * d / 365.25) + 1.5 * np.cos(4 * np.pi * d / 365.25)
    y[:, 2] = y[:, 1]
    y[np.random.default_rng(8).random(T) < 0.2, 2] = np.nan
    temp = xmhw_amd.GridSeries(y, ("time", "cell"), {"time": t, "cell": np.arange(3)})
    out, fit = xmhw_amd.detrend(temp)
    tol = TOL64 * float(np.nanmax(np.abs(y)))
    print("planted 0.3 per decade, fitted:", fit.trend_per_decade)
    np.testing.assert_allclose(fit.trend_per_decade, 0.3, rtol=0, atol=tol)
    np.testing.assert_allclose(fit["const"], 15.0, rtol=0, atol=tol)
    np.testing.assert_allclose(np.hypot(fit["cos1"], fit["sin1"]), [0.0, 4.0, 4.0], rtol=0, atol=tol)   # (phases count from t_ref)
    np.testing.assert_allclose(np.hypot(fit["cos2"], fit["sin2"]), [0.0, 1.5, 1.5], rtol=0, atol=tol)
    # the detrended series has no trend of its own
    _, fit2 = xmhw_amd.detrend(out)
    print("trend of the detrended series:", fit2.trend_per_decade)
    assert np.max(np.abs(fit2.trend_per_decade)) <= tol
    np.testing.assert_allclose(out.values[:, 0], 15.0, rtol=0, atol=tol)
    # float32 input keeps its dtype
    out32, fit32 = xmhw_amd.detrend(xmhw_amd.GridSeries(y.astype(np.float32), temp.dims, temp.coords))
    assert out32.values.dtype == np.float32
    np.testing.assert_allclose(fit32.trend_per_decade, 0.3, atol=1e-5)


# ---- 6. more terms than the kernels take ---------------------------------------------------------------------------------------
def test_eleven_terms_unsupported(gpu):
    from xmhw_amd.device import DeviceBuffer
    T, C, P = 100, 8, 11
    y = np.random.default_rng(1).normal(size=(T, C)).astype(np.float32)
    B = np.random.default_rng(2).normal(size=(T, P))
    d_ts, d_b = DeviceBuffer.from_array(y), DeviceBuffer.from_array(B)
    d_c = DeviceBuffer.from_array(np.full((P, C), -555.0))
    d_n = DeviceBuffer.from_array(np.full(C, -9, dtype=np.int32))
    try:
        with pytest.raises(gpu.HipError, match=r"code 3"):
            gpu.series_fit(d_ts.ptr, 4, T, C, C, d_b.ptr, P, 0, 0, d_c.ptr, C, d_n.ptr)
        with pytest.raises(gpu.HipError, match=r"code 3"):
            gpu.series_remove(d_ts.ptr, 4, T, C, C, d_b.ptr, P, 1, d_c.ptr, C)
        gpu.stream_sync(0)
        np.testing.assert_array_equal(d_ts.to_array((T, C), np.float32), y)
        assert (d_c.to_array((P, C), np.float64) == -555.0).all() and (d_n.to_array((C,), np.int32) == -9).all()
        with pytest.raises(gpu.InvalidArgument):
            gpu.series_remove(d_ts.ptr, 4, T, C, C, d_b.ptr, 4, 5, d_c.ptr, C)
        with pytest.raises(gpu.InvalidArgument):
            gpu.series_fit(d_ts.ptr, 4, T, C, C - 1, d_b.ptr, 4, 0, 0, d_c.ptr, C, 0)
        # nothing is launched for C == 0 or T == 0
        gpu.series_fit(d_ts.ptr, 4, T, 0, 0, d_b.ptr, 4, 0, 0, d_c.ptr, 0, 0)
        gpu.series_fit(d_ts.ptr, 4, 0, C, C, d_b.ptr, 4, 0, 0, d_c.ptr, C, 0)
        gpu.series_remove(d_ts.ptr, 4, 0, C, C, d_b.ptr, 4, 1, d_c.ptr, C)
        gpu.stream_sync(0)
        assert (d_c.to_array((P, C), np.float64) == -555.0).all()
    finally:
        for b in (d_ts, d_b, d_c, d_n):
            b.free()
