"""The host logic of coarsen() without a device: the exports, the refusals of the C entries in their stated order (they
come before the first HIP call), the arguments of the public function, ``space`` in its three forms, the windows from
``time``, ``windows`` and calendar_windows(), trim against pad, the coarse coordinates and ``time_label``, the time blocks
of whole windows, the weight quantisation, the round trip through xarray where it imports, and the coarse series against
plain numpy means.  The device stage is stood in for by the oracle (tests/coarsen_oracle.py); the case list of the GPU
tests is checked to drop at most a quarter of its combinations."""
import importlib

import numpy as np
import numpy.testing as npt
import pytest

import coarsen_cases as cc
import coarsen_oracle as co
import xmhw_amd
from xmhw_amd import GridSeries, calendar_windows, coarsen
from xmhw_amd.exception import XmhwException

cm = importlib.import_module("xmhw_amd.coarsen")                 # (the package attribute of that name is the function)

NY, NX, T = 6, 10, 100
TIME = np.datetime64("2000-01-01") + np.arange(T).astype("timedelta64[D]")
LAT, LON = -10.0 + 0.25 * np.arange(NY), 100.0 + 0.25 * np.arange(NX)
COORDS = {"time": TIME, "lat": LAT, "lon": LON}
STAGE = co.as_stage


def series(dtype=np.float32, seed=1, nan_frac=0.0, dims=("time", "lat", "lon")):
    rng = np.random.default_rng(seed)
    x = rng.normal(15.0, 3.0, (T, NY, NX)).astype(dtype)
    x[rng.random(x.shape) < nan_frac] = np.nan
    order = [("time", "lat", "lon").index(d) for d in dims]
    return GridSeries(np.transpose(x, order), dims, COORDS), x


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def test_exports():
    for name in ("coarsen", "CoarsenInfo", "calendar_windows"):
        assert name in xmhw_amd.__all__
    assert xmhw_amd.coarsen is cm.coarsen and xmhw_amd.CoarsenInfo is cm.CoarsenInfo
    assert xmhw_amd.calendar_windows is cm.calendar_windows


def test_case_list_drops_at_most_a_quarter():
    cases = cc.listed()                                          # (asserts the quarter itself)
    total = len(cc.GRIDS) * len(cc.FACTORS) * len(cc.BOUNDARIES) * len(cc.DTYPES)
    assert 4 * (total - len(cases)) <= total
    assert {(c.ny, c.nx) for c in cases} == set(cc.GRIDS) and {(c.fy, c.fx) for c in cases} == set(cc.FACTORS)
    assert {c.window for c in cases} == set(cc.WINDOWS) and {c.a for c in cases} == set(cc.SHARES)
    assert len({cc.case_id(c) for c in cases}) == len(cases)


def test_c_entry_refusals_in_their_stated_order_need_no_device():
    core = importlib.import_module("xmhw_amd._xmhw_hip")
    m = importlib.import_module("xmhw_amd._xmhw_hip_coarsen")
    assert not any(hasattr(m, n) for n in ("HipError", "Unsupported", "InvalidArgument", "CommError"))
    assert (m.COARSEN_MAX_VOLUME, m.COARSEN_MAX_WEIGHT_BITS, m.COARSEN_BITS) == (cm.MAX_VOLUME, cm.WEIGHT_BITS, cm.BITS)
    w10 = np.arange(0, 11, 5, dtype=np.int32)

    def call(nt=10, ld=12, ny=3, nx=4, fy=2, fx=2, ncy=2, ncx=2, x0=0.0, a=0, win=w10, ldo=4, itemsize=4):
        m.coarsen(0, itemsize, nt, ld, ny, nx, fy, fx, ncy, ncx, 0, x0, a, win, 0, ldo, 0, 0, 0)

    # the cap first: it wins over everything that is invalid as well
    with pytest.raises(core.Unsupported, match="cap of 4096"):
        call(fy=17, fx=241, win=np.array([0, 1], np.int32), a=65537, ld=1)
    with pytest.raises(core.Unsupported, match="cap of 4096"):
        call(nt=4097, win=np.array([0, 4097], np.int32), fy=1, fx=1)
    with pytest.raises(core.Unsupported, match="2\\^31"):
        call(ny=65536, nx=32768, ld=1 << 31)
    for bad in (dict(nt=-1), dict(ny=-1), dict(ld=11), dict(fy=0), dict(fx=0), dict(fx=-2), dict(ncy=3), dict(ncx=-1), dict(ldo=3),
                dict(win=np.array([0, 5, 5], np.int32)), dict(win=np.array([0, 7, 3], np.int32)), dict(win=np.array([-1, 5], np.int32)),
                dict(win=np.array([0, 11], np.int32)), dict(a=65537), dict(a=-1), dict(x0=np.inf), dict(x0=np.nan)):
        with pytest.raises(core.InvalidArgument):
            call(**bad)
    with pytest.raises(core.InvalidArgument, match="itemsize"):
        call(itemsize=2)
    call(win=np.array([3], np.int32))                            # no window: nothing is launched, before any NULL check
    call(ncy=0, ldo=0)                                           # an empty coarse grid likewise
    with pytest.raises(core.InvalidArgument, match="NULL"):
        call()
    for bad in (-1, 3):
        with pytest.raises(core.InvalidArgument):
            m.set_coarsen_variant(bad)
    with pytest.raises(core.InvalidArgument):
        m.set_coarsen_chunk(-1)
    m.set_coarsen_variant(0)
    m.set_coarsen_chunk(0)


def test_alignment_class_of_the_entry():
    m = importlib.import_module("xmhw_amd._xmhw_hip_coarsen")
    assert m.coarsen_class(4096, 8192, 16, 8, 4, 3) == 0 and m.coarsen_class(4096, 8192, 16, 8, 4, 1) == 1
    assert m.coarsen_class(4096, 8192, 16, 8, 4, 2) == 3 and m.coarsen_class(4100, 8192, 16, 8, 4, 2) == 2
    assert m.coarsen_class(4096, 8192, 16, 8, 4, 4) == 5 and m.coarsen_class(4096, 8192, 18, 8, 4, 4) == 4
    assert m.coarsen_class(4096, 8192, 16, 7, 4, 2) == 2 and m.coarsen_class(4096, 8196, 16, 8, 4, 2) == 2
    try:
        m.set_coarsen_variant(1)
        assert m.coarsen_class(4096, 8192, 16, 8, 4, 2) == 2 and m.coarsen_class(4096, 8192, 16, 8, 4, 4) == 4
        m.set_coarsen_variant(2)
        assert m.coarsen_class(4096, 8192, 16, 8, 4, 2) == 0 and m.coarsen_class(4096, 8192, 16, 8, 4, 1) == 0
    finally:
        m.set_coarsen_variant(0)


def test_argument_refusals():
    g, _ = series()
    for kw in (dict(time=5, windows=[0, 5]), dict(time=0), dict(time=2.5), dict(windows=[0, 5, 5]), dict(windows=[5, 0]),
               dict(windows=[0, T + 1]), dict(windows=[[0, 5], [4, 9]]), dict(windows=[0.0, 5.0]), dict(space=0),
               dict(space=(2, 2, 2)), dict(space={"depth": 2}), dict(space="2"), dict(space=2.0), dict(min_fraction=1.5),
               dict(min_fraction=-0.1), dict(min_fraction="half"), dict(boundary="wrap"), dict(time_label="right"),
               dict(offset=np.inf), dict(weights="area"), dict(weights=np.ones((NY, NX + 1))), dict(weights=-np.ones((NY, NX))),
               dict(tdim="t"), dict(space=(8, 16)), dict(space=7, time=101), dict(space=(6, 10), time=100)):
        with pytest.raises(XmhwException):
            coarsen(g, _compute=STAGE, **kw)
    deep = GridSeries(np.zeros((T, 2, NY, NX), np.float32), ("time", "depth", "lat", "lon"), dict(COORDS, depth=np.arange(2.0)))
    with pytest.raises(XmhwException, match="one or two spatial dims"):
        coarsen(deep, _compute=STAGE)
    from xmhw_amd.device import PackedArray
    packed = GridSeries(np.zeros((T, NY, NX), np.int16), ("time", "lat", "lon"), COORDS)
    packed.values = PackedArray(packed.values, dict(scale=0.01, offset=0.0, fill=-32768, out="float32"))      # as open_series() does
    with pytest.raises(XmhwException, match="coarsen does not read packed int16 views: pass decoded floats"):
        coarsen(packed, _compute=STAGE)
    kelvin = GridSeries(g.values + np.float32(273.15), g.dims, COORDS)
    with pytest.raises(XmhwException, match="offset=273.15"):
        coarsen(kelvin, space=2, _compute=STAGE)
    coarsen(kelvin, space=2, offset=273.15, _compute=STAGE)


def test_space_as_int_pair_and_dict():
    g, x = series()
    want = x.astype(np.float64)[:, :, :9].reshape(T, 3, 2, 3, 3).mean(axis=(2, 4))
    for space in ((2, 3), {"lat": 2, "lon": 3}, [2, 3], (np.int64(2), np.int32(3))):
        c, info = coarsen(g, space=space, _compute=STAGE)
        assert c.values.shape == (T, 3, 3) and info.factors == {"lat": 2, "lon": 3}
        assert np.abs(c.values - want).max() <= 2.0 ** -17 + 0.5 * np.spacing(np.float32(32.0))
    both, _ = coarsen(g, space=2, _compute=STAGE)
    assert both.values.shape == (T, 3, 5)
    only, info = coarsen(g, space={"lon": 5}, _compute=STAGE)
    assert only.values.shape == (T, NY, 2) and info.factors == {"lat": 1, "lon": 5}
    same, _ = coarsen(g, _compute=STAGE)                         # (1, 1) and windows of one step: the series, requantised
    assert same.values.shape == (T, NY, NX) and np.abs(same.values - x).max() <= 2.0 ** -17 + 1e-6
    # the input's order of dims is kept; the factors go by name or in STACKED (sorted-name) order
    gt, _ = series(dims=("lon", "time", "lat"))
    c, _ = coarsen(gt, space=(2, 3), _compute=STAGE)
    assert c.dims == ("lon", "time", "lat") and c.values.shape == (3, T, 3)
    npt.assert_array_equal(bits(np.transpose(c.values, (1, 2, 0))), bits(coarsen(g, space=(2, 3), _compute=STAGE)[0].values))


def test_one_spatial_dim_and_time_only():
    rng = np.random.default_rng(4)
    x = rng.normal(10.0, 2.0, (T, 7)).astype(np.float64)
    g = GridSeries(x, ("time", "cell"), {"time": TIME, "cell": np.arange(7.0)})
    c, info = coarsen(g, space=3, time=10, boundary="pad", _compute=STAGE)
    assert c.values.shape == (10, 3) and c.values.dtype == np.float64 and info.factors == {"cell": 3}
    npt.assert_allclose(c.coords["cell"], [1.0, 4.0, 6.0])
    npt.assert_allclose(c.values[:, 2], x[:, 6].reshape(10, 10).mean(axis=1), atol=2.0 ** -17 + 1e-12, rtol=0)
    p = GridSeries(x[:, 0], ("time",), {"time": TIME})
    c, _ = coarsen(p, time=20, _compute=STAGE)
    assert c.dims == ("time",) and c.values.shape == (5,)
    npt.assert_allclose(c.values, x[:, 0].reshape(5, 20).mean(axis=1), atol=2.0 ** -17 + 1e-12, rtol=0)
    with pytest.raises(XmhwException):
        coarsen(p, space=2, _compute=STAGE)


def test_windows_from_time_windows_and_calendar():
    g, x = series(np.float64)
    x64 = x.astype(np.float64)
    c, info = coarsen(g, time=7, _compute=STAGE)                 # trim: 14 whole weeks of 100 days
    assert c.values.shape == (14, NY, NX)
    npt.assert_array_equal(info.windows, np.stack([np.arange(0, 98, 7), np.arange(7, 99, 7)], axis=1))
    npt.assert_allclose(c.values, x64[:98].reshape(14, 7, NY, NX).mean(axis=1), atol=2.0 ** -17 + 1e-12, rtol=0)
    npt.assert_array_equal(c.coords["time"], TIME[0:98:7])
    month = calendar_windows(TIME, "month")
    npt.assert_array_equal(month, [0, 31, 60, 91, 100])           # 2000: a leap year; April is partial and returned as it is
    npt.assert_array_equal(calendar_windows(TIME, "year"), [0, 100])
    two = np.datetime64("2000-12-30") + np.arange(5).astype("timedelta64[D]")
    npt.assert_array_equal(calendar_windows(two, "year"), [0, 2, 5])
    for bad in (dict(time_axis=TIME, unit="week"), dict(time_axis=np.arange(5), unit="month"), dict(time_axis=TIME[::-1], unit="month")):
        with pytest.raises(XmhwException):
            calendar_windows(**bad)
    c, info = coarsen(g, windows=month[:-1], _compute=STAGE)     # the user trims the partial month
    assert c.values.shape == (3, NY, NX)
    for s in range(3):
        npt.assert_allclose(c.values[s], x64[month[s]:month[s + 1]].mean(axis=0), atol=2.0 ** -17 + 1e-12, rtol=0)
    # pairs with uncovered steps between them
    pairs = np.array([[2, 5], [5, 6], [40, 70]])
    c, info = coarsen(g, windows=pairs, time_label="center", _compute=STAGE)
    npt.assert_array_equal(info.windows, pairs)
    for s, (t0, t1) in enumerate(pairs):
        npt.assert_allclose(c.values[s], x64[t0:t1].mean(axis=0), atol=2.0 ** -17 + 1e-12, rtol=0)
    npt.assert_array_equal(c.coords["time"], [TIME[3], TIME[5], TIME[40] + np.timedelta64(14, "D")])


def test_trim_against_pad_and_coordinates():
    g, x = series(np.float64)
    x64 = x.astype(np.float64)
    trim, it = coarsen(g, space=(4, 3), time=30, _compute=STAGE, coverage=True)
    pad, ip = coarsen(g, space=(4, 3), time=30, boundary="pad", _compute=STAGE, coverage=True)
    assert trim.values.shape == (3, 1, 3) and pad.values.shape == (4, 2, 4)
    npt.assert_array_equal(bits(trim.values), bits(pad.values[:3, :1, :3]))
    npt.assert_allclose(pad.values[3, 1, 3], x64[90:, 4:, 9:].mean(), atol=2.0 ** -17 + 1e-12, rtol=0)
    # coverage is relative to what the grid and the record hold: a partial block with all its samples is covered fully
    npt.assert_array_equal(ip.coverage, np.ones((4, 2, 4), np.float32))
    assert ip.coverage.dtype == np.float32 and it.coverage.shape == (3, 1, 3)
    assert ip.n[3, 1, 3] == 10 * 2 * 1 and ip.n[0, 0, 0] == 30 * 4 * 3
    npt.assert_allclose(trim.coords["lat"], [LAT[:4].mean()])
    npt.assert_allclose(pad.coords["lat"], [LAT[:4].mean(), LAT[4:].mean()])
    npt.assert_allclose(pad.coords["lon"], [LON[0:3].mean(), LON[3:6].mean(), LON[6:9].mean(), LON[9]])   # the last: non-uniform
    assert pad.coords["lat"].dtype == np.float64
    npt.assert_array_equal(pad.coords["time"], TIME[[0, 30, 60, 90]])
    mid, _ = coarsen(g, time=30, boundary="pad", time_label="center", _compute=STAGE)
    # the midpoint of the first and last stamps, in the unit of the axis (days: 29 // 2 = 14 and 9 // 2 = 4 days on)
    npt.assert_array_equal(mid.coords["time"], [TIME[14], TIME[44], TIME[74], TIME[94]])
    assert it.coverage is not None and coarsen(g, space=2, _compute=STAGE)[1].coverage is None


def test_min_fraction_in_65536ths_and_coverage():
    g, x = series(np.float64)
    v = x.copy()
    v[:, :2, :2] = np.nan
    v[:, 0, 2] = np.nan                                          # block (0, 1): 3 of 4 points, exactly 0.75
    v[:, 2:4, 0] = np.nan                                        # block (1, 0): 2 of 4
    gl = GridSeries(v, g.dims, COORDS)
    at = {f: coarsen(gl, space=2, min_fraction=f, _compute=STAGE, coverage=True) for f in (0.0, 0.5, 0.75, 0.75 + 2.0 ** -16, 1.0)}
    for f, (c, info) in at.items():
        assert info.a == int(np.rint(f * 65536))
        assert np.isnan(c.values[:, 0, 0]).all()                 # all land: n = 0, whatever the share
        assert np.isnan(c.values[:, 0, 1]).all() == (f > 0.75)   # equality counts as valid
        assert np.isnan(c.values[:, 1, 0]).all() == (f > 0.5)
        assert not np.isnan(c.values[:, 2, 2]).any()
    cov = at[0.0][1].coverage
    npt.assert_array_equal(cov[:, 0, 0], 0.0)
    npt.assert_array_equal(cov[:, 0, 1], 0.75)
    npt.assert_array_equal(cov[:, 1, 0], 0.5)


def test_time_blocks_are_unions_of_whole_windows():
    win = cm.check_windows(100, windows=np.array([[0, 7], [7, 14], [20, 30], [30, 31], [50, 90]]))
    assert cm.window_blocks(win, 8, 10 ** 9) == [(0, 5)]
    assert cm.window_blocks(win, 8, 0, block_steps=14) == [(0, 2), (2, 2), (4, 1)]
    assert cm.window_blocks(win, 8, 0, block_steps=1) == [(k, 1) for k in range(5)]      # one window at least
    assert cm.window_blocks(win, 8, 8 * 31) == [(0, 4), (4, 1)]
    assert cm._runs(win) == [(0, 2), (2, 2), (4, 1)] and cm._runs(win[:1]) == [(0, 1)]
    with pytest.raises(XmhwException):
        cm.window_blocks(win, 8, 0, block_steps=-1)


def test_weight_quantisation_and_coslat():
    g, x = series(np.float64)
    seen = {}

    def stage(field, ny, nx, fy, fx, ncy, ncx, wi, x0, a, win, **kw):
        seen["wi"] = wi
        return STAGE(field, ny, nx, fy, fx, ncy, ncx, wi, x0, a, win, **kw)

    c, info = coarsen(g, space=(6, 1), weights="coslat", _compute=stage)
    w = np.cos(np.deg2rad(LAT))
    npt.assert_array_equal(seen["wi"].reshape(NY, NX)[:, 0], np.rint(w / w.max() * 2 ** 24).astype(np.int32))
    assert seen["wi"].dtype == np.int32 and seen["wi"].max() == 1 << 24
    assert info.weight_unit == w.max() / 2 ** 24 and info.attrs["weights"] == "coslat"
    want = (x.astype(np.float64) * w[None, :, None]).sum(axis=1) / w.sum()
    # the rounding of the weights moves a mean of values within 2**7 of the offset by less than 6 * 2**7 / (6 * 2**23)
    npt.assert_allclose(c.values[:, 0], want, atol=2.0 ** -17 + 2.0 ** -16, rtol=0)
    arr = np.zeros((NY, NX))
    arr[1, :] = 3.0                                              # one row carries all the weight
    c, _ = coarsen(g, space=(6, 1), weights=arr, _compute=stage)
    assert seen["wi"].reshape(NY, NX)[1, 0] == 1 << 24 and seen["wi"].reshape(NY, NX)[0, 0] == 0
    npt.assert_allclose(c.values[:, 0], x[:, 1], atol=2.0 ** -17 + 1e-12, rtol=0)


def test_against_plain_numpy_means():
    """uniform weights, no NaN, float64: |coarse - mean| <= 2**-17 + 1e-12, the quantisation of the definition"""
    g, x = series(np.float64, seed=9)
    c, info = coarsen(g, space=(3, 5), time=10, _compute=STAGE)
    want = x.reshape(10, 10, 2, 3, 2, 5).mean(axis=(1, 3, 5))
    assert np.abs(c.values - want).max() <= 2.0 ** -17 + 1e-12
    assert (np.abs(c.values - want) <= info.quantisation_bound(c.values) + 1e-12).all()
    g32, x32 = series(np.float32, seed=9)
    c32, i32 = coarsen(g32, space=(3, 5), time=10, _compute=STAGE)
    assert c32.values.dtype == np.float32
    want32 = x32.astype(np.float64).reshape(10, 10, 2, 3, 2, 5).mean(axis=(1, 3, 5))
    bound = i32.quantisation_bound(c32.values)
    npt.assert_array_equal(bound, 2.0 ** -17 + 0.5 * np.spacing(np.abs(c32.values)).astype(np.float64))
    assert (np.abs(c32.values.astype(np.float64) - want32) <= bound + 1e-12).all()


def test_stage_shape_is_checked_and_result_feeds_a_stage():
    g, _ = series()
    with pytest.raises(XmhwException, match="coarsen stage returned"):
        coarsen(g, space=2, _compute=lambda *a, **k: (np.zeros((3, 3), np.float32), None, None, 0))
    c, _ = coarsen(g, space=2, time=2, _compute=STAGE)
    assert isinstance(c, GridSeries) and c.coords["time"].dtype == TIME.dtype and c.values.dtype == np.float32
    again, _ = coarsen(c, space={"lon": 5}, time=5, _compute=STAGE)     # an ordinary series: it goes in again
    assert again.values.shape == (10, 3, 1)


def test_xarray_in_and_out():
    xr = pytest.importorskip("xarray")
    g, x = series(np.float32)
    da = xr.DataArray(g.values, dims=g.dims, coords=COORDS, attrs={"units": "degC"}, name="sst")
    da["lat"].attrs["units"] = "degrees_north"
    c, info = coarsen(da, space={"lat": 2, "lon": 5}, time=10, _compute=STAGE, coverage=True)
    want, _ = coarsen(g, space=(2, 5), time=10, _compute=STAGE)
    assert isinstance(c, xr.DataArray) and c.dims == da.dims and c.name == "sst" and c.attrs == {"units": "degC"}
    npt.assert_array_equal(bits(c.values), bits(want.values))
    npt.assert_allclose(c["lat"].values, want.coords["lat"])
    assert c["lat"].attrs == {"units": "degrees_north"}
    ds = info.to_xarray()
    assert ds["coverage"].shape == (10, 3, 2) and ds.attrs["factor_lon"] == 5
