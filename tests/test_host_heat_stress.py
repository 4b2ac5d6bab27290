"""heat_stress() and maximum_monthly_mean() without a GPU: hand cases, the oracle (tests/heat_stress_oracle.py) as the
device stage behind the host layer (class labels, baseline forms, land, derived views, exceptions), and the refusals of
the C entries that come before their first HIP call.  Integers are compared exactly, and so are the derived floats: the
host formula is fixed."""
import importlib

import numpy as np
import numpy.testing as npt
import pytest

import heat_stress_cases as hc
import heat_stress_oracle as ho
from xmhw_amd import (GridSeries, HeatStressDataset, MonthlyMeanDataset, XmhwException, degree_heating_weeks, heat_stress,
                      maximum_monthly_mean)
from xmhw_amd.heat_stress import MAX_CLASSES, check_stress_arguments, levels_q, snapshot_steps

ONE = 65536.0


def days(start, n):
    return np.datetime64(start) + np.arange(n).astype("timedelta64[D]")


def point(values, start="2001-10-01"):
    values = np.asarray(values)
    return GridSeries(values, ("time",), {"time": days(start, values.shape[0])})


def stress(temp, base, **kw):
    return heat_stress(temp, base, _compute=ho.heat_stress_cells, **kw)


def mmm_of(temp, **kw):
    return maximum_monthly_mean(temp, _compute=ho.class_sums_cells, **kw)


@pytest.fixture(scope="module")
def sample(oisst):
    time = oisst["time64"]
    temp = GridSeries(oisst["sst"], ("time", "lat", "lon"), {"time": time, "lat": oisst["lat"], "lon": oisst["lon"]})
    x = oisst["sst"].reshape(time.shape[0], -1)
    keep = ~np.isnan(x).all(axis=0)
    month = time.astype("datetime64[M]").astype(np.int64) % 12
    return {"temp": temp, "time": time, "x": x[:, keep].astype(np.float64), "keep": keep, "month": month, "mmm": mmm_of(temp)}


# ---- the oracle itself -------------------------------------------------------------------------------

def test_oracle_windows_against_a_plain_loop():
    d = hc.synthetic(120, 9, np.float32, 3, 7, D=366)
    f = ho.step_fields(d["ts"], d["base"], d["rows"], 7, 1.0)
    for t in (0, 5, 6, 7, 63, 119):
        npt.assert_array_equal(f["S"][t], f["q"][max(0, t - 6):t + 1].sum(axis=0))
    assert f["hot"].sum() > 0 and (f["q"][f["hot"]] >= ONE).all() and (f["q"][~f["hot"]] == 0).all()
    assert not f["valid"][:, 3].any() and f["n_range"] == 0                       # the cell without a baseline
    r = ho.reduce_by_class(f, *hc.per_year(120), hc.levels(3), [0, 119])
    hc.check_case(r)
    assert (r["counts"][:, 5:] == 0).all() and r["counts"].dtype == np.int32 and r["hsum_q"].dtype == np.int64
    npt.assert_array_equal(r["hsum_q"].sum(axis=0), f["q"].sum(axis=0))


# ---- hand cases --------------------------------------------------------------------------------------

def test_constant_excess_of_two_degrees_is_24_degree_heating_weeks():
    r = stress(point(np.full(200, 22.0, np.float32)), 20.0, at=[82, 83, 199])
    npt.assert_array_equal(r.klass, [2001, 2002])
    npt.assert_array_equal(r.n_steps, [92, 108])
    npt.assert_array_equal(r.dhw_at, [83 * 2.0 / 7.0, 24.0, 24.0])
    npt.assert_array_equal(r.dhw_peak, [24.0, 24.0])
    npt.assert_array_equal(r.peak_t, [83, 92])                   # step 83 in the first year, the first step of the second
    npt.assert_array_equal(r.peak_q, [84 * 2 * 65536] * 2)
    npt.assert_array_equal(r.n_hot, [92, 108])
    npt.assert_array_equal(r.degree_days, [184.0, 216.0])
    # levels 4 and 8: S >= 4 weeks from step 13 (14 days x 2 degrees), >= 8 weeks from step 27
    npt.assert_array_equal(r.n_level, [[92 - 13, 92 - 27], [108, 108]])
    assert r.quantisation_bound() < 1e-3 and r.keep == np.array(True)


def test_a_sample_on_the_floor_counts_and_the_next_float_below_does_not():
    x = np.full(10, 19.0)
    x[2], x[5] = 21.0, np.nextafter(21.0, 0.0)
    r = stress(point(x), 20.0, classes="all", at=[2, 5])
    npt.assert_array_equal(r.n_hot, [1])
    npt.assert_array_equal(r.snap_q, [65536, 65536])              # the step below the floor adds nothing
    r = stress(point(x), 20.0, classes="all", min_hotspot=1.0 - 2.0 ** -40)
    npt.assert_array_equal(r.n_hot, [2])


def test_a_single_hot_day_leaves_the_window_after_W_steps():
    x = np.full(40, 19.0, np.float32)
    x[10] = 23.5
    r = stress(point(x), 20.0, window=7, classes="all", at=[9, 10, 16, 17], levels=())
    npt.assert_array_equal(r.snap_q, [0, 3.5 * 65536, 3.5 * 65536, 0])
    npt.assert_array_equal(r.peak_t, [10])
    npt.assert_array_equal(r.dhw_peak, [0.5])
    assert r.n_level.shape == (1, 0)


# ---- the MMM -----------------------------------------------------------------------------------------

def test_mmm_of_the_oisst_sample_against_plain_numpy(sample):
    mm, x, month = sample["mmm"], sample["x"], sample["month"]
    assert isinstance(mm, MonthlyMeanDataset) and mm.mmm.shape == (8, 2) and int(mm.keep.sum()) == 12
    assert x.shape == (731, 12)
    sum_q = np.stack([np.rint(x[month == m] * ONE).astype(np.int64).sum(axis=0) for m in range(12)])
    n = np.stack([(month == m).sum() * np.ones(12, np.int32) for m in range(12)])
    npt.assert_array_equal(mm.sum_q[:, mm.keep], sum_q)
    npt.assert_array_equal(mm.n_valid[:, mm.keep], n)
    npt.assert_array_equal(mm.monthly_mean[:, mm.keep], sum_q / n.astype(np.float64) / ONE)
    plain = np.stack([x[month == m].mean(axis=0) for m in range(12)])
    assert np.abs(mm.monthly_mean[:, mm.keep] - plain).max() <= 2.0 ** -17 + 1e-12
    npt.assert_array_equal(mm.mmm[mm.keep], (sum_q / n.astype(np.float64) / ONE).max(axis=0))
    assert np.isnan(mm.mmm[~mm.keep]).all() and np.isnan(mm.monthly_mean[:, ~mm.keep]).all()


def test_heat_stress_of_the_oisst_sample(sample):
    """With the MMM of the definition (all steps of a calendar month, both years), h0 = 1.0 and W = 84, plain numpy finds
    159 hot cell-days, every one of the 12 ocean cells with S > 0 and a peak of 2.85 degree heating weeks: levels 4 and
    8 are out of reach on this sample, the tests on it use levels (1, 2).  (The issue that asked for this stage quoted 155
    hot cell-days and a peak of 2.80 for the same sample; plain numpy does not give those for the MMM as defined, nor for
    the mean of the yearly monthly means (149, 2.79), float32 means (159, 2.85) or either year alone.  The figures
    asserted here are computed in this test, by numpy alone, before the stage is called.)"""
    x, month, mm = sample["x"], sample["month"], sample["mmm"]
    plain_mmm = np.stack([x[month == m].mean(axis=0) for m in range(12)]).max(axis=0)
    h = x - plain_mmm
    hot = h >= 1.0
    S = np.stack([np.where(hot, h, 0.0)[max(0, t - 83):t + 1].sum(axis=0) for t in range(731)])
    assert int(hot.sum()) == 159 and int((S.max(axis=0) > 0).sum()) == 12 and round(S.max() / 7.0, 2) == 2.85
    r = stress(sample["temp"], mm, levels=(1, 2), at=[0, 400, 730])
    assert isinstance(r, HeatStressDataset) and r.peak_q.shape == (2, 8, 2)
    npt.assert_array_equal(r.klass, [2003, 2004])
    assert int(r.n_hot.sum()) == 159 and int((r.peak_q.max(axis=0) > 0).sum()) == 12
    assert round(float(np.nanmax(r.dhw_peak)), 2) == 2.85
    assert np.abs(np.nanmax(r.dhw_peak) - S.max() / 7.0) <= r.quantisation_bound() + 84 * 2.0 ** -17 / 7
    assert r.n_level[:, 0].sum() > r.n_level[:, 1].sum() > 0
    # against the oracle on the compact cells
    f = ho.heat_stress_full(sample["x"].astype(np.float32), mm.mmm[mm.keep][None], np.zeros(731, int), 84, 1.0,
                            (sample["time"].astype("datetime64[Y]").astype(int) - 33), 2, levels_q((1, 2), 7.0), [0, 400, 730])
    npt.assert_array_equal(r.peak_q[:, r.keep], f["peak_q"])
    npt.assert_array_equal(r.peak_t[:, r.keep], f["peak_t"])
    npt.assert_array_equal(r.snap_q[:, r.keep], f["snap_q"])
    npt.assert_array_equal(r.hsum_q[:, r.keep], f["hsum_q"])
    npt.assert_array_equal(r.dhw_peak[:, r.keep], f["peak_q"] / (7.0 * ONE))
    npt.assert_array_equal(r.degree_days[:, r.keep], f["hsum_q"] / ONE)
    # land: integers 0 (peak_t -1), floats NaN
    assert (r.peak_q[:, ~r.keep] == 0).all() and (r.peak_t[:, ~r.keep] == -1).all() and np.isnan(r.dhw_peak[:, ~r.keep]).all()
    assert np.isnan(r.dhw_at[:, ~r.keep]).all() and (r.n_valid[:, r.keep] == [[365], [366]]).all()
    both = degree_heating_weeks(sample["temp"], levels=(1, 2), at=[0, 400, 730], _compute=(ho.class_sums_cells, ho.heat_stress_cells))
    npt.assert_array_equal(both.peak_q, r.peak_q)
    npt.assert_array_equal(both.dhw_at, r.dhw_at)


def test_mmm_period_and_offset(sample):
    temp = sample["temp"]
    one = mmm_of(temp, period=(2004, 2004))
    x, month = sample["x"][365:], sample["month"][365:]
    want = np.stack([np.rint(x[month == m] * ONE).astype(np.int64).sum(axis=0) for m in range(12)])
    npt.assert_array_equal(one.sum_q[:, one.keep], want)
    same = mmm_of(temp, period=(np.datetime64("2004-01-01"), np.datetime64("2004-12-31")))
    npt.assert_array_equal(same.sum_q, one.sum_q)
    part = mmm_of(temp, period=(np.datetime64("2003-01-01"), np.datetime64("2003-11-30")))
    assert np.isnan(part.mmm).all() and (part.n_valid[11] == 0).all()          # no December: no MMM
    shifted = mmm_of(temp, offset=10.0)
    assert np.abs(shifted.mmm - sample["mmm"].mmm)[shifted.keep].max() <= 2.0 ** -16
    with pytest.raises(XmhwException, match="selects no time step"):
        mmm_of(temp, period=(1985, 2002))
    with pytest.raises(XmhwException, match="2\\*\\*7 and more from offset"):
        mmm_of(temp, offset=273.15)
    with pytest.raises(XmhwException, match="offset should be finite"):
        mmm_of(temp, offset=np.inf)
    with pytest.raises(XmhwException, match="datetime64 time coordinate"):
        mmm_of(GridSeries(np.zeros(5), ("time",), {"time": np.arange(5)}))


# ---- classes, snapshots, inputs ----------------------------------------------------------------------

def test_class_forms_and_snapshot_dates(sample):
    temp, mm, time = sample["temp"], sample["mmm"], sample["time"]
    kw = dict(levels=(1, 2))
    year, allc, month = stress(temp, mm, **kw), stress(temp, mm, classes="all", **kw), stress(temp, mm, classes="month", **kw)
    npt.assert_array_equal(month.klass, np.arange(1, 13))
    npt.assert_array_equal(allc.n_steps, [731])
    for r in (year, month):                                       # the classes partition the steps
        npt.assert_array_equal(r.hsum_q.sum(axis=0), allc.hsum_q[0])
        npt.assert_array_equal(r.n_hot.sum(axis=0), allc.n_hot[0])
        npt.assert_array_equal(r.n_level.sum(axis=0), allc.n_level[0])
        npt.assert_array_equal(r.peak_q.max(axis=0), allc.peak_q[0])
    labels = np.where(np.arange(731) % 5 == 0, -1, np.arange(731) % 3 + 10)
    arr = stress(temp, mm, classes=labels, **kw)
    npt.assert_array_equal(arr.klass, [10, 11, 12])
    assert arr.n_steps.sum() == 731 - 147 and (arr.hsum_q.sum(axis=0) <= allc.hsum_q[0]).all()
    step = int(allc.peak_t.max())                                 # a step with heat in its window
    none = stress(temp, mm, classes=np.full(731, -1), at=[step], **kw)
    npt.assert_array_equal(none.klass, [0])
    assert (none.peak_t == -1).all() and (none.peak_q == 0).all() and (none.n_valid == 0).all() and none.n_steps[0] == 0
    by_step = stress(temp, mm, at=[step], **kw)
    npt.assert_array_equal(none.snap_q, by_step.snap_q)          # a step of class -1 still feeds the window
    by_date = stress(temp, mm, at=[time[step]], **kw)
    npt.assert_array_equal(by_date.snap_q, by_step.snap_q)
    npt.assert_array_equal(by_date.at, [step])
    assert by_date.time_at[0] == time[step] and by_step.snap_q.max() > 0


def test_base_forms_cold_spells_and_climatology_base(sample):
    temp, mm = sample["temp"], sample["mmm"]
    kw = dict(levels=(1, 2), at=[300])
    ref = stress(temp, mm, **kw)
    full = np.full((8, 4), np.nan)
    full[sample["keep"].reshape(8, 4)] = mm.mmm[mm.keep]
    for base in (full, mm.as_series(), GridSeries(full, ("lat", "lon"), {"lat": temp.coords["lat"], "lon": temp.coords["lon"]})):
        r = stress(temp, base, **kw)
        npt.assert_array_equal(r.peak_q, ref.peak_q)
        npt.assert_array_equal(r.snap_q, ref.snap_q)
    # cold spells: the mirrored series against the mirrored base
    cold = stress(GridSeries(-temp.values, temp.dims, temp.coords), -full, coldSpells=True, **kw)
    npt.assert_array_equal(cold.peak_q, ref.peak_q)              # negation is exact
    npt.assert_array_equal(cold.hsum_q, ref.hsum_q)
    below = stress(temp, full, coldSpells=True, **kw)            # the series itself: its excursions BELOW the base
    assert below.hsum_q.max() > 0 and (below.hsum_q != ref.hsum_q).any()
    # a (doy, lat, lon) base: constant along doy it is the constant base
    clim = np.broadcast_to(full, (366, 8, 4)).copy()
    r = stress(temp, clim, **kw)
    npt.assert_array_equal(r.peak_q, ref.peak_q)
    clim[59] += 50.0                                             # Feb 29 (doy 60) raised: 2004 loses that day's heat only
    r = stress(temp, GridSeries(clim, ("doy", "lat", "lon"), {"doy": np.arange(1, 367), "lat": temp.coords["lat"],
                                                              "lon": temp.coords["lon"]}), **kw)
    assert (r.hsum_q <= ref.hsum_q).all()
    with pytest.raises(XmhwException, match="base should be"):
        stress(temp, np.zeros(4), **kw)


def test_point_series_and_dataset_views():
    x = np.full(120, 19.0, np.float64)
    x[20:60] = 21.5
    x[70] = np.nan
    r = stress(point(x, "2001-01-01"), np.float64(20.0), window=14, unit=7.0, levels=(1.0, 3.0, 3.5), classes="month", at=[59])
    npt.assert_array_equal(r.klass, [1, 2, 3, 4])
    npt.assert_array_equal(r.n_valid, [31, 28, 30, 30])
    npt.assert_array_equal(r.n_hot, [11, 28, 1, 0])
    npt.assert_array_equal(r.dhw_at, [3.0])
    npt.assert_array_equal(r.n_level[:, 2], 0)
    assert r.sdims == () and r.levels.tolist() == [1.0, 3.0, 3.5] and r.window == 14
    assert r.attrs["classes"] == "month" and r.attrs["window"] == 14


def test_to_xarray(sample):
    pytest.importorskip("xarray")
    ds = stress(sample["temp"], sample["mmm"], levels=(1, 2), at=[5]).to_xarray()
    assert ds["dhw_peak"].dims == ("klass", "lat", "lon") and ds["snap_q"].dims == ("at", "lat", "lon")
    assert sample["mmm"].to_xarray()["mmm"].dims == ("lat", "lon")


# ---- refusals ----------------------------------------------------------------------------------------

def test_host_refusals(sample):
    temp, mm = sample["temp"], sample["mmm"]
    cases = [
        (dict(window=0), "window should be"), (dict(window=256), "window should be"), (dict(window=7.5), "window should be"),
        (dict(min_hotspot=0.0), "hot-spot floor"), (dict(min_hotspot=128.0), "hot-spot floor"),
        (dict(min_hotspot=np.nan), "hot-spot floor"), (dict(unit=0.0), "unit should be"),
        (dict(levels=(1, 2, 3, 4, 5, 6, 7)), "at most 6 levels"), (dict(levels=(2, 1)), "strictly ascending"),
        (dict(levels=(1, 1)), "strictly ascending"), (dict(levels=(np.nan,)), "finite"),
        (dict(at=np.arange(65)), "at most 64 snapshot"), (dict(at=[5, 5]), "strictly ascending"), (dict(at=[7, 3]), "strictly ascending"),
        (dict(at=[731]), r"in \[0, 731\)"), (dict(at=[-1]), r"in \[0, 731\)"), (dict(at=[1.5]), "time steps"),
        (dict(at=[np.datetime64("2010-01-01")]), "not on the time axis"),
        (dict(classes="decade"), "classes should be"),
        (dict(classes=np.zeros(5, int)), "one entry per time step"), (dict(tdim="t"), "dimension not present"),
    ]
    for kw, text in cases:
        with pytest.raises(XmhwException, match=text):
            stress(temp, mm, **kw)
    with pytest.raises(XmhwException, match=f"at most {MAX_CLASSES} classes"):
        stress(point(np.zeros(1100)), 0.0, classes=np.arange(1100))
    with pytest.raises(XmhwException, match="2\\*\\*7 and more above their baseline"):
        stress(GridSeries(temp.values + 273.15, temp.dims, temp.coords), mm)
    # the stage-side check raises the same
    with pytest.raises(XmhwException, match="class labels should be in"):
        check_stress_arguments(10, np.full(10, 3), 2, 84, 1.0, np.zeros(0, np.int64), np.zeros(0, np.int64))
    assert levels_q((4, 8), 7.0).tolist() == [4 * 7 * 65536, 8 * 7 * 65536] and snapshot_steps(None, None).shape == (0,)


def test_c_entry_refusals_need_no_device_and_raise_the_exceptions_of_the_core_module():
    core = importlib.import_module("xmhw_amd._xmhw_hip")
    m = importlib.import_module("xmhw_amd._xmhw_hip_stress")
    assert not any(hasattr(m, n) for n in ("HipError", "Unsupported", "InvalidArgument", "CommError"))
    T = 10
    z, none64, none32 = np.zeros(T, np.int32), np.zeros(0, np.int64), np.zeros(0, np.int32)

    def acc(T=T, C=4, ld=4, ldb=4, D=1, rows=z, W=84, h0=1.0, classes=z, K=1, level_q=none64, at=none32, ldo=4, itemsize=4):
        m.heat_stress_accumulate(0, itemsize, T, C, ld, 0, ldb, D, rows, 0, W, h0, classes, K, level_q, at, 0, 0, 0, 0, ldo, 0)

    def sums(T=T, C=4, ld=4, x0=0.0, classes=z, K=1, ldo=4):
        m.class_sums_accumulate(0, 4, T, C, ld, x0, classes, K, 0, 0, ldo, 0)

    unsupported = [lambda: acc(K=0), lambda: acc(K=1025), lambda: acc(W=0), lambda: acc(W=256),
                   lambda: acc(level_q=np.arange(7)), lambda: acc(at=np.arange(65, dtype=np.int32)), lambda: acc(C=1 << 31, ld=1 << 31, ldb=1 << 31, ldo=1 << 31),
                   lambda: sums(K=0), lambda: sums(K=1025), lambda: sums(C=1 << 31, ld=1 << 31, ldo=1 << 31),
                   lambda: m.heat_stress_init(0, 4, 0, 0, 0, 4, 0), lambda: m.class_sums_init(1025, 4, 0, 0, 4, 0),
                   lambda: m.heat_stress_finish(0, 4, 0, 0, 0, 4)]
    for call in unsupported:
        with pytest.raises(core.Unsupported) as e:
            call()
        assert type(e.value) is core.Unsupported and isinstance(e.value, core.HipError) and "(code 3)" in str(e.value)
    invalid = [(lambda: acc(classes=np.full(T, 1, np.int32)), r"class_of_t outside \[-1, K\)"),
               (lambda: acc(classes=np.full(T, -2, np.int32)), r"class_of_t outside"),
               (lambda: acc(rows=np.full(T, 1, np.int32)), r"row_of_t outside \[0, D\)"),
               (lambda: acc(level_q=np.array([5, 5])), "level_q not strictly ascending"),
               (lambda: acc(level_q=np.array([5, 4])), "level_q not strictly ascending"),
               (lambda: acc(at=np.array([3, 3], np.int32)), "snapshot steps"), (lambda: acc(at=np.array([T], np.int32)), "snapshot steps"),
               (lambda: acc(at=np.array([-1], np.int32)), "snapshot steps"),
               (lambda: acc(h0=0.0), "h0 outside"), (lambda: acc(h0=128.0), "h0 outside"), (lambda: acc(h0=np.nan), "h0 outside"),
               (lambda: acc(ld=3), "bad T/C"), (lambda: acc(ldo=3), "bad T/C"), (lambda: acc(D=0), "bad T/C"),
               (lambda: acc(rows=np.zeros(T + 1, np.int32)), "row_of_t length"), (lambda: acc(itemsize=2), "itemsize"),
               (lambda: acc(), "NULL buffer"),
               (lambda: sums(classes=np.full(T, 1, np.int32)), r"class_of_t outside"), (lambda: sums(x0=np.inf), "x0 must be finite"),
               (lambda: sums(ldo=3), "bad T/C"), (lambda: sums(), "NULL buffer"),
               (lambda: m.heat_stress_init(1, 4, 0, 0, 0, 3, 0), "bad C/ldo"), (lambda: m.heat_stress_init(1, 4, 0, 0, 0, 4, 0), "NULL"),
               (lambda: m.class_sums_init(1, 4, 0, 0, 4, 0), "NULL"), (lambda: m.heat_stress_finish(1, 4, 0, 0, 0, 4), "NULL"),
               (lambda: m.set_heat_stress_block(-1), "steps must be")]
    for call, text in invalid:
        with pytest.raises(core.InvalidArgument, match=text) as e:
            call()
        assert type(e.value) is core.InvalidArgument
    # nothing is launched for C == 0: no device is needed either
    acc(C=0, ld=0, ldb=0, ldo=0)
    sums(C=0, ld=0, ldo=0)
    m.heat_stress_finish(1, 0, 0, 0, 0, 0)
    m.set_heat_stress_block(0)
    assert (m.HEAT_STRESS_MAX_CLASSES, m.HEAT_STRESS_CHANNELS, m.HEAT_STRESS_MAX_LEVELS, m.HEAT_STRESS_MAX_SNAPSHOTS,
            m.HEAT_STRESS_MAX_WINDOW, m.HEAT_STRESS_BITS) == (1024, 8, 6, 64, 255, 16)


def test_the_loader_wraps_the_stress_module_like_the_core_module():
    from xmhw_amd import _lib
    hs = _lib.hip_stress()
    assert isinstance(hs, _lib._RetryOnNoMem) and hs is _lib.hip_stress()
    assert hs.HEAT_STRESS_MAX_WINDOW == 255 and callable(hs.heat_stress_accumulate)
