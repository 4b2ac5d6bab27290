"""mhw_days_by() without a GPU: the oracle (tests/days_by_oracle.py) on the cases of the GPU tests, the host layer
(class labels, land, derived fields, exceptions) with the oracle as the device stage, and the cross-check against the
event table that needs no new oracle."""
import numpy as np
import numpy.testing as npt
import pytest

import coverage_cases as cc
import days_by_cases as dc
import days_by_oracle as dbo
from detect_standin import oracle_detect_cells
from test_host_detect import clims, grid
from xmhw_amd import ClassDaysDataset, EventDataset, GridSeries, XmhwException, classes_from_events, mhw_days_by
from xmhw_amd.coverage import CATEGORIES
from xmhw_amd.days_by import MAX_CLASSES, class_labels
from xmhw_amd.detect import _detect


@pytest.fixture(scope="module")
def case257():
    d = cc.synthetic(203, 257, np.float32, seed=257, nan_frac=0.01)
    return d, dbo.states_and_anomalies(d["ts"], d["seas"], d["thresh"], d["doy"], d["doys"])


def test_oracle_on_the_twelve_class_case(case257):
    d, (st, a) = case257
    cls, K = dc.runs_of_17(203)
    r = dbo.reduce_by_class(st, a, cls, K)
    dc.check_case(r)
    assert r["days"].dtype == np.int32 and r["isum_q"].dtype == np.int64 and r["intensity_max"].dtype == np.float64
    assert r["days"][:, 4].sum(axis=1).min() >= 863
    npt.assert_array_equal(r["days"][:, :4].sum(axis=(0, 2)), [2430, 2691, 2474, 5920])
    assert int((r["days"][:, 4] - r["days"][:, 5]).sum()) == 32          # NaN samples of joined gaps
    assert r["n_range"] == 0 and np.nanmax(np.abs(a[st[..., 4]])) < 9
    assert 0.5 < (r["days"][:, 4] > 0).mean() < 0.6
    assert (r["days"][:, 4] >= r["days"][:, :4].sum(axis=1)).all() and (r["days"][:, 4] >= r["days"][:, 5]).all()
    # the classes partition the steps: their sum is the one-class result
    one = dbo.reduce_by_class(st, a, *dc.one_class(203))
    npt.assert_array_equal(r["days"].sum(axis=0), one["days"][0])
    npt.assert_array_equal(r["isum_q"].sum(axis=0), one["isum_q"][0])
    npt.assert_array_equal(np.fmax.reduce(r["intensity_max"], axis=0), one["intensity_max"][0])
    # the quantised mean against math.fsum
    with np.errstate(invalid="ignore"):
        mean = r["isum_q"] / (r["days"][:, 5] * 65536.0)
    ok = r["days"][:, 5] > 0
    assert ok.any() and np.isnan(r["mean_exact"][~ok]).all() and np.isnan(r["intensity_max"][~ok]).all()
    assert np.abs(mean[ok] - r["mean_exact"][ok]).max() <= ClassDaysDataset.quantisation_bound()


def test_oracle_on_labels_that_change_every_step(case257):
    d, (st, a) = case257
    cls, K = dc.every_step(203)
    assert (cls == -1).any() and (np.diff(cls) != 0).mean() > 0.8
    r = dbo.reduce_by_class(st, a, cls, K)
    dc.check_case(r)
    assert r["days"][:, 4].sum(axis=1).min() >= 1423
    one = dbo.reduce_by_class(st[cls >= 0], a[cls >= 0], np.zeros(int((cls >= 0).sum()), np.int32), 1)
    npt.assert_array_equal(r["days"].sum(axis=0), one["days"][0])          # the -1 steps count nowhere


def test_oracle_on_the_block_boundary_case():
    d = cc.synthetic(777, 300, np.float32, seed=3, nan_frac=0.02)
    r = dbo.class_days_full(d["ts"], d["seas"], d["thresh"], d["doy"], d["doys"], *dc.runs_of_17(777))
    dc.check_case(r)
    assert r["days"][:, 4].sum(axis=1).min() >= 4069
    assert int((r["days"][:, 4] - r["days"][:, 5]).sum()) == 288 and r["n_range"] == 0


def test_named_classes_on_a_leap_year():
    time = np.array(["2003-12-31", "2004-01-01", "2004-02-28", "2004-02-29", "2004-03-01", "2004-05-31", "2004-06-01",
                     "2004-08-31", "2004-09-01", "2004-11-30", "2004-12-01", "2005-01-15"], dtype="datetime64[D]")
    npt.assert_array_equal(class_labels("month", time), [12, 1, 2, 2, 3, 5, 6, 8, 9, 11, 12, 1])
    npt.assert_array_equal(class_labels("season", time), [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 0, 0])
    npt.assert_array_equal(class_labels("year", time), [2003, 2004, 2004, 2004, 2004, 2004, 2004, 2004, 2004, 2004, 2004, 2005])
    npt.assert_array_equal(class_labels("all", time), np.zeros(12))
    npt.assert_array_equal(class_labels("month", time.astype("datetime64[ns]")), class_labels("month", time))
    days = np.arange("2004-01-01", "2005-01-01", dtype="datetime64[D]")
    npt.assert_array_equal(np.bincount(class_labels("month", days))[1:], [31, 29, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31])
    npt.assert_array_equal(np.bincount(class_labels("season", days)), [31 + 29 + 31, 92, 92, 91])


def _ocean(oisst, th, se):
    T = oisst["sst"].shape[0]
    stacked = oisst["sst"].reshape(T, -1)
    keep = ~np.isnan(stacked).all(axis=0)
    thc, sec = th.values.reshape(th.values.shape[0], -1), se.values.reshape(se.values.shape[0], -1)
    return stacked[:, keep], sec[:, ~np.isnan(sec).all(axis=0)], thc[:, ~np.isnan(thc).all(axis=0)], keep


def test_grid_by_month_with_land(oisst):
    from xmhw_amd import calendar as cal
    g = grid(oisst)
    th, se = clims(oisst)
    ds = mhw_days_by(g, th, se, _compute=dbo.class_days_cells)
    assert isinstance(ds, ClassDaysDataset) and ds.category == CATEGORIES
    npt.assert_array_equal(ds.klass, np.arange(1, 13))
    T = oisst["sst"].shape[0]
    assert T == 731
    npt.assert_array_equal(ds.n_steps, [62, 28 + 29, 62, 60, 62, 60, 62, 62, 60, 62, 60, 62])       # 2003 and 2004
    ts, sek, thk, keep = _ocean(oisst, th, se)
    assert keep.sum() == 12 and not keep.all()
    month = class_labels("month", oisst["time64"])
    want = dbo.class_days_full(ts, sek, thk, cal.add_doy(oisst["time64"]), th.coords["doy"], month - 1, 12)
    assert want["days"][:, 4].sum() > 0 and (want["days"][:, :4].sum(axis=(0, 2)) > 0).any()
    keepg = keep.reshape(8, 4)
    alive_r, alive_c = keepg.any(axis=1), keepg.any(axis=0)
    kg = keepg[alive_r][:, alive_c]
    npt.assert_array_equal(ds.keep, kg)
    assert ds.days.shape == (12, 5) + kg.shape and ds.days.dtype == np.int32 and ds.isum_q.dtype == np.int64
    npt.assert_array_equal(ds.days[..., kg], want["days"][:, :5])
    npt.assert_array_equal(ds.n_valid[..., kg], want["days"][:, 5])
    npt.assert_array_equal(ds.isum_q[..., kg], want["isum_q"])
    npt.assert_array_equal(ds.intensity_max[..., kg], want["intensity_max"])
    # land: integer fields 0 under the keep mask, float fields NaN
    assert (ds.days[..., ~kg] == 0).all() and (ds.n_valid[..., ~kg] == 0).all()
    for f in (ds.intensity_max, ds.intensity_mean, ds.frequency):
        assert np.isnan(f[..., ~kg]).all()
    assert not np.isnan(ds.frequency[..., kg]).any()
    # derived fields
    npt.assert_array_equal(ds.frequency[..., kg], want["days"][:, 4] / ds.n_steps[:, None])
    ok = want["days"][:, 5] > 0
    got_mean = ds.intensity_mean[..., kg]
    assert ok.any() and np.isnan(got_mean[~ok]).all()
    assert np.abs(got_mean[ok] - want["mean_exact"][ok]).max() <= ds.quantisation_bound() == 2.0 ** -17 + 2.0 ** -45
    cmax = np.zeros(want["days"][:, 4].shape, dtype=int)
    for j in range(4):
        cmax[want["days"][:, j] > 0] = j + 1
    npt.assert_array_equal(ds.category_max[..., kg], cmax)
    assert cmax.max() >= 2 and (ds.category_max[..., ~kg] == 0).all()
    # the table cross-check: with all labels >= 0 the event days of a cell are the durations of its rows
    mhw = _detect(g, th, se, oracle_detect_cells)
    dur = mhw.table[:, mhw.columns.index("duration")]
    per_cell = [dur[mhw.offsets[i]:mhw.offsets[i + 1]].sum() for i in range(mhw.n_cells)]
    npt.assert_array_equal(ds.days[:, 4].sum(axis=0)[kg], per_cell)
    assert sum(per_cell) > 0


def test_table_cross_check_on_a_synthetic_case(case257):
    d, (st, a) = case257
    r = dbo.reduce_by_class(st, a, *dc.runs_of_17(203))
    tab = oracle_detect_cells(d["ts"], d["seas"], d["thresh"], d["doy"], d["doys"])
    dur = tab["table"][:, EventDataset.columns.index("duration")]
    off = tab["offsets"]
    npt.assert_array_equal(r["days"][:, 4].sum(axis=0), [dur[off[c]:off[c + 1]].sum() for c in range(257)])


def test_labels_with_gaps_and_negative_labels(oisst):
    g = grid(oisst)
    th, se = clims(oisst)
    T = oisst["sst"].shape[0]
    lab = np.where(np.arange(T) % 3 == 0, 40, 7)
    lab[100:300] = -5
    lab[300:310] = -1
    ds = mhw_days_by(g, th, se, classes=lab, _compute=dbo.class_days_cells)
    npt.assert_array_equal(ds.klass, [7, 40])
    npt.assert_array_equal(ds.n_steps, [(lab == 7).sum(), (lab == 40).sum()])
    everything = mhw_days_by(g, th, se, classes="all", _compute=dbo.class_days_cells)
    npt.assert_array_equal(everything.klass, [0])
    kept = mhw_days_by(g, th, se, classes=(lab >= 0).astype(int) - 1, _compute=dbo.class_days_cells)
    npt.assert_array_equal(ds.days.sum(axis=0), kept.days[0])
    assert 0 < kept.days[0, 4].sum() < everything.days[0, 4].sum()
    # every label negative: one empty class
    none = mhw_days_by(g, th, se, classes=np.full(T, -1), _compute=dbo.class_days_cells)
    assert none.klass.shape == (1,) and none.n_steps[0] == 0 and none.days.sum() == 0
    # seasons and years on the fixture's own axis
    by_year = mhw_days_by(g, th, se, classes="year", _compute=dbo.class_days_cells)
    npt.assert_array_equal(by_year.klass, [2003, 2004])
    npt.assert_array_equal(by_year.n_steps, [365, 366])
    npt.assert_array_equal(by_year.days.sum(axis=0), everything.days[0])
    by_season = mhw_days_by(g, th, se, classes="season", _compute=dbo.class_days_cells)
    npt.assert_array_equal(by_season.klass, [0, 1, 2, 3])
    npt.assert_array_equal(by_season.isum_q.sum(axis=0), everything.isum_q[0])


def _point(oisst, th, se):
    ts, sek, thk, _ = _ocean(oisst, th, se)
    p = GridSeries(ts[:, 0], ("time",), {"time": oisst["time64"]})
    return (p, GridSeries(thk[:, 0], ("doy",), {"doy": th.coords["doy"]}),
            GridSeries(sek[:, 0], ("doy",), {"doy": se.coords["doy"]}))


def test_point_series_and_cold_spells(oisst):
    th, se = clims(oisst)
    p, thp, sep = _point(oisst, th, se)
    ds = mhw_days_by(p, thp, sep, classes="season", _compute=dbo.class_days_cells)
    assert ds.days.shape == (4, 5) and ds.n_valid.shape == (4,) and ds.intensity_mean.shape == (4,) and ds.sdims == ()
    mhw = _detect(p, thp, sep, oracle_detect_cells)
    assert ds.days[:, 4].sum() == mhw.table[:, mhw.columns.index("duration")].sum() > 0
    g = grid(oisst)
    thc, sec = clims(oisst, coldSpells=True)
    cold = mhw_days_by(g, thc, sec, classes="all", coldSpells=True, _compute=dbo.class_days_cells)
    mhwc = _detect(g, thc, sec, oracle_detect_cells, coldSpells=True)
    assert cold.days[0, 4].sum() == mhwc.table[:, mhwc.columns.index("duration")].sum() > 0
    assert np.nanmax(cold.intensity_max) > 0                 # the device's sign: positive for a cold spell too


def _events(T, spans):
    table = np.zeros((len(spans), len(EventDataset.columns)))
    for i, (s, e) in enumerate(spans):
        table[i, EventDataset.columns.index("index_start")] = s
        table[i, EventDataset.columns.index("index_end")] = e
    time = np.datetime64("2000-01-01") + np.arange(T).astype("timedelta64[D]")
    return EventDataset(table, np.array([0, len(spans)]), time, np.array([0]), np.array([True]), (), (), {}, {}, {}, {}, True)


def test_classes_from_events():
    warm, cold = _events(30, [(2, 6), (15, 20)]), _events(30, [(5, 9), (28, 29)])
    got = classes_from_events(30, warm, cold)
    want = np.zeros(30, dtype=int)
    want[2:7] = 1
    want[15:21] = 1
    want[5:10] = 2                                          # the later dataset wins on steps 5 and 6
    want[28:30] = 2
    npt.assert_array_equal(got, want)
    assert got.dtype == np.int32
    npt.assert_array_equal(classes_from_events(30), np.zeros(30))
    gridded = _events(30, [(1, 2)])
    gridded.point = False
    for bad in ((gridded,), (_events(31, [(1, 2)]),), ("warm",)):
        with pytest.raises(XmhwException):
            classes_from_events(30, *bad)


def test_classes_from_events_with_detect(oisst):
    th, se = clims(oisst)
    p, thp, sep = _point(oisst, th, se)
    mhw = _detect(p, thp, sep, oracle_detect_cells)
    lab = classes_from_events(731, mhw)
    assert lab.sum() == mhw.table[:, mhw.columns.index("duration")].sum() > 0
    ds = mhw_days_by(grid(oisst), th, se, classes=lab, _compute=dbo.class_days_cells)
    npt.assert_array_equal(ds.klass, [0, 1])


def test_to_xarray(oisst):
    pytest.importorskip("xarray")
    ds = mhw_days_by(grid(oisst), *clims(oisst), classes="season", _compute=dbo.class_days_cells)
    x = ds.to_xarray()
    assert x["days"].dims == ("klass", "category", "lat", "lon") and x["frequency"].dims == ("klass", "lat", "lon")
    npt.assert_array_equal(x["intensity_mean"].values, ds.intensity_mean)
    npt.assert_array_equal(x["klass"].values, [0, 1, 2, 3])


def test_argument_errors(oisst):
    g = grid(oisst)
    th, se = clims(oisst)
    T = oisst["sst"].shape[0]
    run = lambda **kw: mhw_days_by(g, th, se, _compute=dbo.class_days_cells, **kw)      # noqa: E731
    for bad in ("week", np.zeros(T), np.zeros(T - 1, dtype=int), np.zeros((T, 1), dtype=int)):
        with pytest.raises(XmhwException):
            run(classes=bad)
    # more distinct labels than the cap: refused before anything else is looked at
    long = GridSeries(np.zeros(MAX_CLASSES + 1), ("time",),
                      {"time": np.datetime64("2000-01-01") + np.arange(MAX_CLASSES + 1).astype("timedelta64[D]")})
    with pytest.raises(XmhwException, match=f"at most {MAX_CLASSES} classes"):
        mhw_days_by(long, th, se, classes=np.arange(MAX_CLASSES + 1), _compute=dbo.class_days_cells)
    with pytest.raises(XmhwException):                       # xmhw.py:373-378
        run(minDuration=3, maxGap=3)
    with pytest.raises(XmhwException):
        run(tdim="t")
    # a named form needs a datetime64 axis
    plain = GridSeries(oisst["sst"], ("time", "lat", "lon"), {"time": np.arange(T), "lat": oisst["lat"], "lon": oisst["lon"]})
    for name in ("month", "season", "year"):
        with pytest.raises(XmhwException, match="integer array"):
            mhw_days_by(plain, th, se, classes=name, _compute=dbo.class_days_cells)
    # a series in kelvin against a climatology in degrees Celsius: every step is in an event and out of range
    hot = GridSeries(oisst["sst"] + 300.0, g.dims, g.coords, time_encoding={"calendar": "proleptic_gregorian"})
    with pytest.raises(XmhwException, match="kelvin"):
        mhw_days_by(hot, th, se, _compute=dbo.class_days_cells)


def test_stage_argument_errors():
    from xmhw_amd.days_by import _check_classes
    for cls, K in ((np.zeros(5, dtype=int), 0), (np.zeros(5, dtype=int), MAX_CLASSES + 1), (np.array([0, 1, 2, 3, 4]), 4),
                   (np.array([0, -2, 0, 0, 0]), 1), (np.zeros(4, dtype=int), 1), (np.zeros(5), 1)):
        with pytest.raises(XmhwException):
            _check_classes(5, cls, K)
    got, K = _check_classes(5, np.array([0, -1, 2, 2, 1]), 3)
    assert got.dtype == np.int32 and K == 3


@pytest.mark.parametrize("lead", [(3,), (2, 3, 4)])
def test_cells_to_grid_against_a_loop(lead):
    """(..., C) per-cell values back on a 4 x 5 grid whose line 2 and column 3 hold no ocean cell: leading shapes of rank 1
    and 3, against a plain loop over the cells"""
    from xmhw_amd.series_stage import cells_to_grid, grid_frame
    sshape, sdims = (4, 5), ("lat", "lon")
    keep = np.random.default_rng(1).random(20) < 0.7
    keep.reshape(sshape)[2, :] = False
    keep.reshape(sshape)[:, 3] = False
    keep[0] = True
    cell_index = np.nonzero(keep)[0]
    coords = {"lat": np.arange(4) * 10.0, "lon": np.arange(5) * 2.0, "time": np.arange(3)}
    alive, out_coords, keep_grid = grid_frame(keep, sdims, sshape, coords)
    rows, cols = [i for i in range(4) if keep.reshape(sshape)[i].any()], [j for j in range(5) if keep.reshape(sshape)[:, j].any()]
    assert 2 not in rows and 3 not in cols
    npt.assert_array_equal(out_coords["lat"], coords["lat"][rows])
    npt.assert_array_equal(out_coords["lon"], coords["lon"][cols])
    npt.assert_array_equal(keep_grid, keep.reshape(sshape)[np.ix_(rows, cols)])
    a = np.random.default_rng(2).integers(1, 1000, lead + (cell_index.shape[0],))
    for fill, dtype in ((0, np.int32), (np.nan, np.float64)):
        got = cells_to_grid(a, cell_index, 20, sshape, alive, fill, dtype)
        want = np.full(lead + (len(rows), len(cols)), fill, dtype=dtype)
        for k, c in enumerate(cell_index):
            want[..., rows.index(c // 5), cols.index(c % 5)] = a[..., k]
        assert got.dtype == dtype and got.flags.c_contiguous
        npt.assert_array_equal(got, want)
