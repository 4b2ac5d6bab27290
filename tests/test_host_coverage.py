"""mhw_coverage() without a GPU: the oracle (tests/coverage_oracle.py) pinned to reference-produced numbers, the
host layer (weights, regions, land mask, exceptions) with the oracle as the device stage, and the generators
of the GPU cases checked for events."""
import math

import numpy as np
import numpy.testing as npt
import pytest

import coverage_cases as cc
import coverage_oracle as co
from detect_standin import oracle_detect_cells
from test_host_detect import clims, grid
from xmhw_amd import CoverageDataset, GridSeries, XmhwException, mhw_coverage
from xmhw_amd.coverage import CATEGORIES, WEIGHT_ONE, quantise_weights
from xmhw_amd.detect import _detect


def test_oracle_reproduces_the_reference_duration_columns():
    """Per event of the 108 reference series, the sums of cells[:, 0, k] over index_start..index_end are the
    reference's duration_moderate / _strong / _severe / _extreme / duration, exactly."""
    nev = gap_days = 0
    seen_gap_day = False
    for ts, se, th, (m, jg, gap), table, cols in cc.golden_series():
        T = ts.shape[0]
        cells, area = co.coverage_cells(ts[:, None], se[:, None], th[:, None], np.arange(T), np.arange(T), [3], [0], 1,
                                        m, jg, gap)
        assert cells.shape == (T, 1, 5) and cells.dtype == np.int64
        npt.assert_array_equal(area, 3 * cells)
        for row in table:
            s, e = int(row[cols.index("index_start")]), int(row[cols.index("index_end")])
            got = cells[s:e + 1, 0].sum(axis=0)
            want = [row[cols.index(c)] for c in ("duration_moderate", "duration_strong", "duration_severe",
                                                 "duration_extreme", "duration")]
            npt.assert_array_equal(got, np.asarray(want, dtype=np.int64))
            nev += 1
        four = cells[:, 0, :4].sum(axis=1)
        assert (cells[:, 0, 4] >= four).all()
        gap_days += int((cells[:, 0, 4] - four).sum())
        seen_gap_day |= bool((cells[:, 0, 4] > four).any())
        assert cells[:, 0, 4].sum() == table[:, cols.index("duration")].sum()
    assert nev == 1795 and gap_days == 582 and seen_gap_day


def test_fast_oracle_equals_the_loop_oracle():
    d = cc.synthetic(150, 40, np.float32, seed=3, nan_frac=0.02)
    reg, wq = cc.scattered_regions(40, 3), cc.weights_q(40)
    a = co.coverage_cells(d["ts"], d["seas"], d["thresh"], d["doy"], d["doys"], wq, reg, 3)
    b = co.coverage_fast(d["ts"], d["seas"], d["thresh"], d["doy"], d["doys"], wq, reg, 3)
    npt.assert_array_equal(a[0], b[0])
    npt.assert_array_equal(a[1], b[1])
    assert a[0][..., 4].sum() > 0 and (a[0][..., :4].sum(axis=(0, 1)) > 0).all()


@pytest.mark.parametrize("kw", [dict(), dict(cold=True), dict(nan_frac=0.03), dict(dtype=np.float64)])
def test_generators_contain_events(kw):
    cold = kw.get("cold", False)
    d = cc.synthetic(200, 65, seed=11, **{"dtype": np.float32, **kw})
    cells, _ = co.coverage_fast(d["ts"], d["seas"], d["thresh"], d["doy"], d["doys"], np.ones(65, np.int64),
                                np.zeros(65, np.int32), 1, coldSpells=cold)
    assert cells[..., 4].sum() > 0
    assert (cells[..., 4] > cells[..., :4].sum(axis=-1)).any() or not kw      # joined gaps exist in the noisy cases


def test_quantise_weights():
    wq, unit = quantise_weights([0.0, 0.5, 2.0])
    npt.assert_array_equal(wq, [0, 1 << 29, 1 << 31])
    assert unit == 2.0 / WEIGHT_ONE
    for bad in ([-1.0, 1.0], [np.nan, 1.0], [np.inf, 1.0], [0.0, 0.0], []):
        with pytest.raises(XmhwException):
            quantise_weights(bad)


def _regions(oisst):
    reg = np.full((8, 4), 5, dtype=np.int64)          # (lat, lon): two regions and an excluded band
    reg[4:] = 2
    reg[3] = -1
    return reg


def test_grid_two_regions_coslat(oisst):
    g = grid(oisst)
    th, se = clims(oisst)
    reg = _regions(oisst)
    cov = mhw_coverage(g, th, se, weights="coslat", regions=reg, _compute=co.coverage_cells)
    assert isinstance(cov, CoverageDataset)
    T = oisst["sst"].shape[0]
    stacked = oisst["sst"].reshape(T, -1)
    keep = ~np.isnan(stacked).all(axis=0)
    assert keep.sum() == 12
    lab = reg.reshape(-1)
    ocean_labels = np.unique(lab[keep & (lab >= 0)])
    npt.assert_array_equal(cov.region, ocean_labels)
    assert cov.cells.shape == (T, len(ocean_labels), 5) == cov.area_q.shape == cov.fraction.shape
    assert cov.cells.dtype == np.int64 and cov.area_q.dtype == np.int64 and cov.category == CATEGORIES
    npt.assert_array_equal(cov.ncells, [np.sum(keep & (lab == r)) for r in ocean_labels])
    # against detect()'s own per-step columns (oracle device stage), reduced in numpy; float weights with fsum
    from xmhw_amd import calendar as cal
    thc, sec = th.values.reshape(th.values.shape[0], -1), se.values.reshape(se.values.shape[0], -1)
    thk, sek = thc[:, ~np.isnan(thc).all(axis=0)], sec[:, ~np.isnan(sec).all(axis=0)]
    inter = oracle_detect_cells(stacked[:, keep], sek, thk, cal.add_doy(oisst["time64"]), th.coords["doy"],
                                intermediate=True)["inter"]
    w = np.repeat(np.cos(np.deg2rad(oisst["lat"].astype(np.float64))), 4)
    ev, cats = np.zeros((T, 32), dtype=bool), np.full((T, 32), np.nan)      # back on the whole grid
    ev[:, keep] = ~np.isnan(inter["events"])
    cats[:, keep] = inter["cats"]
    states = [cats == 1, cats == 2, cats == 3, cats >= 4, ev]
    bound = cov.quantisation_bound()
    assert (bound < 1e-7).all()
    assert (cov.cells[..., 4].sum(axis=0) > 0).all()          # both regions see events
    for j, r in enumerate(ocean_labels):
        members = np.nonzero(keep & (lab == r))[0]
        total = math.fsum(w[members])
        npt.assert_array_equal(cov.total_q[j], quantise_weights(w)[0][members].sum())
        for k, st in enumerate(states):
            npt.assert_array_equal(cov.cells[:, j, k], st[:, members].sum(axis=1))
            for t in range(T):
                exact = math.fsum(w[c] for c in members if st[t, c]) / total
                assert abs(cov.fraction[t, j, k] - exact) <= bound[j]
    assert (cov.cells[..., 4] >= cov.cells[..., :4].sum(axis=-1)).all()
    npt.assert_allclose(cov.area_q * cov.weight_unit, cov.fraction * (cov.total_q * cov.weight_unit)[None, :, None])
    # land and excluded cells count nowhere: all-ocean totals
    assert cov.ncells.sum() == np.sum(keep & (lab >= 0)) < 12


def test_to_xarray(oisst):
    pytest.importorskip("xarray")
    cov = mhw_coverage(grid(oisst), *clims(oisst), _compute=co.coverage_cells)
    ds = cov.to_xarray()
    assert ds["cells"].dims == ("time", "region", "category") and ds.attrs["weight_unit"] == cov.weight_unit
    npt.assert_array_equal(ds["fraction"].values, cov.fraction)


def test_defaults_one_region_uniform_weights(oisst):
    g = grid(oisst)
    th, se = clims(oisst)
    cov = mhw_coverage(g, th, se, _compute=co.coverage_cells)
    npt.assert_array_equal(cov.region, [0])
    npt.assert_array_equal(cov.ncells, [12])
    npt.assert_array_equal(cov.total_q, [12 << 31])
    npt.assert_array_equal(cov.area_q, cov.cells << 31)
    npt.assert_array_equal(cov.fraction, cov.cells / 12)
    mhw = _detect(g, th, se, oracle_detect_cells)
    assert cov.cells[..., 4].sum() == mhw.table[:, mhw.columns.index("duration")].sum() > 0
    # a weight array on the grid; zero weight on a whole region -> NaN fraction
    w = np.ones((8, 4))
    w[4:] = 0
    cov2 = mhw_coverage(g, th, se, weights=w, regions=_regions(oisst), _compute=co.coverage_cells)
    j = list(cov2.region).index(2)
    assert cov2.total_q[j] == 0 and np.isnan(cov2.fraction[:, j]).all() and not np.isnan(cov2.fraction[:, 1 - j]).any()
    npt.assert_array_equal(cov2.cells[:, 1 - j], mhw_coverage(g, th, se, regions=_regions(oisst),
                                                              _compute=co.coverage_cells).cells[:, 1 - j])


def test_argument_errors(oisst):
    g = grid(oisst)
    th, se = clims(oisst)
    run = lambda **kw: mhw_coverage(g, th, se, _compute=co.coverage_cells, **kw)      # noqa: E731
    for w in (-np.ones((8, 4)), np.full((8, 4), np.nan), np.zeros((8, 4)), np.ones((4, 8)), np.ones(32), "area"):
        with pytest.raises(XmhwException):
            run(weights=w)
    for r in (np.zeros((4, 8), dtype=int), np.zeros(32, dtype=int), np.zeros((8, 4))):
        with pytest.raises(XmhwException):
            run(regions=r)
    with pytest.raises(XmhwException):                       # xmhw.py:373-378
        run(minDuration=3, maxGap=3)
    with pytest.raises(XmhwException):                       # detect()'s own checks come along
        run(tdim="t")
    with pytest.raises(XmhwException):
        mhw_coverage(GridSeries(oisst["sst"], ("time", "a", "b"), {"time": oisst["time64"], "a": oisst["lat"],
                                                                   "b": oisst["lon"]}), th, se, weights="coslat",
                     _compute=co.coverage_cells)


def test_point_series_and_cold_spells(oisst):
    th, se = clims(oisst)
    T = oisst["sst"].shape[0]
    stacked = oisst["sst"].reshape(T, -1)
    thc, sec = th.values.reshape(th.values.shape[0], -1), se.values.reshape(se.values.shape[0], -1)
    # ocean cells of the series and of the climatologies pair up by position (threshold() drops all-land lines)
    c = int(np.nonzero(~np.isnan(stacked).all(axis=0))[0][0])
    i = int(np.nonzero(~np.isnan(thc).all(axis=0))[0][0])
    p = GridSeries(stacked[:, c], ("time",), {"time": oisst["time64"]})
    thp = GridSeries(thc[:, i], ("doy",), {"doy": th.coords["doy"]})
    sep = GridSeries(sec[:, i], ("doy",), {"doy": se.coords["doy"]})
    cov = mhw_coverage(p, thp, sep, _compute=co.coverage_cells)
    assert cov.cells.shape == (oisst["sst"].shape[0], 1, 5) and cov.ncells[0] == 1
    mhw = _detect(p, thp, sep, oracle_detect_cells)
    assert cov.cells[..., 4].sum() == mhw.table[:, mhw.columns.index("duration")].sum() > 0
    # cold spells on the grid, against detect()
    g = grid(oisst)
    thc_, sec_ = clims(oisst, coldSpells=True)
    cold = mhw_coverage(g, thc_, sec_, coldSpells=True, _compute=co.coverage_cells)
    mhwc = _detect(g, thc_, sec_, oracle_detect_cells, coldSpells=True)
    assert cold.cells[..., 4].sum() == mhwc.table[:, mhwc.columns.index("duration")].sum() > 0
    assert not np.array_equal(cold.cells, mhw_coverage(g, *clims(oisst), _compute=co.coverage_cells).cells)


def test_dense_ids():
    from xmhw_amd.series_stage import dense_ids
    # labels with gaps, negative labels count nowhere
    labels = np.array([7, -3, 2, 7, 100, -1, 2], dtype=np.int64)
    found, ids, K = dense_ids(labels, 3, "mhw_coverage", "regions")
    npt.assert_array_equal(found, [2, 7, 100])
    npt.assert_array_equal(ids, [1, -1, 0, 1, 2, -1, 0])
    assert ids.dtype == np.int32 and K == 3                   # the cap exactly met
    with pytest.raises(XmhwException, match="mhw_coverage handles at most 2 regions, got 3"):
        dense_ids(labels, 2, "mhw_coverage", "regions")       # ... and exceeded by one
    with pytest.raises(XmhwException, match="mhw_days_by handles at most 2 classes, got 3"):
        dense_ids(labels, 2, "mhw_days_by", "classes")
    # no non-negative label: nothing found, every id -1, one (empty) class
    found, ids, K = dense_ids(np.array([-1, -5, -1], dtype=np.int64), 1, "x", "regions")
    assert found.shape == (0,) and K == 1
    npt.assert_array_equal(ids, [-1, -1, -1])
    found, ids, K = dense_ids(np.zeros(0, dtype=np.int64), 1, "x", "regions")
    assert found.shape == (0,) and ids.shape == (0,) and K == 1


def test_regions_of_result():
    from xmhw_amd.series_stage import dense_ids, regions_of_result
    labels = np.array([5, 5, 9, 9, 2, -1, 2, 40], dtype=np.int64)
    keep = np.array([True, False, False, False, True, True, True, True])     # region 9 has only land cells
    w = np.array([3, 1000, 1000, 1000, 4, 1000, 0, 1 << 31], dtype=np.int64)
    found, rid, Rc = dense_ids(labels, 1024, "x", "regions")
    sel, ncells, total, region = regions_of_result(keep, rid, w, found)
    npt.assert_array_equal(found, [2, 5, 9, 40])
    npt.assert_array_equal(sel, [True, True, False, True])
    npt.assert_array_equal(region, [2, 5, 40])
    npt.assert_array_equal(ncells, [2, 1, 1])
    npt.assert_array_equal(total, [4, 3, 1 << 31])
    assert ncells.dtype == np.int64 and total.dtype == np.int64 and Rc == 4
    # a plain loop gives the same
    for j, r in enumerate(region):
        mine = [i for i in range(8) if keep[i] and labels[i] == r]
        assert ncells[j] == len(mine) and total[j] == sum(int(w[i]) for i in mine)
    # every cell excluded: one empty region 0, nothing to select
    found, rid, Rc = dense_ids(np.full(8, -1, dtype=np.int64), 1024, "x", "regions")
    sel, ncells, total, region = regions_of_result(keep, rid, w, found)
    assert sel is None and Rc == 1
    npt.assert_array_equal(region, [0])
    npt.assert_array_equal(ncells, [0])
    npt.assert_array_equal(total, [0])
