"""region_series() without a GPU: the host layer (weights, regions, land mask, bit budget, exceptions, the derived
fields) with the numpy oracle (tests/region_series_oracle.py) as the device stage."""
import math

import numpy as np
import numpy.testing as npt
import pytest

import region_series_cases as rc
import region_series_oracle as ro
from test_host_detect import clims, grid, oracle_clim
from xmhw_amd import GridSeries, RegionSeriesDataset, XmhwException, mhw_coverage, region_series
from xmhw_amd.region_series import FIELDS, MAX_REGIONS, RANGE_BITS, SERIES_BITS, weight_bits


def stage(ts, wi, region, R, offset=0.0):
    """the stand-in for region_cells()"""
    return ro.region_cells(ts, wi, region, R, offset)


def _regions():
    reg = np.full((8, 4), 5, dtype=np.int64)          # (lat, lon): two regions and an excluded band
    reg[4:] = 2
    reg[3] = -1
    return reg


def _big_grid(nlat=40, nlon=30, T=20):
    rng = np.random.default_rng(4)
    time = np.datetime64("2001-01-01") + np.arange(T).astype("timedelta64[D]")
    return GridSeries(rng.normal(15.0, 2.0, size=(T, nlat, nlon)), ("time", "lat", "lon"),
                      {"time": time, "lat": np.linspace(-60, 60, nlat), "lon": np.arange(nlon, dtype=np.float64)})


def _raised(fn):
    with pytest.raises(XmhwException) as e:
        fn()
    return type(e.value), str(e.value).replace("mhw_coverage", "CALL").replace("region_series", "CALL")


def test_argument_errors_are_those_of_mhw_coverage(oisst):
    g = grid(oisst)
    th, se = clims(oisst)
    bad = [dict(tdim="t"), dict(regions=np.zeros((8, 4))), dict(regions=np.zeros((8, 4), dtype=np.float32)),
           dict(weights=-np.ones((8, 4))), dict(weights=np.zeros((8, 4))), dict(weights=np.full((8, 4), np.nan)),
           dict(weights=np.full((8, 4), np.inf)), dict(weights=np.ones((4, 8))), dict(weights=np.ones(32)),
           dict(regions=np.zeros((4, 8), dtype=int)), dict(regions=np.zeros(32, dtype=int)), dict(weights="area")]
    for kw in bad:
        want = _raised(lambda: mhw_coverage(g, th, se, _compute=None, **kw))     # raised before any device work
        assert _raised(lambda: region_series(g, _compute=stage, **kw)) == want, kw
    # more than 1024 regions (both calls check the labels before they look at anything else)
    big = _big_grid()
    labels = np.arange(40 * 30).reshape(40, 30)
    assert labels.max() + 1 > MAX_REGIONS == 1024
    want = _raised(lambda: mhw_coverage(big, None, None, regions=labels))
    assert _raised(lambda: region_series(big, regions=labels, _compute=stage)) == want
    assert "at most 1024 regions" in want[1]
    region_series(big, regions=labels % MAX_REGIONS, _compute=stage)            # 1024 labels are taken
    with pytest.raises(XmhwException):
        region_series(g, offset=np.inf, _compute=stage)
    with pytest.raises(XmhwException):                                           # weights="coslat" without a latitude
        region_series(GridSeries(oisst["sst"], ("time", "a", "b"), {"time": oisst["time64"], "a": oisst["lat"],
                                                                    "b": oisst["lon"]}), weights="coslat", _compute=stage)


def test_labels_of_the_result(oisst):
    g = grid(oisst)
    reg = _regions()
    rs = region_series(g, regions=reg, _compute=stage)
    assert isinstance(rs, RegionSeriesDataset)
    T = oisst["sst"].shape[0]
    keep = ~np.isnan(oisst["sst"].reshape(T, -1)).all(axis=0)
    lab = reg.reshape(-1)
    want = np.unique(lab[keep & (lab >= 0)])
    npt.assert_array_equal(rs.region, want)                    # sorted, non-negative, found on ocean cells
    npt.assert_array_equal(rs.ncells, [np.sum(keep & (lab == r)) for r in want])
    assert rs.ncells.sum() == np.sum(keep & (lab >= 0)) < 12   # land and excluded cells count nowhere
    for k in FIELDS:
        assert getattr(rs, k).shape == (T, len(want)) and getattr(rs, k).dtype == np.int64
    # a label that lies on land only does not appear; sparse labels keep their values
    reg2 = np.where(keep.reshape(8, 4), 700, 9)
    npt.assert_array_equal(region_series(g, regions=reg2, _compute=stage).region, [700])
    # without regions: one region 0; every cell excluded: one empty region
    one = region_series(g, _compute=stage)
    npt.assert_array_equal(one.region, [0])
    npt.assert_array_equal(one.ncells, [12])
    npt.assert_array_equal(one.total_i, [12 << 31])
    npt.assert_array_equal(one.wsum_i, one.n_valid << 31)
    none = region_series(g, regions=np.full((8, 4), -1), _compute=stage)
    assert none.ncells.tolist() == [0] and np.isnan(none.mean).all() and (none.n_valid == 0).all()


@pytest.mark.parametrize("n_ocean,want", [(1, 31), (1 << 6, 31), ((1 << 7) - 1, 31), (1 << 7, 30), (1 << 20, 17)])
def test_weight_bits(n_ocean, want):
    ib = weight_bits(n_ocean)
    assert ib == want == min(31, 61 - SERIES_BITS - RANGE_BITS - int(n_ocean).bit_length())
    assert n_ocean * 2 ** (ib + SERIES_BITS + RANGE_BITS) < 2 ** 61       # |xsum_q| <= C * 2**(ib + 23)


def test_weight_bits_refuses_a_grid_without_room():
    with pytest.raises(XmhwException):
        weight_bits(1 << 36)
    with pytest.raises(XmhwException):
        weight_bits(1 << 40)


def test_weight_bits_follow_the_ocean_cells_of_the_grid():
    """150 ocean cells of 1200 grid points: ib = 30 (bit_length(150) = 8), not the 27 of the whole grid."""
    big = _big_grid()
    v = big.values.copy()
    v[:, 5:] = np.nan
    g = GridSeries(v, big.dims, big.coords)
    rs = region_series(g, weights="coslat", _compute=stage)
    assert rs.ncells.tolist() == [150] and rs.weight_bits == 30
    w = np.cos(np.deg2rad(big.coords["lat"]))
    assert rs.weight_unit == w.max() / 2 ** 30


def test_mean_against_fsum_within_the_bound(oisst):
    g = grid(oisst)
    reg = _regions()
    rs = region_series(g, weights="coslat", regions=reg, _compute=stage)
    T = oisst["sst"].shape[0]
    stacked = oisst["sst"].reshape(T, -1)
    keep = ~np.isnan(stacked).all(axis=0)
    assert keep.sum() == 12 and (~keep).sum() == 20            # a grid with land
    lab = reg.reshape(-1)
    w = np.repeat(np.cos(np.deg2rad(oisst["lat"].astype(np.float64))), 4)
    bound = rs.quantisation_bound()
    assert bound.shape == (T, 2) and (bound < 2.0 ** -16).all()
    npt.assert_array_equal(bound, 2.0 ** -17 + rs.n_valid * 2.0 ** 7 / rs.wsum_i + 2.0 ** -44)
    worst = 0.0
    for j, r in enumerate(rs.region):
        members = np.nonzero(keep & (lab == r))[0]
        for t in range(T):
            x = stacked[t, members].astype(np.float64)
            ok = ~np.isnan(x)
            exact = math.fsum(w[members][ok] * x[ok]) / math.fsum(w[members][ok])
            err = abs(rs.mean[t, j] - exact)
            assert err <= bound[t, j]
            worst = max(worst, err)
        assert rs.n_valid[:, j].max() == members.shape[0]
    assert 0 < worst                                           # the fixed point is not exact: the bound is used
    npt.assert_array_equal(rs.valid_fraction, rs.wsum_i / rs.total_i[None, :])
    # an offset moves the integers, not the mean beyond the bound
    rk = region_series(GridSeries(oisst["sst"].astype(np.float64) + 273.15, g.dims, g.coords), weights="coslat", regions=reg,
                       offset=273.15, _compute=stage)
    assert rk.offset == 273.15 and np.abs(rk.mean - 273.15 - rs.mean).max() < 2.0 ** -15


def test_series_min_fraction(oisst):
    sst = oisst["sst"].astype(np.float64).copy()
    T = sst.shape[0]
    ocean = np.argwhere(~np.isnan(sst).all(axis=0))
    (a, b), (c, d) = ocean[0], ocean[1]
    sst[3, a, b] = np.nan                                      # one cell missing on step 3, all on step 5
    sst[5] = np.nan
    g = GridSeries(sst, ("time", "lat", "lon"), {"time": oisst["time64"], "lat": oisst["lat"], "lon": oisst["lon"]},
                   attrs={"units": "degC"}, time_encoding={"calendar": "proleptic_gregorian"})
    rs = region_series(g, _compute=stage)
    assert rs.valid_fraction[3, 0] == 11 / 12 and rs.valid_fraction[5, 0] == 0 and np.isnan(rs.mean[5, 0])
    s = rs.series()
    assert isinstance(s, GridSeries) and s.dims == ("time", "region") and s.values.shape == (T, 1)
    npt.assert_array_equal(s.values, rs.mean)
    npt.assert_array_equal(s.coords["region"], rs.region)
    npt.assert_array_equal(s.coords["time"], oisst["time64"])
    assert s.time_encoding == {"calendar": "proleptic_gregorian"} and s.attrs == {"units": "degC"}
    strict = rs.series(min_fraction=0.95).values
    assert np.isnan(strict[3, 0]) and np.isnan(strict[5, 0]) and np.isnan(strict).sum() == 2
    npt.assert_array_equal(rs.series(min_fraction=11 / 12).values[3], rs.mean[3])
    with pytest.raises(XmhwException):
        rs.series(min_fraction=1.5)
    # the series goes into threshold() and detect() as it is (oracle device stages)
    from detect_standin import oracle_detect_cells
    from xmhw_amd.api import _threshold
    from xmhw_amd.detect import _detect, climatology_series
    full = region_series(grid(oisst), regions=_regions(), _compute=stage).series()
    clim = _threshold(full, oracle_clim)
    mhw = _detect(full, climatology_series(clim, "thresh"), climatology_series(clim, "seas"), oracle_detect_cells)
    assert mhw.offsets.shape == (3,) and mhw.n_events > 0


def test_out_of_range_samples_raise(oisst):
    g = grid(oisst)
    kelvin = GridSeries(oisst["sst"].astype(np.float64) + 273.15, g.dims, g.coords)
    n = int((~np.isnan(oisst["sst"])).sum())                   # every sample of an ocean cell is 273 and more from 0
    with pytest.raises(XmhwException, match=rf"^{n} samples .*offset=273\.15") as e:
        region_series(kelvin, _compute=stage)
    assert "kelvin" in str(e.value) and n > 0
    sst = oisst["sst"].astype(np.float64).copy()
    ocean = np.argwhere(~np.isnan(sst).all(axis=0))[0]
    sst[7, ocean[0], ocean[1]] = np.inf
    with pytest.raises(XmhwException, match=r"^1 samples"):
        region_series(GridSeries(sst, g.dims, g.coords), _compute=stage)
    region_series(kelvin, offset=273.15, _compute=stage)


def test_point_series(oisst):
    T = oisst["sst"].shape[0]
    stacked = oisst["sst"].reshape(T, -1)
    c = int(np.nonzero(~np.isnan(stacked).all(axis=0))[0][0])
    p = GridSeries(stacked[:, c], ("time",), {"time": oisst["time64"]})
    rs = region_series(p, _compute=stage)
    assert rs.mean.shape == (T, 1) and rs.ncells.tolist() == [1] and rs.weight_bits == 31
    npt.assert_array_equal(rs.xsum_q[:, 0], np.rint(stacked[:, c].astype(np.float64) * 65536.0).astype(np.int64) << 31)
    assert np.abs(rs.mean[:, 0] - stacked[:, c]).max() <= 2.0 ** -17
    assert rs.series().values.shape == (T, 1)


def test_to_xarray(oisst):
    xr = pytest.importorskip("xarray")
    g = grid(oisst)
    rs = region_series(g, weights="coslat", regions=_regions(), _compute=stage)
    ds = rs.to_xarray()
    assert ds["mean"].dims == ("time", "region") and ds.attrs["weight_bits"] == 31 and ds.attrs["offset"] == 0.0
    npt.assert_array_equal(ds["xsum_q"].values, rs.xsum_q)
    npt.assert_array_equal(ds["region"].values, rs.region)
    npt.assert_array_equal(ds["ncells"].values, rs.ncells)
    # a DataArray goes in as well
    da = xr.DataArray(oisst["sst"], dims=("time", "lat", "lon"), coords={"time": oisst["time64"], "lat": oisst["lat"],
                                                                         "lon": oisst["lon"]}, attrs={"units": "degC"})
    rx = region_series(da, weights="coslat", regions=_regions(), _compute=stage)
    npt.assert_array_equal(rx.xsum_q, rs.xsum_q)
    assert rx.series().attrs == {"units": "degC"}


def test_case_generators_reach_every_path():
    seen = set()
    for C in (1, 63, 64, 65, 255, 257, 3001):
        assert rc.paths_of(rc.uniform_waves(C)) == {"A"}
        for k in (2, 3, 4):
            seen |= rc.paths_of(rc.few_per_wave(C, k, 7))
        seen |= rc.paths_of(rc.many_per_wave(C, 7))
    assert seen == {"A", "B", "C"}
    assert rc.paths_of(np.full(200, -1)) == set()
