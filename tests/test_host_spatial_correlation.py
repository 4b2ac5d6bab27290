"""The host logic of spatial_correlation() without a device: the exports, the refusals of the C entries in their stated
order (they come before the first HIP call), the validation of offsets and reach, the half-plane split and the mirror fill
around the numpy stand-in of the device stage against the oracle run on the full offset list, the derived fields of
SpatialCorrelationDataset on integers made by hand against closed forms, the e-folding length on a constructed r(d), and
the refusal of a result that does not fit."""
import importlib
import math

import numpy as np
import numpy.testing as npt
import pytest

import spatial_correlation_cases as sc
import spatial_correlation_oracle as so
import xmhw_amd
from xmhw_amd import GridSeries, spatial_correlation
from xmhw_amd.exception import XmhwException

sm = importlib.import_module("xmhw_amd.spatial_correlation")    # (the package attribute of that name is the function)

NY, NX, T = 5, 7, 70
TIME = np.datetime64("2001-01-01") + np.arange(T).astype("timedelta64[D]")
LAT, LON = -10.0 + 0.5 * np.arange(NY), 100.0 + 0.25 * np.arange(NX)
COORDS = {"time": TIME, "lat": LAT, "lon": LON}
STAGE = so.spatial_corr_grid
FIELDS = so.FIELDS
ONE = 1 << 16


def grid_series(land="island", seed=3, dtype=np.float32, spoil=False, scale=1.0):
    ts, base, rows, sea = sc.field(T, NY, NX, dtype, seed, land=land, spoil=spoil)
    x = (ts.astype(np.float64) * scale).astype(dtype)
    return GridSeries(x.reshape(T, NY, NX), ("time", "lat", "lon"), COORDS), base.reshape(NY, NX) * scale, sea


def test_exports():
    assert "spatial_correlation" in xmhw_amd.__all__ and "SpatialCorrelationDataset" in xmhw_amd.__all__
    assert xmhw_amd.spatial_correlation is sm.spatial_correlation
    assert xmhw_amd.SpatialCorrelationDataset is sm.SpatialCorrelationDataset


def test_c_entry_refusals_in_their_stated_order_need_no_device():
    core = importlib.import_module("xmhw_amd._xmhw_hip")
    m = importlib.import_module("xmhw_amd._xmhw_hip_spatialcorr")
    assert not any(hasattr(m, n) for n in ("HipError", "Unsupported", "InvalidArgument", "CommError"))
    Tn = 10
    z = np.zeros(Tn, np.int32)
    near = np.array([[0, 0], [0, 1], [1, 0]], np.int32)

    def acc(ld=12, t0=0, nt=Tn, T=Tn, ny=3, nx=4, periodic=0, ldb=12, Dr=1, rows=z, shift=0, classes=z, K=1, offsets=near,
            ldo=12, itemsize=4):
        m.spatial_corr_accumulate(0, itemsize, ld, t0, nt, T, ny, nx, periodic, 0, ldb, Dr, rows, shift, classes, K, offsets,
                                  0, 0, 0, 0, 0, 0, ldo, 0)

    def init(K=1, D=3, ny=3, nx=4, ldo=12):
        m.spatial_corr_init(K, D, ny, nx, 0, 0, 0, 0, 0, 0, ldo, 0)

    long = 1 << 17
    longz = np.zeros(long, np.int32)
    many = np.zeros((65, 2), np.int32)
    wide = dict(nx=32768, ld=3 * 32768, ldb=3 * 32768, ldo=3 * 32768)
    unsupported = [lambda: acc(K=0), lambda: acc(K=65), lambda: acc(offsets=many), lambda: acc(offsets=np.zeros((0, 2), np.int32)),
                   lambda: acc(shift=25), lambda: acc(shift=-1), lambda: acc(T=long, rows=longz, classes=longz),
                   lambda: acc(**wide), lambda: acc(ny=32768, ld=1 << 20, ldb=1 << 20, ldo=1 << 20),
                   lambda: acc(offsets=np.array([[33, 0]], np.int32)), lambda: acc(offsets=np.array([[0, 0], [0, -33]], np.int32)),
                   lambda: init(K=0), lambda: init(K=65), lambda: init(D=0), lambda: init(D=65), lambda: init(nx=32768, ldo=1 << 20)]
    for call in unsupported:
        with pytest.raises(core.Unsupported) as e:
            call()
        assert type(e.value) is core.Unsupported and isinstance(e.value, core.HipError) and "(code 3)" in str(e.value)
    # K is judged before D, D before the shift, the shift before T, T before an axis, an axis before the reach -- and
    # every cap before anything that is merely invalid
    far = np.array([[40, 0]], np.int32)
    with pytest.raises(core.Unsupported, match="K must be in"):
        acc(K=0, offsets=many, shift=30)
    with pytest.raises(core.Unsupported, match="D must be in"):
        acc(offsets=many, shift=30)
    with pytest.raises(core.Unsupported, match="shift must be in"):
        acc(shift=30, T=long, rows=longz, classes=longz)
    with pytest.raises(core.Unsupported, match="2\\^17 steps"):
        acc(T=long, rows=longz, classes=longz, **wide)
    with pytest.raises(core.Unsupported, match="2\\^15 points"):
        acc(offsets=far, **wide)
    with pytest.raises(core.Unsupported, match="reach at most 32"):
        acc(offsets=far, ld=3)
    invalid = [(lambda: acc(ny=-1), "bad ny/nx"), (lambda: acc(nx=-1), "bad ny/nx"),
               (lambda: acc(t0=-1), "bad T/t0/nt"), (lambda: acc(nt=-1), "bad T/t0/nt"), (lambda: acc(t0=4, nt=7), "bad T/t0/nt"),
               (lambda: acc(ld=11), "bad ld/ldb/ldo/Dr"), (lambda: acc(ldb=11), "bad ld/ldb/ldo/Dr"),
               (lambda: acc(ldo=11), "bad ld/ldb/ldo/Dr"), (lambda: acc(Dr=0), "bad ld/ldb/ldo/Dr"),
               (lambda: acc(periodic=1, offsets=np.array([[0, 4]], np.int32)), r"\|di\| must be below nx"),
               (lambda: acc(periodic=1, offsets=np.array([[0, 0], [1, -4]], np.int32)), r"\|di\| must be below nx"),
               (lambda: acc(classes=np.full(Tn, 1, np.int32)), r"class_of_t outside \[-1, K\)"),
               (lambda: acc(classes=np.full(Tn, -2, np.int32)), r"class_of_t outside"),
               (lambda: acc(rows=np.full(Tn, 1, np.int32)), r"row_of_t outside \[0, D\)"),
               (lambda: acc(rows=np.zeros(Tn + 1, np.int32)), "row_of_t length"),
               (lambda: acc(classes=np.zeros(Tn - 1, np.int32)), "class_of_t length"),
               (lambda: acc(offsets=np.zeros((3, 3), np.int32)), r"offsets must be \(D, 2\)"), (lambda: acc(itemsize=2), "itemsize"),
               (lambda: acc(), "NULL buffer"), (lambda: init(ldo=11), "bad ny/nx/ldo"), (lambda: init(ny=-1), "bad ny/nx/ldo"),
               (lambda: init(), "NULL"), (lambda: m.set_spatial_corr_block(-1), "steps must be"),
               (lambda: m.set_spatial_corr_tile(5), "rows must be")]
    for call, text in invalid:
        with pytest.raises(core.InvalidArgument, match=text) as e:
            call()
        assert type(e.value) is core.InvalidArgument
    # without a seam |di| >= nx is no error: the partner is off the grid
    with pytest.raises(core.InvalidArgument, match="NULL buffer"):
        acc(offsets=np.array([[0, 4]], np.int32))
    # a bad dimension is judged before the periodic rule, the periodic rule before a bad label, a label before a row, and
    # all of them before a NULL buffer
    seam = np.array([[0, 5]], np.int32)
    with pytest.raises(core.InvalidArgument, match="bad ld/ldb/ldo/Dr"):
        acc(ld=11, periodic=1, offsets=seam)
    with pytest.raises(core.InvalidArgument, match="must be below nx"):
        acc(periodic=1, offsets=seam, classes=np.full(Tn, 5, np.int32))
    with pytest.raises(core.InvalidArgument, match="class_of_t outside"):
        acc(classes=np.full(Tn, 5, np.int32), rows=np.full(Tn, 5, np.int32))
    # the caps themselves are taken; nothing is launched for nt == 0 or ny * nx == 0: no device is needed either
    cap = np.array([[32, -32], [-32, 32]] * 32, np.int32)
    acc(K=64, offsets=cap, shift=24, nt=0)
    acc(ny=0, ld=0, ldb=0, ldo=0)
    acc(nx=0, ld=0, ldb=0, ldo=0, periodic=1)
    acc(ny=32767, nx=32767, ld=32767 * 32767, ldb=32767 * 32767, ldo=32767 * 32767, nt=0)
    acc(T=long - 1, rows=longz[:-1], classes=longz[:-1], t0=long - 1, nt=0)
    acc(T=0, nt=0, rows=z[:0], classes=z[:0])
    m.set_spatial_corr_block(0)
    m.set_spatial_corr_tile(8)
    m.set_spatial_corr_tile(0)
    assert (m.SPATIAL_CORR_MAX_OFFSETS, m.SPATIAL_CORR_REACH, m.SPATIAL_CORR_MAX_CLASSES, m.SPATIAL_CORR_MAX_STEPS,
            m.SPATIAL_CORR_MAX_AXIS, m.SPATIAL_CORR_BITS, m.SPATIAL_CORR_RANGE_BITS, m.SPATIAL_CORR_MAX_SHIFT) == \
        (64, 32, 64, 1 << 17, 32767, 16, 7, 24)
    assert (sm.MAX_OFFSETS, sm.REACH, sm.MAX_CLASSES, sm.MAX_AXIS, sm.BITS, sm.RANGE_BITS, sm.MAX_SHIFT) == \
        (64, 32, 64, 32767, 16, 7, 24)


def test_offsets_and_reach():
    x, _, _ = grid_series()
    bad = [(dict(offsets=[(0, 33)]), "at most 32 grid points either way"), (dict(offsets=[(-33, 0)]), "at most 32"),
           (dict(offsets=[]), "pairs of whole numbers"), (dict(offsets=[(0.5, 1.0)]), "whole numbers"),
           (dict(offsets=[(1, 2, 3)]), "pairs"), (dict(offsets=5), "pairs"),
           (dict(offsets=[(0, 1)] * 65), "1 to 64 offsets"), (dict(offsets=[(0, 1)], reach=(1, 1)), "offsets or reach, not both"),
           (dict(reach=(33, 1)), r"reach should be in \[0, 32\]"), (dict(reach=(1, -1)), r"reach should be in"),
           (dict(reach=4), "a pair"), (dict(reach=(1.5, 2)), "whole numbers"),
           (dict(offsets=[(0, 7)], periodic="lon"), r"\|di\| < 7"), (dict(periodic="lat"), "name of the longitude dim"),
           (dict(shift=25), r"shift should be in \[0, 24\]"), (dict(shift=1.5), "whole number"),
           (dict(classes=np.arange(T) % 65), "at most 64 classes"),
           (dict(offsets=[(a, b) for a in range(1, 9) for b in range(-4, 5)][:64]), "more than 64")]
    for kw, text in bad:
        with pytest.raises(XmhwException, match=text):
            spatial_correlation(x, _compute=STAGE, **kw)
    with pytest.raises(XmhwException, match="has no neighbours"):
        spatial_correlation(GridSeries(np.zeros(T, np.float32), ("time",), {"time": TIME}), _compute=STAGE)
    with pytest.raises(XmhwException, match="fast axis"):
        spatial_correlation(GridSeries(np.zeros((T, NX, NY), np.float32), ("time", "a_lon", "lat"),
                                       {"time": TIME, "a_lon": LON, "lat": LAT}), lon="a_lon", _compute=STAGE)
    # the cross: (0, 0) and 1, 2, 3, 4, 6, 8, 12, 16, 24, 32 up to the reach either way on each axis, ascending
    npt.assert_array_equal(sm.cross_offsets((2, 3)), [(-2, 0), (-1, 0), (0, -3), (0, -2), (0, -1), (0, 0), (0, 1), (0, 2), (0, 3),
                                                      (1, 0), (2, 0)])
    assert sm.cross_offsets((0, 0)).tolist() == [[0, 0]]
    assert sm.cross_offsets((8, 8)).shape == (25, 2) and sm.cross_offsets((32, 32)).shape == (41, 2)
    assert sorted({abs(int(v)) for v in sm.cross_offsets((32, 5))[:, 0]}) == [0, 1, 2, 3, 4, 6, 8, 12, 16, 24, 32]
    assert sorted({abs(int(v)) for v in sm.cross_offsets((32, 5))[:, 1]}) == [0, 1, 2, 3, 4]
    # the default is the cross of reach (8, 8); 7 columns and no seam: the partners at +-8 are off the grid, n = 0
    ds = spatial_correlation(x, _compute=STAGE)
    npt.assert_array_equal(ds.offset, sm.cross_offsets((8, 8)))
    assert ds.n.shape == (1, 25, NY, NX) and (ds.n[:, ds._at(0, 8)] == 0).all() and (ds.n[:, ds._at(0, 1)] > 0).any()
    # the half-plane: (0, 0) first, every offset once whatever its sign and however often it is asked for
    dev, index, mirrored = sm.half_plane([(0, -1), (1, -2), (-1, 2), (0, 1), (0, 0), (0, 1), (3, 0)])
    assert dev.tolist() == [[0, 0], [0, 1], [1, -2], [3, 0]] and dev.dtype == np.int32
    assert index.tolist() == [1, 2, 2, 1, 0, 1, 3] and mirrored.tolist() == [True, False, True, False, False, False, False]
    seen = {}

    def spy(field, base, rows, classes, K, offsets, ny, nx, **kw):
        seen.update(offsets=offsets.tolist(), kw=kw)
        return STAGE(field, base, rows, classes, K, offsets, ny, nx, **kw)

    spatial_correlation(x, offsets=[(0, -1), (-2, 1), (2, -1), (0, 1)], periodic="lon", shift=2, _compute=spy)
    assert seen["offsets"] == [[0, 0], [0, 1], [2, -1]] and seen["kw"] == dict(periodic=True, shift=2)


@pytest.mark.parametrize("periodic", [None, "lon"])
@pytest.mark.parametrize("land", ["island", "lines", "none"])
def test_mirror_fill_equals_the_oracle_on_the_full_offset_list(periodic, land):
    """the device sees (0, 0) and the half-plane; what comes back for -e is the oracle's own answer for -e"""
    x, base, sea = grid_series(land=land, seed=9, dtype=np.float64)
    request = [(0, 0), (0, 1), (0, -1), (1, 0), (-1, 0), (2, 3), (-2, -3), (-2, 3), (2, -3), (4, 0), (-4, 0), (0, 6), (0, -6),
               (0, 1), (-1, -1), (5, 0), (0, -2)]
    if periodic is None:
        request += [(0, 7), (0, -7), (-5, 6), (32, -32)]                  # partners off the grid: n = 0
    classes, K = sc.every_step(T)
    got = spatial_correlation(x, base=base, offsets=request, classes=classes, periodic=periodic, _compute=STAGE)
    ts = np.asarray(x.values).reshape(T, NY * NX)
    b = np.where(sea, base.reshape(-1), np.nan)[None]
    want = so.spatial_corr_sums(ts, b, np.zeros(T, np.int32), 0, classes, K, request, NY, NX, periodic is not None)
    assert want["n"].sum() > 0 and all((want[k] != 0).any() for k in FIELDS)
    for k in FIELDS:
        a = getattr(got, k)
        assert a.dtype == (np.int32 if k == "n" else np.int64) and a.shape == (K, len(request), NY, NX)
        npt.assert_array_equal(a.reshape(K, len(request), NY * NX), want[k], err_msg=k)
    npt.assert_array_equal(got.offset, request)
    npt.assert_array_equal(got.keep, sea.reshape(NY, NX))
    assert np.isnan(got.r[..., ~got.keep]).all() and (got.n[..., ~got.keep] == 0).all()
    # one point of it pair by pair in Python integers: the oracle itself
    j, i = NY - 1, NX - 1
    slow = so.spatial_corr_point(ts, b, np.zeros(T, np.int32), 0, classes, K, request, NY, NX, periodic is not None, j, i)
    for k in FIELDS:
        assert getattr(got, k)[:, :, j, i].tolist() == slow[k], k


def test_a_doy_base_and_named_classes_reach_the_stage_as_rows_and_ids():
    x, _, sea = grid_series(seed=4)
    rng = np.random.default_rng(0)
    clim = np.round(rng.random((366, NY, NX)), 2)
    seen = {}

    def spy(field, base, rows, classes, K, offsets, ny, nx, **kw):
        seen.update(base=base, rows=rows, classes=classes, K=K)
        return STAGE(field, base, rows, classes, K, offsets, ny, nx, **kw)

    ds = spatial_correlation(x, base=GridSeries(clim, ("doy", "lat", "lon"), dict(COORDS, doy=np.arange(1, 367))),
                             classes="month", reach=(1, 1), _compute=spy)
    assert seen["base"].shape == (366, NY * NX) and seen["K"] == 3 and ds.klass.tolist() == [1, 2, 3]
    # 1 Jan .. 28 Feb 2001 are doy 1 .. 59; 1 Mar is doy 61 in the 366-slot calendar: the row of 29 Feb is skipped
    npt.assert_array_equal(seen["rows"], np.r_[np.arange(59), np.arange(60, 71)])
    npt.assert_array_equal(seen["base"][:, sea], clim.reshape(366, -1)[:, sea])
    assert np.isnan(seen["base"][:, ~sea]).all()
    npt.assert_array_equal(seen["classes"], (TIME.astype("datetime64[M]").astype(int) % 12).astype(np.int32))


def _dataset(n, sx, sy, sxx, syy, sxy, offsets, lat, dlon, nx, shift=0, periodic=False):
    ny = len(lat)
    full = lambda v, dt: np.broadcast_to(np.asarray(v, dtype=dt).reshape(1, -1, 1, 1), (1, len(offsets), ny, nx)).copy()   # noqa: E731
    return sm.SpatialCorrelationDataset(np.zeros(1, np.int64), offsets, full(n, np.int32), full(sx, np.int64), full(sy, np.int64),
                                        full(sxx, np.int64), full(syy, np.int64), full(sxy, np.int64), np.ones((ny, nx), bool),
                                        ("lat", "lon"), {"lat": np.asarray(lat), "lon": dlon * np.arange(nx)}, lat, dlon,
                                        shift, periodic)


def test_derived_fields_on_integers_made_by_hand():
    """pairs (x, y) in units of 2**-16 with shift 3: closed forms in float64, a handful of flops: 1e-12 relative"""
    xs, ys = np.array([3, -1, 4, 1, -5, 9]) * ONE, np.array([2, 7, -1, 8, 2, 8]) * ONE
    n = len(xs)
    sums = (n, int(xs.sum()), int(ys.sum()), int((xs * xs).sum()), int((ys * ys).sum()), int((xs * ys).sum()))
    flat = (4, 8 * ONE, 12 * ONE, 16 * ONE * ONE, 40 * ONE * ONE, 24 * ONE * ONE)          # x is 2, 2, 2, 2: no spread
    one = (1, ONE, ONE, ONE * ONE, ONE * ONE, ONE * ONE)
    none = (0, 0, 0, 0, 0, 0)
    table = list(zip(sums, flat, one, none))
    ds = _dataset(*table, offsets=[(0, 1), (0, 2), (1, 0), (2, 0)], lat=[0.0, 1.0, 2.0], dlon=1.0, nx=4, shift=3)
    x, y = xs / ONE * 8.0, ys / ONE * 8.0                                 # original units: 2**shift
    cov = (x * y).mean() - x.mean() * y.mean()
    want_r = cov / math.sqrt(((x * x).mean() - x.mean() ** 2) * ((y * y).mean() - y.mean() ** 2))
    npt.assert_allclose(ds.mean_x[0, 0], x.mean(), rtol=1e-12)
    npt.assert_allclose(ds.mean_y[0, 0], y.mean(), rtol=1e-12)
    npt.assert_allclose(ds.cov[0, 0], cov, rtol=1e-12)
    npt.assert_allclose(ds.r[0, 0], want_r, rtol=1e-12)
    npt.assert_allclose(ds.r[0, 0], np.corrcoef(x, y)[0, 1], rtol=1e-12)
    npt.assert_allclose(ds.slope[0, 0], cov / ((y * y).mean() - y.mean() ** 2), rtol=1e-12)
    # no spread in x: means and covariance exist, r and slope do not; one pair or none: nothing does
    npt.assert_allclose(ds.mean_x[0, 1], 16.0, rtol=1e-12)
    npt.assert_allclose(ds.cov[0, 1], 0.0, atol=1e-12)
    assert np.isnan(ds.r[0, 1]).all() and np.isnan(ds.slope[0, 1]).all()
    for e in (2, 3):
        assert all(np.isnan(getattr(ds, k)[0, e]).all() for k in ("mean_x", "mean_y", "cov", "r", "slope"))
    # the bound on r: the half unit of a sample, and a finite bound far below the correlation itself here
    qb = ds.quantisation_bound()
    assert qb["unit"] == 2.0 ** (3 - 17) and qb["r"].shape == ds.r.shape
    assert (qb["r"][0, 0] > 0).all() and (qb["r"][0, 0] < 1e-4).all() and np.isnan(qb["r"][0, 1:]).all()
    # ... and where the spread is a unit or two it says so: infinite
    tiny = _dataset([4], [2], [2], [2], [2], [0], offsets=[(0, 1)], lat=[0.0], dlon=1.0, nx=2)
    assert np.isinf(tiny.quantisation_bound()["r"]).all() and not np.isnan(tiny.r).any()


def test_to_xarray():
    xr = pytest.importorskip("xarray")
    ds = _dataset(*([5, 0],) * 6, offsets=[(0, 1), (2, 0)], lat=[0.0, 1.0, 2.0], dlon=1.0, nx=4, shift=3)
    out = ds.to_xarray()
    assert isinstance(out, xr.Dataset) and out["r"].dims == ("klass", "offset", "lat", "lon") and out.attrs["shift"] == 3
    npt.assert_array_equal(out["dj"], [0, 2])
    assert out["distance_km"].dims == ("offset", "lat")


def test_distances_and_the_efolding_length_on_a_constructed_correlation():
    R = 6371.0
    lat, dlon, nx = [0.0, 0.5, 1.0, 1.5], 0.25, 6
    offsets = [(0, 0), (0, 1), (0, -1), (0, 2), (0, -2), (0, 4), (0, -4), (1, 0), (-1, 0), (2, 0), (-2, 0)]
    ds = _dataset(*([0] * len(offsets),) * 6, offsets=offsets, lat=lat, dlon=dlon, nx=nx)
    d = ds.distance_km()
    assert d.shape == (len(offsets), 4) and (d[0] == 0.0).all()
    # on the equator a zonal step is an arc of the equator, whole metres; a meridional step is an arc of the meridian
    for e, s in ((1, 1), (2, 1), (3, 2), (5, 4)):
        npt.assert_allclose(d[e, 0], np.rint(1000.0 * R * math.radians(s * dlon)) / 1000.0, rtol=1e-12)
        assert d[e, 3] < d[e, 0]                                          # ... and shorter away from it
    npt.assert_allclose(d[7, :3], np.rint(1000.0 * R * math.radians(0.5)) / 1000.0, rtol=1e-12)
    npt.assert_allclose(d[9, :2], np.rint(1000.0 * R * math.radians(1.0)) / 1000.0, rtol=1e-12)
    assert np.isnan(d[7, 3]) and np.isnan(d[8, 0]) and np.isnan(d[9, 2:]).all() and np.isnan(d[10, :2]).all()
    # r(d) by construction, zonal: column 0 reached between steps 1 and 2; 1 between 2 and 4; 2 at the first step;
    # 3 not reached; 4 a NaN gap at step 2 and a crossing at step 4: the step before it has no correlation; 5: -e alone
    e1 = math.exp(-1.0)
    r = np.full((1, len(offsets), 4, nx), np.nan)
    for col, (r1, r2, r4) in enumerate([(0.8, 0.2, 0.1), (0.9, 0.5, 0.3), (0.1, 0.9, 0.9), (0.9, 0.8, 0.7), (0.9, np.nan, 0.1),
                                        (0.6, 0.3, 0.0)]):
        for e, v in ((1, r1), (3, r2), (5, r4)):
            r[0, e, :, col] = v + 0.05                                    # +e and -e differ: their mean is what counts
            r[0, e + 1, :, col] = v - 0.05
    r[0, [1, 3, 5], :, 5] = np.nan                                        # column 5 has the western partner alone
    ds.r = r
    L = ds.efolding_length("zonal")
    assert L.shape == (1, 4, nx)
    for j in range(4):
        d1, d2, d4 = d[1, j], d[3, j], d[5, j]
        npt.assert_allclose(L[0, j, 0], d1 + (0.8 - e1) / (0.8 - 0.2) * (d2 - d1), rtol=1e-12)
        npt.assert_allclose(L[0, j, 1], d2 + (0.5 - e1) / (0.5 - 0.3) * (d4 - d2), rtol=1e-12)
        npt.assert_allclose(L[0, j, 2], (1.0 - e1) / (1.0 - 0.1) * d1, rtol=1e-12)
        npt.assert_allclose(L[0, j, 5], d1 + (0.55 - e1) / (0.55 - 0.25) * (d2 - d1), rtol=1e-12)
    assert np.isnan(L[0, :, 3]).all() and np.isnan(L[0, :, 4]).all()
    # meridional: rows 0 and 3 have one neighbour at distance 1 and the other off the grid; crossing between 1 and 2
    r[:] = np.nan
    r[0, 7], r[0, 8], r[0, 9], r[0, 10] = 0.7, 0.5, 0.1, 0.3
    r[0, 7, 3], r[0, 8, 0], r[0, 9, 2:], r[0, 10, :2] = np.nan, np.nan, np.nan, np.nan   # what the grid cannot give
    ds.r = r
    M = ds.efolding_length("meridional")
    step1, step2 = d[7, 0], d[9, 0]
    npt.assert_allclose(M[0, 0], step1 + (0.7 - e1) / (0.7 - 0.1) * (step2 - step1), rtol=1e-12)     # +1 and +2 alone
    npt.assert_allclose(M[0, 1], step1 + (0.6 - e1) / (0.6 - 0.1) * (step2 - step1), rtol=1e-12)     # +-1, +2
    npt.assert_allclose(M[0, 2], step1 + (0.6 - e1) / (0.6 - 0.3) * (step2 - step1), rtol=1e-12)     # +-1, -2
    npt.assert_allclose(M[0, 3], step1 + (0.5 - e1) / (0.5 - 0.3) * (step2 - step1), rtol=1e-12)     # -1 and -2 alone
    ds.r = np.where(np.isnan(r), np.nan, 0.9)
    assert np.isnan(ds.efolding_length("meridional")).all() and np.isnan(ds.anisotropy()).all()
    with pytest.raises(XmhwException, match="one of"):
        ds.efolding_length("diagonal")
    with pytest.raises(XmhwException, match="no zonal offset"):
        _dataset(*([0],) * 6, offsets=[(1, 0)], lat=lat, dlon=dlon, nx=nx).efolding_length("zonal")


def test_a_result_that_does_not_fit_and_samples_out_of_range_are_refused():
    x, _, _ = grid_series()
    called = []
    with pytest.raises(XmhwException, match=r"K = 1 classes x 13 offsets x 35 grid points take 20020 bytes, more than "
                                            r"max_result_bytes = 20019"):
        spatial_correlation(x, max_result_bytes=20019, _compute=lambda *a, **k: called.append(1))
    assert not called
    spatial_correlation(x, max_result_bytes=20020, _compute=STAGE)
    # the device stage says the same before it allocates, and refuses what is out of range in the words of the pattern
    with pytest.raises(XmhwException, match="more than max_result_bytes = 10"):
        sm.spatial_corr_grid(np.zeros((3, 6), np.float32), np.zeros((1, 6)), np.zeros(3, np.int32), np.zeros(3, np.int32), 1,
                             [(0, 0)], 2, 3, max_result_bytes=10)
    texts = sm._range_texts(2)
    assert list(texts) == ["n_range"] and "2**(7 + shift)" in texts["n_range"] and "shift = 2: pass a larger shift" in texts["n_range"]
    for bad, text in (((3, 7), r"should be \(T, 6\)"), ((0, 6), "no time step")):
        with pytest.raises(XmhwException, match=text):
            sm.spatial_corr_grid(np.zeros(bad, np.float32), np.zeros((1, 6)), np.zeros(bad[0], np.int32),
                                 np.zeros(bad[0], np.int32), 1, [(0, 0)], 2, 3)
