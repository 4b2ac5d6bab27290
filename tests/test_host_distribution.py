"""The host logic of anomaly_distribution() without a device: the exports, every refusal and its message, the bins rule and
the nearest admissible hi, levels off an edge, the result-bytes check, the oracle itself on a case worked by hand, the whole
public path around the numpy stand-in of the device stage, the derived fields of DistributionDataset on integers worked by
hand and against exact rational arithmetic, the quantile NaN rules, the stated quantisation bounds on the oracle alone, and
to_xarray()."""
import importlib
from fractions import Fraction

import numpy as np
import numpy.testing as npt
import pytest

import distribution_cases as dc
import distribution_oracle as do
import xmhw_amd
from xmhw_amd import GridSeries, anomaly_distribution
from xmhw_amd.exception import XmhwException

dm = importlib.import_module("xmhw_amd.distribution")

NY, NX, T = 3, 4, 400
TIME = np.datetime64("2001-01-01") + np.arange(T).astype("timedelta64[D]")
COORDS = {"time": TIME, "lat": np.arange(NY) * 0.25, "lon": np.arange(NX) * 0.25}
LAND = np.zeros((NY, NX), bool)
LAND[0, 1] = LAND[2, 2] = True
ONE = 1 << 16
STAGE = do.distribution_cells


def field(seed=1, dtype=np.float32, scale=1.0):
    """a skewed persistent series on the grid, NaN on LAND and on 3 % of the samples"""
    rng = np.random.default_rng(seed)
    e = rng.gamma(2.0, 0.6, (T, NY, NX)) - 1.2
    a = np.zeros_like(e)
    for t in range(1, T):
        a[t] = 0.6 * a[t - 1] + e[t]
    x = np.round(scale * a, 3).astype(dtype)
    x[rng.random(x.shape) < 0.03] = np.nan
    x[:, LAND] = np.nan
    return GridSeries(x, ("time", "lat", "lon"), COORDS)


def test_exports_and_limits():
    assert "anomaly_distribution" in xmhw_amd.__all__ and "DistributionDataset" in xmhw_amd.__all__
    assert xmhw_amd.anomaly_distribution is dm.anomaly_distribution and xmhw_amd.DistributionDataset is dm.DistributionDataset
    assert (dm.MAX_BINS, dm.MAX_CLASSES, dm.MAX_QUANTILES, dm.MAX_LEVELS, dm.MAX_STEPS) == (256, 64, 16, 8, 1 << 17)
    assert (dm.FIELDS, dm.NO_SAMPLE) == (do.FIELDS, do.NO_SAMPLE)


def test_every_refusal_and_its_message():
    x = field()
    bad = [(dict(bins=(-8.0, 8.0, 257)), "at most 256 bins, got 257"), (dict(bins=(-8.0, 8.0, 0)), "n a whole number of bins >= 1"),
           (dict(bins=(-8.0, 8.0, 2.5)), "n a whole number of bins"), (dict(bins=(-8.0, 8.0)), r"bins should be \(lo, hi, n\)"),
           (dict(bins=(3.0, 3.0, 4)), "-128 <= lo < hi <= 128"), (dict(bins=(-200.0, 8.0, 4)), "-128 <= lo < hi <= 128"),
           (dict(bins=(0.0, 1.0, 3)), r"65536 units over 3 bins\): the nearest admissible hi is 0.9999847412109375"),
           (dict(bins=(0.0, 2.0 ** -16, 2)), r"1 units over 2 bins\): the nearest admissible hi is 3.0517578125e-05"),
           (dict(levels=(0.3,)), r"level 0.3 is not on a bin edge: the neighbouring edges are 0.25 and 0.375"),
           (dict(levels=(9.0,)), r"level 9.0 is not on a bin edge: the neighbouring edges are 7.875 and 8.0"),
           (dict(levels=(-8.5,)), r"the neighbouring edges are -8.0 and -7.875"),
           (dict(levels=(np.nan,)), "levels should be finite"), (dict(levels=np.zeros(9)), "at most 8 levels, got 9"),
           (dict(quantiles=(0.5, 1.5)), r"probabilities in \[0, 1\]"), (dict(quantiles=(-0.1,)), r"probabilities in \[0, 1\]"),
           (dict(quantiles=np.linspace(0, 1, 17)), "at most 16 quantiles, got 17"),
           (dict(shift=25), r"shift should be in \[0, 24\]"), (dict(shift=1.5), "shift should be a whole number"),
           (dict(classes=np.arange(T) % 65), "at most 64 classes"), (dict(classes=np.zeros(T - 1, int)), "one entry per time step"),
           (dict(max_result_bytes=1000), r"K = 1 classes x C = 10 cells with 128 bins take 6480 bytes \(the histogram 5200\)")]
    for kw, text in bad:
        with pytest.raises(XmhwException, match=text):
            anomaly_distribution(x, _compute=STAGE, **kw)
    # the caps themselves pass
    anomaly_distribution(x, bins=(-128.0, 128.0, 256), quantiles=np.linspace(0, 1, 16), levels=np.arange(8.0) - 4, shift=24,
                         max_result_bytes=dm.bytes_per_cell_entry(256, 16, 8) * 10, _compute=STAGE)
    long = 1 << 17
    with pytest.raises(XmhwException, match="fewer than 2\\*\\*17 time steps"):
        anomaly_distribution(GridSeries(np.zeros(long, np.float32), ("time",), {"time": np.arange(long)}), _compute=STAGE)
    # out of range: the text names the shift; a larger one passes
    big = GridSeries(np.asarray(x.values) * 100.0, x.dims, COORDS)
    with pytest.raises(XmhwException, match=r"samples lie 2\*\*\(7 \+ shift\) and more .* shift = 1: pass a larger shift"):
        anomaly_distribution(big, shift=1, _compute=STAGE)
    anomaly_distribution(big, shift=3, _compute=STAGE)


def test_bins_levels_and_quantiles_as_integers():
    assert dm.check_bins((-8.0, 8.0, 128)) == (-8 * ONE, 8192, 128)
    assert dm.check_bins((-0.1, 0.1, 2)) == (-6554, 6554, 2)               # the edges are rounded to the unit first
    assert dm.check_bins((0.0, 3 * 2.0 ** -16, 3)) == (0, 1, 3)            # bins of one unit
    level, edges = dm.check_levels((-8.0, 0.0, 8.0, 0.125), -8 * ONE, 8192, 128)
    assert edges.tolist() == [0, 64, 128, 65] and edges.dtype == np.int32 and level.tolist() == [-8.0, 0.0, 8.0, 0.125]
    p, p_q = dm.check_quantiles((0.0, 0.5, 1.0, 2.0 ** -32))
    assert p_q.tolist() == [0, 1 << 31, 1 << 32, 1] and p_q.dtype == np.uint64
    assert dm.check_quantiles(())[1].shape == (0,) and dm.check_levels((), 0, 1, 1)[1].shape == (0,)
    # the rank rule against Python integers
    n = np.array([[0, 1, 2, 3, 65535, 2 ** 31 - 1]], dtype=np.int32)
    for pq in (0, 1, 1 << 31, (1 << 32) - 1, 1 << 32):
        assert dm.ranks(np.array([pq], np.uint64), n)[0, 0].tolist() == [do.rank(pq, int(v)) for v in n[0]]


def test_oracle_on_a_case_worked_by_hand():
    """T = 8, one cell, bins of 1.0 from -1 to 2 (B = 3), classes 0 0 0 0 1 1 -1 0:
      d = -1.5 (UNDER), -1.0 (bin 0), 0.5 (bin 1), NaN, 2.0 (OVER), 1.99998 (bin 2), 300 (class -1: not counted), 200
      (out of range)"""
    x = np.array([[-1.5], [-1.0], [0.5], [np.nan], [2.0], [2.0 - 2.0 ** -16], [300.0], [200.0]])
    classes = np.array([0, 0, 0, 0, 1, 1, -1, 0])
    r = do.distribution_sums(x, np.zeros((1, 1)), np.zeros(8, int), 0, classes, 2, -ONE, ONE, 3, [0, 1 << 31, 1 << 32], [0, 1, 3])
    assert r["hist"][:, :, 0].tolist() == [[1, 1, 1, 0, 0], [0, 0, 0, 1, 1]] and r["n"][:, 0].tolist() == [3, 2]
    assert r["n_range"] == 1 and r["hist"].dtype == np.int32
    h = ONE // 2
    assert r["s1"][:, 0].tolist() == [-3 * h - ONE + h, 2 * ONE + 2 * ONE - 1]
    assert int(r["S3"][0, 0]) == (-3 * h) ** 3 - ONE ** 3 + h ** 3 and int(r["S4"][1, 0]) == (2 * ONE) ** 4 + (2 * ONE - 1) ** 4
    assert r["kmin"][:, 0].tolist() == [-1.5, 2.0 - 2.0 ** -16] and r["kmax"][:, 0].tolist() == [0.5, 2.0]
    # ranks 1, ceil(n / 2), n: class 0 -> rows UNDER, bin 0, bin 1; class 1 -> bin 2, bin 2, OVER
    assert r["qbin"][:, :, 0].tolist() == [[-1, 0, 1], [2, 2, 3]] and r["qbelow"][:, :, 0].tolist() == [[0, 1, 2], [0, 0, 1]]
    assert r["qcount"][:, :, 0].tolist() == [[1, 1, 1], [1, 1, 1]]
    assert r["n_at_least"][:, :, 0].tolist() == [[2, 1, 0], [2, 2, 1]]
    # the words of a negative and of a large sum
    w = do.words(np.array([[-1, 1 << 64, -(1 << 64) - 5]], dtype=object))
    assert w[0].tolist() == [[-1, 0, -5], [-1, 1, -2]]
    npt.assert_array_equal(dm.wide(w), np.array([[-1, 1 << 64, -(1 << 64) - 5]], dtype=object))
    # the cases hold what they say they hold
    lo_q, width_q, B = dc.bins_for(64)
    d = dc.series(300, 40, np.float32, 3, lo_q, width_q, B)
    q, valid, out = do.fixed(d["x"], d["base"], d["rows"], 0)
    rows = do.rows_of(q, lo_q, width_q, B)
    assert (rows[3, 8], rows[4, 8]) == (3, 2) and rows[5:9, 9].tolist() == [1, 0, B + 1, B]
    assert len(set(q[:, 10])) == 1 and valid[:, 10].all() and (rows[:, 11] == 0).all() and (rows[:, 12] == B + 1).all()
    assert not valid[:, 13].any() and not out[:, 13].any() and out[[1, 2, 9, 10], 14].all() and abs(q[20, 14]) > 1 << 22


def test_public_path_around_the_stand_in_equals_the_oracle():
    x = field(seed=5)
    keep = ~LAND.reshape(-1)
    C = int(keep.sum())
    labels = np.where(np.arange(T) % 50 < 45, (np.arange(T) // 100) % 2 * 10 + 3, -1)     # classes 3 and 13, gaps of -1
    kid = np.where(labels < 0, -1, (labels == 13).astype(int))
    base = np.stack([np.where(LAND, np.nan, 0.01 * j) for j in range(366)])                 # a 366-row base
    p, levels = (0.0, 0.1, 0.5, 0.9, 1.0), (-1.0, 0.5)
    got = anomaly_distribution(x, base=base, bins=(-4.0, 4.0, 64), quantiles=p, levels=levels, classes=labels, shift=1,
                               return_histogram=True, _compute=STAGE)
    assert got.klass.tolist() == [3, 13] and got.n.shape == (2, NY, NX) and got.s3.shape == (2, 2, NY, NX)
    assert got.n.dtype == np.int32 and got.s2.dtype == np.int64 and got.histogram.shape == (2, 66, NY, NX)
    from xmhw_amd import calendar as cal
    rows = cal.add_doy(TIME) - 1
    xs = np.asarray(x.values, dtype=np.float64).reshape(T, -1)[:, keep]
    bs = base.reshape(366, -1)[:, keep]
    want = do.distribution_sums(xs, bs, rows, 1, kid, 2, -4 * ONE, 8192, 64, [int(v) for v in dm.check_quantiles(p)[1]], [24, 36])
    assert want["n_range"] == 0 and want["n"].sum() > 3000
    for k, name in (("n", "n"), ("s1", "s1"), ("s2", "s2"), ("s3", "s3"), ("s4", "s4"), ("qbin", "quantile_bin"),
                    ("n_at_least", "exceedance"), ("hist", "histogram")):
        a = getattr(got, name)
        a = a.reshape(a.shape[:-2] + (-1,))
        npt.assert_array_equal(a[..., keep], want[k], err_msg=k)
        assert (a[..., ~keep] == (do.NO_SAMPLE if k == "qbin" else 0)).all()
    npt.assert_array_equal(got.keep, ~LAND)
    # the extremes in the units of the field (shift 1: twice the shifted anomaly), NaN on land
    npt.assert_array_equal(got.minimum.reshape(2, -1)[:, keep], want["kmin"] * 2.0)
    npt.assert_array_equal(got.maximum.reshape(2, -1)[:, keep], want["kmax"] * 2.0)
    assert np.isnan(got.mean[:, LAND]).all() and np.isnan(got.quantile[:, :, LAND]).all()
    assert got.bin_edges.shape == (65,) and got.bin_edges[0] == -8.0 and got.bin_edges[-1] == 8.0
    # the quantile lies in the bin of the exact order statistic; p = 0 and p = 1 are the bins of the extremes
    quant = got.quantile.reshape(2, len(p), -1)[..., keep]
    for k in range(2):
        for j, pq in enumerate(dm.check_quantiles(p)[1]):
            r = np.array([do.rank(int(pq), int(v)) for v in want["n"][k]])
            exact = want["sorted"][k][r - 1, np.arange(C)]
            b = (exact + 4 * ONE) // 8192
            inside = (b >= 0) & (b < 64)
            assert inside.sum() > 0 and np.isnan(quant[k, j][~inside]).all()
            edge = (-4 * ONE + b * 8192) / ONE * 2.0
            assert (edge <= quant[k, j])[inside].all() and (quant[k, j] < edge + 0.25)[inside].all()
    # the stated bounds hold on the oracle alone: numpy float64 on the unquantised anomalies
    bound = got.quantisation_bound()
    assert bound["unit"] == 2.0 ** -16 and bound["mean"] == 2.0 ** -16 and bound["quantile"] == 0.25 + 2.0 ** -16
    a = xs - bs[rows]
    for k in range(2):
        for c in range(C):
            v = a[kid == k, c]
            v = v[~np.isnan(v)]
            m = v.mean()
            m2, m3, m4 = ((v - m) ** 2).mean(), ((v - m) ** 3).mean(), ((v - m) ** 4).mean()
            ref = {"mean": m, "variance": m2, "skewness": m3 / m2 ** 1.5, "kurtosis": m4 / m2 ** 2 - 3.0, "minimum": v.min(),
                   "maximum": v.max()}
            for name, r in ref.items():
                value = getattr(got, name).reshape(2, -1)[:, keep][k, c]
                limit = bound[name] if np.isscalar(bound[name]) else bound[name].reshape(2, -1)[:, keep][k, c]
                slack = 0.0 if name in ("minimum", "maximum") else 1e-12 * max(abs(r), 1.0)     # numpy's own rounding
                assert np.isfinite(limit) and abs(value - r) <= limit + slack, (name, k, c, value, r, limit)
                assert name in ("minimum", "maximum") or limit < 1e-3                       # ... and they say something
    prob = got.exceedance_probability.reshape(2, 2, -1)[..., keep]
    npt.assert_allclose(prob, want["n_at_least"] / want["n"][:, None], rtol=1e-15)


def test_derived_fields_against_exact_rational_arithmetic():
    """one class, five cells of hand-made integers: q = 1, 2, 3, 10 (skewed); two equal samples (no spread); one sample;
    none; and the largest magnitudes, whose third and fourth power sums need both words"""
    cells = [[1, 2, 3, 10], [7, 7], [5], [], [(1 << 23)] * 1000 + [-(1 << 23) + 1] * 3]
    C = len(cells)
    n = np.array([[len(q) for q in cells]], np.int32)
    s1 = np.array([[sum(q) for q in cells]], np.int64)
    s2 = np.array([[sum(v * v for v in q) for q in cells]], np.int64)
    S3 = np.array([[sum(v ** 3 for v in q) for q in cells]], dtype=object)
    S4 = np.array([[sum(v ** 4 for v in q) for q in cells]], dtype=object)
    assert int(S3[0, 4]) >> 64 > 0 and int(S4[0, 4]) >> 64 > 0
    z = np.zeros((1, 0, C), np.int32)
    ext = np.array([[min(q) / ONE if q else np.nan for q in cells]]), np.array([[max(q) / ONE if q else np.nan for q in cells]])
    for shift in (0, 2):
        ds = dm.DistributionDataset([0], n, s1, s2, do.words(S3), do.words(S4), ext[0], ext[1], z, z, z, z, np.ones(C, bool),
                                    ("cell",), {}, (-ONE, ONE, 2), (), (), shift)
        unit = Fraction(2) ** (shift - 16)
        for c, q in enumerate(cells):
            if not q:
                assert all(np.isnan(getattr(ds, k)[0, c]) for k in ("mean", "variance", "skewness", "kurtosis", "minimum", "maximum"))
                continue
            N = len(q)
            m = Fraction(sum(q), N)
            m2, m3, m4 = (sum((v - m) ** p for v in q) / N for p in (2, 3, 4))
            assert ds.mean[0, c] == float(m * unit) and ds.variance[0, c] == pytest.approx(float(m2 * unit ** 2), rel=1e-15)
            assert ds.minimum[0, c] == float(min(q) * unit) and ds.maximum[0, c] == float(max(q) * unit)
            if N < 2 or m2 == 0:
                assert np.isnan(ds.skewness[0, c]) and np.isnan(ds.kurtosis[0, c])
            else:
                assert ds.skewness[0, c] == pytest.approx(float(m3) / float(m2) ** 1.5, rel=1e-14)
                assert ds.kurtosis[0, c] == pytest.approx(float(m4 / (m2 * m2)) - 3.0, rel=1e-14, abs=1e-14)
        assert ds.variance[0, 1] == 0.0 and ds.variance[0, 2] == 0.0
    # cancellation happens in integers: a mean of 2**23 - 1 with a spread of one unit keeps its moments
    q = [(1 << 23) - 2, (1 << 23) - 1, (1 << 23) - 1, (1 << 23)] * 100
    one = lambda v, dt: np.array([[v]], dt)                                                          # noqa: E731
    ds = dm.DistributionDataset([0], one(len(q), np.int32), one(sum(q), np.int64), one(sum(v * v for v in q), np.int64),
                                do.words(one(sum(v ** 3 for v in q), object)), do.words(one(sum(v ** 4 for v in q), object)),
                                one(0.0, float), one(0.0, float), z[:, :, :1], z[:, :, :1], z[:, :, :1], z[:, :, :1],
                                np.ones(1, bool), ("cell",), {}, (-ONE, ONE, 2), (), ())
    assert ds.variance[0, 0] == 0.5 * 2.0 ** -32 and ds.skewness[0, 0] == 0.0 and ds.kurtosis[0, 0] == -1.0


def test_quantile_rules_and_exceedance():
    """ranks in UNDER, in OVER and in an empty class give NaN; inside a bin the samples count as evenly spread"""
    n = np.array([[10, 10, 0]], np.int32)
    zero64 = np.zeros((1, 3), np.int64)
    zero128 = np.zeros((1, 2, 3), np.int64)
    qbin = np.array([[[-1, 2, do.NO_SAMPLE], [1, 4, do.NO_SAMPLE]]], np.int32)        # (K, P = 2, C = 3), B = 4
    qbelow = np.array([[[0, 3, 0], [4, 9, 0]]], np.int32)
    qcount = np.array([[[3, 5, 0], [6, 1, 0]]], np.int32)
    nal = np.array([[[7, 2, 0]]], np.int32)
    ext = np.full((1, 3), 0.0)
    ds = dm.DistributionDataset([0], n, zero64, zero64, zero128, zero128, ext, ext, qbin, qbelow, qcount, nal, np.ones(3, bool),
                                ("cell",), {}, (-2 * ONE, ONE, 4), (0.5, 1.0), (0.0,))
    # p = 0.5: rank 5 -> cell 1: bin 2 = [0, 1), 3 below, 5 inside: 0 + (5 - 3 - 0.5) / 5;  p = 1: rank 10 -> cell 0: bin 1,
    # 4 below, 6 inside: -1 + (10 - 4 - 0.5) / 6
    assert np.isnan(ds.quantile[0, 0, 0]) and ds.quantile[0, 0, 1] == pytest.approx(0.3, rel=1e-14) and np.isnan(ds.quantile[0, 0, 2])
    assert ds.quantile[0, 1, 0] == pytest.approx(-1.0 + 5.5 / 6, rel=1e-14) and np.isnan(ds.quantile[0, 1, 1]) and np.isnan(ds.quantile[0, 1, 2])
    assert ds.exceedance_probability[0, 0, :2].tolist() == [0.7, 0.2] and np.isnan(ds.exceedance_probability[0, 0, 2])
    assert ds.bin_edges.tolist() == [-2.0, -1.0, 0.0, 1.0, 2.0]
    bound = ds.quantisation_bound()
    assert bound["quantile"] == 1.0 + 2.0 ** -17 and np.isnan(bound["variance"][0, 2])
    assert np.isinf(bound["skewness"][0, 0])                                # no spread above the resolution: no bound


def test_to_xarray_on_the_stand_in():
    xr = pytest.importorskip("xarray")
    got = anomaly_distribution(field(seed=9), bins=(-4.0, 4.0, 32), levels=(1.0,), classes="month", return_histogram=True,
                               _compute=STAGE)
    ds = got.to_xarray()
    assert isinstance(ds, xr.Dataset) and ds["n"].dims == ("klass", "lat", "lon") and ds["s3"].dims == ("klass", "word", "lat", "lon")
    assert ds["quantile"].dims == ("klass", "quantile", "lat", "lon") and ds["quantile"].shape == (12, 5, NY, NX)
    assert ds["exceedance"].dims == ("klass", "level", "lat", "lon") and ds["histogram"].shape == (12, 34, NY, NX)
    assert ds["bin_edges"].shape == (33,) and ds.attrs["bins"] == 32 and ds.attrs["classes"] == "month"
    assert ds["klass"].values.tolist() == list(range(1, 13)) and ds["level"].values.tolist() == [1.0]
    npt.assert_array_equal(ds["skewness"].values, got.skewness)


def test_c_entry_refusals_need_no_device_and_raise_the_exceptions_of_the_core_module():
    core = importlib.import_module("xmhw_amd._xmhw_hip")
    m = importlib.import_module("xmhw_amd._xmhw_hip_distribution")
    assert not any(hasattr(m, n) for n in ("HipError", "Unsupported", "InvalidArgument", "CommError"))
    assert (m.DISTRIBUTION_MAX_BINS, m.DISTRIBUTION_MAX_CLASSES, m.DISTRIBUTION_MAX_QUANTILES, m.DISTRIBUTION_MAX_LEVELS,
            m.DISTRIBUTION_MAX_STEPS, m.DISTRIBUTION_BITS, m.DISTRIBUTION_RANGE_BITS, m.DISTRIBUTION_MAX_SHIFT) == (
        dm.MAX_BINS, dm.MAX_CLASSES, dm.MAX_QUANTILES, dm.MAX_LEVELS, dm.MAX_STEPS, dm.BITS, dm.RANGE_BITS, dm.MAX_SHIFT)
    Tn, long = 10, 1 << 17
    z = np.zeros(Tn, np.int32)
    buf = [8] * 8                                   # non-NULL "device" pointers: nothing below reaches a launch

    def acc(T=Tn, C=4, ld=4, ldb=4, Dr=1, rows=z, shift=0, classes=z, K=2, lo_q=0, width_q=1, B=4, ldo=4, ts=8, bufs=buf):
        m.distribution_accumulate(ts, 4, T, C, ld, 8, ldb, Dr, rows, shift, classes, K, lo_q, width_q, B, *bufs, ldo, 8)

    def fin(K=2, B=4, C=4, p_q=(), edge=(), ldo=4, hist=8):
        m.distribution_finish(K, B, C, hist, 8, 8, 8, np.asarray(p_q, np.uint64), np.asarray(edge, np.int32), 8, 8, 8, 8, ldo)

    zl = np.zeros(long, np.int32)
    unsupported = [(lambda: acc(K=0), "K must be in"), (lambda: acc(K=65), r"K must be in \[1, 64\]"),
                   (lambda: acc(B=0), "B must be in"), (lambda: acc(B=257), r"B must be in \[1, 256\]"),
                   (lambda: acc(T=long, rows=zl, classes=zl), "2\\^17 steps"), (lambda: acc(C=1 << 31, ld=1 << 31), "2\\^31 cells"),
                   (lambda: acc(width_q=0), "width_q must be >= 1"), (lambda: acc(lo_q=(1 << 23) + 1), r"lo_q must be in"),
                   (lambda: acc(lo_q=-(1 << 23) - 1), "lo_q must be in"), (lambda: acc(shift=25), r"shift must be in \[0, 24\]"),
                   (lambda: fin(K=65), "K must be in"), (lambda: fin(B=300), "B must be in"),
                   (lambda: fin(p_q=np.zeros(17)), r"P must be in \[0, 16\]"), (lambda: fin(edge=np.zeros(9)), r"L must be in \[0, 8\]"),
                   (lambda: m.distribution_init(0, 4, 4, *buf, 4, 8), "K must be in"),
                   (lambda: m.distribution_init(2, 257, 4, *buf, 4, 8), "B must be in")]
    for call, text in unsupported:
        with pytest.raises(core.Unsupported, match=text) as e:
            call()
        assert type(e.value) is core.Unsupported and isinstance(e.value, core.HipError) and "(code 3)" in str(e.value)
    # K is judged before B, B before T, T before the bins, the bins before the shift, as the header says
    with pytest.raises(core.Unsupported, match="K must be in"):
        acc(K=0, B=0, width_q=0)
    with pytest.raises(core.Unsupported, match="B must be in"):
        acc(B=0, T=long, rows=zl, classes=zl)
    with pytest.raises(core.Unsupported, match="2\\^17 steps"):
        acc(T=long, rows=zl, classes=zl, width_q=0)
    with pytest.raises(core.Unsupported, match="width_q"):
        acc(width_q=0, shift=30)
    invalid = [(lambda: acc(classes=np.full(Tn, 2, np.int32)), r"class_of_t outside \[-1, K\)"),
               (lambda: acc(classes=np.full(Tn, -2, np.int32)), "class_of_t outside"),
               (lambda: acc(rows=np.full(Tn, 1, np.int32)), "row_of_t outside"),
               (lambda: acc(ld=3), "bad T/C"), (lambda: acc(ldb=3), "bad T/C"), (lambda: acc(ldo=3), "bad T/C"),
               (lambda: acc(Dr=0), "bad T/C"), (lambda: acc(rows=np.zeros(Tn - 1, np.int32)), "row_of_t length must equal T"),
               (lambda: acc(ts=0), "NULL buffer"), (lambda: acc(bufs=[8] * 7 + [0]), "NULL buffer"),
               (lambda: fin(p_q=[(1 << 32) + 1]), r"p_q outside \[0, 2\^32\]"), (lambda: fin(edge=[5]), r"edge outside \[0, B\]"),
               (lambda: fin(edge=[-1]), "edge outside"), (lambda: fin(ldo=3), "bad C/ldo"), (lambda: fin(hist=0), "NULL buffer"),
               (lambda: m.distribution_init(2, 4, 4, *buf, 3, 8), "bad C/ldo"),
               (lambda: m.distribution_init(2, 4, 4, *buf, 4, 0), "NULL output buffer"),
               (lambda: m.set_distribution_block(-1), "steps must be >= 0")]
    for call, text in invalid:
        with pytest.raises(core.InvalidArgument, match=text) as e:
            call()
        assert type(e.value) is core.InvalidArgument
    # a bad label is judged before a NULL buffer, a bad leading dimension before a bad label
    with pytest.raises(core.InvalidArgument, match="class_of_t outside"):
        acc(classes=np.full(Tn, 5, np.int32), ts=0)
    with pytest.raises(core.InvalidArgument, match="bad T/C"):
        acc(ld=3, classes=np.full(Tn, 5, np.int32))
    # the caps themselves are taken; nothing is launched for C == 0 or T == 0: no device is needed, NULL buffers pass
    acc(C=0, ld=0, ldb=0, ldo=0, K=64, B=256, lo_q=-(1 << 23), shift=24, ts=0, bufs=[0] * 8)
    acc(T=0, rows=np.zeros(0, np.int32), classes=np.zeros(0, np.int32), ts=0, bufs=[0] * 8)
    fin(C=0, ldo=0, p_q=[0, 1 << 32], edge=[0, 4], hist=0)
    m.set_distribution_block(0)
