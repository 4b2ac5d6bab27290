"""The host logic of lag_correlation() without a device: the exports, argument validation, the oracle itself on a case
worked by hand, the whole public path around the numpy stand-in of the device stage, the derived fields of
LagCorrelationDataset on integers worked by hand and against exact rational arithmetic, and the refusals of the C
entries."""
import importlib
import math
from fractions import Fraction

import numpy as np
import numpy.testing as npt
import pytest

import lag_correlation_cases as lc
import lag_correlation_oracle as lo
import xmhw_amd
from xmhw_amd import GridSeries, lag_correlation
from xmhw_amd.exception import XmhwException

lm = importlib.import_module("xmhw_amd.lag_correlation")        # (the package attribute of that name is the function)

NY, NX, T = 3, 4, 400
TIME = np.datetime64("2001-01-01") + np.arange(T).astype("timedelta64[D]")
COORDS = {"time": TIME, "lat": np.arange(NY) * 0.25, "lon": np.arange(NX) * 0.25}
LAND = np.zeros((NY, NX), bool)
LAND[0, 1] = LAND[2, 2] = True
ONE = 1 << 16
STAGE = lo.lag_corr_cells


def field(land=LAND, seed=1, dtype=np.float32, scale=1.0, lead=0):
    """a persistent series on the grid, NaN on ``land`` and on 3 % of the samples"""
    rng = np.random.default_rng(seed)
    e = rng.normal(0, 1.0, (T + 8, NY, NX))
    a = np.zeros_like(e)
    for t in range(1, T + 8):
        a[t] = 0.7 * a[t - 1] + e[t]
    x = np.round(scale * a[lead:lead + T], 3).astype(dtype)
    x[rng.random(x.shape) < 0.03] = np.nan
    x[:, land] = np.nan
    return GridSeries(x, ("time", "lat", "lon"), COORDS)


def test_exports():
    assert "lag_correlation" in xmhw_amd.__all__ and "LagCorrelationDataset" in xmhw_amd.__all__
    assert xmhw_amd.lag_correlation is lm.lag_correlation and xmhw_amd.LagCorrelationDataset is lm.LagCorrelationDataset


def test_argument_validation():
    x, y = field(), field(seed=2)
    bad = [(dict(lags=(0, 64)), "at most 63 steps either way"), (dict(lags=(-64, 0)), "at most 63 steps"),
           (dict(lags=(1, 5)), r"lo <= 0 <= hi, got \(1, 5\)"), (dict(lags=(-3, -1)), "lo <= 0 <= hi"),
           (dict(lags=5), "a pair"), (dict(lags=(0, 2.5)), "whole numbers of steps"), (dict(lags=(0, 1, 2)), "a pair"),
           (dict(shift_x=25), r"shift_x should be in \[0, 24\]"), (dict(shift_y=-1), r"shift_y should be in \[0, 24\]"),
           (dict(shift_x=1.5), "shift_x should be a whole number"),
           (dict(classes=np.arange(T) % 65), "at most 64 classes"), (dict(classes=np.zeros(T - 1, int)), "one entry per time step"),
           (dict(max_result_bytes=1000), r"K = 1 classes x 31 lags \(0 \.\. 30\) x C = 10 cells take 13640 bytes")]
    for kw, text in bad:
        with pytest.raises(XmhwException, match=text):
            lag_correlation(x, y, _compute=STAGE, **kw)
    lag_correlation(x, y, lags=(-63, 63), _compute=STAGE, max_result_bytes=44 * 127 * 10, shift_x=24, shift_y=24)   # the caps
    with pytest.raises(XmhwException, match="base_y belongs to y"):
        lag_correlation(x, base_y=np.zeros((NY, NX)), _compute=STAGE)
    # the second field: another length, a shifted axis, another grid, a point series
    short = GridSeries(np.asarray(y.values)[:-1], y.dims, dict(COORDS, time=TIME[:-1]))
    with pytest.raises(XmhwException, match="400 and 399 time steps"):
        lag_correlation(x, short, _compute=STAGE)
    with pytest.raises(XmhwException, match="same time axis"):
        lag_correlation(x, GridSeries(y.values, y.dims, dict(COORDS, time=TIME + np.timedelta64(1, "D"))), _compute=STAGE)
    other = GridSeries(np.zeros((T, NY, NX + 1), np.float32), ("time", "lat", "lon"), dict(COORDS, lon=np.arange(NX + 1.0)))
    with pytest.raises(XmhwException, match="not on the same grid"):
        lag_correlation(x, other, _compute=STAGE)
    with pytest.raises(XmhwException, match="single-point series with a grid"):
        lag_correlation(x, GridSeries(np.zeros(T, np.float32), ("time",), {"time": TIME}), _compute=STAGE)
    with pytest.raises(XmhwException, match=r"base_y should be on the grid of x"):
        lag_correlation(x, y, base_y=np.zeros((NY, NX + 1)), _compute=STAGE)
    long = 1 << 17
    with pytest.raises(XmhwException, match="fewer than 2\\*\\*17 time steps"):
        lag_correlation(GridSeries(np.zeros(long, np.float32), ("time",), {"time": np.arange(long)}), _compute=STAGE)
    # out of range: the text names the field and its shift
    big = GridSeries(np.asarray(y.values) * 100.0, y.dims, COORDS)
    with pytest.raises(XmhwException, match=r"samples of y lie .* shift_y = 2: pass a larger shift_y"):
        lag_correlation(x, big, shift_y=2, _compute=STAGE)
    with pytest.raises(XmhwException, match=r"samples of x lie .* shift_x = 0"):
        lag_correlation(big, x, shift_y=2, _compute=STAGE)
    with pytest.raises(XmhwException, match=r"samples of x lie"):
        lag_correlation(big, _compute=STAGE)
    lag_correlation(x, big, shift_y=5, _compute=STAGE)


def test_oracle_on_a_case_worked_by_hand():
    """T = 6, one cell, L = 2, classes 0 0 1 1 -1 0, x with one NaN (step 3), y with one out-of-range value (step 1).
    Pairs (t, t - l) need class(t) >= 0, x(t) valid, y(t - l) valid:
      lag 0: t = 0, 2, 5 (1: y out of range, 3: x NaN, 4: class -1)     -> class 0: t = 0, 5; class 1: t = 2
      lag 1: t = 1 (y0), 5 (y4)  [2: y1 out of range, 3: x NaN]          -> class 0: t = 1, 5
      lag 2: t = 2 (y0), 5 (y3)  [3: x NaN]                              -> class 1: t = 2; class 0: t = 5"""
    x = np.array([[1.0], [2.0], [3.0], [np.nan], [5.0], [6.0]])
    y = np.array([[0.5], [300.0], [-1.0], [2.0], [4.0], [-3.0]])
    classes = np.array([0, 0, 1, 1, -1, 0])
    r = lo.lag_corr_sums(x, y, np.zeros((1, 1)), np.zeros((1, 1)), np.zeros(6, int), 0, 0, classes, 2, 2)
    assert r["n"][:, :, 0].tolist() == [[2, 2, 1], [1, 0, 1]] and r["n"].dtype == np.int32
    assert r["n_range"].tolist() == [0, 1]
    h = ONE // 2
    assert r["sx"][:, :, 0].tolist() == [[7 * ONE, 8 * ONE, 6 * ONE], [3 * ONE, 0, 3 * ONE]]
    assert r["sy"][:, :, 0].tolist() == [[h - 3 * ONE, h + 4 * ONE, 2 * ONE], [-ONE, 0, h]]
    assert r["sxy"][:, :, 0].tolist() == [[ONE * h - 18 * ONE * ONE, 2 * ONE * h + 24 * ONE * ONE, 12 * ONE * ONE],
                                          [-3 * ONE * ONE, 0, 3 * ONE * h]]
    assert r["sxx"][0, :, 0].tolist() == [37 * ONE * ONE, 40 * ONE * ONE, 36 * ONE * ONE]
    assert r["syy"][0, :, 0].tolist() == [h * h + 9 * ONE * ONE, h * h + 16 * ONE * ONE, 4 * ONE * ONE]
    # an out-of-range x on a step of class -1 is not counted; a shift brings y's 300 into range
    x[4, 0] = 1000.0
    r = lo.lag_corr_sums(x, y, np.zeros((1, 1)), np.zeros((1, 1)), np.zeros(6, int), 0, 2, classes, 2, 2)
    assert r["n_range"].tolist() == [0, 0] and r["n"][:, :, 0].tolist() == [[3, 2, 1], [1, 1, 1]]
    assert r["sy"][0, 0, 0] == (h + 300 * ONE - 3 * ONE) // 4
    # the cases hold what they say they hold
    d = lc.series(300, 40, np.float32, 3)
    assert np.isnan(d["y"][:, 2]).all() and np.isnan(d["x"][:, 3]).all() and np.isnan(d["y"][20:20 + lc.LONG_RUN, 4]).all()
    assert lc.LONG_RUN > 63 and 0.02 < np.isnan(d["x"][:, 8:]).mean() < 0.04
    q, valid, out = lo.fixed(d["x"], d["base_x"], d["rows"], 0)
    assert out[:, 6].sum() == 2 and out[[11, 41], 7].all() and out.sum() == 4
    q, valid, out = lo.fixed(d["y"], d["base_y"], d["rows"], 0)
    assert valid[[12, 40], 7].all() and abs(q[12, 7]) == (1 << 23) - 1 and out.sum() == 2


def test_public_path_around_the_stand_in_equals_the_oracle():
    # y has land of its own: (1, 1) is ocean in x alone and has no pair
    yland = LAND.copy()
    yland[1, 1] = True
    x, y = field(seed=5), field(yland, seed=6, scale=20.0, dtype=np.float64)
    keep = ~LAND.reshape(-1)
    C = int(keep.sum())
    labels = np.where(np.arange(T) % 50 < 45, (np.arange(T) // 100) % 2 * 10 + 3, -1)     # classes 3 and 13, gaps of -1
    kid = np.where(labels < 0, -1, (labels == 13).astype(int))
    bx = np.where(LAND, np.nan, 0.5)
    by = np.stack([np.where(yland, np.nan, 1.0 + j) for j in range(366)])                  # a 366-row base beside one row
    got = lag_correlation(x, y, base_x=bx, base_y=by, lags=(-4, 6), classes=labels, shift_x=1, shift_y=3, _compute=STAGE)
    assert got.klass.tolist() == [3, 13] and got.lag.tolist() == list(range(-4, 7)) and not got.auto
    assert got.n.shape == (2, 11, NY, NX) and got.n.dtype == np.int32 and got.sxy.dtype == np.int64
    from xmhw_amd import calendar as cal
    rows = cal.add_doy(TIME) - 1
    xs = np.asarray(x.values, dtype=np.float64).reshape(T, -1)[:, keep]
    ys = np.asarray(y.values).reshape(T, -1)[:, keep]
    bys = np.where(np.isnan(by.reshape(366, -1)[:, keep]), 0.0, by.reshape(366, -1)[:, keep])
    want, n_range = lo.lag_corr_lags(xs, ys, np.full((366, C), 0.5), bys, rows, 1, 3, kid, 2, -4, 6)
    assert n_range == (0, 0) and want[0].sum() > 10000
    for k, w in zip(lo.FIELDS, want):
        a = getattr(got, k).reshape(2, 11, -1)
        npt.assert_array_equal(a[..., keep], w, err_msg=k)
        assert (a[..., ~keep] == 0).all()
    npt.assert_array_equal(got.keep, ~LAND)
    assert np.isnan(got.r[:, :, LAND]).all() and (got.n[:, :, 1, 1] == 0).all() and np.isnan(got.r[:, :, 1, 1]).all()
    # a negative lag pairs x(t) with y(t + l) under the class of step t + l: the oracle with the roles exchanged
    back = lo.lag_corr_sums(ys, xs, bys, np.full((366, C), 0.5), rows, 3, 1, kid, 2, 4)
    npt.assert_array_equal(got.sx.reshape(2, 11, -1)[:, 0][..., keep], back["sy"][:, 4])
    npt.assert_array_equal(got.sxy.reshape(2, 11, -1)[:, 3][..., keep], back["sxy"][:, 1])
    # y=None: the autocorrelation; base=None is zero on the ocean of x; negative lags mirror the positive ones
    auto = lag_correlation(x, lags=(-2, 5), classes=labels, shift_x=1, _compute=STAGE)
    w = lo.lag_corr_sums(xs, xs, np.zeros((1, C)), np.zeros((1, C)), np.zeros(T, int), 1, 1, kid, 2, 5)
    assert auto.auto and auto.lag.tolist() == list(range(-2, 6))
    for k, s in zip(lo.FIELDS, lo.SWAPPED):
        a = getattr(auto, k).reshape(2, 8, -1)[..., keep]
        npt.assert_array_equal(a[:, 2:], w[k], err_msg=k)
        npt.assert_array_equal(a[:, 0], w[s][:, 2], err_msg=k)
    assert (auto.r[:, 2][:, ~LAND] == 1.0).all()
    # a point series
    p = lag_correlation(GridSeries(xs[:, 0], ("time",), {"time": TIME}), GridSeries(ys[:, 0], ("time",), {"time": TIME}),
                        base_y=2.0, lags=(0, 3), shift_y=3, _compute=STAGE)
    wp = lo.lag_corr_sums(xs[:, :1], ys[:, :1], np.zeros((1, 1)), np.full((1, 1), 2.0), np.zeros(T, int), 0, 3, np.zeros(T, int), 1, 3)
    assert p.n.shape == (1, 4) and p.sxy.tolist() == wp["sxy"][..., 0].tolist()


def _dataset(n, sx, sy, sxx, syy, sxy, lag, auto=False, **kw):
    a = lambda v, dt: np.asarray(v, dtype=dt)                                                    # noqa: E731
    C = np.asarray(n).shape[-1]
    return lm.LagCorrelationDataset([0], lag, a(n, np.int32), a(sx, np.int64), a(sy, np.int64), a(sxx, np.int64),
                                    a(syy, np.int64), a(sxy, np.int64), np.ones(C, bool), ("cell",), {"cell": np.arange(C)},
                                    auto, **kw)


def _sums(x, y):
    x, y = np.asarray(x) * ONE, np.asarray(y) * ONE
    return len(x), int(x.sum()), int(y.sum()), int((x * x).sum()), int((y * y).sum()), int((x * y).sum())


def test_derived_fields_on_integers_worked_by_hand():
    """one class, one lag, six cells: y = x, y = -x, y = 2 x + 1, one pair, a constant x, a constant y"""
    xs = [1, 2, 3, 6]
    cells = [_sums(xs, xs), _sums(xs, [-v for v in xs]), _sums(xs, [2 * v + 1 for v in xs]), _sums([4], [5]),
             _sums([3, 3, 3], [1, 2, 4]), _sums([1, 2, 4], [7, 7, 7])]
    cols = [[[list(c)]] for c in zip(*cells)]                            # (1, 1, 6) each
    ds = _dataset(*cols, lag=[0])
    assert ds.r[0, 0, :3].tolist() == [1.0, -1.0, 1.0] and ds.slope[0, 0, :3].tolist() == [1.0, -1.0, 0.5]
    assert ds.mean_x[0, 0, 0] == 3.0 and ds.mean_y[0, 0, 2] == 7.0 and ds.cov[0, 0, 0] == 3.5 and ds.cov[0, 0, 1] == -3.5
    # n < 2: everything is NaN; a zero variance: r and slope are NaN, the means and the covariance are not
    assert all(np.isnan(getattr(ds, k)[0, 0, 3]) for k in ("mean_x", "mean_y", "cov", "r", "slope"))
    assert np.isnan(ds.r[0, 0, 4:]).all() and np.isnan(ds.slope[0, 0, 4:]).all()
    assert ds.mean_x[0, 0, 4] == 3.0 and ds.cov[0, 0, 4] == 0.0 and ds.mean_y[0, 0, 5] == 7.0
    # a constant far from zero, where float64 alone would leave a residue: 3 samples of 100.3
    q = int(round(100.3 * ONE))
    far = _dataset([[[3]]], [[[3 * q]]], [[[6 * ONE]]], [[[3 * q * q]]], [[[14 * ONE * ONE]]], [[[6 * q * ONE]]], lag=[0])
    assert np.isnan(far.r[0, 0, 0]) and np.isnan(far.slope[0, 0, 0])
    # the shifts scale means, covariance and slope, not r
    sh = _dataset(*cols, lag=[0], shift_x=4, shift_y=1)
    assert sh.mean_x[0, 0, 0] == 48.0 and sh.mean_y[0, 0, 2] == 14.0 and sh.cov[0, 0, 0] == 3.5 * 32.0
    assert sh.slope[0, 0, 2] == 0.5 * 8.0 and sh.r[0, 0, :3].tolist() == [1.0, -1.0, 1.0]
    # the methods of an autocorrelation refuse two fields; p_value of two fields needs n_eff
    for name in ("efolding_time", "integral_time_scale", "n_eff", "p_value"):
        with pytest.raises(XmhwException, match="autocorrelation"):
            getattr(ds, name)()
    lag, r = ds.lag_of_max()
    assert lag[0, :3].tolist() == [0.0, 0.0, 0.0] and r[0, :3].tolist() == [1.0, -1.0, 1.0] and np.isnan(lag[0, 3:]).all()


def _acf(rs, n0=1000):
    """an autocorrelation dataset whose r at the lags 0, 1, 2, ... is rs[cell]: unit variance, zero mean, sxy = r n"""
    rs = np.asarray(rs, dtype=np.float64).T[None]                       # (1, lags, cells)
    n = np.full(rs.shape, n0, np.int64)
    one = np.full(rs.shape, n0 * 4096, np.int64)                          # sxx = syy = n * 64**2
    sxy = np.rint(rs * n0 * 4096).astype(np.int64)
    zero = np.zeros(rs.shape, np.int64)
    return _dataset(n, zero, zero, one, one, sxy, lag=np.arange(rs.shape[1]), auto=True)


def test_time_scales_of_an_autocorrelation_worked_by_hand():
    e = math.exp(-1.0)
    ds = _acf([[1.0, 0.75, 0.5, 0.25, 0.125],        # crosses 1 / e between the lags 2 and 3
               [1.0, 0.875, 0.75, 0.625, 0.5],       # never below 1 / e: +inf
               [1.0, 0.25, -0.5, 0.75, 0.5],         # below at lag 1; r <= 0 at lag 2 cuts the integral
               [1.0, 0.5, 0.0, 0.5, 0.5]])           # r = 0 at lag 2 cuts it as well
    assert ds.r[0, :, 0].tolist() == [1.0, 0.75, 0.5, 0.25, 0.125]
    tau = ds.efolding_time()
    npt.assert_allclose(tau[0, 0], 2.0 + (0.5 - e) / 0.25, rtol=1e-15)
    assert np.isposinf(tau[0, 1])
    npt.assert_allclose(tau[0, 2], (1.0 - e) / 0.75, rtol=1e-15)
    tint = ds.integral_time_scale()
    assert tint[0].tolist() == [1.0 + 2.0 * 1.625, 1.0 + 2.0 * 2.75, 1.5, 2.0]
    ne = ds.n_eff()
    assert ne[0].tolist() == [1000.0 / 4.25, 1000.0 / 6.5, 1000.0 / 1.5, 500.0]
    # clipping: n_0 = 3 and a long memory -> 2; an anticorrelated lag 1 alone -> n_0
    small = _acf([[1.0, 0.875, 0.75], [1.0, -0.5, 0.25]], n0=3)
    assert small.integral_time_scale()[0].tolist() == [4.25, 1.0] and small.n_eff()[0].tolist() == [2.0, 3.0]
    # the p-value: Student's t with n_eff - 2 degrees of freedom, the default n_eff the dataset's own
    p = ds.p_value()
    assert p.shape == (1, 5, 4) and p[0, 0, 0] == 0.0                   # r = 1: t is infinite
    dof = 1000.0 / 4.25 - 2.0
    npt.assert_allclose(p[0, 3, 0], lm._t_two_sided(0.25 * math.sqrt(dof / (1.0 - 0.0625)), dof), rtol=1e-14)
    assert np.isnan(small.p_value()[0, 1, 0])                           # n_eff = 2: no degree of freedom
    # two fields: an array, or the two autocorrelations (Bretherton: n (1 - r1x r1y) / (1 + r1x r1y))
    cross = _acf([[0.5, 0.25, 0.125, 0.0, 0.0]] * 4)
    cross.auto = False
    with pytest.raises(XmhwException, match="needs n_eff"):
        cross.p_value()
    given = cross.p_value(n_eff=np.full((1, 4), 102.0))
    npt.assert_allclose(given[0, 0, 0], lm._t_two_sided(0.5 * math.sqrt(100.0 / 0.75), 100.0), rtol=1e-14)
    both = cross.p_value(n_eff=(ds, ds))
    ne = 1000.0 * (1.0 - 0.75 * 0.75) / (1.0 + 0.75 * 0.75)
    npt.assert_allclose(both[0, 1, 0], lm._t_two_sided(0.25 * math.sqrt((ne - 2.0) / (1.0 - 0.0625)), ne - 2.0), rtol=1e-14)
    with pytest.raises(XmhwException, match="AUTOcorrelation datasets"):
        cross.p_value(n_eff=(ds, cross))


def test_r_and_slope_against_exact_rational_arithmetic():
    """20 sampled entries of a run over the case series: r**2 and the slope from the integers in exact rational
    arithmetic, 1e-12 relative.  The float64 formula subtracts mx my from sxy / n: with |mean| <= standard deviation in both
    fields the minuend is at most twice the covariance's scale, so the dozen roundings of 2**-53 on the way are amplified
    by a small factor only -- far inside 1e-12.  The condition is asserted, so the case cannot drift."""
    d = lc.series(300, 40, np.float64, 19)
    classes, K = lc.seasons(300)
    w = lo.lag_corr_sums(d["x"], d["y"], d["base_x"], d["base_y"], d["rows"], 0, 1, classes, K, 12)
    C = 40
    ds = lm.LagCorrelationDataset(np.arange(K), np.arange(13), *(w[k] for k in lo.FIELDS), np.ones(C, bool), ("cell",),
                                  {"cell": np.arange(C)}, False, 0, 1)
    rng = np.random.default_rng(4)
    picked = 0
    for k, l, c in zip(rng.integers(0, K, 400), rng.integers(0, 13, 400), rng.integers(8, C, 400)):
        n, sx, sy, sxx, syy, sxy = (int(w[f][k, l, c]) for f in lo.FIELDS)
        if n < 20:
            continue
        vx, vy = Fraction(n * sxx - sx * sx, n * n), Fraction(n * syy - sy * sy, n * n)
        if not (Fraction(sx, n) ** 2 <= vx and Fraction(sy, n) ** 2 <= vy):
            continue                                                    # |mean| <= standard deviation in both fields
        cov = Fraction(n * sxy - sx * sy, n * n)
        if abs(cov) * 20 < abs(Fraction(sx * sy, n * n)) or cov == 0:
            continue                                                    # ... and a covariance that is not a small difference
        assert abs(ds.mean_x[k, l, c]) <= math.sqrt(vx) / ONE * (1 + 1e-9) and abs(ds.mean_y[k, l, c]) <= 2 * math.sqrt(vy) / ONE
        r2 = cov * cov / (vx * vy)
        npt.assert_allclose(ds.r[k, l, c], math.copysign(math.sqrt(r2), cov), rtol=1e-12)
        npt.assert_allclose(ds.slope[k, l, c], float(cov / vy) * 0.5, rtol=1e-12)
        picked += 1
        if picked == 20:
            break
    assert picked == 20


def test_c_entry_refusals_need_no_device_and_raise_the_exceptions_of_the_core_module():
    core = importlib.import_module("xmhw_amd._xmhw_hip")
    m = importlib.import_module("xmhw_amd._xmhw_hip_lagcorr")
    assert not any(hasattr(m, n) for n in ("HipError", "Unsupported", "InvalidArgument", "CommError"))
    Tn = 10
    z = np.zeros(Tn, np.int32)

    def acc(T=Tn, C=4, ldx=4, ldy=4, ldbx=4, ldby=4, Dr=1, rows=z, shift_x=0, shift_y=0, classes=z, K=1, L=3, ldo=4, itemsize=4):
        m.lag_corr_accumulate(0, ldx, 0, ldy, itemsize, T, C, 0, ldbx, 0, ldby, Dr, rows, shift_x, shift_y, classes, K, L,
                              0, 0, 0, 0, 0, 0, ldo, 0)

    def init(K=1, L=3, C=4, ldo=4):
        m.lag_corr_init(K, L, C, 0, 0, 0, 0, 0, 0, ldo, 0)

    long = (1 << 17)
    big = dict(C=1 << 31, ldx=1 << 31, ldy=1 << 31, ldbx=1 << 31, ldby=1 << 31, ldo=1 << 31)
    unsupported = [lambda: acc(K=0), lambda: acc(K=65), lambda: acc(L=64), lambda: acc(L=-1), lambda: acc(shift_x=25),
                   lambda: acc(shift_x=-1), lambda: acc(shift_y=25), lambda: acc(shift_y=-1),
                   lambda: acc(T=long, rows=np.zeros(long, np.int32), classes=np.zeros(long, np.int32)),
                   lambda: acc(**big), lambda: init(K=0), lambda: init(K=65), lambda: init(L=-1), lambda: init(L=64)]
    for call in unsupported:
        with pytest.raises(core.Unsupported) as e:
            call()
        assert type(e.value) is core.Unsupported and isinstance(e.value, core.HipError) and "(code 3)" in str(e.value)
    # K is judged before L, L before a shift, a shift before T, T before C, as the header says
    with pytest.raises(core.Unsupported, match="K must be in"):
        acc(K=0, L=100, shift_x=30)
    with pytest.raises(core.Unsupported, match="max_lag must be in"):
        acc(L=100, shift_y=30)
    with pytest.raises(core.Unsupported, match="shifts must be in"):
        acc(shift_y=30, T=long, rows=np.zeros(long, np.int32), classes=np.zeros(long, np.int32))
    with pytest.raises(core.Unsupported, match="2\\^17 steps"):
        acc(T=long, rows=np.zeros(long, np.int32), classes=np.zeros(long, np.int32), **big)
    invalid = [(lambda: acc(classes=np.full(Tn, 1, np.int32)), r"class_of_t outside \[-1, K\)"),
               (lambda: acc(classes=np.full(Tn, -2, np.int32)), r"class_of_t outside"),
               (lambda: acc(rows=np.full(Tn, 1, np.int32)), r"row_of_t outside \[0, D\)"),
               (lambda: acc(ldx=3), "bad T/C"), (lambda: acc(ldy=3), "bad T/C"), (lambda: acc(ldbx=3), "bad T/C"),
               (lambda: acc(ldby=3), "bad T/C"), (lambda: acc(ldo=3), "bad T/C"), (lambda: acc(Dr=0), "bad T/C"),
               (lambda: acc(rows=np.zeros(Tn + 1, np.int32)), "row_of_t length"),
               (lambda: acc(classes=np.zeros(Tn - 1, np.int32)), "class_of_t length"), (lambda: acc(itemsize=2), "itemsize"),
               (lambda: acc(), "NULL buffer"), (lambda: init(ldo=3), "bad C/ldo"), (lambda: init(), "NULL"),
               (lambda: m.set_lag_corr_block(-1), "steps must be")]
    for call, text in invalid:
        with pytest.raises(core.InvalidArgument, match=text) as e:
            call()
        assert type(e.value) is core.InvalidArgument
    # a bad label is judged before a NULL buffer, a bad leading dimension before a bad label
    with pytest.raises(core.InvalidArgument, match="bad T/C"):
        acc(ldx=3, classes=np.full(Tn, 5, np.int32))
    # the caps themselves are taken; nothing is launched for C == 0 or T == 0: no device is needed either
    none = dict(C=0, ldx=0, ldy=0, ldbx=0, ldby=0, ldo=0)
    acc(K=64, L=63, shift_x=24, shift_y=24, **none)
    acc(T=long - 1, rows=np.zeros(long - 1, np.int32), classes=np.zeros(long - 1, np.int32), **none)
    acc(T=0, rows=np.zeros(0, np.int32), classes=np.zeros(0, np.int32))
    m.set_lag_corr_block(0)
    assert (m.LAG_CORR_MAX_LAG, m.LAG_CORR_MAX_CLASSES, m.LAG_CORR_MAX_STEPS, m.LAG_CORR_BITS, m.LAG_CORR_RANGE_BITS,
            m.LAG_CORR_MAX_SHIFT) == (63, 64, 1 << 17, 16, 7, 24)
    assert (lm.MAX_LAG, lm.MAX_CLASSES, lm.MAX_STEPS, lm.BITS, lm.RANGE_BITS, lm.MAX_SHIFT) == (63, 64, 1 << 17, 16, 7, 24)
