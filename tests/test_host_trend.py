"""Host side of mean_trend() (xmhw_amd/trend.py) and the oracle that defines its device stage
(tests/trend_oracle.py).  The oracle is pinned to independent code -- exact rational arithmetic, scipy where it
is installed, the golden cases of tools/make_golden_trend.py --, the host layer runs with the oracle plugged in
through ``_compute=``, and the C ABI's argument checks run without a device."""
import math
import os
from fractions import Fraction

import numpy as np
import numpy.testing as npt
import pytest

import trend_oracle as to
from xmhw_amd import BlockDataset, XmhwException, mean_trend
from xmhw_amd import trend as tr

GOLD = os.path.join(os.path.dirname(__file__), "golden")
U = 2.0 ** -53


def series(rng, n, kind):
    if kind == 0:
        y = rng.normal(size=n) * 10.0 ** rng.integers(-3, 4)
    elif kind == 1:
        y = rng.integers(0, 4, n).astype(np.float64)
    else:
        y = 20 + 0.1 * np.arange(n) + rng.normal(size=n)
    y[rng.random(n) < rng.choice([0.0, 0.2, 0.5])] = np.nan
    return y


def exact_ols(x, y):
    """least squares on the valid points in rational arithmetic: (mean at x = 0, trend)"""
    v = ~np.isnan(y)
    xs, ys = [Fraction(float(a)) for a in x[v]], [Fraction(float(a)) for a in y[v]]
    m = len(xs)
    xb, yb = sum(xs) / m, sum(ys) / m
    sxx = sum((a - xb) ** 2 for a in xs)
    sxy = sum((a - xb) * (b - yb) for a, b in zip(xs, ys))
    return yb - sxy / sxx * xb, sxy / sxx, xb, yb, sxx, xs, ys


def test_ols_against_exact_rational_arithmetic():
    rng = np.random.default_rng(1)
    n_checked = 0
    for rep in range(300):
        n = int(rng.integers(3, 60))
        y = series(rng, n, rep % 3)
        x = tr.centred_years(np.arange(n) * int(rng.integers(1, 4)) + 1982.0)
        if (~np.isnan(y)).sum() < 2:
            continue
        mean, trend, _ = to.ols_oracle(y[:, None], x, tr.tcrit_table(0.05, n))[:, 0]
        e_mean, e_trend, xb, yb, sxx, xs, ys = exact_ols(x, y)
        m = len(xs)
        # Derivation.  The closed form is two dot products of m terms over centred data and one division.  A
        # recursive dot product of m terms whose factors carry one rounding each (the subtraction of the centre) has
        # relative error <= gamma_{m+2} against sum|.||.| (Higham, Accuracy and Stability, s. 3.1: m-1 additions,
        # one product, one rounding per centred factor -> m+2 factors (1+d)); the division adds one and the
        # quotient of two such sums one more: gamma with k = m+4, on sum|x-xb||y-yb| / Sxx.  The centres xb, yb are
        # themselves rounded sums (gamma_m relative to mean|x|, mean|y|): a shift dxb of the centre changes Sxy by
        # at most dxb * sum|y-yb| (and likewise dyb * sum|x-xb|), which is "the same term for the centring".
        k = m + 4
        gamma = k * U / (1 - k * U)
        ax = [abs(a - xb) for a in xs]
        ay = [abs(b - yb) for b in ys]
        main = gamma * float(sum(a * b for a, b in zip(ax, ay)) / sxx)
        centring = gamma * float((sum(abs(a) for a in xs) / m * sum(ay) + sum(abs(b) for b in ys) / m * sum(ax)) / sxx)
        bound = main + centring
        assert abs(Fraction(float(trend)) - e_trend) <= bound, (rep, float(e_trend), trend, bound)
        # mean = yb - trend * xb: the error of yb (gamma_m mean|y|), of trend times |xb|, two more roundings
        bound_mean = gamma * float(sum(abs(b) for b in ys) / m) + bound * float(abs(xb)) \
            + 2 * U * (abs(float(e_mean)) + abs(float(e_trend * xb)))
        assert abs(Fraction(float(mean)) - e_mean) <= bound_mean, (rep, float(e_mean), mean, bound_mean)
        n_checked += 1
    assert n_checked > 250


def test_ols_on_dyadic_data_is_correctly_rounded():
    """small integers on an odd number of yearly blocks, no gaps: x, xb = 0, every sum and product are exact in
    float64, so trend is the rational result rounded once"""
    rng = np.random.default_rng(2)
    for n in (3, 5, 9, 21, 41):
        x = tr.centred_years(np.arange(n) + 1982.0)
        assert np.all(x == np.round(x))
        for _ in range(20):
            y = rng.integers(-8, 9, n).astype(np.float64) * 4.0
            y[0] -= y.sum() % n                                          # sum(y) a multiple of n: yb is exact too
            assert y.sum() % n == 0
            mean, trend, _ = to.ols_oracle(y[:, None], x, tr.tcrit_table(0.05, n))[:, 0]
            e_mean, e_trend = exact_ols(x, y)[:2]
            assert trend == e_trend.numerator / e_trend.denominator      # int / int: one correctly rounded division
            assert mean == float(e_mean)


def test_golden_cases():
    g = np.load(os.path.join(GOLD, "trend_cases.npz"))
    x = tr.centred_years(g["years"])
    y = g["y"]
    ols = to.ols_oracle(y, x, tr.tcrit_table(0.05, y.shape[0]))
    npt.assert_allclose(ols[:2], g["ols_mean_trend"], rtol=1e-12, atol=1e-13)
    ts = to.theil_sen_oracle(y, x)
    npt.assert_array_equal(ts[0], g["ts_trend_s_var"][0])
    npt.assert_array_equal(ts[2:], g["ts_trend_s_var"][1:])
    assert ts[3, 4] == 0 and ts[2, 4] == 0                        # the all-equal series
    n = y.shape[0]
    assert ts[2, 5] == n * (n - 1) // 2 and ts[2, 6] == -n * (n - 1) // 2


def test_tie_term_equals_the_textbook_group_sum():
    rng = np.random.default_rng(3)
    for _ in range(50):
        n = int(rng.integers(3, 40))
        y = rng.integers(0, 4, n).astype(np.float64)
        y[rng.random(n) < 0.1] = -0.0 * 1
        x = tr.centred_years(np.arange(n))
        var = to.theil_sen_oracle(y[:, None], x)[3, 0]
        t = np.unique(y, return_counts=True)[1]
        assert var == (n * (n - 1) * (2 * n + 5) - int((t * (t - 1) * (2 * t + 5)).sum())) / 18.0


def test_theil_sen_edges():
    x = tr.centred_years(np.arange(6) + 2000.0)
    nan = np.nan
    y = np.array([[nan] * 6, [nan, 2.5, nan, nan, nan, nan], [nan, 1.0, nan, nan, 4.0, nan], [1, 2, 3, 4, 5, 6.0],
                  [1, np.inf, 3, 4, 5, 6.0], [0.0, -0.0, 0.0, -0.0, 0.0, -0.0]]).T
    t = to.theil_sen_oracle(y, x)
    assert np.isnan(t[:, 0]).all() and np.isnan(t[:, 4]).all()
    assert np.isnan(t[0, 1]) and t[1, 1] == 2.5 and np.isnan(t[2:, 1]).all()
    assert t[0, 2] == 1.0 and t[1, 2] == 2.5 - 1.0 * 0.0 and np.isnan(t[2:, 2]).all()
    assert t[0, 3] == 1.0 and t[2, 3] == 15 and t[3, 3] == 6 * 5 * 17 / 18
    assert t[0, 5] == 0 and t[2, 5] == 0 and t[3, 5] == 0
    o = to.ols_oracle(y, x, tr.tcrit_table(0.05, 6))
    assert np.isnan(o[:, 0]).all() and np.isnan(o[:, 4]).all()
    assert o[0, 1] == 2.5 and np.isnan(o[1:, 1]).all()
    assert o[1, 2] == 1.0 and np.isnan(o[2, 2])
    assert o[1, 3] == 1.0 and o[0, 3] == 3.5 and o[2, 3] == 0.0


# ---- against scipy (figures measured with 1.15.3) -----------------------------------------------------------------
def test_tcrit_against_scipy():
    st = pytest.importorskip("scipy.stats")
    worst = worst_polished = worst_resid = 0.0
    for alpha in (0.01, 0.05, 0.1, 0.32):
        for dof in range(1, 201):
            q = alpha / 2
            mine = tr.student_t_isf(q, dof)
            ref = st.t.isf(q, dof)
            worst = max(worst, abs(mine - ref) / ref)
            # scipy's isf stops its own root find early (its sf(isf(q)) misses q by up to 7.5e-11 relative): one
            # Newton step on scipy's sf / pdf polishes it
            polished = ref + (st.t.sf(ref, dof) - q) / st.t.pdf(ref, dof)
            worst_polished = max(worst_polished, abs(mine - polished) / polished)
            worst_resid = max(worst_resid, abs(st.t.sf(mine, dof) - q) / q)
    print(f"tcrit vs t.isf: {worst:.3e}; vs polished t.isf: {worst_polished:.3e}; |t.sf(tcrit) - q|/q: {worst_resid:.3e}")
    # Measured (scipy 1.15.3): 4.742e-11 against t.isf as it is -- that is t.isf's own stopping error, not this
    # module's: by scipy's own t.sf, |t.sf(t) - q|/q is up to 7.5e-11 for t = t.isf(q) and at most 1.025e-12 for this
    # module's values.  Against t.isf polished by one Newton step (the converged yardstick): 3.046e-13, below the
    # 1e-12 that would mean an inverse CDF that has not converged; what is left is the rounding of the lgamma
    # differences in the density's constant.  Asserted: 4 x each measured figure.
    assert worst <= 4 * 4.742e-11
    assert worst_polished <= 4 * 3.046e-13
    assert worst_resid <= 4 * 1.025e-12


def test_oracle_against_scipy():
    st = pytest.importorskip("scipy.stats")
    rng = np.random.default_rng(4)
    w_trend = w_dtrend = w_p = 0.0
    n_tied = 0
    for rep in range(400):
        n = int(rng.integers(4, 50))
        y = series(rng, n, rep % 3)
        years = np.arange(n) + 1982.0
        x = tr.centred_years(years)
        v = ~np.isnan(y)
        m = int(v.sum())
        if m < 3:
            continue
        tc = tr.tcrit_table(0.05, n)
        o = to.ols_oracle(y[:, None], x, tc)[:, 0]
        lr = st.linregress(years[v], y[v])
        if lr.slope != 0:
            w_trend = max(w_trend, abs(o[1] - lr.slope) / abs(lr.slope))
        d = st.t.isf(0.025, m - 2) * lr.stderr
        if d > 1e-9 * abs(lr.slope):
            w_dtrend = max(w_dtrend, abs(o[2] - d) / d)
        t = to.theil_sen_oracle(y[:, None], x)[:, 0]
        # bit for bit (values compared with ==: the sign of a zero median is the total order's, see trend.py)
        assert t[0] == st.theilslopes(y[v], x[v])[0]
        i, j = np.triu_indices(m, 1)
        assert t[0] == np.median((y[v][j] - y[v][i]) / (x[v][j] - x[v][i]))
        assert t[1] == np.median(y[v]) - t[0] * np.median(x[v])
        if t[3] > 0:
            p = math.erfc(abs(t[2]) / math.sqrt(2 * t[3]))
            q = st.kendalltau(x[v], y[v], method="asymptotic").pvalue
            w_p = max(w_p, abs(p - q) / q)
            n_tied += rep % 3 == 1
        # the continuity-corrected statistic mean_trend() returns: the host formula restated
        z, pv = tr.mann_kendall_z(t[2], t[3])
        if t[3] > 0:
            want = 0.0 if t[2] == 0 else (t[2] - np.sign(t[2])) / np.sqrt(t[3])
            assert z == want and pv == math.erfc(abs(want) / math.sqrt(2.0))
        else:
            assert np.isnan(z) and np.isnan(pv)
    print(f"trend vs linregress {w_trend:.3e}; dtrend {w_dtrend:.3e}; MK p vs kendalltau {w_p:.3e} ({n_tied} tied series)")
    assert n_tied > 100
    assert w_p <= 1e-13                                   # set by the issue
    # Measured on this set (scipy 1.15.3): trend 3.691e-14 (rounding noise between two float64 routes), dtrend
    # 2.471e-11 (t.isf's own stopping error, see test_tcrit_against_scipy).  Asserted: 4 x the measured figures.
    assert w_trend <= 4 * 3.691e-14
    assert w_dtrend <= 4 * 2.471e-11


# ---- the host layer with the oracle plugged in ---------------------------------------------------------------------
def block(nb, sshape=(2, 3), names=("ecount", "duration", "total_days"), seed=0, land=(1,)):
    rng = np.random.default_rng(seed)
    ncol = int(np.prod(sshape, dtype=np.int64))
    data = {}
    for k in names:
        v = rng.integers(0, 5, (nb, ncol)).astype(np.float64) if k != "duration" else rng.normal(size=(nb, ncol)) + 10
        v[:, list(land)] = np.nan
        data[k] = v.reshape((nb,) + sshape)
    years = np.arange(1990, 1990 + nb)
    if sshape == ():
        return BlockDataset(data, ("years",), {"years": years}, np.arange(1990, 1991 + nb))
    coords = {"years": years, "lat": np.arange(sshape[0]) * 1.0, "lon": np.arange(sshape[1]) + 100.0}
    return BlockDataset(data, ("years", "lat", "lon"), coords, np.arange(1990, 1991 + nb))


@pytest.mark.parametrize("method", ["ols", "theil_sen"])
def test_gridded_block_dataset(method):
    blk = block(12)
    res = mean_trend(blk, alpha=0.1, method=method, _compute=to.trend_oracle)
    assert tuple(res.keys()) == tr.WHAT[method]
    assert res.dims == ("lat", "lon") and set(res.coords) == {"lat", "lon"}
    npt.assert_array_equal(res.coords["lon"], [100.0, 101.0, 102.0])
    assert res.attrs["alpha"] == 0.1 and res.attrs["method"] == method
    npt.assert_array_equal(res.attrs["years"], np.arange(1990, 2002))
    x = tr.centred_years(np.arange(1990, 2002))
    for what in res.keys():
        assert set(res[what]) == {"ecount", "duration", "total_days"}
        for k, v in res[what].items():
            assert v.shape == (2, 3)
            assert np.isnan(v[0, 1])                                     # land
    y = blk["duration"][:, 1, 2]
    if method == "ols":
        want = to.ols_oracle(y[:, None], x, tr.tcrit_table(0.1, 12))[:, 0]
        got = [res[w]["duration"][1, 2] for w in ("mean", "trend", "dtrend")]
        npt.assert_array_equal(got, want)
        assert np.isfinite(got).all()
    else:
        want = to.theil_sen_oracle(y[:, None], x)[:, 0]
        got = [res[w]["duration"][1, 2] for w in ("trend", "mean", "mk_s", "mk_var")]
        npt.assert_array_equal(got, want)
        z, p = tr.mann_kendall_z(want[2], want[3])
        assert res["mk_z"]["duration"][1, 2] == z and res["p_value"]["duration"][1, 2] == p and 0 < p <= 1


@pytest.mark.parametrize("method", ["ols", "theil_sen"])
def test_point_block_dataset(method):
    blk = block(9, sshape=(), land=())
    res = mean_trend(blk, method=method, _compute=to.trend_oracle)
    assert res.dims == () and res.coords == {}
    for what in res.keys():
        assert res[what]["ecount"].shape == ()
    assert np.isfinite(res["trend"]["duration"])


@pytest.mark.parametrize("nb", [0, 1, 2, 3])
def test_few_blocks(nb):
    blk = block(nb, land=())
    o = mean_trend(blk, method="ols", _compute=to.trend_oracle)
    t = mean_trend(blk, method="theil_sen", _compute=to.trend_oracle)
    for res in (o, t):
        for what in res.keys():
            assert res[what]["ecount"].shape == (2, 3)
    if nb < 2:
        assert all(np.isnan(v).all() for w in ("trend", "dtrend") for v in o[w].values())
        assert all(np.isnan(v).all() for w in ("trend", "mk_s", "mk_var", "mk_z", "p_value") for v in t[w].values())
        for res in (o, t):
            if nb == 0:
                assert np.isnan(res["mean"]["duration"]).all()
            else:
                npt.assert_array_equal(res["mean"]["duration"], blk["duration"][0])
    if nb == 2:
        assert np.isfinite(o["trend"]["duration"]).all() and np.isnan(o["dtrend"]["duration"]).all()
        npt.assert_array_equal(o["trend"]["duration"], blk["duration"][1] - blk["duration"][0])
        assert np.isfinite(t["trend"]["duration"]).all() and np.isnan(t["p_value"]["duration"]).all()
    if nb == 3:
        assert np.isfinite(o["dtrend"]["duration"]).all() and np.isfinite(t["mk_var"]["duration"]).all()


def test_exceptions():
    blk = block(5)
    with pytest.raises(XmhwException, match="BlockDataset"):
        mean_trend({"ecount": np.zeros((5, 2))})
    with pytest.raises(XmhwException, match="BlockDataset"):
        mean_trend(np.zeros((5, 2)))
    for alpha in (0, 1, -0.1, 1.5, np.nan, "x"):
        with pytest.raises(XmhwException, match="alpha"):
            mean_trend(blk, alpha=alpha, _compute=to.trend_oracle)
    with pytest.raises(XmhwException, match="method"):
        mean_trend(blk, method="lstsq", _compute=to.trend_oracle)
    with pytest.raises(XmhwException, match="at most 128 blocks"):
        mean_trend(block(129), method="theil_sen", _compute=to.trend_oracle)
    mean_trend(block(129), method="ols", _compute=to.trend_oracle)            # no cap on this path


def test_c_abi_rejects_bad_arguments():
    """argument checks of the two entry points come before any device work: error code and xmhw_last_error"""
    import ctypes
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = ctypes.CDLL(os.path.join(root, "xmhw_amd", "libxmhw_amd.so"))
    lib.xmhw_last_error.restype = ctypes.c_char_p
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    ols = lib.xmhw_block_trend_ols
    ols.restype = ctypes.c_int
    ols.argtypes = [vp, i32, i32, i64, i64, vp, vp, vp, i64, vp]
    ts = lib.xmhw_block_trend_theil_sen
    ts.restype = ctypes.c_int
    ts.argtypes = [vp, i32, i32, i64, i64, vp, vp, i64, vp]
    assert ols(None, 0, 40, 100, 100, None, None, None, 100, None) == 0          # nothing to do
    assert ts(None, 22, 40, 0, 0, None, None, 0, None) == 0
    p = 4096                                                                      # never dereferenced: the checks fail first
    for f, args, code, msg in (
            (ols, (p, -1, 40, 10, 10, p, p, p, 10, None), 1, b"nstat"),
            (ols, (p, 2, -1, 10, 10, p, p, p, 10, None), 1, b"nb"),
            (ols, (p, 2, 40, -1, 10, p, p, p, 10, None), 1, b"C"),
            (ols, (p, 2, 40, 10, 9, p, p, p, 10, None), 1, b"ld must"),
            (ols, (p, 2, 40, 10, 10, p, p, p, 9, None), 1, b"ldo"),
            (ols, (None, 2, 40, 10, 10, p, p, p, 10, None), 1, b"NULL"),
            (ols, (p, 2, 40, 10, 10, None, p, p, 10, None), 1, b"NULL"),
            (ols, (p, 2, 40, 10, 10, p, None, p, 10, None), 1, b"tcrit"),
            (ols, (p, 2, 40, 10, 10, p, p, None, 10, None), 1, b"NULL"),
            (ts, (p, 2, 40, 10, 9, p, p, 10, None), 1, b"ld must"),
            (ts, (p, 2, 40, 10, 10, p, p, 9, None), 1, b"ldo"),
            (ts, (None, 2, 40, 10, 10, p, p, 10, None), 1, b"NULL"),
            (ts, (p, 2, 40, 10, 10, p, None, 10, None), 1, b"NULL"),
            (ts, (p, 2, 129, 10, 10, p, p, 10, None), 3, b"cap of 128"),
            (ts, (p, 2, 100000, 0, 0, p, p, 0, None), 3, b"cap of 128")):
        assert f(*args) == code, args
        assert msg in lib.xmhw_last_error(), (args, lib.xmhw_last_error())
