"""index_regression() without a GPU: hand cases, the oracle (tests/index_regression_oracle.py) as the device stage behind
the host layer (predictor table, listwise deletion, class labels, land, derived fields, exceptions), and the refusals of
the C entries that come before their first HIP call."""
import importlib

import numpy as np
import numpy.testing as npt
import pytest

import index_regression_oracle as ro
from xmhw_amd import GridSeries, IndexRegressionDataset, XmhwException, index_regression
from xmhw_amd.index_regression import (MAX_CLASSES, MAX_PREDICTORS, check_regress_arguments, class_totals, lagged_predictors,
                                       quantise_predictors)
from xmhw_amd.trend import _t_sf

ONE = 65536.0


def days(start, n):
    return np.datetime64(start) + np.arange(n).astype("timedelta64[D]")


def point(values, start="2001-01-01"):
    values = np.asarray(values)
    return GridSeries(values, ("time",), {"time": days(start, values.shape[0])})


def regress(temp, base, indices, **kw):
    return index_regression(temp, base, indices, _compute=ro.regress_cells, **kw)


def ar1(rng, T, phi, sd):
    x = np.zeros(T)
    for t in range(1, T):
        x[t] = phi * x[t - 1] + rng.normal(0, sd)
    return x


@pytest.fixture(scope="module")
def driven():
    """a 6 x 5 grid with land, 900 daily steps: anomalies that follow two AR(1) indices at lags 0 and 20, plus AR(1)
    noise; scattered NaN.  Zero-mean series on both sides (mean <= sd: test_derived_fields asserts it)."""
    rng = np.random.default_rng(3)
    T, ny, nx = 900, 6, 5
    u, v = ar1(rng, T, 0.9, 0.3), ar1(rng, T, 0.7, 0.5)
    u[100], v[455] = np.nan, np.nan
    gain = rng.normal(0, 0.8, (2, ny, nx))
    noise = np.stack([ar1(rng, T, 0.8, 0.3) for _ in range(ny * nx)], axis=1).reshape(T, ny, nx)
    lagged_v = np.concatenate([np.zeros(20), np.nan_to_num(v)[:-20]])
    a = np.nan_to_num(u)[:, None, None] * gain[0] + lagged_v[:, None, None] * gain[1] + noise
    base = np.round(15.0 + 5.0 * rng.random((ny, nx)), 2)
    x = base + a
    x[rng.random(x.shape) < 0.02] = np.nan
    x[:, rng.random((ny, nx)) < 0.25] = np.nan
    x[:, 4, :] = np.nan                                               # a dead grid line
    base[np.isnan(x).all(axis=0)] = np.nan                            # the base pairs with the ocean cells
    temp = GridSeries(x, ("time", "lat", "lon"), {"time": days("2001-01-01", T), "lat": np.arange(ny) * 1.0, "lon": np.arange(nx) * 1.0})
    return {"temp": temp, "base": base, "indices": {"u": u, "v": v}, "x": x, "T": T}


# ---- the oracle itself -------------------------------------------------------------------------------

def test_oracle_against_a_hand_case():
    ts = np.array([[1.5], [np.nan], [2.0], [3.0], [200.0], [1.0]])
    zq = np.array([[2], [3], [5], [7], [11], [13]], np.int64)
    r = ro.regress_sums(ts, np.array([[1.0]]), np.zeros(6, int), np.array([0, 0, 0, 0, 0, -1]), 1, zq)
    h = 32768
    assert r["n"][0, 0] == 3 and r["sa"][0, 0] == h + 2 * h + 4 * h and r["saa"][0, 0] == h * h * (1 + 4 + 16)
    assert r["n1"][0, 0] == 1 and r["saa1"][0, 0] == 2 * h * 4 * h                # the pair (2, 3) alone
    assert r["saz"][0, 0, 0] == h * 2 + 2 * h * 5 + 4 * h * 7
    assert r["mz"][0, 0, 0] == 3 + 11 and r["mzz"][0, 0, 0] == 9 + 121 and r["n_range"] == 1
    assert r["n"].dtype == np.int32 and r["saz"].dtype == np.int64


# ---- the predictor table -----------------------------------------------------------------------------

def test_lag_shifting_and_listwise_deletion_by_hand():
    x = np.arange(10.0)
    y = np.arange(10.0) * 10.0
    y[4] = np.nan
    names, lags, X = lagged_predictors({"x": x, "y": y}, (0, 2, -1), 10)
    assert names == ("x", "y") and lags.tolist() == [0, 2, -1] and X.shape == (10, 2, 3)
    npt.assert_array_equal(X[:, 0, 0], x)
    npt.assert_array_equal(X[:, 0, 1], [np.nan, np.nan, 0, 1, 2, 3, 4, 5, 6, 7])          # the index leads by 2
    npt.assert_array_equal(X[:, 0, 2], [1, 2, 3, 4, 5, 6, 7, 8, 9, np.nan])               # the index lags by 1
    # missing anywhere: steps 0, 1 (lag 2), 9 (lag -1), and y's NaN at 4 seen at t = 4, 6 and 3
    kid, n_dropped, zq, means, scales = quantise_predictors(X, np.where(np.arange(10) == 8, -1, 0), False)
    npt.assert_array_equal(kid, [-1, -1, 0, -1, -1, 0, -1, 0, -1, -1])
    assert n_dropped == 6 and zq.shape == (10, 6) and (zq[kid < 0] == 0).all()
    npt.assert_array_equal(zq[5], np.array([5, 3, 6, 50, 30, 60]) * 65536)
    assert (means == 0).all() and (scales == 1).all()
    # standardised over the used steps 2, 5, 7 alone
    kid, _, zq, means, scales = quantise_predictors(X, np.where(np.arange(10) == 8, -1, 0), True)
    npt.assert_allclose(means[0], [np.mean([2, 5, 7]), np.mean([0, 3, 5]), np.mean([3, 6, 8])])
    npt.assert_allclose(scales[1, 0], np.std([20.0, 50.0, 70.0]))
    npt.assert_array_equal(zq[:, 0], np.rint(np.where(kid >= 0, (x - means[0, 0]) / scales[0, 0], 0.0) * ONE))
    # the dataset reports the same
    r = regress(point(np.ones(10)), 0.0, {"x": x, "y": y}, lags=(0, 2, -1))
    assert r.n_dropped == 6 and r.n_steps.tolist() == [4] and r.n[0] == 4 and r.index == ("x", "y") and r.lag.tolist() == [0, 2, -1]


def test_a_region_series_is_taken_as_it_is():
    T = 50
    x = np.sin(np.arange(T) / 5.0)
    series = GridSeries(x[:, None], ("time", "region"), {"time": days("2001-01-01", T), "region": np.array([0])})
    a = regress(point(x * 2.0 + 1.0), 1.0, {"nino": series})
    b = regress(point(x * 2.0 + 1.0), 1.0, {"nino": x})
    npt.assert_array_equal(a.saz, b.saz)
    npt.assert_allclose(a.slope, 2.0, atol=1e-4)
    npt.assert_allclose(a.intercept, 0.0, atol=1e-4)


def test_standardisation_is_undone_in_the_reported_slope():
    rng = np.random.default_rng(8)
    T = 400
    x = 300.0 + 40.0 * ar1(rng, T, 0.8, 0.5)                        # far outside (-2**7, 2**7) as it is
    y = 0.03 * (x - 290.0) + rng.normal(0, 0.1, T)
    r = regress(point(y + 5.0), 5.0, {"x": x})
    want = np.polyfit(x, y, 1)
    sb, rb = r.quantisation_bound()
    assert abs(r.slope[0, 0, 0] - want[0]) <= sb[0, 0, 0] < 1e-5
    assert abs(r.intercept[0, 0, 0] - want[1]) <= sb[0, 0, 0] * np.abs(x).max() + 2.0 ** -16
    assert abs(r.means[0, 0] - x.mean()) < 1e-9 and abs(r.scales[0, 0] - x.std()) < 1e-9
    # a scaled copy of the index: the standardised table is the same, the slope scales back
    r2 = regress(point(y + 5.0), 5.0, {"x": x * 4.0})
    npt.assert_array_equal(r2.saz, r.saz)
    npt.assert_allclose(r2.slope, r.slope / 4.0, rtol=1e-12)
    npt.assert_array_equal(r2.r, r.r)
    with pytest.raises(XmhwException, match="standardize"):
        regress(point(y + 5.0), 5.0, {"x": x}, standardize=False)
    small = x / 400.0
    raw = regress(point(y + 5.0), 5.0, {"x": small}, standardize=False)
    assert abs(raw.slope[0, 0, 0] - want[0] * 400.0) <= raw.quantisation_bound()[0][0, 0, 0]


# ---- the derived fields ------------------------------------------------------------------------------

def _cells(ds):
    return [tuple(int(v) for v in c) for c in np.argwhere(ds.keep)]


def test_derived_fields_against_the_exact_rational_evaluation(driven):
    ds = regress(driven["temp"], driven["base"], driven["indices"], lags=(0, 20), classes="season")
    assert isinstance(ds, IndexRegressionDataset) and ds.slope.shape == (4, 2, 2, 5, 5) and ds.mean.shape == (4, 5, 5)
    assert ds.klass.tolist() == [0, 1, 2, 3] and ds.keep.shape == (5, 5) and 10 < ds.keep.sum() < 25
    kid, K = np.searchsorted(ds.klass, (driven["temp"].coords["time"].astype("datetime64[M]").astype(int) % 12 + 1) % 12 // 3), 4
    _, _, X = lagged_predictors(driven["indices"], (0, 20), driven["T"])
    kid, n_dropped, zq, means, scales = quantise_predictors(X, kid, True)
    assert n_dropped == ds.n_dropped == 20 + 2 + 2 and ds.n_steps.sum() == 900 - n_dropped
    checked = 0
    for k in range(K):
        for j in range(4):
            i, l = divmod(j, 2)
            tot = ro.class_totals(kid.tolist(), k, zq[:, j])
            for c in _cells(ds):
                at, at3 = (k,) + c, (k, i, l) + c
                # the inputs the tolerance is meant for: mean <= sd on both sides
                n = int(ds.n[at])
                ma, va = ds.sa[at] / n, ds.saa[at] / n - (ds.sa[at] / n) ** 2
                sz, szz = tot["Z"] - int(ds.mz[at3]), tot["ZZ"] - int(ds.mzz[at3])
                assert abs(ma) <= np.sqrt(va) and abs(sz / n) <= np.sqrt(szz / n - (sz / n) ** 2)
                want = ro.derived_exact(ds.n[at], ds.sa[at], ds.saa[at], ds.n1[at], ds.saa1[at], ds.saz[at3], ds.mz[at3],
                                        ds.mzz[at3], tot, means[i, l], scales[i, l])
                for name in ("slope", "intercept", "r", "n_eff"):
                    npt.assert_allclose(getattr(ds, name)[at3], want[name], rtol=1e-9, atol=1e-11, err_msg=name)
                for name in ("mean", "r1"):
                    npt.assert_allclose(getattr(ds, name)[at], want[name], rtol=1e-9, atol=1e-11, err_msg=name)
                npt.assert_allclose(ds.r1z[k, i, l], want["r1z"], rtol=1e-9, atol=1e-11)
                checked += 1
    assert checked == 16 * int(ds.keep.sum())
    # land: integers 0, floats NaN
    assert (ds.n[:, ~ds.keep] == 0).all() and (ds.saz[..., ~ds.keep] == 0).all()
    for name in ("mean", "slope", "intercept", "r", "r1", "n_eff", "p_value"):
        assert np.isnan(getattr(ds, name)[..., ~ds.keep]).all() and not np.isnan(getattr(ds, name)[..., ds.keep]).any(), name


def test_slope_and_r_against_numpy_on_the_unquantised_data(driven):
    ds = regress(driven["temp"], driven["base"], driven["indices"], lags=(0, 20))
    sb, rb = ds.quantisation_bound()
    assert sb.shape == ds.slope.shape and np.isinf(sb[..., ~ds.keep]).all()
    assert sb[..., ds.keep].max() < 1e-4 and rb[..., ds.keep].max() < 1e-4            # the bound is of the order of 2**-16
    _, _, X = lagged_predictors(driven["indices"], (0, 20), driven["T"])
    used = ~np.isnan(X).any(axis=(1, 2))
    x = driven["x"][:, [i for i in range(6) if i != 4]]                               # the dead grid line is dropped
    for c in _cells(ds):
        a = x[(slice(None),) + c] - driven["base"][[i for i in range(6) if i != 4]][c]
        ok = used & ~np.isnan(a)
        assert ok.sum() == ds.n[(0,) + c]
        for i in range(2):
            for l in range(2):
                slope, _ = np.polyfit(X[ok, i, l], a[ok], 1)
                r = np.corrcoef(X[ok, i, l], a[ok])[0, 1]
                at = (0, i, l) + c
                assert abs(ds.slope[at] - slope) <= sb[at], (at, ds.slope[at], slope, sb[at])
                assert abs(ds.r[at] - r) <= rb[at], (at, ds.r[at], r, rb[at])
    # the strong links are found where they were put: u at lag 0 and v at lag 20 beat the other lag
    strong = np.abs(ds.r[0][..., ds.keep])
    assert (strong[1, 1] > strong[1, 0]).mean() > 0.8


def test_effective_sample_size_and_p_value_directly(driven):
    ds = regress(driven["temp"], driven["base"], driven["indices"], lags=(0, 20), classes="season")
    K, I, L = ds.r.shape[:3]
    n = ds.n.astype(np.float64)[:, None, None]
    rr = ds.r1[:, None, None] * ds.r1z.reshape(K, I, L, 1, 1)
    with np.errstate(invalid="ignore"):
        want = np.clip(n * (1 - rr) / (1 + rr), 2.0, n * np.ones_like(rr))
    npt.assert_array_equal(ds.n_eff[..., ds.keep], want[..., ds.keep])
    assert (ds.n_eff[..., ds.keep] < n[..., ds.keep]).mean() > 0.9                  # autocorrelated on both sides: fewer
    assert 0.5 < np.nanmedian(ds.r1) < 1.0 and (ds.r1z > 0.5).all()
    p = ds.p_value
    assert p is ds.p_value
    for at in [tuple(int(v) for v in a) for a in np.argwhere(~np.isnan(ds.r))][::7]:
        dof = ds.n_eff[at] - 2.0
        t = abs(ds.r[at]) * np.sqrt(dof / (1.0 - ds.r[at] ** 2))
        assert p[at] == min(1.0, 2.0 * _t_sf(t, dof))
    assert ((p[..., ds.keep] >= 0) & (p[..., ds.keep] <= 1)).all() and (p[..., ds.keep] < 0.05).any() and (p[..., ds.keep] > 0.05).any()
    # with n - 2 degrees of freedom the same correlations would look far more significant
    at = tuple(int(v) for v in np.argwhere(~np.isnan(ds.r))[0])
    naive = 2.0 * _t_sf(abs(ds.r[at]) * np.sqrt((ds.n[at[:1] + at[3:]] - 2.0) / (1.0 - ds.r[at] ** 2)), ds.n[at[:1] + at[3:]] - 2.0)
    assert naive <= p[at]


def test_class_forms_partition_the_sums(driven):
    temp, base, ix = driven["temp"], driven["base"], driven["indices"]
    allc = regress(temp, base, ix, standardize=False)
    for classes in ("season", "month", "year", np.arange(900) % 3):
        r = regress(temp, base, ix, classes=classes, standardize=False)
        for k in ("n", "sa", "saa", "saz", "mz", "mzz"):
            npt.assert_array_equal(getattr(r, k).sum(axis=0), getattr(allc, k)[0], err_msg=k)
        assert (r.n1.sum(axis=0) <= allc.n1[0]).all()
    none = regress(temp, base, ix, classes=np.full(900, -1))
    assert none.klass.tolist() == [0] and (none.n == 0).all() and none.n_steps.tolist() == [0] and np.isnan(none.slope).all()
    t = class_totals(np.array([0, 0, -1, 0, 0, 0], np.int32), 1, np.arange(6, dtype=np.int32)[:, None])
    assert t["N"].tolist() == [5] and t["N1"].tolist() == [3] and t["Z01"][0, 0] == 0 * 1 + 3 * 4 + 4 * 5
    assert t["Z0"][0, 0] == 0 + 3 + 4 and t["Z1"][0, 0] == 1 + 4 + 5


def test_to_xarray(driven):
    pytest.importorskip("xarray")
    ds = regress(driven["temp"], driven["base"], driven["indices"], lags=(0, 20), classes="season").to_xarray()
    assert ds["slope"].dims == ("klass", "index", "lag", "lat", "lon") and ds["mean"].dims == ("klass", "lat", "lon")
    assert ds["p_value"].shape == ds["r"].shape and list(ds["index"].values) == ["u", "v"]


# ---- refusals ----------------------------------------------------------------------------------------

def test_host_refusals(driven):
    temp, base, ix = driven["temp"], driven["base"], driven["indices"]
    u = ix["u"]
    cases = [
        (dict(indices={}), "non-empty dict"), (dict(indices=[u]), "non-empty dict"),
        (dict(indices={"u": u[:-1]}), "one value per time step"), (dict(indices={"u": np.zeros((900, 2))}), "one value per time step"),
        (dict(indices={"u": np.where(np.arange(900) == 5, np.inf, 0.0)}), "infinite"),
        (dict(lags=(0.5,)), "whole numbers"), (dict(lags=()), "whole numbers"), (dict(lags=(3, 3)), "distinct"),
        (dict(lags=tuple(range(17))), "at most 32 predictors"),
        (dict(indices={"c": np.ones(900)}), "constant over the used steps"),
        (dict(indices={"big": 1000.0 * np.nan_to_num(u)}, standardize=False), "standardize=True"),
        (dict(classes="decade"), "classes should be"), (dict(classes=np.zeros(5, int)), "one entry per time step"),
        (dict(classes=np.arange(900) % 65), f"at most {MAX_CLASSES} classes"), (dict(tdim="t"), "dimension not present"),
        (dict(base=np.zeros(4)), "base should be"),
    ]
    for kw, text in cases:
        args = dict(temp=temp, base=base, indices=ix)
        args.update(kw)
        with pytest.raises(XmhwException, match=text):
            regress(**args)
    with pytest.raises(XmhwException, match="2\\*\\*7 and more from their base"):
        regress(temp, base - 273.15, ix)
    with pytest.raises(XmhwException, match="fewer than 2\\*\\*17 time steps"):
        regress(GridSeries(np.zeros(1 << 17), ("time",), {"time": np.arange(1 << 17)}), 0.0, {"x": np.arange(1 << 17)})
    # the stage-side check raises the same
    z = np.zeros((10, 1), np.int32)
    for args, text in [((10, np.full(10, 3), 2, z), "class labels should be in"), ((10, np.zeros(10, int), 65, z), "at most 64 classes"),
                       ((10, np.zeros(10, int), 1, np.zeros((10, 33), np.int32)), f"1 to {MAX_PREDICTORS} predictors"),
                       ((10, np.zeros(10, int), 1, np.zeros((10, 0), np.int32)), "1 to 32 predictors"),
                       ((10, np.zeros(10, int), 1, np.zeros((9, 1), np.int32)), "integer table"),
                       ((10, np.zeros(10, int), 1, np.zeros((10, 1))), "integer table"),
                       ((10, np.zeros(10, int), 1, np.full((10, 1), 1 << 23)), "inside \\(-2\\*\\*23, 2\\*\\*23\\)")]:
        with pytest.raises(XmhwException, match=text):
            check_regress_arguments(*args)


def test_c_entry_refusals_need_no_device_and_raise_the_exceptions_of_the_core_module():
    core = importlib.import_module("xmhw_amd._xmhw_hip")
    m = importlib.import_module("xmhw_amd._xmhw_hip_regress")
    assert not any(hasattr(m, n) for n in ("HipError", "Unsupported", "InvalidArgument", "CommError"))
    T = 10
    z, zq1 = np.zeros(T, np.int32), np.zeros((T, 1), np.int32)

    def acc(T=T, C=4, ld=4, ldb=4, D=1, rows=z, classes=z, K=1, zq=zq1, ldo=4, itemsize=4):
        m.index_regress_accumulate(0, itemsize, T, C, ld, 0, ldb, D, rows, classes, K, zq, 0, 0, 0, 0, 0, 0, 0, 0, ldo, 0)

    def init(K=1, J=1, C=4, ldo=4):
        m.index_regress_init(K, J, C, 0, 0, 0, 0, 0, 0, 0, 0, ldo, 0)

    long = (1 << 17)
    unsupported = [lambda: acc(K=0), lambda: acc(K=65), lambda: acc(zq=np.zeros((T, 0), np.int32)), lambda: acc(zq=np.zeros((T, 33), np.int32)),
                   lambda: acc(T=long, rows=np.zeros(long, np.int32), classes=np.zeros(long, np.int32), zq=np.zeros((long, 1), np.int32)),
                   lambda: acc(C=1 << 31, ld=1 << 31, ldb=1 << 31, ldo=1 << 31), lambda: init(K=0), lambda: init(K=65), lambda: init(J=0),
                   lambda: init(J=33)]
    for call in unsupported:
        with pytest.raises(core.Unsupported) as e:
            call()
        assert type(e.value) is core.Unsupported and isinstance(e.value, core.HipError) and "(code 3)" in str(e.value)
    # K is judged before J, as the header says
    with pytest.raises(core.Unsupported, match="K must be in"):
        acc(K=0, zq=np.zeros((T, 0), np.int32))
    invalid = [(lambda: acc(classes=np.full(T, 1, np.int32)), r"class_of_t outside \[-1, K\)"),
               (lambda: acc(classes=np.full(T, -2, np.int32)), r"class_of_t outside"),
               (lambda: acc(rows=np.full(T, 1, np.int32)), r"row_of_t outside \[0, D\)"),
               (lambda: acc(zq=np.full((T, 1), 1 << 23, np.int32)), "zq outside"),
               (lambda: acc(zq=np.full((T, 2), -(1 << 23), np.int32)), "zq outside"),
               (lambda: acc(ld=3), "bad T/C"), (lambda: acc(ldb=3), "bad T/C"), (lambda: acc(ldo=3), "bad T/C"), (lambda: acc(D=0), "bad T/C"),
               (lambda: acc(rows=np.zeros(T + 1, np.int32)), "row_of_t length"), (lambda: acc(classes=np.zeros(T - 1, np.int32)), "class_of_t length"),
               (lambda: acc(zq=np.zeros((T + 1, 1), np.int32)), r"zq must be a \(T, J\) table"), (lambda: acc(zq=np.zeros(T, np.int32)), "zq must be"),
               (lambda: acc(itemsize=2), "itemsize"), (lambda: acc(), "NULL buffer"),
               (lambda: init(ldo=3), "bad C/ldo"), (lambda: init(), "NULL"), (lambda: m.set_index_regress_block(-1), "steps must be")]
    for call, text in invalid:
        with pytest.raises(core.InvalidArgument, match=text) as e:
            call()
        assert type(e.value) is core.InvalidArgument
    # the largest zq and T that are taken; nothing is launched for C == 0: no device is needed either
    acc(C=0, ld=0, ldb=0, ldo=0, zq=np.full((T, 32), (1 << 23) - 1, np.int32))
    acc(C=0, ld=0, ldb=0, ldo=0, T=long - 1, rows=np.zeros(long - 1, np.int32), classes=np.zeros(long - 1, np.int32),
        zq=np.zeros((long - 1, 1), np.int32))
    m.set_index_regress_block(0)
    assert (m.INDEX_REGRESS_MAX_PREDICTORS, m.INDEX_REGRESS_MAX_CLASSES, m.INDEX_REGRESS_MAX_STEPS, m.INDEX_REGRESS_BITS,
            m.INDEX_REGRESS_RANGE_BITS, m.INDEX_REGRESS_PREDICTOR_BITS) == (32, 64, 1 << 17, 16, 7, 23)


def test_the_loader_wraps_the_regress_module_like_the_core_module():
    from xmhw_amd import _lib
    hr = _lib.hip_regress()
    assert isinstance(hr, _lib._RetryOnNoMem) and hr is _lib.hip_regress()
    assert hr.INDEX_REGRESS_MAX_PREDICTORS == 32 and callable(hr.index_regress_accumulate)
