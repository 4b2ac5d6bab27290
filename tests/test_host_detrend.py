"""Host logic of xmhw_amd.detrend without a GPU: the design matrix against closed forms, the exceptions, the
plumbing of detrend() and threshold_detect(detrend=...) around numpy stand-ins for the device stages, and the CPU
experiment the tolerances of tests/test_gpu_detrend.py come from."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import detrend_oracle as dor  # noqa: E402

import xmhw_amd  # noqa: E402
from xmhw_amd import GridSeries, XmhwException  # noqa: E402
import importlib  # noqa: E402
dmod = importlib.import_module("xmhw_amd.detrend")          # (xmhw_amd.detrend itself is the function)
from xmhw_amd.detrend import DetrendSpec, _detrend  # noqa: E402


def daily(a, b):
    return np.arange(a, b, dtype="datetime64[D]")


# ---- the design matrix ---------------------------------------------------------------------------------------------------
def test_terms_and_sizes():
    t = daily("1982-01-01", "1984-01-01")
    for order in (1, 2, 3):
        for harmonics in (0, 1, 2, 3):
            s = DetrendSpec(t, order, harmonics)
            assert s.P == order + 1 + 2 * harmonics == s.basis.shape[1] and s.R == order
            assert s.terms[:order] == [f"x{k}" for k in range(1, order + 1)] and s.terms[order] == "const"
            assert s.min_valid == s.P and s.weight.all() and s.all_steps
    assert DetrendSpec(t, 1, 2).terms == ["x1", "const", "cos1", "sin1", "cos2", "sin2"]
    assert DetrendSpec(t, min_valid=100).min_valid == 100 and DetrendSpec(t, min_valid=1).min_valid == 6


def test_basis_daily_closed_form():
    t = daily("1982-01-01", "2022-01-01")
    T = t.shape[0]
    assert T == 14610
    s = DetrendSpec(t, 3, 3)
    d = np.arange(T) - (T - 1) / 2.0                        # days since the midpoint of the first and last step
    np.testing.assert_array_equal(s.basis[:, 0], d / 3652.5)
    np.testing.assert_allclose(s.basis[:, 1], (d / 3652.5) ** 2, rtol=1e-15)
    np.testing.assert_allclose(s.basis[:, 2], (d / 3652.5) ** 3, rtol=1e-15)
    np.testing.assert_array_equal(s.basis[:, 3], 1.0)
    for h in (1, 2, 3):
        np.testing.assert_allclose(s.basis[:, 2 + 2 * h], np.cos(2 * np.pi * h * d / 365.25), atol=1e-13)
        np.testing.assert_allclose(s.basis[:, 3 + 2 * h], np.sin(2 * np.pi * h * d / 365.25), atol=1e-13)
    np.testing.assert_allclose(s.basis, dor.design(d, 3, 3), atol=1e-13)
    assert s.t_ref == np.datetime64("2001-12-31T12:00:00")


def test_removed_columns_are_zero_at_reference():
    t = daily("1982-01-01", "2022-01-01")
    s = DetrendSpec(t, 3, 2, reference="2000-01-01")
    k = int(np.nonzero(t == np.datetime64("2000-01-01"))[0][0])
    assert (s.basis[k, :3] == 0.0).all() and s.basis[k, 3] == 1.0 and s.basis[k, 4] == 1.0 and s.basis[k, 5] == 0.0
    np.testing.assert_array_equal(s.basis[:, 0], (np.arange(t.shape[0]) - k) / 3652.5)
    # odd length: the default reference is a step of the axis
    t2 = daily("1982-01-01", "1982-01-12")
    s2 = DetrendSpec(t2, 2, 0)
    assert (s2.basis[5, :2] == 0.0).all()


def test_basis_six_hourly():
    t = np.arange("2000-01-01", "2001-01-01", dtype="datetime64[6h]")
    s = DetrendSpec(t, 1, 1, reference="2000-01-01")
    d = np.arange(t.shape[0]) * 0.25
    np.testing.assert_array_equal(s.basis[:, 0], d / 3652.5)
    np.testing.assert_allclose(s.basis[:, 2], np.cos(2 * np.pi * d / 365.25), atol=1e-14)


def test_basis_numeric_axis():
    t = np.arange(0.5, 1000.5, 1.0)                         # days
    s = DetrendSpec(t, 2, 1, reference=100.5)
    np.testing.assert_array_equal(s.basis[:, 0], (t - 100.5) / 3652.5)
    np.testing.assert_allclose(s.basis[:, 4], np.sin(2 * np.pi * (t - 100.5) / 365.25), atol=1e-14)
    assert s.t_ref == 100.5 and (s.basis[100, :2] == 0).all()
    s = DetrendSpec(t, 1, 0, fitPeriod=[100, 200.5])        # coordinate bounds on a numeric axis
    assert s.weight.sum() == 101 and s.weight[100] and s.weight[200] and not s.weight[99] and not s.weight[201]
    assert s.x_ref == 150.5


class NoLeapDate:
    """a cftime-like date of the 365-day calendar: year / month / dayofyr, subtraction gives a timedelta"""
    calendar = "noleap"

    def __init__(self, n):
        self.n = n
        self.year, self.dayofyr = 2000 + n // 365, n % 365 + 1
        self.month = 1 + int(np.searchsorted(np.cumsum([31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31]), self.dayofyr - 1,
                                             side="right"))

    def __sub__(self, other):
        import datetime
        return datetime.timedelta(days=self.n - other.n)


def test_basis_noleap_axis():
    t = np.array([NoLeapDate(n) for n in range(3 * 365)], dtype=object)
    s = DetrendSpec(t, 1, 1)
    d = np.arange(3 * 365) - (3 * 365 - 1) / 2.0
    np.testing.assert_array_equal(s.basis[:, 0], d / 3652.5)
    np.testing.assert_allclose(s.basis[:, 2], np.cos(2 * np.pi * d / 365.25), atol=1e-14)
    s = DetrendSpec(t, 1, 0, fitPeriod=[2001, 2001])
    assert s.weight.sum() == 365 and s.weight[365] and not s.weight[364] and not s.weight[730]


def test_fit_period_years():
    t = daily("1982-01-01", "2022-01-01")
    s = DetrendSpec(t, 1, 2, fitPeriod=[1991, 2020])
    yrs = t.astype("datetime64[Y]").astype(int) + 1970
    np.testing.assert_array_equal(s.weight != 0, (yrs >= 1991) & (yrs <= 2020))
    assert not s.all_steps
    assert s.t_ref == np.datetime64("2005-12-31T12:00:00")   # midpoint of 1991-01-01 and 2020-12-31
    s = DetrendSpec(t, 1, 2, fitPeriod=[None, 1990])
    assert (s.weight != 0).sum() == int((yrs <= 1990).sum())


def test_exceptions():
    t = daily("1982-01-01", "1984-01-01")
    for bad in (0, 4, 1.5, True, "1"):
        with pytest.raises(XmhwException):
            DetrendSpec(t, order=bad)
    for bad in (-1, 4, 0.5, True):
        with pytest.raises(XmhwException):
            DetrendSpec(t, harmonics=bad)
    with pytest.raises(XmhwException):
        DetrendSpec(t, fitPeriod=[1990, 1995])               # empty
    with pytest.raises(XmhwException):
        DetrendSpec(t, fitPeriod=[1983, 1982])
    with pytest.raises(XmhwException):
        DetrendSpec(t[::-1])                                 # not monotonic
    with pytest.raises(XmhwException):
        DetrendSpec(np.concatenate([t[:5], t[4:9]]))         # duplicate step
    with pytest.raises(XmhwException):
        DetrendSpec(t[:0])
    with pytest.raises(XmhwException):
        DetrendSpec(t, min_valid=-1)
    with pytest.raises(XmhwException):
        DetrendSpec(t, reference="not a date")
    with pytest.raises(XmhwException):
        dmod.make_spec({"degree": 2}, t)
    with pytest.raises(XmhwException):
        dmod.make_spec(3, t)
    assert dmod.make_spec(None, t) is None and dmod.make_spec(True, t).P == 6
    assert dmod.make_spec({"order": 2, "harmonics": 0}, t).P == 3


# ---- detrend(): host plumbing around the stand-ins -----------------------------------------------------------------------
def make_grid(rng, dims=("time", "lat", "lon"), dtype=np.float32, nlat=3, nlon=4, years=3):
    t = daily("2000-01-01", f"{2000 + years}-01-01")
    d = np.arange(t.shape[0], dtype=np.float64)
    y = dor.sst_like(d, nlat * nlon, rng, dtype).reshape(t.shape[0], nlat, nlon)
    y[:, 1, 2] = np.nan                                     # land
    y[5:40, 0, 0] = np.nan                                  # a gap
    order = [("time", "lat", "lon").index(k) for k in dims]
    coords = {"time": t, "lat": np.arange(nlat) * 1.0, "lon": np.arange(nlon) * 2.0}
    return GridSeries(np.transpose(y, order), dims, coords, attrs={"units": "degC"}), y, t


def run(temp, **kw):
    return _detrend(temp, dor.standin_cells, grid_compute=dor.standin_grid, **kw)


def test_detrend_grid_plumbing():
    rng = np.random.default_rng(1)
    temp, y, t = make_grid(rng)
    out, fit = run(temp, order=1, harmonics=2)
    assert isinstance(out, GridSeries) and out.dims == temp.dims and out.values.shape == y.shape
    assert out.values.dtype == np.float32 and out.attrs == {"units": "degC"}
    assert np.isnan(out.values[:, 1, 2]).all() and np.isnan(fit.coef[:, 1, 2]).all() and fit.n_valid[1, 2] == 0
    assert fit.dims == ("lat", "lon") and fit.coef.shape == (6, 3, 4) and fit.n_failed == 0
    assert fit.n_valid[0, 0] == t.shape[0] - 35 and fit.n_valid[2, 3] == t.shape[0]
    assert np.isnan(out.values[5:40, 0, 0]).all() and not np.isnan(out.values[40:, 0, 0]).any()
    assert fit.terms == ["x1", "const", "cos1", "sin1", "cos2", "sin2"]
    np.testing.assert_array_equal(fit.trend_per_decade, fit["x1"])
    # one cell by hand
    s = DetrendSpec(t, 1, 2)
    beta, n, _ = dor.fit_cell(y[:, 2, 1], s.basis, s.weight, 6)
    np.testing.assert_array_equal(fit.coef[:, 2, 1], beta)
    np.testing.assert_array_equal(out.values[:, 2, 1], dor.remove_cell(y[:, 2, 1], s.basis, beta, 1).astype(np.float32))
    assert fit.t_ref == s.t_ref and fit.fit_period == (None, None)


def test_detrend_dims_order_and_host_compaction():
    rng = np.random.default_rng(2)
    temp, y, t = make_grid(rng, dims=("lon", "time", "lat"), dtype=np.float64)
    out, fit = run(temp, order=2, harmonics=1)
    assert out.dims == ("lon", "time", "lat") and out.values.shape == (4, t.shape[0], 3) and out.values.dtype == np.float64
    ref, fit_ref = run(GridSeries(y, ("time", "lat", "lon"), temp.coords), order=2, harmonics=1)
    np.testing.assert_array_equal(np.transpose(out.values, (1, 2, 0)), ref.values)
    np.testing.assert_array_equal(fit.coef, fit_ref.coef)
    assert fit.dims == ("lat", "lon")
    # without a grid stage the mask and the placement run in numpy: same result
    out2, fit2 = _detrend(temp, dor.standin_cells, order=2, harmonics=1)
    np.testing.assert_array_equal(out2.values, out.values)
    np.testing.assert_array_equal(fit2.coef, fit.coef)
    np.testing.assert_array_equal(fit2.n_valid, fit.n_valid)


def test_detrend_failed_cell_and_anynans():
    rng = np.random.default_rng(3)
    temp, y, t = make_grid(rng)
    v = temp.values.copy()
    v[:, 2, 2] = np.nan
    v[10:14, 2, 2] = 15.0                                   # four samples: not land, too few for six terms
    out, fit = run(GridSeries(v, temp.dims, temp.coords))
    assert fit.n_failed == 1 and fit.n_valid[2, 2] == 4
    assert np.isnan(out.values[:, 2, 2]).all() and np.isnan(fit.coef[:, 2, 2]).all()
    out, fit = run(GridSeries(v, temp.dims, temp.coords), anynans=True)
    assert fit.n_failed == 0 and np.isnan(out.values[:, 0, 0]).all() and fit.n_valid[0, 0] == 0


def test_detrend_point_and_errors():
    rng = np.random.default_rng(4)
    t = daily("2000-01-01", "2003-01-01")
    y = dor.sst_like(np.arange(t.shape[0]), 1, rng, np.float64, trend=0.3)[:, 0]
    out, fit = run(GridSeries(y, ("time",), {"time": t}))
    assert out.values.shape == y.shape and fit.coef.shape == (6,) and fit.n_valid.shape == () and fit.dims == ()
    assert abs(float(fit.trend_per_decade) - 0.3) < 2.0     # three noisy years: only that it is a number
    with pytest.raises(XmhwException):
        run(GridSeries(y, ("time",), {"time": t}), tdim="t")
    with pytest.raises(XmhwException):
        run(GridSeries(np.full((t.shape[0], 2), np.nan), ("time", "x"), {"time": t, "x": np.arange(2)}))
    # integer input: float64 output
    out, _ = run(GridSeries(np.arange(t.shape[0] * 2).reshape(-1, 2), ("time", "x"), {"time": t, "x": np.arange(2)}), harmonics=0)
    assert out.values.dtype == np.float64
    np.testing.assert_allclose(out.values[:, 0], out.values[(t.shape[0] - 1) // 2, 0], atol=1e-7)   # a pure line: flat


def test_detrend_xarray_if_present():
    xr = pytest.importorskip("xarray")
    rng = np.random.default_rng(5)
    temp, y, t = make_grid(rng)
    da = xr.DataArray(y, dims=("time", "lat", "lon"), coords=temp.coords, attrs={"units": "degC"})
    out, fit = run(da)
    ref, _ = run(temp)
    assert isinstance(out, xr.DataArray) and out.dims == da.dims and out.attrs == da.attrs
    np.testing.assert_array_equal(out.values, ref.values)
    ds = fit.to_xarray()
    assert ds["coef"].dims == ("term", "lat", "lon") and list(ds["term"].values) == fit.terms


def test_exported():
    assert xmhw_amd.detrend is dmod.detrend and xmhw_amd.DetrendSpec is DetrendSpec and xmhw_amd.FitDataset is dmod.FitDataset
    assert "detrend" in xmhw_amd.__all__


# ---- threshold_detect(detrend=...) ---------------------------------------------------------------------------------------
def test_threshold_detect_period_cut_raises():
    rng = np.random.default_rng(6)
    temp, _, _ = make_grid(rng, years=4)
    with pytest.raises(XmhwException, match=r"detrend\(temp, fitPeriod=\[2001, 2002\]\)"):
        xmhw_amd.threshold_detect(temp, climatologyPeriod=[2001, 2002], detrend=True)
    with pytest.raises(XmhwException, match="unknown arguments"):
        xmhw_amd.threshold_detect(temp, detrend={"degree": 1})
    with pytest.raises(XmhwException):
        xmhw_amd.threshold_detect(temp, detrend={"order": 7})
    with pytest.raises(XmhwException):                       # detect()'s own check still comes first
        xmhw_amd.threshold_detect(temp, detrend=True, maxGap=5, minDuration=5)


class RecordingSpec:
    """what the host stages hand to the device stage as ``pad`` when a DetrendSpec is present"""


def test_threshold_stage_receives_recipe():
    from xmhw_amd.api import _threshold
    from xmhw_amd.detrend import SeriesRecipe
    rng = np.random.default_rng(7)
    temp, y, t = make_grid(rng)
    spec = DetrendSpec(t)
    seen = {}

    def grid(stacked, doy, anynans, pctile, w, smooth, width, tstep, cold, pad=None):
        seen["pad"] = pad
        N = stacked.shape[1]
        return np.ones(N, dtype=bool), np.arange(1, 367), np.zeros((366, N)), np.zeros((366, N))

    clim = _threshold(temp, None, grid_compute=grid, detrend=spec)
    assert isinstance(seen["pad"], SeriesRecipe) and seen["pad"].spec is spec and seen["pad"].pad is None
    assert "order 1 polynomial" in clim.attrs["xmhw_detrend"] and "2 annual harmonics" in clim.attrs["xmhw_detrend"]
    clim = _threshold(temp, None, grid_compute=grid, detrend=spec, maxPadLength=np.timedelta64(3, "D"))
    assert seen["pad"].pad is not None and seen["pad"].pad.max_gap == 3 * 86400e9
    clim = _threshold(temp, None, grid_compute=grid)
    assert seen["pad"] is None and "xmhw_detrend" not in clim.attrs


# ---- where the tolerances of the GPU tests come from ------------------------------------------------------------------------
def kahan(terms):
    """compensated sum of the rows of `terms`, in order"""
    tot = np.zeros(terms.shape[1])
    comp = np.zeros(terms.shape[1])
    for row in terms:
        term = row - comp
        nxt = tot + term
        comp = (nxt - tot) - term
        tot = nxt
    return tot


def cholesky_solve(G, r, dtype=np.float64):
    G, r = G.astype(dtype), r.astype(dtype)
    P = r.shape[0]
    L = np.zeros((P, P), dtype)
    for j in range(P):
        L[j, j] = np.sqrt(G[j, j] - np.sum(L[j, :j] ** 2))
        for i in range(j + 1, P):
            L[i, j] = (G[i, j] - np.sum(L[i, :j] * L[j, :j])) / L[j, j]
    z = np.zeros(P, dtype)
    for i in range(P):
        z[i] = (r[i] - np.sum(L[i, :i] * z[:i])) / L[i, i]
    beta = np.zeros(P, dtype)
    for i in range(P - 1, -1, -1):
        beta[i] = (z[i] - np.sum(L[i + 1:, i] * beta[i + 1:])) / L[i, i]
    return beta


def restatement(y, B, w, plain=False):
    """The arithmetic of csrc/kernels_fit.hip in float64 numpy (all steps weighted): r summed over the eight rows of a
    batch from 0.0 (a NaN enters as 0.0), each batch joined by a compensated add; Gfull a compensated sum; G = Gfull
    less the plainly summed outer products of the missing steps, or -- more missing than valid -- a compensated
    sum over the valid steps; Cholesky, two triangular solves.  ``plain``: running sums without any compensation,
    what the kernels did at first."""
    assert (np.asarray(w) != 0).all()
    T, P = B.shape
    valid = ~np.isnan(y)
    y0 = np.where(valid, y.astype(np.float64), 0.0)
    outer = (B[:, :, None] * B[:, None, :]).reshape(T, P * P)
    if plain:
        G = np.cumsum(outer[valid], axis=0)[-1].reshape(P, P)                # cumsum adds in order
        r = np.cumsum(B[valid] * y0[valid, None], axis=0)[-1]
        return cholesky_solve(G, r)
    terms = B * y0[:, None]
    pad = (-T) % 8
    terms = np.concatenate([terms, np.zeros((pad, P))]).reshape(-1, 8, P)
    part = np.zeros((terms.shape[0], P))
    for u in range(8):
        part = part + terms[:, u]
    r = kahan(part)
    n = int(valid.sum())
    if T - n > n:
        G = kahan(outer[valid])
    else:
        A = np.zeros(P * P)
        for row in outer[~valid]:
            A = A + row
        G = kahan(outer) - A
    return cholesky_solve(G.reshape(P, P), r)


@pytest.mark.parametrize("T,order,harmonics,nan_frac", [(14610, 1, 0, 0.0), (14610, 1, 2, 0.05), (4383, 3, 2, 0.3),
                                                         (730, 3, 3, 0.05), (730, 3, 0, 0.3), (730, 3, 3, 0.6),
                                                         (14610, 3, 3, 0.3)])
def test_normal_equations_against_lstsq_on_the_cpu(T, order, harmonics, nan_frac):
    """The experiment behind the 1e-11 * max|y| tolerance of tests/test_gpu_detrend.py, on SST-like float32 data: the
    kernels' arithmetic restated in numpy against the oracle's lstsq, held to that tolerance (raw coefficients and
    detrended values), and the detrended float32 samples to the 1e-4 cap.  Printed beside it: the same with plain
    running sums, which on the two-year axis miss the tolerance in the x^3 coefficient (x in decades: the column has
    an rms of 4e-4 and its coefficient is of the order of 1e3 K) -- the reason the kernels compensate their sums."""
    rng = np.random.default_rng(T + 10 * order + harmonics)
    C = 6
    d = np.arange(T, dtype=np.float64)
    y = dor.sst_like(d, C, rng, np.float32)
    y[rng.random(y.shape) < nan_frac] = np.nan
    B = dor.design(d - (T - 1) / 2.0, order, harmonics)
    w = np.ones(T, dtype=np.uint8)
    worst_c = worst_v = worst_p = 0.0
    differ = 0
    for c in range(C):
        beta, n, ratio = dor.fit_cell(y[:, c], B, w, B.shape[1])
        assert ratio > 1e-3
        mine = restatement(y[:, c], B, w)
        scale = np.nanmax(np.abs(y[:, c]))
        worst_c = max(worst_c, np.max(np.abs(mine - beta)) / scale)
        worst_p = max(worst_p, np.max(np.abs(restatement(y[:, c], B, w, plain=True) - beta)) / scale)
        a, b = dor.remove_cell(y[:, c], B, mine, order), dor.remove_cell(y[:, c], B, beta, order)
        worst_v = max(worst_v, np.nanmax(np.abs(a - b)) / scale)
        ok = ~np.isnan(a)
        differ += int((a.astype(np.float32)[ok] != b.astype(np.float32)[ok]).sum())
    print(f"T={T} P={B.shape[1]} {nan_frac:.0%} NaN: coefficient error {worst_c:.2e} (plain running sums: {worst_p:.2e}), "
          f"value error {worst_v:.2e} of max|y|; {differ} float32 samples differ")
    assert worst_c <= 1e-11 and worst_v <= 1e-11
    assert differ <= 1e-4 * C * T


def long_double_solution(B, y):
    """the least-squares solution in numpy.longdouble: columns scaled to unit norm, modified Gram-Schmidt twice"""
    L = np.longdouble
    B, y = B.astype(L), y.astype(L)
    norm = np.sqrt((B * B).sum(axis=0))
    Q = B / norm
    P = B.shape[1]
    R = np.zeros((P, P), L)
    for j in range(P):
        for _ in range(2):
            for i in range(j):
                h = (Q[:, i] * Q[:, j]).sum()
                R[i, j] += h
                Q[:, j] -= h * Q[:, i]
        R[j, j] = np.sqrt((Q[:, j] ** 2).sum())
        Q[:, j] /= R[j, j]
    z = Q.T @ y
    beta = np.zeros(P, L)
    for i in range(P - 1, -1, -1):
        beta[i] = (z[i] - (R[i, i + 1:] * beta[i + 1:]).sum()) / R[i, i]
    return beta / norm


@pytest.mark.skipif(np.finfo(np.longdouble).eps > 1e-18, reason="numpy.longdouble is no wider than float64 here")
def test_oracle_resolves_its_tolerance_against_long_double():
    """Why the oracle scales the columns by powers of two before lstsq: on the two-year axis plain float64 lstsq owes
    the columns' units an error in the x^3 coefficient of the size of the tolerance it is the reference for (printed).
    Asserted against a long-double solve: the scaled lstsq stays within half of 1e-11 max|y|, so that a reference
    error and an equal error of the code under test still fit the tolerance together."""
    T = 730
    d = np.arange(T, dtype=np.float64)
    worst_scaled = worst_plain = 0.0
    for order, harmonics in ((3, 0), (3, 3)):
        B = dor.design(d - (T - 1) / 2.0, order, harmonics)
        for seed in range(3):
            rng = np.random.default_rng(seed)
            y = dor.sst_like(d, 4, rng, np.float32)
            y[rng.random(y.shape) < 0.05] = np.nan
            for c in range(4):
                ok = ~np.isnan(y[:, c])
                yy = y[ok, c].astype(np.float64)
                exact = long_double_solution(B[ok], yy)
                scale = np.abs(yy).max()
                beta, _, _ = dor.fit_cell(y[:, c], B, np.ones(T, np.uint8), B.shape[1])
                plain = np.linalg.lstsq(B[ok], yy, rcond=None)[0]
                worst_scaled = max(worst_scaled, float(np.max(np.abs(beta - exact))) / scale)
                worst_plain = max(worst_plain, float(np.max(np.abs(plain - exact))) / scale)
    print(f"two-year cubic, against long double: lstsq {worst_plain:.2e}, lstsq on scaled columns {worst_scaled:.2e} of max|y|")
    assert worst_scaled <= 5e-12
