"""The vectorised oracle must reproduce the dumb oracle (which is pinned to the
reference fixtures) including NaN samples, empty pools and the tstep path."""
import numpy as np
import numpy.testing as npt
import pytest

import xmhw_oracle as ora
import oracle_fast as fast


def _series(T, C, seed, nanfrac=0.0, dtype=np.float32):
    rng = np.random.default_rng(seed)
    t = np.arange(T)[:, None]
    x = 15 + rng.uniform(2, 10, C) * np.sin(2 * np.pi * (t - rng.uniform(0, 365, C)) / 365.25) \
        + rng.normal(size=(T, C))
    x = x.astype(dtype)
    if nanfrac:
        x[rng.random((T, C)) < nanfrac] = np.nan
    return x


@pytest.mark.parametrize("smooth", [False, True])
@pytest.mark.parametrize("nanfrac", [0.0, 0.07])
def test_fast_matches_dumb_daily(smooth, nanfrac):
    time = np.arange("2001-01-01", "2005-01-01", dtype="datetime64[D]")   # 2004 is leap
    doy = ora.add_doy(time)
    x = _series(time.shape[0], 6, 3, nanfrac)
    d0, t0, s0 = ora.threshold_cells(x, doy, smoothPercentile=smooth, windowHalfWidth=5)
    d1, t1, s1 = fast.threshold_cells_fast(x, doy, smoothPercentile=smooth, windowHalfWidth=5)
    npt.assert_array_equal(d0, d1)
    npt.assert_allclose(t1, t0, rtol=1e-13, atol=0, equal_nan=True)
    npt.assert_allclose(s1, s0, rtol=1e-13, atol=0, equal_nan=True)


def test_fast_matches_dumb_absent_groups():
    """A cell that is NaN for a whole season has no group for those doys: the
    per-cell series is shorter and the smoothing rolls across the gap."""
    time = np.arange("2001-01-01", "2004-01-01", dtype="datetime64[D]")
    doy = ora.add_doy(time)
    x = _series(time.shape[0], 3, 5).astype(np.float64)
    x[(doy >= 150) & (doy <= 230), 1] = np.nan
    d0, t0, s0 = ora.threshold_cells(x, doy, windowHalfWidth=3, smoothPercentileWidth=11, pctile=75)
    d1, t1, s1 = fast.threshold_cells_fast(x, doy, windowHalfWidth=3, smoothPercentileWidth=11, pctile=75)
    assert np.isnan(t0[:, 1]).sum() > 50 and np.isfinite(t0[:, 0]).all()
    npt.assert_allclose(t1, t0, rtol=1e-13, equal_nan=True)
    npt.assert_allclose(s1, s0, rtol=1e-13, equal_nan=True)


def test_fast_matches_dumb_tstep_and_cold():
    T, n = 5 * 73, 73
    doy = np.tile(np.arange(1, n + 1), 5)
    x = _series(T, 4, 7, 0.02)
    d0, t0, s0 = ora.threshold_cells(x, doy, tstep=True, windowHalfWidth=2,
                                     smoothPercentileWidth=5, coldSpells=True, pctile=10)
    d1, t1, s1 = fast.threshold_cells_fast(x, doy, tstep=True, windowHalfWidth=2,
                                           smoothPercentileWidth=5, coldSpells=True, pctile=10)
    npt.assert_array_equal(d0, np.arange(1, n + 1))
    npt.assert_allclose(t1, t0, rtol=1e-13, equal_nan=True)
    npt.assert_allclose(s1, s0, rtol=1e-13, equal_nan=True)


def test_percell_baseline_matches_dumb():
    import oracle_percell as opc
    time = np.arange("2001-01-01", "2005-01-01", dtype="datetime64[D]")
    doy = ora.add_doy(time)
    x = _series(time.shape[0], 5, 31, 0.05)
    x[(doy >= 100) & (doy <= 140), 2] = np.nan
    for kw in (dict(), dict(smoothPercentile=False, skipna=True), dict(coldSpells=True, pctile=10, windowHalfWidth=2)):
        d0, t0, s0 = ora.threshold_cells(x, doy, **kw)
        d1, t1, s1 = opc.threshold_cells_percell(x, doy, **kw)
        npt.assert_array_equal(d0, d1)
        npt.assert_array_equal(t1, t0)
        npt.assert_array_equal(s1, s0)


@pytest.mark.parametrize("negate", [False, True])
@pytest.mark.parametrize("scale,offset,fill", [(0.01, 1.5, -32768), (-0.0021973, 0.3, 0), (0.5, -7.25, None)])
def test_packed_mean_f64_is_the_mean_of_the_decoded_series(negate, scale, offset, fill):
    """oracle_fast.packed_mean_f64 (the restatement of the int16 kernels' float64 mean: exact sum of codes, one
    division, decode) against raw_clim's mean of numpy's float64 decode, within rounding; NaN where raw_clim has NaN"""
    rng = np.random.default_rng(17)
    time = np.arange("2001-01-01", "2013-01-01", dtype="datetime64[D]")
    doy = ora.add_doy(time)
    T, C = time.shape[0], 9
    codes = rng.integers(-32768, 32768, size=(T, C)).astype(np.int16)
    codes[:, 2] = rng.integers(-300, 300, size=T)            # values near 0: the atol
    if fill is not None:
        codes[rng.random((T, C)) < 0.05] = fill
        codes[:, 4] = fill
        codes[(doy >= 100) & (doy <= 120), 5] = fill
    x = codes.astype(np.float64) * scale + offset
    if fill is not None:
        x[codes == fill] = np.nan
    _, _, se = fast.raw_clim(-x if negate else x, doy, 0.9, 5)
    got = fast.packed_mean_f64(codes, doy, 5, scale, offset, fill=fill, negate=negate)
    npt.assert_array_equal(np.isnan(got), np.isnan(se))
    amax = np.nanmax(np.abs(x))
    npt.assert_allclose(got, se, rtol=1e-12, atol=1e-13 * amax)
    if fill is not None:
        assert np.isnan(got[:, 4]).all() and np.isnan(got[105 - 1, 5])


def _dyadic(rng, shape):
    """values k/64 with |k| < 2**19: every window sum of up to 45 of them (and of the Feb-29 means that
    oracle_fast.dyadic_feb29 makes k/64 too) is exact in float64"""
    return rng.integers(-(2 ** 19) + 1, 2 ** 19, size=shape) / 64.0


def _nan_patterns(rng, D):
    """NaN masks of one column: none, all, one present, runs across the wrap, single rows, random"""
    pats = [np.zeros(D, bool), np.ones(D, bool)]
    one = np.ones(D, bool)
    one[rng.integers(D)] = False
    pats.append(one)
    wrap = np.zeros(D, bool)
    wrap[-min(5, D - 1):] = True
    wrap[:min(4, D - 1)] = True
    pats.append(wrap)
    for r in (0, D - 1, min(59, D - 1)):
        p = np.zeros(D, bool)
        p[r] = True
        pats.append(p)
    for frac in (0.05, 0.5, 0.9):
        pats.append(rng.random(D) < frac)
    return pats


@pytest.mark.parametrize("D", [1, 5, 12, 61, 63, 100, 366])
def test_finish_exact_is_finish_cell_on_dyadic_data(D):
    """On data whose every sum is exact, oracle_fast.finish_exact (math.fsum) and finish_cell (numpy) compute the same
    thing the same way: bit for bit, NaN positions included, for feb29 on/off, smoothing off and widths 1 .. 45"""
    rng = np.random.default_rng(D)
    doys = np.arange(1, D + 1)
    for pat in _nan_patterns(rng, D):
        col = _dyadic(rng, D)
        col[pat] = np.nan
        for feb29_fix in (False, True):
            c = fast.dyadic_feb29(doys, col[:, None].copy())[:, 0] if feb29_fix else col
            for smooth, width in [(False, 31)] + [(True, w) for w in range(1, 46, 2)]:
                want = fast.finish_cell(doys, c, not feb29_fix, smooth, width)
                got, M = fast.finish_exact(doys, c, feb29_fix, smooth, width)
                npt.assert_array_equal(got, want)
                got2, M2 = fast.finish_exact(doys, c, feb29_fix, smooth, width, dyadic=True)
                npt.assert_array_equal(got2, want)
                npt.assert_array_equal(M2, M)
                npt.assert_array_equal(np.isnan(M), pat)


def test_finish_exact_feb29_row_is_the_exact_mean():
    """the 3-point Feb-29 mean of the present rows 59/60/61, from one rounding of the exact sum"""
    doys = np.arange(1, 367)
    col = np.full(366, 1.0)
    col[58], col[59], col[60] = 1e16, 1.0, -1e16          # numpy: (1e16 + 1) - 1e16 = 0
    got, _ = fast.finish_exact(doys, col, True, False, 1)
    assert got[59] == 1.0 / 3
    col[60] = np.nan                                         # 61 absent: the mean of two
    got, _ = fast.finish_exact(doys, col, True, False, 1)
    assert got[59] == (1e16 + 1.0) / 2 and np.isnan(got[60])
    col[58] = np.inf
    got, _ = fast.finish_exact(doys, col, True, True, 3)
    assert got[59] == np.inf and got[58] == np.inf and got[61] == np.inf and got[57] == np.inf


def test_finish_exact_infinities_follow_numpy_mean():
    """a window with +inf (-inf) is +inf (-inf), with both NaN; math.fsum is never handed inf - inf"""
    doys = np.arange(1, 21)
    col = np.arange(20.0)
    col[3], col[6] = np.inf, -np.inf
    col[10] = np.nan
    for width in (1, 3, 5, 7, 9, 25):
        want = fast.finish_cell(doys, col, True, True, width)
        got, M = fast.finish_exact(doys, col, False, True, width)
        npt.assert_array_equal(np.isnan(got), np.isnan(want))
        npt.assert_array_equal(got[np.isinf(want)], want[np.isinf(want)])
        fin = np.isfinite(want)
        npt.assert_allclose(got[fin], want[fin], rtol=1e-15)
        assert np.isfinite(M[~np.isnan(col)]).all()
    got, _ = fast.finish_exact(doys, col, False, True, 5)
    assert np.isnan(got[4]) and np.isnan(got[5]) and got[2] == np.inf and got[8] == -np.inf and np.isnan(got[10])


@pytest.mark.parametrize("kind", ["arctic", "anomaly", "kelvin"])
def test_finish_exact_bounds_finish_cell_on_float_data(kind):
    """On ordinary float data the numpy restatement (pairwise sums) stays within 4 eps M of the exact one: M is a
    scale that holds for mixed-sign data, where a relative tolerance means nothing"""
    rng = np.random.default_rng({"arctic": 1, "anomaly": 2, "kelvin": 3}[kind])
    eps = np.finfo(np.float64).eps
    worst = 0.0
    for D in (12, 63, 366, 1460):
        doys = np.arange(1, D + 1)
        t = np.arange(D)
        for _ in range(6):
            if kind == "arctic":
                col = 0.6 + 2.4 * np.sin(2 * np.pi * (t - rng.uniform(0, D)) / D) + 0.3 * rng.normal(size=D)
                col = np.clip(col, -1.8, 3.0)
            elif kind == "anomaly":
                col = rng.normal(size=D) * rng.uniform(0.1, 3)
            else:
                col = 273.0 + 2 * np.sin(2 * np.pi * t / D) + rng.normal(size=D) * 0.1
            col[rng.random(D) < rng.choice([0.0, 0.1, 0.6])] = np.nan
            for feb29_fix in (False, True):
                for width in (1, 5, 11, 31, 33, 45):
                    want = fast.finish_cell(doys, col, not feb29_fix, True, width)
                    got, M = fast.finish_exact(doys, col, feb29_fix, True, width)
                    npt.assert_array_equal(np.isnan(got), np.isnan(want))
                    ok = ~np.isnan(got)
                    err = np.abs(got[ok] - want[ok]) / (eps * M[ok])
                    assert (err <= 4).all(), (D, width, feb29_fix, err.max())
                    worst = max(worst, float(err.max(initial=0)))
    assert worst > 0          # the two do differ somewhere: the comparison is not vacuous
