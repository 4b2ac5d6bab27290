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
