"""mean_trend() on the device (csrc/kernels_trend.hip) against the numpy definition (tests/trend_oracle.py), bit
for bit and for both kernels: the golden cases, synthetic planes of every block count around the kernels' LDS
classes and every cell count around a tile, heavy ties, all-equal and monotone series, signed zeros, every NaN
pattern, +-Inf, magnitudes from 1e-300 to 1e300, non-default leading dimensions with canary columns, the cap on
the block count, run-to-run identity, threshold() -> detect() -> block_average() -> mean_trend(), and a
200,000-column case."""
import os

import numpy as np
import numpy.testing as npt
import pytest

import trend_oracle as to
from xmhw_amd import XmhwException
from xmhw_amd import trend as tr

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
METHODS = ("ols", "theil_sen")


@pytest.fixture(scope="module")
def gpu():
    from xmhw_amd._lib import require_gpu
    require_gpu()
    return tr


def same(got, want, what=""):
    """bit-for-bit equality, NaN where NaN"""
    assert got.shape == want.shape, what
    npt.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=what)
    ok = ~np.isnan(want)
    npt.assert_array_equal(np.ascontiguousarray(got[ok]).view(np.uint64), np.ascontiguousarray(want[ok]).view(np.uint64),
                           err_msg=what)


def abscissa(nb, step=1):
    return tr.centred_years(1982.0 + step * np.arange(nb))


def check(gpu, planes, x=None, alpha=0.05):
    nb = planes.shape[1]
    x = abscissa(nb) if x is None else x
    tc = tr.tcrit_table(alpha, nb)
    for method in METHODS:
        got = gpu.trend_device(planes, x, tc, method)
        want = to.trend_oracle(planes, x, tc, method)
        same(got, want, f"{method} {planes.shape}")
    return want


def synth(nstat, nb, C, seed):
    """statistic s cycles through: integers 0-3 (heavy ties), normal, counts with a trend, signed zeros and small
    integers, magnitudes over 600 decades, monotone; NaN patterns per column: none, sparse, half, all, one valid,
    two valid; some +-Inf"""
    rng = np.random.default_rng(seed)
    p = np.empty((nstat, nb, C))
    ramp = np.arange(nb, dtype=np.float64)[:, None]
    for s in range(nstat):
        k = s % 6
        if k == 0:
            v = rng.integers(0, 4, (nb, C)).astype(np.float64)
        elif k == 1:
            v = rng.normal(size=(nb, C)) * 3 + 20
        elif k == 2:
            v = rng.poisson(2.0, (nb, C)) + np.floor(ramp / 7)
        elif k == 3:
            v = rng.integers(-1, 2, (nb, C)).astype(np.float64)
            z = v == 0
            v[z] = np.where(rng.random(int(z.sum())) < 0.5, -0.0, 0.0)
        elif k == 4:
            v = rng.normal(size=(nb, C)) * 10.0 ** rng.integers(-300, 301, (nb, C))
        else:
            v = np.where(rng.random(C) < 0.5, 1.0, -1.0) * (ramp * rng.uniform(0.1, 3, C) + rng.normal(size=C))
        p[s] = v
    if nb:
        pat = rng.integers(0, 8, C)
        p[:, :, pat == 1] = np.where(rng.random((nstat, nb, int((pat == 1).sum()))) < 0.1, np.nan, p[:, :, pat == 1])
        p[:, :, pat == 2] = np.where(rng.random((nstat, nb, int((pat == 2).sum()))) < 0.5, np.nan, p[:, :, pat == 2])
        p[:, :, pat == 3] = np.nan                                           # land
        for c in np.nonzero(pat == 4)[0]:                                    # a single valid block
            keep = p[:, rng.integers(0, nb), c].copy()
            b = rng.integers(0, nb)
            p[:, :, c] = np.nan
            p[:, b, c] = keep
        for c in np.nonzero(pat == 5)[0]:                                    # two valid blocks
            if nb >= 2:
                b = rng.choice(nb, 2, replace=False)
                keep = p[:, b, c].copy()
                p[:, :, c] = np.nan
                p[:, b, c] = keep
        inf = np.nonzero(rng.random(C) < 0.03)[0]
        for c in inf:
            p[rng.integers(0, nstat), rng.integers(0, nb), c] = rng.choice([np.inf, -np.inf])
        if C > 9:
            p[:, :, 7] = 3.0                                                 # all equal
            p[:, :, 8] = ramp[:, 0]                                             # strictly increasing: mk_s = N
            p[:, :, 9] = -ramp[:, 0] ** 2                                       # strictly decreasing: mk_s = -N
    return p


def test_golden_cases(gpu):
    g = np.load(os.path.join(GOLD, "trend_cases.npz"))
    y = g["y"]
    x = tr.centred_years(g["years"])
    want = check(gpu, y[None], x)
    ts = gpu.trend_device(y[None], x, None, "theil_sen")[:, 0]
    npt.assert_array_equal(ts[0], g["ts_trend_s_var"][0])
    npt.assert_array_equal(ts[2:], g["ts_trend_s_var"][1:])
    ols = gpu.trend_device(y[None], x, tr.tcrit_table(0.05, y.shape[0]), "ols")[:, 0]
    npt.assert_allclose(ols[:2], g["ols_mean_trend"], rtol=1e-12, atol=1e-13)
    assert want.shape == (4, 1, y.shape[1])


@pytest.mark.parametrize("nb", [0, 1, 2, 3, 4, 5, 7, 8, 31, 40, 41, 64, 85, 128])
def test_block_counts(gpu, nb):
    for C, nstat in ((1, 1), (63, 2), (64, 3), (65, 6), (1000, 7)):
        if nb >= 85 and C == 1000:
            nstat = 6
        check(gpu, synth(nstat, nb, C, seed=nb * 10007 + C))


@pytest.mark.parametrize("nb,nstat", [(5, 22), (40, 22), (128, 2)])
def test_4097_cells(gpu, nb, nstat):
    check(gpu, synth(nstat, nb, 4097, seed=nb + nstat), abscissa(nb, step=3))


def test_monotone_and_equal_series(gpu):
    for nb in (3, 40, 128):
        p = synth(3, nb, 16, seed=nb)
        want = check(gpu, p)
        N = nb * (nb - 1) // 2
        ts = gpu.trend_device(p, abscissa(nb), None, "theil_sen")
        npt.assert_array_equal(ts[2, :, 8], N)
        npt.assert_array_equal(ts[2, :, 9], -N)
        npt.assert_array_equal(ts[2:, :, 7], 0)
        npt.assert_array_equal(ts[0, :, 8], 1.0)
        npt.assert_array_equal(ts[3, :, 8], nb * (nb - 1) * (2 * nb + 5) / 18.0)
        assert want.shape == (4, 3, 16)


def test_leading_dimensions_and_canaries(gpu):
    """ld and ldo wider than C: the input's padding columns hold values that must not be read into any result, the
    output's padding columns a sentinel that must stay"""
    from xmhw_amd._lib import hip
    from xmhw_amd.device import DeviceBuffer
    h = hip()
    nstat, nb, C, ld, ldo = 5, 40, 77, 91, 80
    p = synth(nstat, nb, C, seed=9)
    x = abscissa(nb)
    tc = tr.tcrit_table(0.05, nb)
    wide = np.full((nstat, nb, ld), 1e30)
    wide[:, :, :C] = p
    bufs = []
    try:
        d_in = DeviceBuffer.from_array(wide); bufs.append(d_in)
        d_x = DeviceBuffer.from_array(x); bufs.append(d_x)
        d_t = DeviceBuffer.from_array(tc); bufs.append(d_t)
        for method, nwhat in (("ols", 3), ("theil_sen", 4)):
            d_out = DeviceBuffer.from_array(np.full((nwhat, nstat, ldo), 12345.5)); bufs.append(d_out)
            if method == "ols":
                h.block_trend_ols(d_in.ptr, nstat, nb, C, ld, d_x.ptr, d_t.ptr, d_out.ptr, ldo)
            else:
                h.block_trend_theil_sen(d_in.ptr, nstat, nb, C, ld, d_x.ptr, d_out.ptr, ldo)
            h.stream_sync(0)
            got = d_out.to_array((nwhat, nstat, ldo), np.float64)
            same(got[:, :, :C], to.trend_oracle(p, x, tc, method), method)
            npt.assert_array_equal(got[:, :, C:], 12345.5)
    finally:
        for b in bufs:
            b.free()


def test_cap_and_refusals(gpu):
    from xmhw_amd import BlockDataset, mean_trend
    from xmhw_amd._lib import hip
    from xmhw_amd.device import DeviceBuffer
    h = hip()
    d = DeviceBuffer(8 * 4 * 129 * 4)
    try:
        with pytest.raises(h.HipError, match=r"cap of 128.*code 3"):          # XMHW_ERR_UNSUPPORTED
            h.block_trend_theil_sen(d.ptr, 1, 129, 4, 4, d.ptr, d.ptr, 4)
        with pytest.raises(h.InvalidArgument, match="ld must"):
            h.block_trend_theil_sen(d.ptr, 1, 40, 4, 3, d.ptr, d.ptr, 4)
        with pytest.raises(h.InvalidArgument, match="ldo"):
            h.block_trend_ols(d.ptr, 1, 40, 4, 4, d.ptr, d.ptr, d.ptr, 3)
        with pytest.raises(h.InvalidArgument, match="NULL"):
            h.block_trend_ols(0, 1, 40, 4, 4, d.ptr, d.ptr, d.ptr, 4)
        with pytest.raises(h.InvalidArgument, match="tcrit"):
            h.block_trend_ols(d.ptr, 1, 40, 4, 4, d.ptr, 0, d.ptr, 4)
        with pytest.raises(h.InvalidArgument, match="nstat"):
            h.block_trend_theil_sen(d.ptr, -1, 40, 4, 4, d.ptr, d.ptr, 4)
        h.block_trend_ols(0, 0, 40, 4, 4, 0, 0, 0, 4)                          # nothing to do
        h.block_trend_theil_sen(0, 3, 40, 0, 0, 0, 0, 0)
    finally:
        d.free()
    years = np.arange(1900, 2029)
    blk = BlockDataset({"ecount": np.zeros((129, 2))}, ("years", "cell"), {"years": years, "cell": np.arange(2)},
                       np.arange(1900, 2030))
    with pytest.raises(XmhwException, match="at most 128 blocks"):
        mean_trend(blk, method="theil_sen")
    with pytest.raises(XmhwException, match="at most 128 blocks"):
        gpu.trend_device(np.zeros((1, 129, 2)), abscissa(129), None, "theil_sen")
    res = mean_trend(blk, method="ols")                                      # no cap on the OLS path
    npt.assert_array_equal(res["trend"]["ecount"], 0.0)


def test_run_to_run(gpu):
    p = synth(22, 40, 3000, seed=77)
    x = abscissa(40)
    tc = tr.tcrit_table(0.05, 40)
    for method in METHODS:
        a = gpu.trend_device(p, x, tc, method)
        b = gpu.trend_device(p, x, tc, method)
        npt.assert_array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.parametrize("cold", [False, True])
def test_oisst_end_to_end(gpu, cold):
    import xmhw_amd
    from xmhw_amd import GridSeries, climatology_series
    g = np.load(os.path.join(GOLD, "oisst_2003_2004.npz"))
    time = np.datetime64("2003-01-01") + g["time"].astype("timedelta64[D]")
    temp = GridSeries(g["sst"], ("time", "lat", "lon"), {"time": time, "lat": g["lat"], "lon": g["lon"]},
                      time_encoding={"calendar": "proleptic_gregorian"})
    clim = xmhw_amd.threshold(temp, pctile=80, coldSpells=cold)
    mhw, inter = xmhw_amd.detect(temp, climatology_series(clim, "thresh"), climatology_series(clim, "seas"),
                                 coldSpells=cold, intermediate=True)
    assert mhw.n_events > 20
    # monthly-length blocks do not exist: the fixture's two years are two yearly blocks; a second BlockDataset on the
    # same events with the period stretched to five years gives five blocks (three of them without events)
    for blk in (xmhw_amd.block_average(mhw, dstime=inter, blockLength=1),
                xmhw_amd.block_average(mhw, period=[2001, 2005], blockLength=1)):
        assert blk.dims == ("years", "lat", "lon")
        for method in METHODS:
            got = xmhw_amd.mean_trend(blk, method=method)
            want = xmhw_amd.mean_trend(blk, method=method, _compute=to.trend_oracle)
            assert got.dims == want.dims == ("lat", "lon") and tuple(got.keys()) == tr.WHAT[method]
            for what in want.keys():
                assert set(got[what]) == set(blk.data_vars)
                for k in want[what]:
                    same(got[what][k], want[what][k], f"{method} {what} {k}")
        assert np.isfinite(got["trend"]["ecount"]).any()


def test_scale(gpu):
    """22 statistics x 40 blocks x 200,000 columns, a third of them land: a 4,096-column sample against the oracle,
    every all-NaN column NaN"""
    rng = np.random.default_rng(5)
    nstat, nb, C = 22, 40, 200_000
    p = rng.normal(size=(nstat, nb, C))
    p[::2] = rng.poisson(2.0, (nstat // 2, nb, C))
    p[rng.random((nstat, nb, C)) < 0.02] = np.nan
    land = rng.random(C) < 1 / 3
    p[:, :, land] = np.nan
    x = abscissa(nb)
    tc = tr.tcrit_table(0.05, nb)
    sample = np.sort(rng.choice(C, 4096, replace=False))
    for method in METHODS:
        got = gpu.trend_device(p, x, tc, method)
        assert np.isnan(got[:, :, land]).all()
        assert np.isfinite(got[:, :, ~land]).all()
        same(got[:, :, sample], to.trend_oracle(p[:, :, sample], x, tc, method), method)
