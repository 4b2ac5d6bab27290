"""mhw_coverage() on the device against tests/coverage_oracle.py: exact integer equality everywhere."""
import numpy as np
import numpy.testing as npt
import pytest

import coverage_cases as cc
import coverage_oracle as co
import pad_oracle as po

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from xmhw_amd._lib import require_gpu
    require_gpu()
    import xmhw_amd.device as d
    return d


def _check(got, want):
    """Exact equality of (cells, area_q); the case must contain events."""
    assert got[0].dtype == np.int64 and got[1].dtype == np.int64
    assert want[0][..., 4].sum() > 0, "a case without events proves nothing"
    npt.assert_array_equal(got[0], want[0])
    npt.assert_array_equal(got[1], want[1])


def _both(d, wq, reg, R, **kw):
    from xmhw_amd.coverage import coverage_cells
    dkw = {k: v for k, v in kw.items() if k != "max_batch_bytes"}
    got = coverage_cells(d["ts"], d["seas"], d["thresh"], d["doy"], d["doys"], wq, reg, R, **kw)
    want = co.coverage_fast(d["ts"], d["seas"], d["thresh"], d["doy"], d["doys"], wq, reg, R, **dkw)
    _check(got, want)
    return got


def test_golden_series(dev):
    """The 108 reference series, each as one cell with its own parameters."""
    from xmhw_amd.coverage import coverage_cells
    total = 0
    for ts, se, th, (m, jg, gap), table, cols in cc.golden_series():
        T = ts.shape[0]
        args = (ts[:, None], se[:, None], th[:, None], np.arange(T), np.arange(T), np.array([7], np.int64),
                np.array([0], np.int32), 1, m, jg, gap)
        want = co.coverage_cells(*args)
        _check(coverage_cells(*args), want)
        total += int(want[0][..., 4].sum())
    assert total > 10000


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("C", [1, 63, 64, 65, 255, 257, 3001])
def test_cell_counts_around_a_wave_and_a_tile(dev, dtype, C):
    d = cc.synthetic(203, C, dtype, seed=C, nan_frac=0.01)           # T is not a multiple of 64
    for R in (1, 2, 7):
        _both(d, cc.weights_q(C, seed=R), cc.scattered_regions(C, R, seed=R), R)
    _both(d, cc.weights_q(C), cc.wave_regions(C, 7), 7)              # one region per wave


@pytest.mark.parametrize("kw", [dict(minDuration=3, maxGap=1), dict(minDuration=8, maxGap=4), dict(joinGaps=False),
                                dict(minDuration=5, maxGap=0), dict(coldSpells=True)])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_filter_variants_and_cold_spells(dev, kw, dtype):
    d = cc.synthetic(331, 200, dtype, seed=5, nan_frac=0.02, cold=kw.get("coldSpells", False))
    _both(d, cc.weights_q(200), cc.scattered_regions(200, 3), 3, **kw)


def test_nan_gaps_with_and_without_maxPadLength(dev):
    from xmhw_amd.coverage import coverage_cells
    from xmhw_amd.padding import make_pad
    T, C = 300, 130
    d = cc.synthetic(T, C, np.float64, seed=8, nan_frac=0.06)
    time = np.datetime64("2001-01-01") + np.arange(T).astype("timedelta64[D]")
    wq, reg = cc.weights_q(C), cc.scattered_regions(C, 2)
    plain = _both(d, wq, reg, 2)
    pad = make_pad(np.timedelta64(3, "D"), time)
    try:
        got = coverage_cells(d["ts"], d["seas"], d["thresh"], d["doy"], d["doys"], wq, reg, 2, pad=pad)
    finally:
        pad.free()
    filled = po.interpolate_na(d["ts"], po.interp_index(time), 3 * 86400e9)
    want = co.coverage_fast(filled, d["seas"], d["thresh"], d["doy"], d["doys"], wq, reg, 2)
    _check(got, want)
    assert not np.array_equal(got[0], plain[0])                      # the interpolation matters


def test_region_cap(dev):
    from xmhw_amd import XmhwException
    from xmhw_amd._lib import hip
    from xmhw_amd.coverage import MAX_REGIONS, coverage_cells
    h = hip()
    assert MAX_REGIONS == h.COVERAGE_MAX_REGIONS >= 1024
    C = 3000
    d = cc.synthetic(130, C, np.float32, seed=9)
    reg = cc.scattered_regions(C, MAX_REGIONS, excluded=0.0)
    assert len(np.unique(reg)) == MAX_REGIONS
    _both(d, cc.weights_q(C), reg, MAX_REGIONS)
    with pytest.raises(XmhwException):
        coverage_cells(d["ts"], d["seas"], d["thresh"], d["doy"], d["doys"], cc.weights_q(C), reg, MAX_REGIONS + 1)
    # the C ABI itself: XMHW_ERR_UNSUPPORTED (code 3) above the cap, before anything is touched
    with pytest.raises(h.HipError, match=r"code 3"):
        h.coverage_accumulate(8, 4, 130, C, C, 8, 8, C, np.zeros(130, np.int32), 0, 8, C, 5, 1, 2, 8, 8, MAX_REGIONS + 1, 8, 8)
    # ... raised as its own type, which is a HipError still
    with pytest.raises(h.HipError) as raised:
        h.coverage_accumulate(8, 4, 130, C, C, 8, 8, C, np.zeros(130, np.int32), 0, 8, C, 5, 1, 2, 8, 8, MAX_REGIONS + 1, 8, 8)
    assert isinstance(raised.value, h.Unsupported) and isinstance(raised.value, h.HipError)
    assert issubclass(h.Unsupported, h.HipError) and h.Unsupported is not h.HipError


def test_weights_zero_and_one(dev):
    C = 500
    d = cc.synthetic(140, C, np.float32, seed=10)
    reg = np.zeros(C, np.int32)
    z = _both(d, np.zeros(C, np.int64), reg, 1)
    assert z[1].sum() == 0 and z[0].sum() > 0
    one = _both(d, np.full(C, 1 << 31, np.int64), reg, 1)
    npt.assert_array_equal(one[1], one[0] << 31)


def test_leading_dimensions_with_canary_columns(dev):
    """Series, climatologies and bits wider than the slab: the extra columns hold values that would be extreme
    events if a kernel read them; the accumulators are compared whole."""
    from xmhw_amd._lib import hip
    from xmhw_amd.detect_front import _check_inputs
    h = hip()
    T, C, pad_cols, R = 150, 70, 5, 3
    for dtype in (np.float32, np.float64):
        d = cc.synthetic(T, C, dtype, seed=12)
        wq, reg = cc.weights_q(C), cc.scattered_regions(C, R)
        ts = np.full((T, C + pad_cols), 1e6, dtype=dtype)
        ts[:, :C] = d["ts"]
        D = d["seas"].shape[0]
        se, th = np.zeros((D, C + pad_cols)), np.ones((D, C + pad_cols))
        se[:, :C], th[:, :C] = d["seas"], d["thresh"]
        _, _, _, rows = _check_inputs(d["ts"], d["seas"], d["thresh"], d["doy"], d["doys"])
        W = (T + 63) // 64
        bufs = [dev.DeviceBuffer.from_array(a) for a in (ts, se, th, wq, reg)]
        d_ts, d_se, d_th, d_wq, d_reg = bufs
        d_bits = dev.DeviceBuffer.from_array(np.full((W, C + pad_cols), 0xFFFFFFFFFFFFFFFF, dtype=np.uint64))
        acc = [dev.DeviceBuffer.from_array(np.zeros((T, R, 5), np.int64)) for _ in range(2)]
        try:
            ld = C + pad_cols
            h.exceed_bits(d_ts.ptr, ts.dtype.itemsize, T, C, ld, d_th.ptr, ld, D, rows, 0, d_bits.ptr, ld)
            h.coverage_accumulate(d_ts.ptr, ts.dtype.itemsize, T, C, ld, d_se.ptr, d_th.ptr, ld, rows, 0, d_bits.ptr, ld,
                                  5, 1, 2, d_wq.ptr, d_reg.ptr, R, acc[0].ptr, acc[1].ptr)
            h.stream_sync(0)
            got = acc[0].to_array((T, R, 5), np.int64), acc[1].to_array((T, R, 5), np.int64)
            bits = d_bits.to_array((W, ld), np.uint64)
        finally:
            for b in bufs + [d_bits] + acc:
                b.free()
        _check(got, co.coverage_fast(d["ts"], d["seas"], d["thresh"], d["doy"], d["doys"], wq, reg, R))
        assert (bits[:, C:] == 0xFFFFFFFFFFFFFFFF).all()              # the canary words are untouched


def test_batches_and_runs_are_bit_identical(dev):
    C = 1500
    d = cc.synthetic(260, C, np.float32, seed=13, nan_frac=0.01)
    wq, reg = cc.weights_q(C), cc.scattered_regions(C, 7)
    a = _both(d, wq, reg, 7)
    per_cell = 260 * 5 + 260 // 4 + 2 * 37 * 8 + 64
    for mbb in (per_cell * 64, per_cell * 333, per_cell * 1499):
        b = _both(d, wq, reg, 7, max_batch_bytes=mbb)
        npt.assert_array_equal(a[0], b[0])
        npt.assert_array_equal(a[1], b[1])
    c = _both(d, wq, reg, 7)
    npt.assert_array_equal(a[0], c[0])
    npt.assert_array_equal(a[1], c[1])


def test_two_hundred_thousand_cells(dev):
    """204,800 cells: 512 distinct series, each 400 times with its own weight and region, so that the oracle
    runs once per distinct series and the expected sums are numpy int64 adds."""
    from xmhw_amd.coverage import coverage_cells
    T, K, reps, R = 140, 512, 400, 5
    base = cc.synthetic(T, K, np.float32, seed=14, nan_frac=0.005)
    C = K * reps
    idx = np.random.default_rng(15).permutation(np.tile(np.arange(K), reps))
    wq, reg = cc.weights_q(C), cc.scattered_regions(C, R)
    rows = co.rows_of(base["doy"], base["doys"])
    want_c, want_a = np.zeros((T, R, 5), np.int64), np.zeros((T, R, 5), np.int64)
    for k in range(K):
        st = co.cell_states(base["ts"][:, k], base["seas"][:, k], base["thresh"][:, k], rows).astype(np.int64)
        mine = idx == k
        for r in range(R):
            sel = mine & (reg == r)
            want_c[:, r] += st * int(sel.sum())
            want_a[:, r] += st * int(wq[sel].sum())
    got = coverage_cells(base["ts"][:, idx], base["seas"][:, idx], base["thresh"][:, idx], base["doy"], base["doys"], wq,
                         reg, R)
    _check(got, (want_c, want_a))
    got1 = coverage_cells(base["ts"][:, idx], base["seas"][:, idx], base["thresh"][:, idx], base["doy"], base["doys"], wq,
                          np.where(reg >= 0, 0, -1).astype(np.int32), 1)
    npt.assert_array_equal(got1[0][:, 0], want_c.sum(axis=1))
    npt.assert_array_equal(got1[1][:, 0], want_a.sum(axis=1))


def test_threshold_to_coverage_end_to_end(dev, oisst):
    """threshold() -> mhw_coverage() on the land-masked fixture grid against the route it replaces:
    detect(..., intermediate=True) and numpy on `cats`."""
    from xmhw_amd import GridSeries, climatology_series, detect, mhw_coverage, threshold
    for cold in (False, True):
        g = GridSeries(oisst["sst"], ("time", "lat", "lon"), {"time": oisst["time64"], "lat": oisst["lat"],
                                                              "lon": oisst["lon"]},
                       time_encoding={"calendar": "proleptic_gregorian"})
        clim = threshold(g, coldSpells=cold)
        th, se = climatology_series(clim, "thresh"), climatology_series(clim, "seas")
        reg = np.zeros((8, 4), dtype=np.int64)
        reg[:, 2:] = 3
        cov = mhw_coverage(g, th, se, weights="coslat", regions=reg, coldSpells=cold)
        mhw, inter = detect(g, th, se, coldSpells=cold, intermediate=True)
        T = oisst["sst"].shape[0]
        keep = ~np.isnan(oisst["sst"].reshape(T, -1)).all(axis=0)
        ev = np.asarray(inter["events"]).reshape(T, -1)
        cats = np.asarray(inter["cats"]).reshape(T, -1)
        alive = ~np.isnan(np.asarray(inter["ts"]).reshape(T, -1)).all(axis=0)
        assert alive.sum() == keep.sum() == 12
        ev, cats = ev[:, alive], cats[:, alive]                       # the 12 ocean cells, in stacked order
        lab = reg.reshape(-1)[keep]
        from xmhw_amd.coverage import quantise_weights
        wq = quantise_weights(np.repeat(np.cos(np.deg2rad(oisst["lat"].astype(np.float64))), 4))[0][keep]
        states = np.stack([cats == 1, cats == 2, cats == 3, cats >= 4, ~np.isnan(ev)], axis=-1)
        assert states[..., 4].sum() == mhw.table[:, mhw.columns.index("duration")].sum() > 0
        npt.assert_array_equal(cov.region, np.unique(lab))
        for j, r in enumerate(cov.region):
            sel = lab == r
            npt.assert_array_equal(cov.cells[:, j], states[:, sel].sum(axis=1))
            npt.assert_array_equal(cov.area_q[:, j], (states[:, sel] * wq[sel][None, :, None]).sum(axis=1))
            assert cov.total_q[j] == wq[sel].sum() and cov.ncells[j] == sel.sum()
        assert cov.cells[..., 4].sum() > 0
