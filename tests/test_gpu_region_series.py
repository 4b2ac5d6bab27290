"""region_series() on the device against tests/region_series_oracle.py: exact integer equality everywhere."""
import math

import numpy as np
import numpy.testing as npt
import pytest

import region_series_cases as rc
import region_series_oracle as ro

pytestmark = pytest.mark.gpu

T0 = 203                        # not a multiple of 64 nor of any block of steps the kernel uses


@pytest.fixture(scope="module")
def dev():
    from xmhw_amd._lib import require_gpu
    require_gpu()
    import xmhw_amd.device as d
    return d


def _wi(C, seed=2):
    """integer weights within the bit budget of a grid of C cells, both ends present"""
    from xmhw_amd.region_series import weight_bits
    return rc.weights_i(C, weight_bits(C), seed)


def _both(ts, wi, reg, R, x0=0.0, n_range=0, **kw):
    """the device stage against the oracle: exact equality of the accumulator and of the range counter"""
    from xmhw_amd.region_series import region_cells
    got, got_range = region_cells(ts, wi, reg, R, x0, **kw)
    want, want_range = ro.region_cells(ts, wi, reg, R, x0)
    assert got.dtype == np.int64 and got.shape == (ts.shape[0], R, 3)
    assert want[..., 0].sum() > 0, "a case without samples proves nothing"
    npt.assert_array_equal(got, want)
    assert got_range == want_range == n_range
    return got


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("C", [1, 63, 64, 65, 255, 257, 3001])
def test_cell_counts_around_a_wave_and_a_tile(dev, dtype, C):
    ts = rc.series(T0, C, dtype, seed=C, nan_frac=0.01)
    for R in (1, 2, 7):
        _both(ts, _wi(C, seed=R), rc.scattered_regions(C, R, seed=R), R)
    _both(ts, _wi(C), rc.uniform_waves(C, 7), 7)                      # path A
    for k in (2, 3, 4):
        _both(ts, _wi(C, seed=k), rc.few_per_wave(C, k, 7), 7)        # path B
    _both(ts, _wi(C), rc.many_per_wave(C, 7), 7)                      # path C, adds in LDS
    _both(ts, _wi(C), rc.many_per_wave(C, 70), 70)                    # path C, adds in global memory


def test_both_wave_sums_give_the_same_bits(dev):
    from xmhw_amd._lib import hip
    h = hip()
    C = 1000
    ts = rc.series(T0, C, np.float32, seed=21, nan_frac=0.02)
    wi = _wi(C)
    try:
        for variant in (0, 1):
            h.set_region_wave_sum(variant)
            _both(ts, wi, rc.uniform_waves(C, 7), 7)
            _both(ts, wi, rc.few_per_wave(C, 3, 7), 7)
            _both(ts, wi, rc.uniform_waves(C, 100), 100)
    finally:
        h.set_region_wave_sum(1)


def test_lds_to_global_switch_and_region_cap(dev):
    from xmhw_amd import XmhwException
    from xmhw_amd._lib import hip
    from xmhw_amd.region_series import MAX_REGIONS, SERIES_BITS, region_cells
    h = hip()
    assert MAX_REGIONS == h.REGION_MAX_REGIONS == 1024 and SERIES_BITS == h.REGION_SERIES_BITS == 16
    C = 3000
    ts = rc.series(130, C, np.float32, seed=9, nan_frac=0.01)
    wi = _wi(C)
    for R in (64, 65, MAX_REGIONS):
        reg = rc.scattered_regions(C, R, excluded=0.0)
        assert len(np.unique(reg)) == R
        _both(ts, wi, reg, R)
        _both(ts, wi, (rc.wave_regions(C, R) * 7 % R).astype(np.int32), R)    # one region per wave at the same R
    reg = rc.scattered_regions(C, MAX_REGIONS, excluded=0.0)
    with pytest.raises(XmhwException):
        region_cells(ts, wi, reg, MAX_REGIONS + 1)
    # the C ABI itself: XMHW_ERR_UNSUPPORTED (code 3) above the cap, before anything is touched (the pointers are not)
    with pytest.raises(h.Unsupported, match=r"code 3"):
        h.region_accumulate(8, 4, 130, C, C, 0.0, 8, 8, MAX_REGIONS + 1, 8, 8)
    with pytest.raises(h.HipError):
        h.region_accumulate(8, 8, 130, C, C, 0.0, 8, 8, MAX_REGIONS + 1, 8, 8)


@pytest.mark.parametrize("x0", [0.0, 273.15])
def test_signs_and_the_precomputed_wave_weight(dev, x0):
    from xmhw_amd.region_series import region_cells
    T, C, R = 200, 700, 4
    ts = rc.series(T, C, np.float64, seed=31, x0=x0)                           # NaN-free, on both sides of x0
    reg = rc.uniform_waves(C, R)
    ts[:, reg == 1] = x0 - np.abs(ts[:, reg == 1] - x0) - 0.25                 # region 1 lies below x0
    wi = _wi(C)
    wi[reg == 1] |= 1
    a = _both(ts, wi, reg, R, x0)
    assert (a[:, 1, 2] < 0).all() and (a[:, 0, 2] > 0).any() and (a[:, 0, 2] < 0).any()
    npt.assert_array_equal(a[:, :, 0], np.bincount(reg, minlength=R)[None, :].repeat(T, axis=0))
    # one NaN in one lane at one step of every 64-step block: the results differ exactly there
    holes = [(blk * 64 + (17 * blk + 5) % min(64, T - blk * 64), (97 * blk + 3) % C) for blk in range((T + 63) // 64)]
    assert len(holes) == 4 and all(t < T for t, _ in holes)
    tn = ts.copy()
    for t, c in holes:
        tn[t, c] = np.nan
    b = _both(tn, wi, reg, R, x0)
    differ = np.zeros((T, R), dtype=bool)
    for t, c in holes:
        differ[t, reg[c]] = True
    npt.assert_array_equal((a[..., 0] != b[..., 0]), differ)
    npt.assert_array_equal((a != b).any(axis=2), differ)
    for t, c in holes:
        assert a[t, reg[c], 0] - b[t, reg[c], 0] == 1 and a[t, reg[c], 1] - b[t, reg[c], 1] == wi[c]
    # a step where a whole region is NaN
    tn[11, reg == 2] = np.nan
    c_ = _both(tn, wi, reg, R, x0)
    assert (c_[11, 2] == 0).all() and np.isnan(ro.mean_of(c_, x0)[11, 2]) and not np.isnan(ro.mean_of(c_, x0)[11, 1])
    got, _ = region_cells(tn.astype(np.float32), wi, reg, R, x0)
    npt.assert_array_equal(got, ro.region_cells(tn.astype(np.float32), wi, reg, R, x0)[0])


@pytest.mark.parametrize("x0", [0.0, 273.15])
def test_samples_out_of_range_are_left_out_and_counted(dev, x0):
    from xmhw_amd import GridSeries, XmhwException, region_series
    T, nlat, nlon = 70, 10, 13
    C = nlat * nlon
    ts = rc.series(T, C, np.float64, seed=41, nan_frac=0.01, x0=x0)
    odd = {(3, 0): np.inf, (9, 64): -np.inf, (20, 65): x0 + 127.99999, (33, 100): x0 + 128.0, (69, C - 1): x0 - 128.0}
    for (t, c), v in odd.items():
        ts[t, c] = v
    assert abs(ts[20, 65] - x0) < 128.0 and ts[33, 100] - x0 == 128.0 and ts[69, C - 1] - x0 == -128.0
    wi, reg = _wi(C), rc.scattered_regions(C, 3, excluded=0.0)
    wi[[0, 64, 65, 100, C - 1]] |= 1
    got = _both(ts, wi, reg, 3, x0, n_range=4)
    # the in-range sums are those of the series without the four samples
    without = ts.copy()
    for (t, c) in ((3, 0), (9, 64), (33, 100), (69, C - 1)):
        without[t, c] = np.nan
    npt.assert_array_equal(got, _both(without, wi, reg, 3, x0))
    _both(ts.astype(np.float32), wi, reg, 3, x0, n_range=ro.region_cells(ts.astype(np.float32), wi, reg, 3, x0)[1])
    g = GridSeries(ts.reshape(T, nlat, nlon), ("time", "lat", "lon"),
                   {"time": np.datetime64("2001-01-01") + np.arange(T).astype("timedelta64[D]"),
                    "lat": np.linspace(-40, 40, nlat), "lon": np.arange(nlon, dtype=np.float64)})
    with pytest.raises(XmhwException, match=r"^4 samples .*offset=273\.15"):
        region_series(g, weights="coslat", offset=x0)
    ok = region_series(GridSeries(without.reshape(T, nlat, nlon), g.dims, g.coords), weights="coslat", offset=x0)
    assert ok.n_valid.sum() == (~np.isnan(without)).sum()


def test_weights_zero_and_one(dev):
    C = 500
    ts = rc.series(140, C, np.float32, seed=10, nan_frac=0.01)
    reg = np.zeros(C, np.int32)
    z = _both(ts, np.zeros(C, np.int64), reg, 1)
    assert z[..., 1].sum() == 0 and z[..., 2].sum() == 0 and z[..., 0].sum() > 0
    from xmhw_amd.region_series import weight_bits
    ib = weight_bits(C)
    one = _both(ts, np.full(C, 1 << ib, np.int64), reg, 1)
    assert ib == 29
    npt.assert_array_equal(one[..., 1], one[..., 0] << ib)


def test_leading_dimensions_with_canary_columns(dev):
    """Series wider than the slab, wi / region longer than it: the extra columns hold samples out of range, region 0
    and the largest weight; the accumulator and the range counter are compared whole."""
    from xmhw_amd._lib import hip
    h = hip()
    T, C, pad_cols, R = 150, 70, 5, 3
    ld = C + pad_cols
    for dtype in (np.float32, np.float64):
        ts = np.full((T, ld), 1e6, dtype=dtype)
        ts[:, :C] = rc.series(T, C, dtype, seed=12, nan_frac=0.01)
        wi, reg = np.full(ld, 1 << 31, np.int64), np.zeros(ld, np.int32)
        wi[:C], reg[:C] = _wi(C), rc.scattered_regions(C, R)
        bufs = [dev.DeviceBuffer.from_array(a) for a in (ts, wi, reg, np.zeros((T, R, 3), np.int64), np.zeros(1, np.int64))]
        d_ts, d_wi, d_reg, d_acc, d_nr = bufs
        try:
            h.region_accumulate(d_ts.ptr, ts.dtype.itemsize, T, C, ld, 0.0, d_wi.ptr, d_reg.ptr, R, d_acc.ptr, d_nr.ptr)
            h.stream_sync(0)
            got, n_range = d_acc.to_array((T, R, 3), np.int64), int(d_nr.to_array((1,), np.int64)[0])
        finally:
            for b in bufs:
                b.free()
        want, _ = ro.region_cells(ts[:, :C], wi[:C], reg[:C], R)
        assert n_range == 0 and want[..., 0].sum() > 0
        npt.assert_array_equal(got, want)


def test_batches_and_runs_are_bit_identical(dev):
    C, T = 1500, 260
    ts = rc.series(T, C, np.float32, seed=13, nan_frac=0.01)
    wi, reg = _wi(C), rc.scattered_regions(C, 7)
    a = _both(ts, wi, reg, 7)
    per_cell = T * 4 + 16
    for mbb in (per_cell * 64, per_cell * 333, per_cell * 1499):
        npt.assert_array_equal(a, _both(ts, wi, reg, 7, max_batch_bytes=mbb))
    npt.assert_array_equal(a, _both(ts, wi, reg, 7))
    few = rc.few_per_wave(C, 3, 7)
    npt.assert_array_equal(_both(ts, wi, few, 7), _both(ts, wi, few, 7, max_batch_bytes=per_cell * 333))


def test_two_hundred_thousand_cells(dev):
    """204,800 cells: 512 distinct series, each 400 times with its own weight and region; the expected sums are numpy
    int64 products of the per-series integers with the per-(series, region) counts and weight sums."""
    from xmhw_amd.region_series import region_cells, weight_bits
    T, K, reps, R = 140, 512, 400, 5
    base = rc.series(T, K, np.float32, seed=14, nan_frac=0.005)
    C = K * reps
    ib = weight_bits(C)
    assert ib == 20
    idx = np.random.default_rng(15).permutation(np.tile(np.arange(K), reps))
    wi, reg = rc.weights_i(C, ib), rc.scattered_regions(C, R)
    xq, ok, out = ro.quantised(base)
    assert not out.any()
    cnt, wsum = np.zeros((K, R), np.int64), np.zeros((K, R), np.int64)
    live = reg >= 0
    np.add.at(cnt, (idx[live], reg[live]), 1)
    np.add.at(wsum, (idx[live], reg[live]), wi[live])
    ok = ok.astype(np.int64)
    want = np.stack([ok @ cnt, ok @ wsum, (ok * xq) @ wsum], axis=-1)
    got, n_range = region_cells(base[:, idx], wi, reg, R)
    assert n_range == 0 and want[..., 0].sum() > 0 and np.abs(want[..., 2]).max() < 2 ** 61
    npt.assert_array_equal(got, want)
    got1, _ = region_cells(base[:, idx], wi, np.where(reg >= 0, 0, -1).astype(np.int32), 1)
    npt.assert_array_equal(got1[:, 0], want.sum(axis=1))


def test_end_to_end_on_the_fixture_grid(dev, oisst):
    from xmhw_amd import GridSeries, region_series, threshold_detect
    from xmhw_amd.device import PackedArray, decode_through_device
    from xmhw_amd.gridweights import quantise_weights
    from xmhw_amd.region_series import region_grid
    g = GridSeries(oisst["sst"], ("time", "lat", "lon"), {"time": oisst["time64"], "lat": oisst["lat"], "lon": oisst["lon"]},
                   time_encoding={"calendar": "proleptic_gregorian"})
    reg = np.zeros((8, 4), dtype=np.int64)
    reg[4:] = 3                                                # two bands of latitude, both with ocean
    rs = region_series(g, weights="coslat", regions=reg)
    assert rs.region.tolist() == [0, 3]
    T = oisst["sst"].shape[0]
    stacked = oisst["sst"].reshape(T, -1)
    keep = ~np.isnan(stacked).all(axis=0)
    assert keep.sum() == 12
    lab = reg.reshape(-1)
    w = np.repeat(np.cos(np.deg2rad(oisst["lat"].astype(np.float64))), 4)
    wi = quantise_weights(w, 31)[0]
    assert rs.weight_bits == 31
    npt.assert_array_equal(rs.region, np.unique(lab[keep]))
    bound = rs.quantisation_bound()
    for j, r in enumerate(rs.region):
        members = np.nonzero(keep & (lab == r))[0]
        assert rs.ncells[j] == members.shape[0] and rs.total_i[j] == wi[members].sum()
        for t in range(T):
            x = stacked[t, members].astype(np.float64)
            ok = ~np.isnan(x)
            exact = math.fsum(w[members][ok] * x[ok]) / math.fsum(w[members][ok])
            assert abs(rs.mean[t, j] - exact) <= bound[t, j]
    want, _ = ro.region_cells(stacked[:, keep], wi[keep], np.searchsorted(rs.region, lab[keep]).astype(np.int32), 2)
    npt.assert_array_equal(np.stack([rs.n_valid, rs.wsum_i, rs.xsum_q], axis=-1), want)
    # the regional index into threshold_detect(): a table with one cell per region
    clim, mhw = threshold_detect(rs.series())
    assert mhw.offsets.shape == (len(rs.region) + 1,) and mhw.n_events > 0
    assert clim["thresh"].shape[1:] == (len(rs.region),)
    # a packed int16 view of the grid through region_grid() equals the decoded float route exactly
    codes = np.where(np.isnan(stacked), -32768, np.rint(np.nan_to_num(stacked) * 100.0)).astype(np.int16)
    packed = PackedArray(codes, dict(scale=0.01, offset=0.0, fill=-32768, out="float32"))
    decoded = decode_through_device(packed)
    assert decoded.dtype == np.float32 and np.isnan(decoded[:, ~keep]).all() and not np.isnan(decoded[:, keep]).any()
    rid = np.searchsorted(rs.region, lab).astype(np.int32)
    wi_of = lambda n: quantise_weights(w, 31)[0]                                # noqa: E731
    a, na, keep_a = region_grid(packed, False, wi_of, rid, 2)
    b, nb, keep_b = region_grid(decoded, False, wi_of, rid, 2)
    npt.assert_array_equal(a, b)
    npt.assert_array_equal(keep_a, keep)
    npt.assert_array_equal(keep_b, keep)
    assert na == nb == 0 and a[..., 0].sum() == 12 * T - np.isnan(stacked[:, keep]).sum()
    npt.assert_array_equal(a, ro.region_cells(decoded[:, keep], wi[keep], rid[keep], 2)[0])
    # several slabs: the two-pass route gives the same bits
    c, _, keep_c = region_grid(decoded, False, wi_of, rid, 2, max_batch_bytes=T * 4 * 4 * 5)
    npt.assert_array_equal(c, b)
    npt.assert_array_equal(keep_c, keep)
