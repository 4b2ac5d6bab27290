"""lag_correlation() on the device against tests/lag_correlation_oracle.py: exact equality of the six arrays and both
counters.  The C entries are called raw, on pitched inputs (the columns past C hold valid samples in range) and outputs
pre-filled with a bit pattern that must be gone inside [0, C) and intact beyond it; every forced block length must give the
same bits.  Then the public function on a 20-year grid with land, in several slabs, against the oracle."""
import functools

import numpy as np
import numpy.testing as npt
import pytest

import lag_correlation_cases as lc
import lag_correlation_oracle as lo

pytestmark = pytest.mark.gpu

EXTRA = 5                       # columns past C in every pitched array
FILL32, FILL64 = -0x5A5A5A5B, -0x5A5A5A5A5A5A5A5B
FIELDS = lo.FIELDS
DTYPES = {k: np.int32 if k == "n" else np.int64 for k in FIELDS}
T0, C0 = 300, 300               # a full and a ragged workgroup


@pytest.fixture(scope="module")
def dev():
    from xmhw_amd._lib import require_gpu
    require_gpu()
    import xmhw_amd.device as d
    return d


@pytest.fixture(autouse=True)
def automatic_block_afterwards():
    yield
    from xmhw_amd._lib import hip_lagcorr
    hip_lagcorr().set_lag_corr_block(0)


@functools.lru_cache(maxsize=None)
def _case(T, C, dtype, seed, Dr=1):
    return lc.series(T, C, np.dtype(dtype).type, seed, Dr=Dr)


@functools.lru_cache(maxsize=None)
def _want(T, C, dtype, seed, Dr, pattern, L, shift_x=0, shift_y=0, auto=False):
    d = _case(T, C, dtype, seed, Dr)
    classes, K = pattern(T)
    if auto:
        return lo.lag_corr_sums(d["x"], d["x"], d["base_x"], d["base_x"], d["rows"], shift_x, shift_x, classes, K, L)
    return lo.lag_corr_sums(d["x"], d["y"], d["base_x"], d["base_y"], d["rows"], shift_x, shift_y, classes, K, L)


def _pitched(a, ld, fill):
    out = np.full(a.shape[:-1] + (ld,), fill, dtype=a.dtype)
    out[..., :a.shape[-1]] = a
    return out


def buffers(dev, K, L, C):
    from xmhw_amd._lib import hip_lagcorr
    ldo = C + EXTRA
    b = {k: dev.DeviceBuffer.from_array(np.full((K, L + 1, ldo), FILL32 if dt is np.int32 else FILL64, dt))
         for k, dt in DTYPES.items()}
    b.update(cnt=dev.DeviceBuffer.from_array(np.full(2, 123, np.int64)), ldo=ldo, K=K, L=L, C=C)
    hip_lagcorr().lag_corr_init(K, L, C, *(b[k].ptr for k in FIELDS), ldo, b["cnt"].ptr)
    return b


def raw_accumulate(dev, d, classes, K, L, shift_x=0, shift_y=0, block=0, c0=0, n=None, out=None, auto=False):
    """xmhw_lag_corr_accumulate_* on the columns c0 .. c0 + n - 1 of the case (all of them by default) into the buffers
    ``out``; the inputs are pitched by EXTRA columns of valid samples in range.  ``auto``: y is the very buffer of x."""
    from xmhw_amd._lib import hip, hip_lagcorr
    x = d["x"]
    T, C = x.shape
    n = C - c0 if n is None else n
    ld = n + EXTRA
    hip_lagcorr().set_lag_corr_block(block)
    held = [dev.DeviceBuffer.from_array(_pitched(x[:, c0:c0 + n], ld, 21.0)),
            dev.DeviceBuffer.from_array(_pitched(d["base_x"][:, c0:c0 + n], ld, 20.0))]
    if not auto:
        held += [dev.DeviceBuffer.from_array(_pitched(d["y"][:, c0:c0 + n], ld, -1.0)),
                 dev.DeviceBuffer.from_array(_pitched(d["base_y"][:, c0:c0 + n], ld, -2.0))]
    d_x, d_bx, d_y, d_by = held if not auto else held + held
    ptrs = [out[k].ptr + np.dtype(dt).itemsize * c0 for k, dt in DTYPES.items()]
    try:
        hip_lagcorr().lag_corr_accumulate(d_x.ptr, ld, d_y.ptr, ld, x.dtype.itemsize, T, n, d_bx.ptr, ld, d_by.ptr, ld,
                                          d["base_x"].shape[0], d["rows"], shift_x, shift_x if auto else shift_y, classes, K,
                                          L, *ptrs, out["ldo"], out["cnt"].ptr)
        hip().stream_sync(0)
    finally:
        for b in held:
            b.free()


def result(b):
    """read back, check the columns past C, free"""
    K, L, C, ldo = b["K"], b["L"], b["C"], b["ldo"]
    try:
        got = {k: b[k].to_array((K, L + 1, ldo), dt) for k, dt in DTYPES.items()}
        cnt = b["cnt"].to_array((2,), np.int64)
    finally:
        for v in b.values():
            if hasattr(v, "free"):
                v.free()
    for k, a in got.items():
        assert (a[..., C:] == (FILL32 if a.dtype == np.int32 else FILL64)).all(), f"{k}: a column past C was touched"
    out = {k: a[..., :C] for k, a in got.items()}
    out["n_range"] = cnt
    return out


def run_whole(dev, d, classes, K, L, **kw):
    b = buffers(dev, K, L, d["x"].shape[1])
    raw_accumulate(dev, d, classes, K, L, out=b, **kw)
    return result(b)


def same(got, want):
    for k in FIELDS:
        assert got[k].dtype == want[k].dtype, k
        npt.assert_array_equal(got[k], want[k], err_msg=k)
    npt.assert_array_equal(got["n_range"], want["n_range"])


def check_case(want, L):
    """on the oracle's side: a case without pairs at its largest lag or without non-zero sums proves nothing"""
    assert want["n"][:, L].sum() > 0 and all((want[k] != 0).any() for k in FIELDS)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("L", lc.DEPTH_LAGS)
def test_every_ring_depth_and_lag_group_edge(dev, dtype, L):
    d = _case(T0, C0, dtype, 11)
    for pattern in lc.PATTERNS:
        classes, K = pattern(T0)
        want = _want(T0, C0, dtype, 11, 1, pattern, L)
        check_case(want, L)
        assert want["n_range"].min() > 0 and (want["n"][..., 2] == 0).all() and (want["n"][..., 3] == 0).all()
        for block in (0, 83):
            same(run_whole(dev, d, classes, K, L, block=block), want)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_forced_blocks_give_identical_bits(dev, dtype):
    """1 / 7 / 64 / 83 / T / 10**6 / automatic: a block rebuilds ring and mask from the L steps before it, wherever it
    starts, and counts nothing twice"""
    d = _case(T0, C0, dtype, 7)
    for L in (5, 63):
        for pattern in (lc.every_step, lc.long_runs_of_minus_one):
            classes, K = pattern(T0)
            want = _want(T0, C0, dtype, 7, 1, pattern, L)
            check_case(want, L)
            for block in (1, 7, 64, 83, T0, 10 ** 6, 0):
                same(run_whole(dev, d, classes, K, L, block=block), want)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_bases_of_five_rows_that_are_not_monotone(dev, dtype):
    d = _case(T0, C0, dtype, 44, 5)
    assert d["rows"].max() == 4 and (np.diff(d["rows"]) < 0).any() and d["base_y"].shape[0] == 5
    for L in (9, 40):
        classes, K = lc.seasons(T0)
        want = _want(T0, C0, dtype, 44, 5, lc.seasons, L)
        check_case(want, L)
        for block in (0, 7):
            same(run_whole(dev, d, classes, K, L, block=block), want)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_shifts_that_differ(dev, dtype):
    d = _case(T0, C0, dtype, 5)
    classes, K = lc.long_runs_of_minus_one(T0)
    for sx, sy in ((3, 0), (0, 2), (24, 1)):
        want = _want(T0, C0, dtype, 5, 1, lc.long_runs_of_minus_one, 12, sx, sy)
        if sx < 24:
            check_case(want, 12)
        assert want["n"].sum() > 0
        same(run_whole(dev, d, classes, K, 12, shift_x=sx, shift_y=sy), want)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_y_aliasing_x_equals_a_separate_copy(dev, dtype):
    d = _case(T0, C0, dtype, 21)
    copy = dict(d, y=d["x"].copy(), base_y=d["base_x"].copy())
    for L, pattern in ((20, lc.every_step), (63, lc.long_runs_of_minus_one)):
        classes, K = pattern(T0)
        want = _want(T0, C0, dtype, 21, 1, pattern, L, auto=True)
        check_case(want, L)
        npt.assert_array_equal(want["sxx"][:, 0], want["sxy"][:, 0])
        for block in (0, 64):
            aliased = run_whole(dev, d, classes, K, L, block=block, auto=True)
            same(aliased, want)
            same(run_whole(dev, copy, classes, K, L, block=block), aliased)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_lags_past_the_axis_stay_zero(dev, dtype):
    for T, L in ((1, 0), (1, 10), (5, 10)):
        d = _case(T, 70, dtype, 90 + T)
        for pattern in (lc.one_class, lc.every_step):
            classes, K = pattern(T)
            want = lo.lag_corr_sums(d["x"], d["y"], d["base_x"], d["base_y"], d["rows"], 0, 0, classes, K, L)
            assert want["n"][:, 0].sum() > 0 and all((want[k][:, T:] == 0).all() for k in FIELDS)
            for block in (0, 1, 2):
                same(run_whole(dev, d, classes, K, L, block=block), want)


def test_two_slabs_equal_one_call_and_init_clears_its_columns_alone(dev):
    d = _case(T0, C0, "float32", 77)
    classes, K = lc.seasons(T0)
    L = 17
    want = _want(T0, C0, "float32", 77, 1, lc.seasons, L)
    check_case(want, L)
    b = buffers(dev, K, L, C0)
    raw_accumulate(dev, d, classes, K, L, c0=0, n=130, out=b)
    raw_accumulate(dev, d, classes, K, L, c0=130, n=C0 - 130, out=b)
    same(result(b), want)                                           # (the counters add up as well)
    # init alone: zeros inside [0, C), the fill beyond (result() checks it), both counters zero
    got = result(buffers(dev, K, L, C0))
    assert all((got[k] == 0).all() for k in FIELDS) and (got["n_range"] == 0).all()


# ---- the public function ---------------------------------------------------------------------------------------------

NY, NX = 12, 20


@pytest.fixture(scope="module")
def fields(dev):
    """20 years of a 12 x 20 grid with land: a persistent SST-like field and a flux that leads it, with more land"""
    from xmhw_amd import GridSeries
    rng = np.random.default_rng(12)
    time = np.arange("2000-01-01", "2020-01-01", dtype="datetime64[D]")
    T = time.shape[0]
    e = rng.normal(0, 1.0, (T, NY, NX))
    a = np.zeros_like(e)
    for t in range(1, T):
        a[t] = 0.9 * a[t - 1] + 0.45 * e[t]
    sst = (18.0 + a).astype(np.float32)
    flux = (40.0 * np.roll(e, -4, axis=0) + rng.normal(0, 15.0, e.shape)).astype(np.float32)
    for v in (sst, flux):
        v[rng.random(v.shape) < 0.01] = np.nan
    land = rng.random((NY, NX)) < 0.25
    land[0, 0], land[1, 1], land[5, 7] = True, False, False
    assert (~land).any(axis=0).all() and (~land).any(axis=1).all() and (~land).sum() > 150
    sst[:, land] = np.nan
    more_land = land.copy()
    more_land[1, 1] = True
    flux[:, more_land] = np.nan
    coords = {"time": time, "lat": np.arange(NY) * 0.25, "lon": np.arange(NX) * 0.25}
    return dict(time=time, land=land, sst=GridSeries(sst, ("time", "lat", "lon"), coords),
                flux=GridSeries(flux, ("time", "lat", "lon"), coords))


def _compare_public(got, want, keep):
    K, nl = want[0].shape[:2]
    for k, w in zip(FIELDS, want):
        a = getattr(got, k).reshape(K, nl, -1)
        assert a.dtype == w.dtype, k
        npt.assert_array_equal(a[..., keep], w, err_msg=k)
        assert (a[..., ~keep] == 0).all()
    npt.assert_array_equal(got.keep.reshape(-1), keep)
    assert np.isnan(got.r.reshape(K, nl, -1)[..., ~keep]).all()


def test_public_autocorrelation_in_several_slabs(dev, fields):
    from xmhw_amd import lag_correlation
    g = fields
    T = g["time"].shape[0]
    keep = ~g["land"].reshape(-1)
    x = np.asarray(g["sst"].values).reshape(T, -1)[:, keep]
    zero, rows = np.zeros(T, np.int32), np.zeros(T, np.int32)
    base = np.full((NY, NX), 18.0)
    want, n_range = lo.lag_corr_lags(x, x, np.full((1, x.shape[1]), 18.0), np.full((1, x.shape[1]), 18.0), rows, 0, 0, zero, 1,
                                     -3, 40)
    assert n_range == (0, 0) and want[0][0, -1].min() > 6000
    per_cell = T * 16 + 4 * 8 + 64
    for kw in (dict(), dict(max_batch_bytes=50 * per_cell)):
        got = lag_correlation(g["sst"], base_x=base, lags=(-3, 40), **kw)
        assert got.auto and got.lag.tolist() == list(range(-3, 41))
        _compare_public(got, want, keep)
    r = got.r.reshape(44, -1)[:, keep]
    assert (r[3] == 1.0).all() and np.allclose(r[4], 0.9, atol=0.03) and np.array_equal(r[2], r[4])
    tau = got.efolding_time().reshape(-1)[keep]
    assert np.all((tau > 7.0) & (tau < 13.0))                       # -1 / ln 0.9 = 9.5 steps
    assert np.all(got.n_eff().reshape(-1)[keep] < 0.1 * want[0][0, 3])


def test_public_two_fields_negative_lags_and_monthly_classes(dev, fields):
    from xmhw_amd import lag_correlation
    from xmhw_amd.exception import XmhwException
    g = fields
    time = g["time"]
    T = time.shape[0]
    keep = ~g["land"].reshape(-1)
    x = np.asarray(g["sst"].values).reshape(T, -1)[:, keep]
    y = np.asarray(g["flux"].values).reshape(T, -1)[:, keep]
    month = (time.astype("datetime64[M]").astype(int) % 12).astype(np.int32)
    rows = np.zeros(T, np.int32)
    C = x.shape[1]
    want, n_range = lo.lag_corr_lags(x, y, np.full((1, C), 18.0), np.zeros((1, C)), rows, 0, 3, month, 12, -10, 20)
    assert n_range == (0, 0) and want[0].sum() > 10 ** 6
    per_cell = T * 4 * 6 + 4 * 8 + 64
    for kw in (dict(), dict(max_batch_bytes=60 * per_cell)):
        got = lag_correlation(g["sst"], g["flux"], base_x=np.full((NY, NX), 18.0), lags=(-10, 20), classes="month", shift_y=3,
                              **kw)
        assert not got.auto and got.klass.shape == (12,)
        _compare_public(got, want, keep)
    cell = int(np.nonzero(keep)[0].tolist().index(1 * NX + 1))      # land in the flux alone: no pair
    assert (want[0][..., cell] == 0).all()
    lag, r = got.lag_of_max()
    assert np.nanmedian(lag) == 4.0 and np.nanmedian(r) > 0.15      # the flux leads by 4 steps
    with pytest.raises(XmhwException, match="shift_y"):
        lag_correlation(g["sst"], g["flux"], base_x=np.full((NY, NX), 18.0), lags=(0, 2))
