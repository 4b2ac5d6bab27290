"""index_regression() on the device against tests/index_regression_oracle.py: exact equality of every array.  The C
entries are called raw, on pitched inputs and outputs pre-filled with a bit pattern that must be gone inside [0, C) and
intact beyond it; every forced block length must give the same bits."""
import functools

import numpy as np
import numpy.testing as npt
import pytest

import index_regression_cases as rc
import index_regression_oracle as ro

pytestmark = pytest.mark.gpu

EXTRA = 5                       # columns past C in every pitched array
FILL32, FILL64 = -0x5A5A5A5B, -0x5A5A5A5A5A5A5A5B
FIELDS = ro.FIELDS


@pytest.fixture(scope="module")
def dev():
    from xmhw_amd._lib import require_gpu
    require_gpu()
    import xmhw_amd.device as d
    return d


@pytest.fixture(autouse=True)
def automatic_block_afterwards():
    yield
    from xmhw_amd._lib import hip_regress
    hip_regress().set_index_regress_block(0)


@functools.lru_cache(maxsize=None)
def _case(T, C, dtype, seed, J, D=1):
    zq = rc.predictors(T, J, seed + 1)
    return rc.synthetic(T, C, np.dtype(dtype).type, seed, D=D, zq=zq), zq


@functools.lru_cache(maxsize=None)
def _want(T, C, dtype, seed, J, D, pattern):
    d, zq = _case(T, C, dtype, seed, J, D)
    classes, K = pattern(T)
    return ro.regress_sums(d["ts"], d["base"], d["rows"], classes, K, zq)


def _pitched(a, ld, fill):
    out = np.full(a.shape[:-1] + (ld,), fill, dtype=a.dtype)
    out[..., :a.shape[-1]] = a
    return out


def _shapes(K, J, ldo):
    return {k: ((K, ldo), np.int32) if k in ("n", "n1") else ((K, J, ldo), np.int64) if k in ("saz", "mz", "mzz") else
            ((K, ldo), np.int64) for k in FIELDS}


def buffers(dev, K, J, C):
    from xmhw_amd._lib import hip_regress
    ldo = C + EXTRA
    b = {k: dev.DeviceBuffer.from_array(np.full(shape, FILL32 if dt is np.int32 else FILL64, dt))
         for k, (shape, dt) in _shapes(K, J, ldo).items()}
    b.update(cnt=dev.DeviceBuffer.from_array(np.full(1, 123, np.int64)), ldo=ldo, K=K, J=J, C=C)
    hip_regress().index_regress_init(K, J, C, *(b[k].ptr for k in FIELDS), ldo, b["cnt"].ptr)
    return b


def raw_accumulate(dev, d, zq, classes, K, block=0, c0=0, n=None, out=None):
    """xmhw_index_regress_accumulate_* on the columns c0 .. c0 + n - 1 of the case (all of them by default) into the
    buffers ``out``; the inputs are pitched by EXTRA columns that would be in range and valid if a kernel read them."""
    from xmhw_amd._lib import hip, hip_regress
    ts, base = d["ts"], d["base"]
    T, C = ts.shape
    n = C - c0 if n is None else n
    ld = n + EXTRA
    hip_regress().set_index_regress_block(block)
    d_ts = dev.DeviceBuffer.from_array(_pitched(ts[:, c0:c0 + n], ld, 21.0))
    d_base = dev.DeviceBuffer.from_array(_pitched(base[:, c0:c0 + n], ld, 20.0))
    ptrs = [out[k].ptr + np.dtype(dt).itemsize * c0 for k, (_, dt) in _shapes(K, zq.shape[1], out["ldo"]).items()]
    try:
        hip_regress().index_regress_accumulate(d_ts.ptr, ts.dtype.itemsize, T, n, ld, d_base.ptr, ld, base.shape[0], d["rows"],
                                               classes, K, zq, *ptrs, out["ldo"], out["cnt"].ptr)
        hip().stream_sync(0)
    finally:
        d_ts.free()
        d_base.free()


def result(b):
    """read back, check the columns past C, free"""
    K, J, C, ldo = b["K"], b["J"], b["C"], b["ldo"]
    try:
        got = {k: b[k].to_array(shape, dt) for k, (shape, dt) in _shapes(K, J, ldo).items()}
        cnt = b["cnt"].to_array((1,), np.int64)
    finally:
        for v in b.values():
            if hasattr(v, "free"):
                v.free()
    for k, a in got.items():
        assert (a[..., C:] == (FILL32 if a.dtype == np.int32 else FILL64)).all(), f"{k}: a column past C was touched"
    out = {k: a[..., :C] for k, a in got.items()}
    out["n_range"] = int(cnt[0])
    return out


def run_whole(dev, d, zq, classes, K, block=0):
    b = buffers(dev, K, zq.shape[1], d["ts"].shape[1])
    raw_accumulate(dev, d, zq, classes, K, block=block, out=b)
    return result(b)


def same(got, want):
    for k in FIELDS:
        assert got[k].dtype == want[k].dtype, k
        npt.assert_array_equal(got[k], want[k], err_msg=k)
    assert got["n_range"] == want["n_range"]


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("C", [1, 63, 64, 65, 255, 256, 257, 600])
def test_cell_counts_around_a_wave_and_a_workgroup(dev, dtype, C):
    T, J = 300, 3
    d, zq = _case(T, C, dtype, 1000 + C, J)
    for pattern in rc.PATTERNS:
        classes, K = pattern(T)
        want = _want(T, C, dtype, 1000 + C, J, 1, pattern)
        if C >= 63:
            rc.check_case(want)
        for block in (0, 64):
            same(run_whole(dev, d, zq, classes, K, block=block), want)


@pytest.mark.parametrize("J", [1, 7, 8, 9, 16, 17, 32])
def test_predictor_counts_around_the_group_sizes(dev, J):
    """every instantiation, full and with padded columns: outputs are [K][J][ldo], so a padded column that leaked would
    land in the next class's rows or past the end, where the fill pattern is checked"""
    T, C = 300, 130
    d, zq = _case(T, C, "float32", 50 + J, J)
    for pattern in (rc.runs, rc.every_step):
        classes, K = pattern(T)
        want = _want(T, C, "float32", 50 + J, J, 1, pattern)
        rc.check_case(want)
        for block in (0, 65):
            same(run_whole(dev, d, zq, classes, K, block=block), want)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_forced_blocks_give_identical_bits(dev, dtype):
    """1 / 64 / 65 / 10**6 / automatic on a series with NaN at step 0, at t0 - 1, at t0 and in pairs, class changes and
    runs of -1 on and beside the block edges, labels that change every step: the n1 / saa1 rule across block, class and
    NaN boundaries"""
    T, C, J = 400, 200, 9
    d, zq = _case(T, C, dtype, 7, J)
    ts = d["ts"]
    assert np.isnan(ts[0]).any() and np.isnan(ts[63]).any() and np.isnan(ts[64]).any() and np.isnan(ts[65]).any()
    assert (np.isnan(ts[63]) & np.isnan(ts[64])).any() and (np.isnan(ts[63]) & ~np.isnan(ts[64])).any()
    for pattern in rc.PATTERNS:
        classes, K = pattern(T)
        want = _want(T, C, dtype, 7, J, 1, pattern)
        rc.check_case(want)
        for block in (1, 64, 65, 10 ** 6, 0):
            same(run_whole(dev, d, zq, classes, K, block=block), want)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_a_climatology_base_with_its_rows(dev, dtype):
    T, C, J = 400, 257, 4
    d, zq = _case(T, C, dtype, 44, J, 366)
    assert d["rows"].max() == 365 and (np.diff(d["rows"]) < 0).any()
    for pattern in (rc.runs, rc.every_step):
        classes, K = pattern(T)
        want = _want(T, C, dtype, 44, J, 366, pattern)
        rc.check_case(want)
        for block in (0, 1, 83):
            same(run_whole(dev, d, zq, classes, K, block=block), want)


def test_missing_data_and_out_of_range_samples(dev):
    T, C, J = 200, 70, 5
    d, zq = _case(T, C, "float32", 5, J)
    classes, K = rc.every_step(T)
    clean = ro.regress_sums(d["ts"], d["base"], d["rows"], classes, K, zq)
    # the cell that is all NaN: nothing valid, the deficits are the class totals
    assert np.isnan(d["ts"][:, 2]).all() and (clean["n"][:, 2] == 0).all()
    for k in range(K):
        npt.assert_array_equal(clean["mz"][k, :, 2], zq[classes == k].astype(np.int64).sum(axis=0))
    bad = dict(d, ts=d["ts"].copy())
    steps = [t for t in range(T) if classes[t] >= 0]
    spots = [(steps[3], 0), (steps[4], 5), (steps[-2], 64), (steps[-1], 69)]
    for (t, c), v in zip(spots, (500.0, np.inf, -np.inf, -160.0)):
        bad["ts"][t, c] = v
    t_skipped = int(np.nonzero(classes < 0)[0][0])
    bad["ts"][t_skipped, 7] = 900.0                                # a step of class -1 is not read: not counted either
    want = ro.regress_sums(bad["ts"], bad["base"], bad["rows"], classes, K, zq)
    assert want["n_range"] == 4 and clean["n_range"] == 0
    got = run_whole(dev, bad, zq, classes, K)
    same(got, want)
    untouched = np.ones(C, bool)
    untouched[[0, 5, 64, 69]] = False
    for k in FIELDS:
        npt.assert_array_equal(got[k][..., untouched], clean[k][..., untouched])


def test_largest_magnitudes_do_not_overflow(dev):
    """T = 2**17 - 1, samples at +-(2**7 - 2**-16) from the base, zq = +-(2**23 - 1) with a fixed sign pattern: the sums
    reach within a few parts in 10**5 of 2**63 and equal the Python-integer sums.  The one place a 64-bit overflow or a
    sign slip in the multiply-add would show."""
    T, C, J = (1 << 17) - 1, 64, 2
    t, c = np.arange(T)[:, None], np.arange(C)[None, :]
    big = 128.0 - 2.0 ** -16
    # cells 0..31 keep one sign throughout, the others alternate in runs of c steps: both the extreme and the cancelling sums
    sign_a = np.where(c < 32, np.where(c % 2 == 0, 1.0, -1.0), np.where((t // (c + 1)) % 2 == 0, 1.0, -1.0))
    ts = 1.0 + sign_a * big                                          # float64: exact
    zq = np.empty((T, J), np.int32)
    zq[:, 0] = (1 << 23) - 1
    zq[:, 1] = np.where(np.arange(T) % 3 == 0, -1, 1) * ((1 << 23) - 1)
    d = {"ts": ts, "base": np.ones((1, C)), "rows": np.zeros(T, np.int32)}
    classes = np.zeros(T, np.int32)
    want = ro.regress_sums(ts, d["base"], d["rows"], classes, 1, zq)
    q = (1 << 23) - 1
    assert want["saz"][0, 0, 0] == T * q * q and want["saz"][0, 0, 1] == -T * q * q and want["saa"][0, 0] == T * q * q
    assert want["saz"][0, 0, 0] > (1 << 63) - (1 << 47) and want["n_range"] == 0
    same(run_whole(dev, d, zq, classes, 1), want)


def test_slabs_add_up_to_the_whole(dev):
    T, C, J = 300, 330, 6
    d, zq = _case(T, C, "float32", 77, J)
    classes, K = rc.runs(T)
    want = _want(T, C, "float32", 77, J, 1, rc.runs)
    for cuts in ((0, 129, C), (0, 1, 257, C), (0, 64, 65, C)):
        b = buffers(dev, K, J, C)
        for c0, c1 in zip(cuts[:-1], cuts[1:]):
            raw_accumulate(dev, d, zq, classes, K, c0=c0, n=c1 - c0, out=b)
        same(result(b), want)
    # a single-cell slab alone: the other columns keep the zeros of init
    b = buffers(dev, K, J, C)
    raw_accumulate(dev, d, zq, classes, K, c0=200, n=1, out=b)
    got = result(b)
    for k in FIELDS:
        npt.assert_array_equal(got[k][..., 200], want[k][..., 200])
        assert (got[k][..., :200] == 0).all() and (got[k][..., 201:] == 0).all()


def _grid(T, ny, nx, seed):
    rng = np.random.default_rng(seed)
    time = np.datetime64("2001-01-01") + np.arange(T).astype("timedelta64[D]")
    x = (20.0 + 3.0 * np.sin(2 * np.pi * np.arange(T) / 365.25)[:, None, None] + rng.normal(0, 1.2, (T, ny, nx))).astype(np.float32)
    x[:, rng.random((ny, nx)) < 0.3] = np.nan
    x[:, 2, :] = np.nan                                              # a dead grid line
    x[rng.random(x.shape) < 0.01] = np.nan
    from xmhw_amd import GridSeries
    return GridSeries(x, ("time", "lat", "lon"), {"time": time, "lat": np.arange(ny) * 0.25, "lon": np.arange(nx) * 0.25})


DATASET_FIELDS = FIELDS + ("klass", "n_steps", "keep", "mean", "slope", "intercept", "r", "r1", "r1z", "n_eff", "p_value")


def test_public_function_equals_the_host_path_with_the_oracle(dev, oisst):
    from xmhw_amd import GridSeries, index_regression
    temp = GridSeries(oisst["sst"], ("time", "lat", "lon"), {"time": oisst["time64"], "lat": oisst["lat"], "lon": oisst["lon"]})
    for series in (temp, _grid(500, 9, 14, 4)):
        T = series.values.shape[0]
        rng = np.random.default_rng(T)
        nino = np.cumsum(rng.normal(0, 0.1, T))
        nino[T // 2] = np.nan
        indices = {"nino34": nino, "iod": np.sin(np.arange(T) / 40.0) + rng.normal(0, 0.2, T)}
        land = np.isnan(series.values).all(axis=0)                   # the base pairs with the ocean cells
        base = np.where(land, np.nan, 20.0 if series is not temp else np.nan_to_num(np.nanmax(np.where(land, 0.0, series.values), axis=0)) - 3.0)
        for kw in (dict(), dict(max_batch_bytes=1 << 14), dict(classes="season", lags=(0, 30, 60), standardize=False)):
            got = index_regression(series, base, indices, **kw)
            host = index_regression(series, base, indices, _compute=ro.regress_cells,
                                    **{k: v for k, v in kw.items() if k != "max_batch_bytes"})
            for k in DATASET_FIELDS:
                npt.assert_array_equal(getattr(got, k), getattr(host, k), err_msg=k)
            assert got.keep.sum() > 0 and got.n.sum() > 0 and got.n_dropped > 0
    # a point series
    p = GridSeries(oisst["sst"][:, 2, 2], ("time",), {"time": oisst["time64"]})
    ix = {"x": np.cos(np.arange(p.values.shape[0]) / 25.0)}
    a, b = index_regression(p, 27.0, ix, lags=(0, 5)), index_regression(p, 27.0, ix, lags=(0, 5), _compute=ro.regress_cells)
    for k in DATASET_FIELDS:
        npt.assert_array_equal(getattr(a, k), getattr(b, k), err_msg=k)
