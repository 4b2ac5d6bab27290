"""anomaly_distribution() on the device against tests/distribution_oracle.py: exact equality of every integer -- the
histogram rows, n, the 64-bit and the 128-bit sums in both words, the ranks and the level counts of the finish pass, the
counter -- and of the two extremes.  The C entries are called raw, on pitched inputs (the columns past C hold valid samples
in range) and outputs pre-filled with a bit pattern that must be gone inside [0, C) and intact beyond it; every forced block
length must give the same bits.  Then the public function on a grid with land, in several slabs, against the oracle and
against numpy on the unquantised anomalies within quantisation_bound()."""
import functools

import numpy as np
import numpy.testing as npt
import pytest

import distribution_cases as dc
import distribution_oracle as do
import lag_correlation_cases as lc

pytestmark = pytest.mark.gpu

EXTRA_IN, EXTRA_OUT = 5, 3      # columns past C in the pitched inputs and outputs
FILL32, FILL64 = -0x5A5A5A5B, -0x5A5A5A5A5A5A5A5B
T0, C0 = 400, 300               # a full and a ragged workgroup
ACC = {"hist": np.int32, "n": np.int32, "s1": np.int64, "s2": np.int64, "s3": np.int64, "s4": np.int64, "kmin": np.int64,
       "kmax": np.int64}
FIN = ("qbin", "qbelow", "qcount", "n_at_least")
P5 = (0.05, 0.25, 0.5, 0.75, 0.95)


def p_q_of(p):
    return np.rint(np.asarray(p, dtype=np.float64) * 4294967296.0).astype(np.uint64)


@pytest.fixture(scope="module")
def dev():
    from xmhw_amd._lib import require_gpu
    require_gpu()
    import xmhw_amd.device as d
    return d


@pytest.fixture(autouse=True)
def automatic_block_afterwards():
    yield
    from xmhw_amd._lib import hip_distribution
    hip_distribution().set_distribution_block(0)


@functools.lru_cache(maxsize=None)
def _case(T, C, dtype, seed, bins, Dr=1, shift=0):
    return dc.series(T, C, np.dtype(dtype).type, seed, *bins, Dr=Dr, shift=shift)


@functools.lru_cache(maxsize=None)
def _want(T, C, dtype, seed, bins, Dr, shift, pattern, p, edges, K=None):
    d = _case(T, C, dtype, seed, bins, Dr, shift)
    classes, K0 = pattern(T)
    return do.distribution_sums(d["x"], d["base"], d["rows"], shift, classes, K or K0, *bins, [int(v) for v in p_q_of(p)],
                                list(edges))


def _pitched(a, ld, fill):
    out = np.full(a.shape[:-1] + (ld,), fill, dtype=a.dtype)
    out[..., :a.shape[-1]] = a
    return out


def _shapes(K, B, P, L, ldo):
    return {"hist": (K, B + 2, ldo), "n": (K, ldo), "s1": (K, ldo), "s2": (K, ldo), "s3": (K, 2, ldo), "s4": (K, 2, ldo),
            "kmin": (K, ldo), "kmax": (K, ldo), "qbin": (K, P, ldo), "qbelow": (K, P, ldo), "qcount": (K, P, ldo),
            "n_at_least": (K, L, ldo)}


def buffers(dev, K, B, C, P=0, L=0, init=True):
    from xmhw_amd._lib import hip_distribution
    ldo = C + EXTRA_OUT
    shp = _shapes(K, B, P, L, ldo)
    b = {k: dev.DeviceBuffer.from_array(np.full(shp[k], FILL32 if dt is np.int32 else FILL64, dt)) for k, dt in ACC.items()}
    b.update({k: dev.DeviceBuffer.from_array(np.full(shp[k] if np.prod(shp[k]) else (1,), FILL32, np.int32)) for k in FIN})
    b.update(cnt=dev.DeviceBuffer.from_array(np.full(1, 123, np.int64)), ldo=ldo, K=K, B=B, C=C, P=P, L=L)
    if init:
        hip_distribution().distribution_init(K, B, C, *(b[k].ptr for k in ACC), ldo, b["cnt"].ptr)
    return b


def raw_accumulate(dev, d, classes, K, bins, shift=0, block=0, c0=0, n=None, out=None):
    """xmhw_distribution_accumulate_* on the columns c0 .. c0 + n - 1 of the case (all of them by default) into the buffers
    ``out``; the inputs are pitched by EXTRA_IN columns of valid samples in range"""
    from xmhw_amd._lib import hip, hip_distribution
    x = d["x"]
    T, C = x.shape
    n = C - c0 if n is None else n
    ld = n + EXTRA_IN
    hip_distribution().set_distribution_block(block)
    held = [dev.DeviceBuffer.from_array(_pitched(x[:, c0:c0 + n], ld, 21.0)),
            dev.DeviceBuffer.from_array(_pitched(d["base"][:, c0:c0 + n], ld, 20.0))]
    ptrs = [out[k].ptr + np.dtype(dt).itemsize * c0 for k, dt in ACC.items()]
    try:
        hip_distribution().distribution_accumulate(held[0].ptr, x.dtype.itemsize, T, n, ld, held[1].ptr, ld,
                                                   d["base"].shape[0], d["rows"], shift, classes, K, *bins, *ptrs, out["ldo"],
                                                   out["cnt"].ptr)
        hip().stream_sync(0)
    finally:
        for b in held:
            b.free()


def finish(b, p=(), edges=()):
    from xmhw_amd._lib import hip, hip_distribution
    hip_distribution().distribution_finish(b["K"], b["B"], b["C"], b["hist"].ptr, b["n"].ptr, b["kmin"].ptr, b["kmax"].ptr,
                                           p_q_of(p), np.asarray(edges, dtype=np.int32), *(b[k].ptr for k in FIN), b["ldo"])
    hip().stream_sync(0)


def result(b, finished=True):
    """read back, check the columns past C, free; the extremes as float64 where the finish pass has run"""
    K, B, C, ldo, P, L = b["K"], b["B"], b["C"], b["ldo"], b["P"], b["L"]
    shp = _shapes(K, B, P, L, ldo)
    try:
        got = {k: b[k].to_array(shp[k], dt) for k, dt in ACC.items()}
        got.update({k: b[k].to_array(shp[k], np.int32) if np.prod(shp[k]) else np.zeros(shp[k], np.int32) for k in FIN})
        cnt = b["cnt"].to_array((1,), np.int64)
    finally:
        for v in b.values():
            if hasattr(v, "free"):
                v.free()
    for k, a in got.items():
        assert (a[..., C:] == (FILL32 if a.dtype == np.int32 else FILL64)).all(), f"{k}: a column past C was touched"
    out = {k: np.ascontiguousarray(a[..., :C]) for k, a in got.items()}
    if finished:
        out["kmin"], out["kmax"] = out["kmin"].view(np.float64), out["kmax"].view(np.float64)
    out["n_range"] = int(cnt[0])
    return out


def run_whole(dev, d, classes, K, bins, p=(), edges=(), **kw):
    b = buffers(dev, K, bins[2], d["x"].shape[1], len(p), len(edges))
    raw_accumulate(dev, d, classes, K, bins, out=b, **kw)
    finish(b, p, edges)
    return result(b)


def same(got, want, fields=None):
    for k in fields or (tuple(ACC) + FIN):
        assert got[k].dtype == want[k].dtype, k
        npt.assert_array_equal(got[k], want[k], err_msg=k)                  # (NaN equals NaN here: no sample)
    assert got["n_range"] == want["n_range"]


def check_case(want, B):
    """on the oracle's side: a case without samples in every kind of row, or without a 128-bit sum that needs its high
    word, proves nothing"""
    h = want["hist"]
    assert h[:, 0].sum() > 0 and h[:, B + 1].sum() > 0 and h[:, 1:B + 1].sum() > 0 and want["n_range"] > 0
    assert (want["s3"][:, 1] != 0).any() and (want["s3"][:, 1] != -1).any() and (want["s4"][:, 1] > 0).any()
    assert (want["n"] == 0).any() and (want["n"] == h.sum(axis=1)).all()


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("B", dc.BIN_COUNTS)
def test_every_bin_count_class_pattern_and_kind_of_width(dev, dtype, B):
    """an odd B and both sides of each LDS size; the four class patterns; a width that is a power of two (a shift) and an
    odd one (the reciprocal and its correction step)"""
    for i, pattern in enumerate(dc.PATTERNS):
        bins = dc.bins_for(B, odd_width=i % 2 == 1)
        assert (bins[1] & (bins[1] - 1) == 0) == (i % 2 == 0)
        edges = (0, B // 2, B)
        d = _case(T0, C0, dtype, 11, bins)
        classes, K = pattern(T0)
        want = _want(T0, C0, dtype, 11, bins, 1, 0, pattern, P5, edges)
        check_case(want, B)
        same(run_whole(dev, d, classes, K, bins, P5, edges, block=(0, 83)[i // 2]), want)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_forced_blocks_give_identical_bits(dev, dtype):
    """1 / 7 / 64 / 400 / automatic: a block starts from an empty column and leaves one behind"""
    bins = dc.bins_for(65, odd_width=True)
    d = _case(T0, C0, dtype, 7, bins)
    for pattern in (lc.every_step, lc.long_runs_of_minus_one):
        classes, K = pattern(T0)
        want = _want(T0, C0, dtype, 7, bins, 1, 0, pattern, P5, (1,))
        check_case(want, 65)
        for block in (1, 7, 64, 400, 0):
            same(run_whole(dev, d, classes, K, bins, P5, (1,), block=block), want)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_base_of_five_rows_that_are_not_monotone_and_a_shift(dev, dtype):
    bins = dc.bins_for(128)
    for Dr, shift in ((5, 0), (5, 3), (1, 3)):
        d = _case(T0, C0, dtype, 44, bins, Dr, shift)
        assert d["rows"].max() == Dr - 1 and (Dr == 1 or (np.diff(d["rows"]) < 0).any())
        classes, K = lc.seasons(T0)
        want = _want(T0, C0, dtype, 44, bins, Dr, shift, lc.seasons, P5, (64,))
        assert want["hist"][:, 1:129].sum() > 0 and want["n_range"] > 0 and (want["s3"][:, 1] != 0).any()
        for block in (0, 7):
            same(run_whole(dev, d, classes, K, bins, P5, (64,), shift=shift, block=block), want)


def test_two_slabs_equal_one_call_and_init_clears_its_columns_alone(dev):
    bins = dc.bins_for(64)
    d = _case(T0, C0, "float32", 77, bins)
    classes, K = lc.seasons(T0)
    want = _want(T0, C0, "float32", 77, bins, 1, 0, lc.seasons, P5, (0, 64))
    check_case(want, 64)
    b = buffers(dev, K, 64, C0, 5, 2)
    raw_accumulate(dev, d, classes, K, bins, c0=0, n=170, out=b)
    raw_accumulate(dev, d, classes, K, bins, c0=170, n=C0 - 170, out=b)
    finish(b, P5, (0, 64))
    same(result(b), want)                                                   # (the counter adds up as well)
    # init alone: zeros inside [0, C), the fill beyond (result() checks it), the counter zero
    got = result(buffers(dev, K, 64, C0), finished=False)
    assert all((got[k] == 0).all() for k in ACC) and got["n_range"] == 0
    # init on the columns of the second slab alone clears those alone
    from xmhw_amd._lib import hip, hip_distribution
    b = buffers(dev, K, 64, C0, init=False)
    hip_distribution().distribution_init(K, 64, C0 - 170, *(b[k].ptr + np.dtype(dt).itemsize * 170 for k, dt in ACC.items()),
                                         b["ldo"], b["cnt"].ptr)
    hip().stream_sync(0)
    got = result(b, finished=False)
    for k, dt in ACC.items():
        assert (got[k][..., 170:] == 0).all() and (got[k][..., :170] == (FILL32 if dt is np.int32 else FILL64)).all(), k


LONG_T, LONG_C = 70000, 64


@pytest.mark.parametrize("odd", [False, True])
def test_a_half_never_receives_more_than_it_holds(dev, odd):
    """70,000 steps of one class in ONE block, a constant series: the one bin holds 70,000 -- the run was flushed at 65,535
    steps -- and the other half of its dword holds 0"""
    bins = (-4 * 65536, 65536, 8)                                           # bins of 1.0 from -4
    b = 4 + int(odd)
    x = np.full((LONG_T, LONG_C), b - 4 + 0.25, np.float32)
    d = {"x": x, "base": np.zeros((1, LONG_C)), "rows": np.zeros(LONG_T, np.int32)}
    got = run_whole(dev, d, np.zeros(LONG_T, np.int32), 1, bins, block=LONG_T)
    assert (got["hist"][0, 1 + b] == LONG_T).all() and (got["hist"][0, 1 + (b ^ 1)] == 0).all()
    assert got["hist"].sum() == LONG_T * LONG_C and (got["n"] == LONG_T).all() and got["n_range"] == 0
    q = int((b - 4 + 0.25) * 65536)
    assert (got["s1"] == LONG_T * q).all() and (got["s2"] == LONG_T * q * q).all()


@pytest.mark.parametrize("pattern", [lc.every_step, lc.one_class])
def test_sums_of_128_bits_in_both_words(dev, pattern):
    """a column of 127.99 and a column alternating +-127.99 over 70,000 steps: with labels that change every step every
    step is a flush and the carries cross flushes of many blocks; s3 and s4 equal the Python integers in both words"""
    x = np.full((LONG_T, LONG_C), 127.99, np.float32)
    x[1::2, 1::2] = -x[1::2, 1::2]                                          # odd columns alternate
    q = int(np.rint(np.float64(np.float32(127.99)) * 65536.0))
    assert q > (1 << 23) - 2000
    d = {"x": x, "base": np.zeros((1, LONG_C)), "rows": np.zeros(LONG_T, np.int32)}
    classes, K = pattern(LONG_T)
    bins = (-128 * 65536, 65536, 256)
    got = run_whole(dev, d, classes, K, bins)
    S3, S4 = np.zeros((K, LONG_C), object), np.zeros((K, LONG_C), object)
    t = np.arange(LONG_T)
    for k in range(K):
        nk = int((classes == k).sum())
        odd_steps = int(((classes == k) & (t % 2 == 1)).sum())
        S3[k, 0::2], S4[k, :] = nk * q ** 3, nk * q ** 4
        S3[k, 1::2] = (nk - 2 * odd_steps) * q ** 3
        assert (got["n"][k] == nk).all()
    assert int(S4.max()) >> 64 > 0 and int(S3[:, 0].max()) >> 64 > 0
    npt.assert_array_equal(got["s3"], do.words(S3))
    npt.assert_array_equal(got["s4"], do.words(S4))
    assert (got["hist"][:, 1 + 255, 0::2] == got["n"][:, 0::2]).all()         # 127.99 is in the last bin


def test_finish_ranks_and_levels(dev):
    """16 probabilities with 0, 1 and duplicates, ranks that fall in UNDER and in OVER, a class without a sample; 8 levels
    with the edges 0 and B"""
    bins = (-65536, 32768, 4)                                               # four bins of 0.5 from -1: most samples outside
    p = (0.0, 1.0, 0.5, 0.5, 0.01, 0.99, 0.3, 0.45, 0.55, 0.7, 0.25, 0.75, 2.0 ** -32, 1.0 - 2.0 ** -32, 0.499999, 1.0)
    edges = (0, 4, 1, 2, 3, 2, 0, 4)
    d = _case(T0, C0, "float32", 3, bins)
    classes, _ = lc.long_runs_of_minus_one(T0)
    want = _want(T0, C0, "float32", 3, bins, 1, 0, lc.long_runs_of_minus_one, p, edges, K=3)
    assert (want["qbin"] == -1).any() and (want["qbin"] == 4).any() and (want["qbin"][2] == do.NO_SAMPLE).all()
    assert ((want["qbin"] >= 0) & (want["qbin"] < 4)).any() and (want["n"][2] == 0).all()
    assert (want["n_at_least"][:, 0] == want["n"] - want["hist"][:, 0]).all()
    assert (want["n_at_least"][:, 1] == want["hist"][:, 5]).all() and want["n_at_least"][:, 1].sum() > 0
    got = run_whole(dev, d, classes, 3, bins, p, edges)
    same(got, want)
    assert np.isnan(got["kmin"][2]).all() and np.isnan(got["kmax"][2]).all()


# ---- the public function ---------------------------------------------------------------------------------------------

NY, NX = 9, 14


@pytest.fixture(scope="module")
def field():
    """four years of a 9 x 14 grid with land: a skewed, persistent anomaly around a mean of 18"""
    from xmhw_amd import GridSeries
    rng = np.random.default_rng(12)
    time = np.arange("2000-01-01", "2004-01-01", dtype="datetime64[D]")
    T = time.shape[0]
    e = rng.gamma(2.0, 0.6, (T, NY, NX)) - 1.2
    a = np.zeros_like(e)
    for t in range(1, T):
        a[t] = 0.7 * a[t - 1] + e[t]
    sst = (18.0 + a).astype(np.float32)
    sst[rng.random(sst.shape) < 0.01] = np.nan
    land = rng.random((NY, NX)) < 0.25
    land[0, 0], land[1, 1] = True, False
    assert (~land).any(axis=0).all() and (~land).any(axis=1).all() and (~land).sum() > 80
    sst[:, land] = np.nan
    coords = {"time": time, "lat": np.arange(NY) * 0.25, "lon": np.arange(NX) * 0.25}
    return dict(time=time, land=land, sst=GridSeries(sst, ("time", "lat", "lon"), coords))


def test_public_function_in_several_slabs(dev, field):
    from xmhw_amd import anomaly_distribution
    g = field
    T = g["time"].shape[0]
    keep = ~g["land"].reshape(-1)
    x = np.asarray(g["sst"].values).reshape(T, -1)[:, keep]
    C = x.shape[1]
    month = (g["time"].astype("datetime64[M]").astype(int) % 12).astype(np.int32)
    season = ((month + 1) % 12) // 3
    rows = np.zeros(T, np.int32)
    lo_q, width_q, B = -6 * 65536, 4096, 192                                # bins of 1/16 from -6 to 6
    p, levels = (0.05, 0.5, 0.95, 0.99), (1.0, 2.5)
    edges = [int((v * 65536 - lo_q) // width_q) for v in levels]
    want = do.distribution_sums(x, np.full((1, C), 18.0), rows, 0, season, 4, lo_q, width_q, B, [int(v) for v in p_q_of(p)], edges)
    assert want["n_range"] == 0 and want["n"].min() > 300
    per_cell = T * 4 + 4 * 8 + 64
    for kw in (dict(), dict(max_batch_bytes=30 * per_cell)):
        got = anomaly_distribution(g["sst"], base=np.full((NY, NX), 18.0), bins=(-6.0, 6.0, 192), quantiles=p, levels=levels,
                                   classes="season", return_histogram=True, **kw)
        assert got.klass.tolist() == [0, 1, 2, 3]
        for k, name in (("n", "n"), ("s1", "s1"), ("s2", "s2"), ("s3", "s3"), ("s4", "s4"), ("qbin", "quantile_bin"),
                        ("n_at_least", "exceedance"), ("hist", "histogram")):
            a = getattr(got, name)
            a = a.reshape(a.shape[:-2] + (-1,))
            assert a.dtype == want[k].dtype, k
            npt.assert_array_equal(a[..., keep], want[k], err_msg=k)
            assert (a[..., ~keep] == (do.NO_SAMPLE if k == "qbin" else 0)).all()
        npt.assert_array_equal(got.keep.reshape(-1), keep)
    # the quantile brackets the exact order statistic of the quantised samples within its bin
    quant = got.quantile.reshape(4, len(p), -1)[..., keep]
    for k in range(4):
        for j, pq in enumerate(p_q_of(p)):
            r = np.array([do.rank(int(pq), int(v)) for v in want["n"][k]])
            exact = want["sorted"][k][r - 1, np.arange(C)]                  # q of the r-th smallest
            b = (exact - lo_q) // width_q
            assert ((b >= 0) & (b < B)).all()
            edge = (lo_q + b * width_q) / 65536.0
            assert (edge <= exact / 65536.0).all() and (exact / 65536.0 < edge + width_q / 65536.0).all()
            assert (edge <= quant[k, j]).all() and (quant[k, j] < edge + width_q / 65536.0).all()
    # the moments against numpy float64 on the unquantised anomalies, within the stated bounds
    bound = got.quantisation_bound()
    a = x.astype(np.float64) - 18.0
    for k in range(4):
        for c in range(C):
            v = a[season == k, c]
            v = v[~np.isnan(v)]
            m = v.mean()
            m2, m3, m4 = ((v - m) ** 2).mean(), ((v - m) ** 3).mean(), ((v - m) ** 4).mean()
            ref = {"mean": m, "variance": m2, "skewness": m3 / m2 ** 1.5, "kurtosis": m4 / m2 ** 2 - 3.0, "minimum": v.min(),
                   "maximum": v.max()}
            for name, r in ref.items():
                value = getattr(got, name).reshape(4, -1)[:, keep][k, c]
                limit = bound[name] if np.isscalar(bound[name]) else bound[name].reshape(4, -1)[:, keep][k, c]
                # (numpy's own rounding of a moment, a few ulps of terms of its size: 1e-12 of it; the extremes are exact)
                slack = 0.0 if name in ("minimum", "maximum") else 1e-12 * max(abs(r), 1.0)
                assert np.isfinite(limit) and abs(value - r) <= limit + slack, (name, k, c, value, r, limit)
    assert np.nanmedian(got.skewness) > 0.3                                 # the gamma noise is skewed to the warm side
    prob = got.exceedance_probability.reshape(4, 2, -1)[..., keep]
    assert (prob[:, 0] > prob[:, 1]).all() and (prob[:, 1] > 0).any()
    assert np.isnan(got.mean.reshape(4, -1)[:, ~keep]).all()
