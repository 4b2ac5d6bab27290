"""mhw_composite() on the device against tests/composite_oracle.py: exact equality of every array.  The C entries are
called raw, on pitched inputs and outputs pre-filled with a bit pattern that must be gone inside [0, C) and intact beyond
it; every forced block length must give the same bits.  Then the public function on a 40-year grid with land, against
the oracle fed with the same detect() table."""
import functools

import numpy as np
import numpy.testing as npt
import pytest

import composite_cases as cc
import composite_oracle as co

pytestmark = pytest.mark.gpu

EXTRA = 5                       # columns past C in every pitched array
FILL32, FILL64 = -0x5A5A5A5B, -0x5A5A5A5A5A5A5A5B
FIELDS = co.FIELDS
DTYPES = {"n": np.int32, "s": np.int64, "ss": np.int64}


@pytest.fixture(scope="module")
def dev():
    from xmhw_amd._lib import require_gpu
    require_gpu()
    import xmhw_amd.device as d
    return d


@pytest.fixture(autouse=True)
def automatic_block_afterwards():
    yield
    from xmhw_amd._lib import hip_composite
    hip_composite().set_composite_block(0)


@functools.lru_cache(maxsize=None)
def _case(T, C, dtype, seed, Dr=1):
    return cc.series(T, C, np.dtype(dtype).type, seed, Dr=Dr)


@functools.lru_cache(maxsize=None)
def _anchors(T, C, D):
    return cc.anchor_columns(T, C, D)


@functools.lru_cache(maxsize=None)
def _want(T, C, dtype, seed, Dr, pattern, before, after, shift=0):
    d = _case(T, C, dtype, seed, Dr)
    classes, K = pattern(T)
    return co.composite_sums(d["ts"], d["base"], d["rows"], shift, _anchors(T, C, before + after + 1), classes, K, before, after)


def _pitched(a, ld, fill):
    out = np.full(a.shape[:-1] + (ld,), fill, dtype=a.dtype)
    out[..., :a.shape[-1]] = a
    return out


def buffers(dev, K, D, C):
    from xmhw_amd._lib import hip_composite
    ldo = C + EXTRA
    b = {k: dev.DeviceBuffer.from_array(np.full((K, D, ldo), FILL32 if dt is np.int32 else FILL64, dt)) for k, dt in DTYPES.items()}
    b.update(cnt=dev.DeviceBuffer.from_array(np.full(1, 123, np.int64)), ldo=ldo, K=K, D=D, C=C)
    hip_composite().composite_init(K, D, C, *(b[k].ptr for k in FIELDS), ldo, b["cnt"].ptr)
    return b


def raw_accumulate(dev, d, anchors, classes, K, before, after, shift=0, block=0, c0=0, n=None, out=None):
    """xmhw_composite_accumulate_* on the columns c0 .. c0 + n - 1 of the case (all of them by default) into the buffers
    ``out``; the inputs are pitched by EXTRA columns that would be in range, valid and full of anchors if a kernel read
    them."""
    from xmhw_amd._lib import hip, hip_composite
    ts, base = d["ts"], d["base"]
    T, C = ts.shape
    n = C - c0 if n is None else n
    ld = n + EXTRA
    hip_composite().set_composite_block(block)
    d_ts = dev.DeviceBuffer.from_array(_pitched(ts[:, c0:c0 + n], ld, 21.0))
    d_base = dev.DeviceBuffer.from_array(_pitched(base[:, c0:c0 + n], ld, 20.0))
    d_bits = dev.DeviceBuffer.from_array(_pitched(cc.bitmap(anchors[:, c0:c0 + n]), ld, np.uint64(0xFFFFFFFFFFFFFFFF)))
    ptrs = [out[k].ptr + np.dtype(dt).itemsize * c0 for k, dt in DTYPES.items()]
    try:
        hip_composite().composite_accumulate(d_ts.ptr, ts.dtype.itemsize, T, n, ld, d_base.ptr, ld, base.shape[0], d["rows"],
                                             shift, d_bits.ptr, ld, classes, K, before, after, *ptrs, out["ldo"],
                                             out["cnt"].ptr)
        hip().stream_sync(0)
    finally:
        d_ts.free()
        d_base.free()
        d_bits.free()


def result(b):
    """read back, check the columns past C, free"""
    K, D, C, ldo = b["K"], b["D"], b["C"], b["ldo"]
    try:
        got = {k: b[k].to_array((K, D, ldo), dt) for k, dt in DTYPES.items()}
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


def run_whole(dev, d, anchors, classes, K, before, after, shift=0, block=0):
    b = buffers(dev, K, before + after + 1, d["ts"].shape[1])
    raw_accumulate(dev, d, anchors, classes, K, before, after, shift=shift, block=block, out=b)
    return result(b)


def same(got, want):
    for k in FIELDS:
        assert got[k].dtype == want[k].dtype, k
        npt.assert_array_equal(got[k], want[k], err_msg=k)
    assert got["n_range"] == want["n_range"]


def check_case(want):
    """on the oracle's side: a case without samples or without a non-zero sum proves nothing"""
    assert want["n"].sum() > 0 and (want["s"] != 0).any() and (want["ss"] > 0).any()


@pytest.mark.parametrize("window", cc.WINDOWS)
def test_window_lengths_one_and_two_words(dev, window):
    """every window shape, D = 64 (the full single word) and D = 65 (the first two-word case) among them, on columns
    whose anchors sit at steps 0 and T - 1, on the word edges, 1 and D - 1 apart, on every step, and nowhere"""
    before, after = window
    T, C = 300, 130
    d, A = _case(T, C, "float32", 11), _anchors(T, C, before + after + 1)
    assert A[:, 4].all() and not A[:, 5].any() and A[0, 0] and A[T - 1, 0] and A[[63, 64, 127, 128], 1].all()
    for pattern in cc.PATTERNS:
        classes, K = pattern(T)
        want = _want(T, C, "float32", 11, 1, pattern, before, after)
        check_case(want)
        for block in (0, 100):
            same(run_whole(dev, d, A, classes, K, before, after, block=block), want)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("T", [1, 64, 65, 130, 300])
def test_series_lengths_around_the_word_edges(dev, dtype, T):
    C = 70
    d = _case(T, C, dtype, 20 + T)
    for before, after in ((0, 0), (30, 30), (63, 64)):
        A = _anchors(T, C, before + after + 1)
        for pattern in (cc.every_step, cc.stretches_of_minus_one):
            classes, K = pattern(T)
            want = _want(T, C, dtype, 20 + T, 1, pattern, before, after)
            if T > 1:
                check_case(want)
            for block in (0, 64):
                same(run_whole(dev, d, A, classes, K, before, after, block=block), want)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("C", [1, 63, 64, 65, 257, 600])
def test_cell_counts_around_a_wave_and_a_workgroup(dev, dtype, C):
    T = 130
    d = _case(T, C, dtype, 1000 + C)
    for before, after in ((5, 7), (40, 40)):
        A = _anchors(T, C, before + after + 1)
        for pattern in (cc.one_class, cc.every_step):
            classes, K = pattern(T)
            want = _want(T, C, dtype, 1000 + C, 1, pattern, before, after)
            check_case(want)
            for block in (0, 7):
                same(run_whole(dev, d, A, classes, K, before, after, block=block), want)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_forced_blocks_give_identical_bits(dev, dtype):
    """1 / 7 / 64 / 100 / T / automatic: a block builds its window from bitmap words alone, wherever it starts"""
    T, C = 300, 200
    d = _case(T, C, dtype, 7)
    for before, after in ((30, 30), (63, 64)):
        A = _anchors(T, C, before + after + 1)
        for pattern in (cc.every_step, cc.stretches_of_minus_one):
            classes, K = pattern(T)
            want = _want(T, C, dtype, 7, 1, pattern, before, after)
            check_case(want)
            for block in (1, 7, 64, 100, T, 0):
                same(run_whole(dev, d, A, classes, K, before, after, block=block), want)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_a_base_of_five_rows_that_is_not_monotone(dev, dtype):
    T, C = 200, 257
    d = _case(T, C, dtype, 44, 5)
    assert d["rows"].max() == 4 and (np.diff(d["rows"]) < 0).any() and d["base"].shape[0] == 5
    for before, after in ((4, 9), (70, 20)):
        A = _anchors(T, C, before + after + 1)
        classes, K = cc.every_step(T)
        want = _want(T, C, dtype, 44, 5, cc.every_step, before, after)
        check_case(want)
        for block in (0, 1, 83):
            same(run_whole(dev, d, A, classes, K, before, after, block=block), want)


def test_the_class_is_the_anchors_not_the_samples(dev):
    """anchors on the isolated steps of class 1, every other step of class 0: class 0 stays empty, and class 1 holds the
    whole windows although all their other samples lie on steps of class 0"""
    T, C, before, after = 300, 66, 20, 30
    d = _case(T, C, "float32", 3)
    classes, K = cc.anchor_class_apart(T)
    A = np.zeros((T, C), dtype=bool)
    A[classes == 1] = True
    A[:, 1::2] = False
    want = co.composite_sums(d["ts"], d["base"], d["rows"], 0, A, classes, K, before, after)
    assert want["n"][0].sum() == 0 and (want["n"][1, :, 0] > 0).all() and want["n"][1].sum() > 1000
    for block in (0, 64):
        same(run_whole(dev, d, A, classes, K, before, after, block=block), want)
    # the same anchors one step later: every anchor is of class 0
    B = np.roll(A, 1, axis=0)
    want = co.composite_sums(d["ts"], d["base"], d["rows"], 0, B, classes, K, before, after)
    assert want["n"][1].sum() == 0 and want["n"][0].sum() > 1000
    same(run_whole(dev, d, B, classes, K, before, after), want)


def test_missing_and_out_of_range_samples(dev):
    T, C, before, after = 200, 70, 10, 12
    d = _case(T, C, "float32", 5)
    classes, K = cc.stretches_of_minus_one(T)
    A = _anchors(T, C, before + after + 1)
    clean = co.composite_sums(d["ts"], d["base"], d["rows"], 0, A, classes, K, before, after)
    assert clean["n_range"] == 0 and (clean["n"][:, :, 2] == 0).all() and (clean["n"][:, :, 3] == 0).all()
    bad = dict(d, ts=d["ts"].astype(np.float64), base=d["base"].copy())
    touched = [0, 4, 7, 12, 15]                                      # ends, all ones, dense, all ones, dense
    bad["base"][0, touched] = 20.0
    # exactly +-2**7 from the base is out of range, one unit of the fixed point inside is not; infinities count
    for (t, c), v in zip(((5, 0), (51, 4), (52, 12), (60, 15), (61, 15), (62, 7)),
                         (148.0, -108.0, np.inf, 148.0 - 2.0 ** -16, -108.0 + 2.0 ** -16, -np.inf)):
        bad["ts"][t, c] = v
    bad["ts"][70, 5] = 900.0                                         # column 5 holds no anchor: read by nobody
    assert not A[:, 5].any() and A[:, 4].all()
    want = co.composite_sums(bad["ts"], bad["base"], bad["rows"], 0, A, classes, K, before, after)
    assert want["n_range"] > 4 and abs(want["s"][:, :, 15]).max() >= (1 << 23) - 1
    got = run_whole(dev, bad, A, classes, K, before, after)
    same(got, want)
    untouched = np.ones(C, bool)
    untouched[touched] = False
    for k in FIELDS:
        npt.assert_array_equal(got[k][..., untouched], clean[k][..., untouched])


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_shift_scales_exactly(dev, dtype):
    """values near 2**30 against a base of zero: out of range at shift 0 and 3, in range at shift 24, where
    q = value * 2**-8 exactly; and a unit-sized series at shift 3"""
    T, C, before, after = 130, 65, 6, 6
    rng = np.random.default_rng(8)
    ts = ((1 << 30) - 256.0 * rng.integers(0, 1000, (T, C))) * rng.choice([-1.0, 1.0], (T, C))
    d = {"ts": ts.astype(dtype), "base": np.zeros((1, C)), "rows": np.zeros(T, np.int32)}
    assert np.array_equal(d["ts"].astype(np.float64), ts)
    A = _anchors(T, C, before + after + 1)
    classes, K = cc.every_step(T)
    for shift in (0, 3, 24):
        want = co.composite_sums(d["ts"], d["base"], d["rows"], shift, A, classes, K, before, after)
        if shift == 24:
            check_case(want)
            assert want["n_range"] == 0 and abs(want["s"]).max() > 1 << 22
        else:
            assert want["n"].sum() == 0 and want["n_range"] > 1000
        same(run_whole(dev, d, A, classes, K, before, after, shift=shift), want)
    small = _case(T, C, dtype, 77)
    for shift in (0, 3):
        want = co.composite_sums(small["ts"], small["base"], small["rows"], shift, A, classes, K, before, after)
        check_case(want)
        same(run_whole(dev, small, A, classes, K, before, after, shift=shift), want)


def test_slabs_add_up_and_a_second_call_doubles(dev):
    T, C, before, after = 300, 330, 30, 40
    d = _case(T, C, "float32", 77)
    A = _anchors(T, C, before + after + 1)
    classes, K = cc.stretches_of_minus_one(T)
    want = _want(T, C, "float32", 77, 1, cc.stretches_of_minus_one, before, after)
    check_case(want)
    for cuts in ((0, 129, C), (0, 1, 257, C)):
        b = buffers(dev, K, before + after + 1, C)
        for c0, c1 in zip(cuts[:-1], cuts[1:]):
            raw_accumulate(dev, d, A, classes, K, before, after, c0=c0, n=c1 - c0, out=b)
        same(result(b), want)
    # accumulate ADDS: twice the call, twice every entry
    b = buffers(dev, K, before + after + 1, C)
    for block in (0, 64):
        raw_accumulate(dev, d, A, classes, K, before, after, block=block, out=b)
    got = result(b)
    for k in FIELDS:
        npt.assert_array_equal(got[k], 2 * want[k], err_msg=k)
    # a single-cell slab alone: the other columns keep the zeros of init
    b = buffers(dev, K, before + after + 1, C)
    raw_accumulate(dev, d, A, classes, K, before, after, c0=204, n=1, out=b)
    got = result(b)
    for k in FIELDS:
        npt.assert_array_equal(got[k][..., 204], want[k][..., 204])
        assert (got[k][..., :204] == 0).all() and (got[k][..., 205:] == 0).all()


# ---- the public function ---------------------------------------------------------------------------------------------

NY, NX = 6, 8


@pytest.fixture(scope="module")
def detected(dev):
    """40 years of a 6 x 8 grid with land, its detect() table and a second field with more land"""
    from xmhw_amd import GridSeries, threshold_detect
    rng = np.random.default_rng(12)
    time = np.arange("1982-01-01", "2022-01-01", dtype="datetime64[D]")
    T = time.shape[0]
    tt = np.arange(T)[:, None, None]
    noise = rng.normal(0, 1.0, (T, NY, NX))
    for t in range(1, T):                                            # persistence: events of a week and more
        noise[t] = 0.9 * noise[t - 1] + 0.45 * noise[t]
    sst = (18.0 + 4.0 * np.sin(2 * np.pi * tt / 365.25) + noise).astype(np.float32)
    land = rng.random((NY, NX)) < 0.2
    land[0, 0], land[1, 1], land[5, 7] = True, False, False
    assert (~land).any(axis=0).all() and (~land).any(axis=1).all()
    sst[:, land] = np.nan
    coords = {"time": time, "lat": np.arange(NY) * 0.25, "lon": np.arange(NX) * 0.25}
    temp = GridSeries(sst, ("time", "lat", "lon"), coords)
    clim, mhw = threshold_detect(temp)
    flux = (rng.normal(0, 40.0, (T, NY, NX)) - 30.0 * noise).astype(np.float32)
    flux[rng.random(flux.shape) < 0.01] = np.nan
    more_land = land.copy()
    more_land[1, 1], more_land[5, 7] = True, True
    assert not land[5, 7] and (~more_land).any(axis=0).all() and (~more_land).any(axis=1).all()
    flux[:, more_land] = np.nan
    return dict(time=time, temp=temp, clim=clim, mhw=mhw, land=land, more_land=more_land,
                flux=GridSeries(flux, ("time", "lat", "lon"), coords))


def _oracle_public(field, keep, base_rows, rows, mhw, anchor, select, kid, K, before, after, shift):
    """the oracle fed with detect()'s table: the anchors of the ocean cells of ``field`` by grid position"""
    T = field.shape[0]
    ts = field.reshape(T, -1)[:, keep]
    column_of_point = np.full(keep.shape[0], -1)
    column_of_point[keep] = np.arange(int(keep.sum()))
    A = np.zeros(ts.shape, dtype=bool)
    col = mhw.columns.index({"start": "index_start", "peak": "index_peak", "end": "index_end"}[anchor])
    cell_of_row = np.repeat(np.arange(mhw.n_cells), np.diff(mhw.offsets))
    for r in range(mhw.n_events):
        j = column_of_point[mhw.cell_index[cell_of_row[r]]]
        if j >= 0 and (select is None or select[r]):
            A[int(mhw.table[r, col]), j] = True
    return co.composite_sums(ts, base_rows[:, keep], rows, shift, A, kid, K, before, after), A


def _compare_public(got, want, A, kid, K, keep):
    D = want["n"].shape[1]
    for name, k in (("n", "n"), ("sum_q", "s"), ("sumsq_q", "ss")):
        a = getattr(got, name).reshape(K, D, -1)
        npt.assert_array_equal(a[..., keep], want[k], err_msg=name)
        assert (a[..., ~keep] == 0).all()
    n_anchors = np.stack([A[kid == k].sum(axis=0) for k in range(K)])
    npt.assert_array_equal(got.n_anchors.reshape(K, -1)[:, keep], n_anchors)
    npt.assert_array_equal(got.keep.reshape(-1), keep)
    assert np.isnan(got.mean.reshape(K, D, -1)[..., ~keep]).all()
    some = want["n"] >= 2
    npt.assert_allclose(got.mean.reshape(K, D, -1)[..., keep][some], (want["s"][some] / want["n"][some]) * 2.0 ** (got.shift - 16),
                        rtol=1e-14)
    assert np.isnan(got.mean.reshape(K, D, -1)[..., keep][~some]).all()


def test_public_function_on_a_grid_with_land(dev, detected):
    from xmhw_amd import climatology_series, mhw_composite
    from xmhw_amd import calendar as cal
    g = detected
    time, mhw = g["time"], g["mhw"]
    T = time.shape[0]
    assert mhw.n_events > 200
    sst, keep = np.asarray(g["temp"].values), ~g["land"].reshape(-1)
    month = time.astype("datetime64[M]").astype(int) % 12 + 1
    season = ((month % 12) // 3).astype(np.int32)
    zero = np.zeros(T, np.int32)
    # the SST anomaly around onset, peak and end: base = the seasonal climatology of threshold()
    seas = np.asarray(g["clim"]["seas"]).reshape(366, -1)
    assert seas.shape[1] == NY * NX
    rows = np.searchsorted(np.asarray(g["clim"].coords["doy"]), cal.add_doy(time))
    for anchor in ("start", "peak", "end"):
        got = mhw_composite(g["temp"], climatology_series(g["clim"], "seas"), mhw, anchor=anchor, before=20, after=25)
        want, A = _oracle_public(sst, keep, seas, rows, mhw, anchor, None, zero, 1, 20, 25, 0)
        assert want["n"].sum() > 10000 and got.n_cells_dropped == 0 and got.anchor == anchor
        _compare_public(got, want, A, zero, 1, keep)
    # the anomaly at the onset of an event is above the threshold: the composite says so
    start = mhw_composite(g["temp"], climatology_series(g["clim"], "seas"), mhw, before=3, after=3)
    assert np.nanmin(start.mean[0, 3]) > 0.5 and np.nanmax(start.p[0, 3]) < 1e-3
    # another field with more land, by season, a select mask, base=None, shift, three slabs
    flux, keep2 = np.asarray(g["flux"].values), ~g["more_land"].reshape(-1)
    select = mhw.table[:, mhw.columns.index("duration")] >= 8
    assert 0 < select.sum() < mhw.n_events
    per_cell = T * 16 + 4 * 8 + T // 8 + 64
    for kw in (dict(), dict(max_batch_bytes=20 * per_cell + 1000)):
        got = mhw_composite(g["flux"], None, mhw, anchor="peak", before=10, after=5, classes="season", select=select, shift=4,
                            **kw)
        want, A = _oracle_public(flux, keep2, np.zeros((1, NY * NX)), zero, mhw, "peak", select, season, 4, 10, 5, 4)
        assert want["n"].sum() > 1000 and got.n_cells_dropped == 2 and (got.klass == np.arange(4)).all()
        _compare_public(got, want, A, season, 4, keep2)
    # shift = 0 is too small for a flux of tens of W m-2
    from xmhw_amd.exception import XmhwException
    with pytest.raises(XmhwException, match="shift"):
        mhw_composite(g["flux"], None, mhw, shift=0)


def test_public_function_on_a_point_series(dev, detected):
    """the cells route: a single-point series and the events of its own detection"""
    from xmhw_amd import GridSeries, mhw_composite, threshold_detect
    g = detected
    j, i = np.argwhere(~g["land"])[3]
    x = np.asarray(g["temp"].values)[:, j, i]
    point = GridSeries(x, ("time",), {"time": g["time"]})
    _, ev = threshold_detect(point)
    assert ev.point and ev.n_events > 5
    T = x.shape[0]
    year = g["time"].astype("datetime64[Y]").astype(int)
    labels = np.where(year % 2 == 0, 7, -1)                            # one class, label 7; odd years count nowhere
    got = mhw_composite(point, 18.0, ev, anchor="end", before=5, after=40, classes=labels)
    A = np.zeros((T, 1), dtype=bool)
    A[ev.table[:, ev.columns.index("index_end")].astype(int), 0] = True
    kid = np.where(labels >= 0, 0, -1).astype(np.int32)
    want = co.composite_sums(x[:, None], np.full((1, 1), 18.0), np.zeros(T, np.int32), 0, A, kid, 1, 5, 40)
    assert want["n"].sum() > 100 and got.klass.tolist() == [7]
    for name, k in (("n", "n"), ("sum_q", "s"), ("sumsq_q", "ss")):
        npt.assert_array_equal(getattr(got, name), want[k][..., 0], err_msg=name)
    assert got.n_anchors.tolist() == [int(A[kid == 0].sum())]
