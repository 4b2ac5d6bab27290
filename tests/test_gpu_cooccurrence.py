"""mhw_cooccurrence() on the device against tests/cooccurrence_oracle.py: exact equality of every integer."""
import functools

import numpy as np
import numpy.testing as npt
import pytest

import cooccurrence_cases as cx
import cooccurrence_oracle as co
import coverage_cases as cc
import days_by_cases as dc

pytestmark = pytest.mark.gpu

TS = (1, 63, 64, 65, 130, 203)
CS = (1, 63, 64, 65, 257, 300)
PATTERNS = dc.PATTERNS + (cx.runs_with_gaps,)
ONES = np.uint64(0xFFFFFFFFFFFFFFFF)


@pytest.fixture(scope="module")
def dev():
    from xmhw_amd._lib import require_gpu
    require_gpu()
    import xmhw_amd.device as d
    return d


def lag_set(T):
    """the lags of the issue, without repeats (T - 1 is 0 for T = 1, T is 64 for T = 64 ...), in this order"""
    out = []
    for v in (0, 1, -1, 5, -7, 63, 64, 65, -63, -64, -65, 128, T - 1, -(T - 1), T, T + 100):
        if v not in out:
            out.append(v)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _case(T, C):
    """Two tables (B correlated with A on even C, independent seeds on odd C) and their dense arrays, computed once."""
    ta = cx.table(T, C, seed=1000 + T + C)
    tb = cx.correlated(ta, T, seed=7 + C) if C % 2 == 0 else cx.table(T, C, seed=2000 + T + C)
    A = co.dense(ta["start"], ta["end"], ta["offsets"], range(C), T)
    B = co.dense(tb["start"], tb["end"], tb["offsets"], range(C), T)
    return ta, tb, A, B


@functools.lru_cache(maxsize=None)
def _want(T, C, pattern, lags):
    _, _, A, B = _case(T, C)
    cls, K = PATTERNS[pattern](T)
    return cls, K, co.reduce_dense(A, B, cls, K, lags)


def rasterise(dev, tab, cells, T, ldb, fill=ONES):
    """xmhw_event_table_bits on a (W, ldb) buffer pre-filled with ``fill``: the whole buffer afterwards"""
    from xmhw_amd._lib import hip
    h = hip()
    W = (T + 63) // 64
    cells = np.asarray(cells, dtype=np.int64)
    with dev.DeviceScope() as s:
        d_start = s.upload(tab["start"] if tab["n"] else np.zeros(1, np.int32))
        d_end = s.upload(tab["end"] if tab["n"] else np.zeros(1, np.int32))
        d_off, d_cell = s.upload(tab["offsets"]), s.upload(cells)
        d_bits = s.upload(np.full((W, ldb), fill, dtype=np.uint64))
        h.event_table_bits(d_start.ptr, d_end.ptr, d_off.ptr, d_cell.ptr, cells.shape[0], T, d_bits.ptr, ldb)
        h.stream_sync(0)
        return d_bits.to_array((W, ldb), np.uint64)


@pytest.mark.parametrize("T", TS)
def test_rasteriser_alone(dev, T):
    for C in CS:
        ta, _, A, _ = _case(T, C)
        want = co.pack_bits(A)
        if T % 64:
            assert (want[-1] >> np.uint64(T % 64) == 0).all()
        maps = [np.arange(C), np.arange(C)[::-1]]
        if C > 1:
            maps.append(np.arange(0, C, 2))                              # skips every other cell
            maps.append(np.array([C - 1, 0]))
        for cells in maps:
            n, ldb = cells.shape[0], C + 5
            got = rasterise(dev, ta, cells, T, ldb)
            npt.assert_array_equal(got[:, :n], want[:, cells])           # fully overwritten, tail bits zero
            assert (got[:, n:] == ONES).all()                            # columns >= C never touched
    assert T < 63 or A.any()


def counts_on_device(T, C, cls, K, lags, **kw):
    from xmhw_amd.cooccurrence import cooccur_tables
    ta, tb, _, _ = _case(T, C)
    return cooccur_tables(ta, tb, np.arange(C), np.arange(C), T, cls, K, lags, **kw)


@pytest.mark.parametrize("T", TS)
def test_reduction_on_every_shape(dev, T):
    """Every T x C, every class pattern, the sixteen lags; forced blocks of 1, 2, 3 and 10^6 words and the automatic one:
    identical to each other because each is identical to the oracle."""
    from xmhw_amd._lib import hip
    h = hip()
    lags = lag_set(T)
    seen = np.zeros(4, dtype=np.int64)
    try:
        for words in (0, 1, 2, 3, 1000000):
            h.set_cooccur_block(words)
            for C in CS:
                for p in range(len(PATTERNS)):
                    cls, K, want = _want(T, C, p, lags)
                    got = counts_on_device(T, C, cls, K, lags)
                    assert got.dtype == np.int32 and got.shape == want.shape
                    npt.assert_array_equal(got, want, err_msg=f"C={C} pattern={PATTERNS[p].__name__} block={words}")
                    seen += want.sum(axis=(0, 1, 3))
    finally:
        h.set_cooccur_block(0)
    if T >= 63:
        assert (seen > 0).all()                                          # every channel occurs


@pytest.mark.parametrize("L", [1, 8, 9, 64])
def test_lag_list_lengths_at_the_group_edges(dev, L):
    lags = tuple(int(v) for v in np.random.default_rng(3).permutation(np.arange(-40, 41))[:L])
    for T, C in ((203, 300), (65, 63), (130, 257)):
        for p in (1, 3):
            cls, K, want = _want(T, C, p, lags)
            assert want[:, :, 0].sum() > 0
            npt.assert_array_equal(counts_on_device(T, C, cls, K, lags), want)


def test_forced_blocks_on_a_longer_record(dev):
    from xmhw_amd._lib import hip
    h = hip()
    T, C = 777, 257                                                      # 13 words
    lags = lag_set(T)
    try:
        for p in (2, 3):
            cls, K, want = _want(T, C, p, lags)
            assert (want.sum(axis=(0, 1, 3)) > 0).all()
            for words in (1, 2, 3, 1000000, 0):
                h.set_cooccur_block(words)
                npt.assert_array_equal(counts_on_device(T, C, cls, K, lags), want, err_msg=f"block of {words} words")
    finally:
        h.set_cooccur_block(0)
    with pytest.raises(h.InvalidArgument):
        h.set_cooccur_block(-1)


def test_slabs_are_identical(dev):
    T, C = 203, 300
    lags = lag_set(T)
    cls, K, want = _want(T, C, 1, lags)
    W = 4
    for cells_per_slab in (299, 64, 7):
        mbb = 4 * 4 * K * len(lags) * C + cells_per_slab * (16 * W + 8 * 30 + 32)
        npt.assert_array_equal(counts_on_device(T, C, cls, K, lags, max_batch_bytes=mbb), want)


def _resident(dev, s, T, C, extra=0):
    """both bitmaps of _case(T, C) on the device, leading dimension C + extra (extra columns all ones)"""
    ta, tb, A, B = _case(T, C)
    out = []
    for X in (A, B):
        full = np.full(((T + 63) // 64, C + extra), ONES, dtype=np.uint64)
        full[:, :C] = co.pack_bits(X)
        out.append(s.upload(full))
    return out


def test_two_halves_and_a_wide_accumulator(dev):
    """ldo > C with the accumulator pre-filled with -77: init clears columns < C only; two accumulate calls on the two
    halves of the columns (pointer offsets into bitmaps and accumulator) against one call."""
    from xmhw_amd._lib import hip
    h = hip()
    T, C, extra = 203, 300, 5
    ldo = C + extra
    lags = np.asarray(lag_set(T), dtype=np.int32)
    L = lags.shape[0]
    cls, K, want = _want(T, C, 3, tuple(int(v) for v in lags))
    half = 131
    got = []
    with dev.DeviceScope() as s:
        d_a, d_b = _resident(dev, s, T, C, extra)
        for pieces in (((0, C),), ((0, half), (half, C))):
            d_counts = s.upload(np.full((K, L, 4, ldo), -77, dtype=np.int32))
            h.cooccur_init(K, L, C, d_counts.ptr, ldo)
            after_init = d_counts.to_array((K, L, 4, ldo), np.int32)
            assert (after_init[..., :C] == 0).all() and (after_init[..., C:] == -77).all()
            for c0, c1 in pieces:
                h.cooccur_accumulate(d_a.ptr + 8 * c0, ldo, d_b.ptr + 8 * c0, ldo, T, c1 - c0, cls, K, lags,
                                     d_counts.ptr + 4 * c0, ldo)
            h.stream_sync(0)
            got.append(d_counts.to_array((K, L, 4, ldo), np.int32))
    for g in got:
        npt.assert_array_equal(g[..., :C], want)
        assert (g[..., C:] == -77).all()                                 # the extra columns survive both calls
    # accumulate ADDS: a second call doubles the counts
    with dev.DeviceScope() as s:
        d_a, d_b = _resident(dev, s, T, C)
        d_counts = s.alloc(4 * K * L * 4 * C)
        h.cooccur_init(K, L, C, d_counts.ptr, C)
        for _ in range(2):
            h.cooccur_accumulate(d_a.ptr, C, d_b.ptr, C, T, C, cls, K, lags, d_counts.ptr, C)
        h.stream_sync(0)
        npt.assert_array_equal(d_counts.to_array((K, L, 4, C), np.int32), 2 * want)


def test_refusals_touch_nothing(dev):
    from xmhw_amd import XmhwException
    from xmhw_amd._lib import hip
    from xmhw_amd.cooccurrence import CHANNELS, MAX_CLASSES, MAX_LAGS, cooccur_tables
    h = hip()
    assert MAX_CLASSES == h.COOCCUR_MAX_CLASSES == 1024 and MAX_LAGS == h.COOCCUR_MAX_LAGS == 64
    assert CHANNELS == h.COOCCUR_CHANNELS == 4
    T, C = 130, 65
    zeros = np.zeros(T, dtype=np.int32)
    sentinel = np.full((2, 2, 4, C), -77, dtype=np.int32)
    with dev.DeviceScope() as s:
        d_a, d_b = _resident(dev, s, T, C)
        d_counts = s.upload(sentinel)
        acc = lambda cls, K, lags: h.cooccur_accumulate(d_a.ptr, C, d_b.ptr, C, T, C, cls, K,           # noqa: E731
                                                        np.asarray(lags, dtype=np.int32), d_counts.ptr, C)
        for K, lags in ((0, [0]), (1025, [0]), (1, []), (1, list(range(65)))):
            with pytest.raises(h.Unsupported):
                acc(zeros, K, lags)
            with pytest.raises(h.Unsupported):
                h.cooccur_init(K, len(lags), C, d_counts.ptr, C)
        bad = zeros.copy()
        bad[77] = 2                                                      # a label K
        with pytest.raises(h.InvalidArgument, match="class_of_t"):
            acc(bad, 2, [0, 1])
        bad[77] = -2
        with pytest.raises(h.InvalidArgument, match="class_of_t"):
            acc(bad, 2, [0, 1])
        with pytest.raises(h.Unsupported):                               # 2**31 cells
            h.cooccur_accumulate(d_a.ptr, 1 << 31, d_b.ptr, 1 << 31, T, 1 << 31, zeros, 1, np.zeros(1, np.int32), d_counts.ptr,
                                 1 << 31)
        with pytest.raises(h.Unsupported):
            h.event_table_bits(8, 8, 8, 8, 1 << 31, T, 8, 1 << 31)
        h.stream_sync(0)
        npt.assert_array_equal(d_counts.to_array(sentinel.shape, np.int32), sentinel)
    # the stage turns them into XmhwException
    ta, tb, _, _ = _case(T, C)
    for cls, K, lags in ((zeros, 0, (0,)), (zeros, 1025, (0,)), (bad, 2, (0,)), (zeros, 1, ()), (zeros, 1, tuple(range(65)))):
        with pytest.raises(XmhwException):
            cooccur_tables(ta, tb, np.arange(C), np.arange(C), T, cls, K, lags)


@functools.lru_cache(maxsize=None)
def _detected(seed, nan_cells):
    """detect() on a synthetic leap year of daily samples on a 6 x 5 grid, some cells all-NaN (land)"""
    from xmhw_amd import GridSeries, detect
    T, ny, nx = 366, 6, 5
    d = cc.synthetic(T, ny * nx, np.float32, seed=seed, D=366, nan_frac=0.01)
    ts, se, th = d["ts"].copy(), d["seas"].copy(), d["thresh"].copy()
    for x in (ts, se, th):
        x[:, list(nan_cells)] = np.nan
    time = np.datetime64("2004-01-01") + np.arange(T).astype("timedelta64[D]")
    sp = {"lat": np.arange(ny) * 1.0, "lon": np.arange(nx) * 1.0}
    temp = GridSeries(ts.reshape(T, ny, nx), ("time", "lat", "lon"), dict(sp, time=time),
                      time_encoding={"calendar": "proleptic_gregorian"})
    clim = [GridSeries(x.reshape(366, ny, nx), ("doy", "lat", "lon"), dict(sp, doy=np.arange(1, 367))) for x in (th, se)]
    return temp, clim[0], clim[1], detect(temp, clim[0], clim[1])


def test_public_call_against_the_oracle_on_two_detections(dev):
    from xmhw_amd import mhw_cooccurrence
    from xmhw_amd.days_by import class_labels
    a = _detected(31, ())[3]
    b = _detected(32, (3, 10, 11, 12, 13, 14))[3]                         # extra land, a whole grid line among it
    assert a.n_cells == 30 and b.n_cells == 24 and a.n_events > 0 and b.n_events > 0
    lags = (-2, 0, 2)
    got = mhw_cooccurrence(a, b, "season", lags=lags)
    va, vb = a.compact_view(), b.compact_view()
    common = np.intersect1d(a.cell_index, b.cell_index)
    kid = class_labels("season", a.time)
    want = co.cooccur_tables(va, vb, np.searchsorted(a.cell_index, common), np.searchsorted(b.cell_index, common), 366, kid, 4,
                             lags)
    assert (want.sum(axis=(0, 1, 3)) > 0).all()
    npt.assert_array_equal(got.klass, [0, 1, 2, 3])
    assert got.both.shape == (4, 3, 5, 5)                                # the line that is land in b is gone
    kg = got.keep
    assert kg.sum() == 24
    for j, name in enumerate(("both", "a_only", "b_only", "onsets")):
        npt.assert_array_equal(getattr(got, name)[..., kg], want[:, :, j], err_msg=name)
    # the same through the host path with the oracle as the stage: every field
    ref = mhw_cooccurrence(a, b, "season", lags=lags, _compute=co.cooccur_tables)
    for f in ("n_pairs", "neither", "keep", "p_a", "p_b", "p_both", "lmf", "hit_rate", "false_alarm_rate", "false_alarm_ratio",
              "csi", "sedi"):
        npt.assert_array_equal(getattr(got, f), getattr(ref, f), err_msg=f)


def test_cross_check_through_mhw_days_by(dev):
    """b = a, lag 0, classes = month: `both` is the event-day count of mhw_days_by(), whose in-event bitmap comes from
    the exceedance walk, not from the table."""
    from xmhw_amd import mhw_cooccurrence, mhw_days_by
    temp, th, se, a = _detected(32, (3, 10, 11, 12, 13, 14))
    got = mhw_cooccurrence(a, a, "month", lags=(0,))
    days = mhw_days_by(temp, th, se, classes="month")
    assert days.days[:, 4].sum() > 0
    npt.assert_array_equal(got.klass, days.klass)
    npt.assert_array_equal(got.keep, days.keep)
    npt.assert_array_equal(got.both[:, 0], days.days[:, 4])
    assert (got.a_only == 0).all() and (got.b_only == 0).all()
