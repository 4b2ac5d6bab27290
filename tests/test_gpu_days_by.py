"""mhw_days_by() on the device against tests/days_by_oracle.py: exact equality of every array."""
import functools

import numpy as np
import numpy.testing as npt
import pytest

import coverage_cases as cc
import days_by_cases as dc
import days_by_oracle as dbo
import pad_oracle as po

pytestmark = pytest.mark.gpu

FILTERS = [dict(minDuration=3, maxGap=1), dict(minDuration=8, maxGap=4), dict(joinGaps=False), dict(minDuration=5, maxGap=0),
           dict(coldSpells=True)]


@pytest.fixture(scope="module")
def dev():
    from xmhw_amd._lib import require_gpu
    require_gpu()
    import xmhw_amd.device as d
    return d


@functools.lru_cache(maxsize=None)
def _case(T, C, dtype, seed, nan_frac, kw=()):
    """A synthetic series and the class-independent half of the oracle, computed once and shared."""
    kw = dict(kw)
    d = cc.synthetic(T, C, np.dtype(dtype).type, seed=seed, nan_frac=nan_frac, cold=kw.get("coldSpells", False))
    return d, dbo.states_and_anomalies(d["ts"], d["seas"], d["thresh"], d["doy"], d["doys"], **kw)


def _same(got, want):
    assert got[0].dtype == np.int32 and got[1].dtype == np.int64 and got[2].dtype == np.float64
    npt.assert_array_equal(got[0], want["days"])
    npt.assert_array_equal(got[1], want["isum_q"])
    npt.assert_array_equal(got[2], want["intensity_max"])                # NaN == NaN here


def _both(d, sa, classes, K, **kw):
    from xmhw_amd.days_by import class_days_cells
    want = dbo.reduce_by_class(*sa, classes, K)
    dc.check_case(want)
    counters = {}
    got = class_days_cells(d["ts"], d["seas"], d["thresh"], d["doy"], d["doys"], classes, K, counters=counters, **kw)
    _same(got, want)
    assert counters["n_range"] == want["n_range"] == 0
    return got


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("C", [1, 63, 64, 65, 255, 257, 3001])
def test_cell_counts_around_a_wave_and_a_tile(dev, dtype, C):
    # (a single cell with event days in every run of 17 steps is rare: seed 1108 is one, found on the oracle)
    d, sa = _case(203, C, dtype, 1108 if C == 1 else C, 0.01)             # T is not a multiple of 64
    for pattern in dc.PATTERNS:
        _both(d, sa, *pattern(203))


def test_leading_dimensions_with_sentinel_columns(dev):
    """Series, climatologies, bits and outputs wider than the slab: the extra input columns hold values that would be
    extreme events if a kernel read them, the extra output columns a sentinel that must survive."""
    from xmhw_amd._lib import hip
    from xmhw_amd.detect_front import _check_inputs
    h = hip()
    T, C, extra = 203, 70, 5
    ld = C + extra
    W = (T + 63) // 64
    for dtype in ("float32", "float64"):
        d, sa = _case(T, C, dtype, 12, 0.01)
        classes, K = dc.runs_of_17(T)
        want = dbo.reduce_by_class(*sa, classes, K)
        dc.check_case(want)
        ts = np.full((T, ld), 1e6, dtype=dtype)
        ts[:, :C] = d["ts"]
        D = d["seas"].shape[0]
        se, th = np.zeros((D, ld)), np.ones((D, ld))
        se[:, :C], th[:, :C] = d["seas"], d["thresh"]
        _, _, _, rows = _check_inputs(d["ts"], d["seas"], d["thresh"], d["doy"], d["doys"])
        bufs = [dev.DeviceBuffer.from_array(a) for a in (
            ts, se, th, np.full((W, ld), 0xFFFFFFFFFFFFFFFF, dtype=np.uint64), np.full((K, 6, ld), -77, dtype=np.int32),
            np.full((K, ld), -78, dtype=np.int64), np.full((K, ld), -79.5), np.full(1, 123, dtype=np.int64))]
        d_ts, d_se, d_th, d_bits, d_days, d_isum, d_imax, d_cnt = bufs
        try:
            h.class_days_init(K, C, d_days.ptr, d_isum.ptr, d_imax.ptr, ld, d_cnt.ptr)
            h.exceed_bits(d_ts.ptr, ts.dtype.itemsize, T, C, ld, d_th.ptr, ld, D, rows, 0, d_bits.ptr, ld)
            h.class_days_accumulate(d_ts.ptr, ts.dtype.itemsize, T, C, ld, d_se.ptr, d_th.ptr, ld, rows, 0, d_bits.ptr, ld,
                                    5, 1, 2, classes, K, d_days.ptr, d_isum.ptr, d_imax.ptr, ld, d_cnt.ptr)
            h.class_days_finish(K, C, d_imax.ptr, ld)
            h.stream_sync(0)
            days, isum = d_days.to_array((K, 6, ld), np.int32), d_isum.to_array((K, ld), np.int64)
            imax, cnt = d_imax.to_array((K, ld), np.float64), d_cnt.to_array((1,), np.int64)
        finally:
            for b in bufs:
                b.free()
        _same((days[..., :C], isum[:, :C], imax[:, :C]), want)
        assert cnt[0] == 0
        assert (days[..., C:] == -77).all() and (isum[:, C:] == -78).all() and (imax[:, C:] == -79.5).all()


@pytest.mark.parametrize("kw", FILTERS)
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_filter_variants_and_cold_spells(dev, kw, dtype):
    d, sa = _case(331, 200, dtype, 5, 0.02, tuple(sorted(kw.items())))
    _both(d, sa, *dc.runs_of_17(331), **kw)
    _both(d, sa, *dc.every_step(331), **kw)


def test_nan_gaps_with_and_without_maxPadLength(dev):
    from xmhw_amd.days_by import class_days_cells
    from xmhw_amd.padding import make_pad
    T, C = 300, 130
    d, sa = _case(T, C, "float64", 8, 0.06)
    classes, K = dc.runs_of_17(T)
    plain = _both(d, sa, classes, K)
    time = np.datetime64("2001-01-01") + np.arange(T).astype("timedelta64[D]")
    pad = make_pad(np.timedelta64(3, "D"), time)
    try:
        got = class_days_cells(d["ts"], d["seas"], d["thresh"], d["doy"], d["doys"], classes, K, pad=pad)
    finally:
        pad.free()
    filled = po.interpolate_na(d["ts"], po.interp_index(time), 3 * 86400e9)
    want = dbo.class_days_full(filled, d["seas"], d["thresh"], d["doy"], d["doys"], classes, K)
    dc.check_case(want)
    _same(got, want)
    assert not np.array_equal(got[0], plain[0])                          # the interpolation matters


def test_block_lengths_give_the_same_bits(dev):
    from xmhw_amd._lib import hip
    from xmhw_amd.days_by import class_days_cells
    h = hip()
    d, sa = _case(777, 300, "float32", 3, 0.02)
    try:
        for pattern in (dc.runs_of_17, dc.every_step):
            classes, K = pattern(777)
            want = dbo.reduce_by_class(*sa, classes, K)
            dc.check_case(want)
            for steps in (1, 64, 65, 1000000, 0):
                h.set_class_days_block(steps)
                _same(class_days_cells(d["ts"], d["seas"], d["thresh"], d["doy"], d["doys"], classes, K), want)
    finally:
        h.set_class_days_block(0)
    with pytest.raises(h.InvalidArgument):
        h.set_class_days_block(-1)


def test_batches_are_bit_identical(dev):
    from xmhw_amd.days_by import class_days_cells
    T, C = 203, 3001
    d, sa = _case(T, C, "float32", C, 0.01)
    classes, K = dc.every_step(T)
    a = _both(d, sa, classes, K)
    per_cell = T * 5 + T // 4 + 2 * 37 * 8 + 64
    for mbb in (per_cell * 1000, per_cell * 333, per_cell * 64):         # 4, 10 and 47 batches
        b = class_days_cells(d["ts"], d["seas"], d["thresh"], d["doy"], d["doys"], classes, K, max_batch_bytes=mbb)
        for x, y in zip(a, b):
            npt.assert_array_equal(x, y)


def test_class_cap(dev):
    from xmhw_amd import XmhwException
    from xmhw_amd._lib import hip
    from xmhw_amd.days_by import CHANNELS, MAX_CLASSES, class_days_cells
    h = hip()
    assert MAX_CLASSES == h.CLASS_DAYS_MAX_CLASSES == 1024 and CHANNELS == h.CLASS_DAYS_CHANNELS == 6
    T, C = 1100, 130
    d, sa = _case(T, C, "float32", 9, 0.0)
    classes = (np.arange(T) % MAX_CLASSES).astype(np.int32)
    assert len(np.unique(classes)) == MAX_CLASSES
    _both(d, sa, classes, MAX_CLASSES)
    with pytest.raises(XmhwException):
        class_days_cells(d["ts"], d["seas"], d["thresh"], d["doy"], d["doys"], classes, MAX_CLASSES + 1)
    # the C ABI itself: XMHW_ERR_UNSUPPORTED above the cap and below 1, before anything is touched
    for K in (MAX_CLASSES + 1, 0):
        with pytest.raises(h.Unsupported):
            h.class_days_accumulate(8, 4, T, C, C, 8, 8, C, np.zeros(T, np.int32), 0, 8, C, 5, 1, 2, np.zeros(T, np.int32), K,
                                    8, 8, 8, C, 8)
        with pytest.raises(h.Unsupported):
            h.class_days_init(K, C, 8, 8, 8, C, 8)
        with pytest.raises(h.Unsupported):
            h.class_days_finish(K, C, 8, C)
    with pytest.raises(h.Unsupported):                                   # 2**31 cells
        h.class_days_accumulate(8, 4, T, 1 << 31, 1 << 31, 8, 8, 1 << 31, np.zeros(T, np.int32), 0, 8, 1 << 31, 5, 1, 2,
                                np.zeros(T, np.int32), 1, 8, 8, 8, 1 << 31, 8)


def test_label_out_of_range_raises_before_a_launch(dev):
    from xmhw_amd import XmhwException
    from xmhw_amd._lib import hip
    from xmhw_amd.days_by import class_days_cells
    h = hip()
    T, C = 203, 64
    d, _ = _case(T, C, "float32", 64, 0.01)
    for bad in (7, -2):
        classes = np.zeros(T, np.int32)
        classes[100] = bad
        with pytest.raises(XmhwException):
            class_days_cells(d["ts"], d["seas"], d["thresh"], d["doy"], d["doys"], classes, 7)
        # the C ABI: the host copy is checked before any pointer is used (these pointers are not device memory)
        with pytest.raises(h.InvalidArgument, match="class_of_t"):
            h.class_days_accumulate(8, 4, T, C, C, 8, 8, C, np.zeros(T, np.int32), 0, 8, C, 5, 1, 2, classes, 7, 8, 8, 8, C, 8)


def test_out_of_range_samples_are_counted_and_left_out(dev, oisst):
    from xmhw_amd import GridSeries, XmhwException, mhw_days_by
    from xmhw_amd.days_by import class_days_cells
    T, C = 203, 65
    d, sa = _case(T, C, "float32", 65, 0.01)
    st = sa[0]
    inside = np.nonzero(st[:, 7, 4] & st[:, 7, :4].any(axis=1))[0][:10]  # ten in-event samples above the threshold
    assert inside.shape == (10,)
    ts = d["ts"].copy()
    ts[inside, 7] += 300.0
    classes, K = dc.runs_of_17(T)
    want = dbo.class_days_full(ts, d["seas"], d["thresh"], d["doy"], d["doys"], classes, K)
    dc.check_case(want)
    assert want["n_range"] == 10
    counters = {}
    got = class_days_cells(ts, d["seas"], d["thresh"], d["doy"], d["doys"], classes, K, counters=counters)
    assert counters["n_range"] == 10
    _same(got, want)
    with pytest.raises(XmhwException, match="kelvin"):
        class_days_cells(ts, d["seas"], d["thresh"], d["doy"], d["doys"], classes, K)
    # the public call: a series in kelvin against a climatology in degrees Celsius
    g, th, se = _oisst_inputs(oisst)
    hot = GridSeries(oisst["sst"] + np.float32(300.0), g.dims, g.coords, time_encoding={"calendar": "proleptic_gregorian"})
    with pytest.raises(XmhwException, match="kelvin"):
        mhw_days_by(hot, th, se)


def test_golden_series(dev):
    """The 108 reference series, each as one cell with its own parameters and classes = t % 3."""
    from xmhw_amd.days_by import class_days_cells
    total = np.zeros(6, dtype=np.int64)
    for ts, se, th, (m, jg, gap), table, cols in cc.golden_series():
        T = ts.shape[0]
        classes = (np.arange(T) % 3).astype(np.int32)
        args = (ts[:, None], se[:, None], th[:, None], np.arange(T), np.arange(T), classes, 3, m, jg, gap)
        want = dbo.class_days_full(*args)
        _same(class_days_cells(*args), want)
        assert want["days"][:, 4].sum() == table[:, cols.index("duration")].sum()
        total += want["days"].sum(axis=(0, 2))
    assert total[4] > 10000 and (total[:4] > 0).all()


def _oisst_inputs(oisst):
    from xmhw_amd import GridSeries, climatology_series, threshold
    g = GridSeries(oisst["sst"], ("time", "lat", "lon"), {"time": oisst["time64"], "lat": oisst["lat"], "lon": oisst["lon"]},
                   time_encoding={"calendar": "proleptic_gregorian"})
    clim = threshold(g)
    return g, climatology_series(clim, "thresh"), climatology_series(clim, "seas")


def _assert_same_dataset(a, b):
    npt.assert_array_equal(a.klass, b.klass)
    npt.assert_array_equal(a.n_steps, b.n_steps)
    for f in ("days", "n_valid", "isum_q", "intensity_max", "keep", "frequency", "intensity_mean", "category_max"):
        npt.assert_array_equal(getattr(a, f), getattr(b, f), err_msg=f)


def test_public_call_on_a_grid_with_land(dev, oisst):
    """mhw_days_by() by month on the land-masked fixture grid, float and packed int16, against the host path with the
    oracle as the device stage."""
    from xmhw_amd import GridSeries, mhw_days_by
    from xmhw_amd.device import PackedArray, decode_through_device
    g, th, se = _oisst_inputs(oisst)
    want = mhw_days_by(g, th, se, _compute=dbo.class_days_cells)
    got = mhw_days_by(g, th, se)
    assert want.days[:, 4].sum() > 0 and not want.keep.all() and want.klass.shape == (12,)
    _assert_same_dataset(got, want)
    # slabs of the grid path: the bits do not change
    _assert_same_dataset(mhw_days_by(g, th, se, max_batch_bytes=40000), want)
    # packed int16 codes: the series the device decodes is the series the host decodes
    sst = oisst["sst"]
    codes = np.where(np.isnan(sst), -32768, np.rint((sst.astype(np.float64) - 10.0) / 0.005)).astype(np.int16)
    packed = PackedArray(codes, dict(scale=0.005, offset=10.0, fill=-32768, out="float32"))
    T = sst.shape[0]
    decoded = decode_through_device(packed.reshape(T, -1)).reshape(sst.shape)          # what the device decodes
    assert decoded.dtype == np.float32 and np.array_equal(np.isnan(decoded), np.isnan(sst))
    kw = dict(time_encoding={"calendar": "proleptic_gregorian"})
    want_p = mhw_days_by(GridSeries(decoded, g.dims, g.coords, **kw), th, se, _compute=dbo.class_days_cells)
    view = GridSeries(decoded, g.dims, g.coords, **kw)
    view.values = packed                                                 # as open_series() hands a file view over
    got_p = mhw_days_by(view, th, se)
    assert want_p.days[:, 4].sum() > 0
    _assert_same_dataset(got_p, want_p)


def test_event_days_equal_the_table_durations(dev):
    """With all labels >= 0 the event days of a cell, summed over the classes, are the durations of its rows in the table
    of xmhw_events_from_bits (detect_front.detect_cells) on the same inputs."""
    from xmhw_amd.days_by import class_days_cells
    from xmhw_amd.detect import EVENT_COLUMNS
    from xmhw_amd.detect_front import detect_cells
    d, _ = _case(203, 257, "float32", 257, 0.01)
    classes, K = dc.runs_of_17(203)
    got = class_days_cells(d["ts"], d["seas"], d["thresh"], d["doy"], d["doys"], classes, K)
    res = detect_cells(d["ts"], d["seas"], d["thresh"], d["doy"], d["doys"])
    dur, off = res["table"][:, EVENT_COLUMNS.index("duration")], res["offsets"]
    per_cell = np.array([dur[off[c]:off[c + 1]].sum() for c in range(257)])
    assert per_cell.sum() > 0
    npt.assert_array_equal(got[0][:, 4].sum(axis=0), per_cell)
