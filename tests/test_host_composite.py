"""The host logic of mhw_composite() without a device: argument validation, the anchor table of a hand-written
EventDataset (order, the dummy cell, dropped land cells), the derived fields of CompositeDataset on integers worked by
hand, the whole public path around the numpy stand-in of the device stage against the oracle, the refusals of the C
entries, and the exports."""
import importlib
import math

import numpy as np
import numpy.testing as npt
import pytest

import composite_cases as cc
import composite_oracle as co
import xmhw_amd
from xmhw_amd import GridSeries, mhw_composite
from xmhw_amd import composite as cm
from xmhw_amd.detect import EVENT_COLUMNS, EventDataset
from xmhw_amd.exception import XmhwException

NY, NX, T = 3, 4, 400
TIME = np.datetime64("2001-01-01") + np.arange(T).astype("timedelta64[D]")
COORDS = {"time": TIME, "lat": np.arange(NY) * 0.25, "lon": np.arange(NX) * 0.25}
# the events' ocean: (0, 1) and (2, 2) are land; every grid line keeps an ocean cell
EVENT_LAND = np.zeros((NY, NX), bool)
EVENT_LAND[0, 1] = EVENT_LAND[2, 2] = True
# (start, peak, end) of the events of every ocean cell, by grid point
EVENTS = {0: [(0, 2, 6), (20, 25, 31), (390, 395, 399)], 2: [(63, 64, 70)], 3: [], 4: [(100, 110, 130), (140, 141, 146)],
          5: [(10, 12, 15)], 6: [(127, 128, 133), (250, 255, 262)], 7: [(5, 9, 11)], 8: [(300, 301, 306)], 9: [(40, 44, 47)],
          11: [(199, 200, 204), (210, 214, 215), (220, 222, 226)]}


def events_dataset(time=TIME):
    keep = ~EVENT_LAND.reshape(-1)
    cell_index = np.nonzero(keep)[0]
    rows, offsets = [], [0]
    for p in cell_index:
        for s, pk, e in EVENTS[int(p)]:
            r = np.zeros(len(EVENT_COLUMNS))
            r[0] = s
            r[EVENT_COLUMNS.index("index_start")], r[EVENT_COLUMNS.index("index_peak")], r[EVENT_COLUMNS.index("index_end")] = s, pk, e
            r[EVENT_COLUMNS.index("duration")] = e - s + 1
            rows.append(r)
        offsets.append(len(rows))
    table = np.array(rows)
    return EventDataset(table, np.array(offsets, np.int64), time, cell_index, keep, ("lat", "lon"), (NY, NX),
                        {"lat": COORDS["lat"], "lon": COORDS["lon"]}, {"xmhw_parameters": ""}, {}, {}, False)


def field(land=EVENT_LAND, seed=1, dtype=np.float32):
    rng = np.random.default_rng(seed)
    x = np.round(rng.normal(0, 3.0, (T, NY, NX)), 3).astype(dtype)
    x[rng.random(x.shape) < 0.03] = np.nan
    x[:, land] = np.nan
    return GridSeries(x, ("time", "lat", "lon"), COORDS)


def test_exports():
    assert "mhw_composite" in xmhw_amd.__all__ and "CompositeDataset" in xmhw_amd.__all__
    assert xmhw_amd.mhw_composite is cm.mhw_composite and xmhw_amd.CompositeDataset is cm.CompositeDataset


def test_argument_validation():
    ev, f = events_dataset(), field()
    stage = co.composite_cells
    bad = [(dict(before=64, after=64), "at most 128 offsets"), (dict(before=128, after=0), "at most 128"),
           (dict(before=-1), "before and after should be >= 0"), (dict(after=-3), "before and after should be >= 0"),
           (dict(before=2.5), "before should be a whole number"), (dict(shift=25), r"shift should be in \[0, 24\]"),
           (dict(shift=-1), "shift should be in"), (dict(anchor="middle"), "anchor should be one of"),
           (dict(classes=np.arange(T) % 65), "at most 64 classes"), (dict(classes=np.zeros(T - 1, int)), "one entry per time step"),
           (dict(select=np.ones(3, bool)), "select should be a boolean array with one entry per event"),
           (dict(select=np.ones(ev.n_events, int)), "select should be a boolean array"),
           (dict(max_result_bytes=1000), r"K = 1 classes x D = 61 offsets x C = 10 cells takes 12200 bytes")]
    for kw, text in bad:
        with pytest.raises(XmhwException, match=text):
            mhw_composite(f, None, ev, _compute=stage, **kw)
    mhw_composite(f, None, ev, before=63, after=64, _compute=stage, max_result_bytes=20 * 128 * 10)   # the caps themselves
    with pytest.raises(XmhwException, match="expects the EventDataset"):
        mhw_composite(f, None, {"table": 0}, _compute=stage)
    # mismatched time axes: another length, and the same length shifted by a day
    with pytest.raises(XmhwException, match="400 and 399 time steps"):
        mhw_composite(f, None, events_dataset(TIME[:-1]), _compute=stage)
    with pytest.raises(XmhwException, match="same time axis"):
        mhw_composite(f, None, events_dataset(TIME + np.timedelta64(1, "D")), _compute=stage)
    # another grid, a point series against a grid
    other = GridSeries(np.zeros((T, NY, NX + 1), np.float32), ("time", "lat", "lon"), dict(COORDS, lon=np.arange(NX + 1.0)))
    with pytest.raises(XmhwException, match="not on the same grid"):
        mhw_composite(other, None, ev, _compute=stage)
    with pytest.raises(XmhwException, match="single-point series with a grid"):
        mhw_composite(GridSeries(np.zeros(T, np.float32), ("time",), {"time": TIME}), None, ev, _compute=stage)
    # T of 2**17 and more, before anything else is looked at
    long = 1 << 17
    with pytest.raises(XmhwException, match="fewer than 2\\*\\*17 time steps"):
        mhw_composite(GridSeries(np.zeros(long, np.float32), ("time",), {"time": np.arange(long)}), None, ev, _compute=stage)
    # an anchor outside the time axis
    broken = events_dataset()
    broken.table[2, EVENT_COLUMNS.index("index_end")] = T
    with pytest.raises(XmhwException, match="index_end outside the time axis"):
        mhw_composite(f, None, broken, anchor="end", _compute=stage)


def test_anchor_table_order_dummy_cell_and_selection():
    ev = events_dataset()
    for anchor, col in (("start", 0), ("peak", 1), ("end", 2)):
        v = cm.anchor_table(ev, anchor)
        assert v["C"] == ev.n_cells + 1 and v["n"] == ev.n_events and v["start"] is v["end"] and v["start"].dtype == np.int32
        assert v["offsets"].dtype == np.int64 and v["offsets"][-1] == v["offsets"][-2] == v["n"]     # the dummy cell is empty
        for i, p in enumerate(ev.cell_index):
            assert v["start"][v["offsets"][i]:v["offsets"][i + 1]].tolist() == [e[col] for e in EVENTS[int(p)]]
    # a selection: the long events only; cells may become empty
    long = ev.table[:, EVENT_COLUMNS.index("duration")] >= 10
    v = cm.anchor_table(ev, "peak", long)
    assert v["n"] == int(long.sum()) == 4
    want = {int(p): [e[1] for e in EVENTS[int(p)] if e[2] - e[0] + 1 >= 10] for p in ev.cell_index}
    for i, p in enumerate(ev.cell_index):
        assert v["start"][v["offsets"][i]:v["offsets"][i + 1]].tolist() == want[int(p)]
    # rows out of time order within a cell are put in order
    shuffled = events_dataset()
    shuffled.table[[0, 1]] = shuffled.table[[1, 0]]
    shuffled.table[:, EVENT_COLUMNS.index("index_end")] = 399            # compact_view() wants end >= start
    assert cm.anchor_table(shuffled, "start")["start"][:3].tolist() == [0, 20, 390]
    # grid points without a table cell point at the dummy
    of_point = cm.table_cell_of_point(cm.anchor_table(ev), NY * NX)
    assert of_point[[1, 10]].tolist() == [10, 10] and of_point[ev.cell_index].tolist() == list(range(10))


@pytest.mark.parametrize("anchor", ["start", "peak", "end"])
def test_public_path_around_the_stand_in_equals_the_oracle(anchor):
    ev = events_dataset()
    # the field has land of its own: (1, 1) has events and is dropped, (0, 1) is land in both, (2, 2) is ocean without a
    # table cell
    land = np.zeros((NY, NX), bool)
    land[0, 1] = land[1, 1] = True
    f = field(land, seed=5)
    keep = ~land.reshape(-1)
    base = np.where(land, np.nan, 0.5)
    labels = np.where(np.arange(T) % 50 < 45, (np.arange(T) // 100) % 2 * 10 + 3, -1)     # classes 3 and 13, some steps in none
    select = np.ones(ev.n_events, bool)
    select[1] = False
    got = mhw_composite(f, base, ev, anchor=anchor, before=7, after=9, classes=labels, select=select, shift=1,
                        _compute=co.composite_cells)
    assert got.klass.tolist() == [3, 13] and got.offset.tolist() == list(range(-7, 10)) and got.n_cells_dropped == 1
    assert got.anchor == anchor and got.shift == 1 and got.n.shape == (2, 17, NY, NX) and got.n.dtype == np.int32
    A = np.zeros((T, NY * NX), bool)
    col = {"start": 0, "peak": 1, "end": 2}[anchor]
    r = 0
    for p in ev.cell_index:
        for e in EVENTS[int(p)]:
            if select[r]:
                A[e[col], p] = True
            r += 1
    kid = np.where(labels < 0, -1, (labels == 13).astype(int))
    x = np.asarray(f.values).reshape(T, -1)
    want = co.composite_sums(x[:, keep], np.full((1, int(keep.sum())), 0.5), np.zeros(T, int), 1, A[:, keep], kid, 2, 7, 9)
    assert want["n"].sum() > 100
    for name, k in (("n", "n"), ("sum_q", "s"), ("sumsq_q", "ss")):
        a = getattr(got, name).reshape(2, 17, -1)
        npt.assert_array_equal(a[..., keep], want[k], err_msg=name)
        assert (a[..., ~keep] == 0).all()
    npt.assert_array_equal(got.n_anchors.reshape(2, -1), np.stack([(A[kid == k] & keep).sum(axis=0) for k in (0, 1)]))
    npt.assert_array_equal(got.keep, ~land)
    assert np.isnan(got.mean[:, :, land]).all() and np.isnan(got.mean[:, :, 2, 2]).all() and (got.n[:, :, 2, 2] == 0).all()
    # base=None is a base of zero on the ocean of the field
    zero = mhw_composite(f, None, ev, anchor=anchor, before=7, after=9, classes=labels, select=select, shift=1,
                         _compute=co.composite_cells)
    want0 = co.composite_sums(x[:, keep], np.zeros((1, int(keep.sum()))), np.zeros(T, int), 1, A[:, keep], kid, 2, 7, 9)
    npt.assert_array_equal(zero.sum_q.reshape(2, 17, -1)[..., keep], want0["s"])
    # out of range: the text points to shift
    with pytest.raises(XmhwException, match="pass a larger shift"):
        mhw_composite(GridSeries(np.asarray(f.values) * 100.0, f.dims, COORDS), None, ev, _compute=co.composite_cells)


def test_derived_fields_on_integers_worked_by_hand():
    """one class, offsets -1..1, four cells.  Cell 0: samples 1.0, 2.0, 3.0 and 6.0 at shift 0 -> mean 3, variance
    (4 + 1 + 0 + 9) / 3, t = 3 / sqrt(14 / 3 / 4); cell 1: one sample; cell 2: none; cell 3: two equal samples."""
    one = 1 << 16
    q0 = np.array([1, 2, 3, 6]) * one
    n = np.zeros((1, 3, 4), np.int32)
    s, ss = np.zeros((1, 3, 4), np.int64), np.zeros((1, 3, 4), np.int64)
    n[0, 1] = [4, 1, 0, 2]
    s[0, 1] = [q0.sum(), 5 * one, 0, 2 * 7 * one]
    ss[0, 1] = [(q0 ** 2).sum(), (5 * one) ** 2, 0, 2 * (7 * one) ** 2]
    ds = cm.CompositeDataset([0], [-1, 0, 1], n, s, ss, np.array([[4, 1, 0, 2]], np.int32), np.ones(4, bool), ("cell",),
                             {"cell": np.arange(4)})
    assert ds.mean[0, 1, 0] == 3.0 and ds.std[0, 1, 0] == math.sqrt(14.0 / 3.0)
    npt.assert_allclose(ds.t[0, 1, 0], 3.0 / math.sqrt(14.0 / 3.0 / 4.0), rtol=1e-15)
    # Student's t with 3 degrees of freedom: the two-sided p of t = 2.7775 lies between 0.05 (t = 3.182) and 0.1 (t = 2.353)
    assert 0.05 < ds.p[0, 1, 0] < 0.1
    for a in (ds.mean, ds.std, ds.t, ds.p):
        assert np.isnan(a[0, 1, 1:3]).all() and np.isnan(a[0, 0]).all() and np.isnan(a[0, 2]).all()
    # no spread: the mean is certain
    assert ds.mean[0, 1, 3] == 7.0 and ds.std[0, 1, 3] == 0.0 and np.isinf(ds.t[0, 1, 3]) and ds.p[0, 1, 3] == 0.0
    # shift scales mean and std, not t
    sh = cm.CompositeDataset([0], [-1, 0, 1], n, s, ss, np.array([[4, 1, 0, 2]], np.int32), np.ones(4, bool), ("cell",),
                             {"cell": np.arange(4)}, shift=4)
    assert sh.mean[0, 1, 0] == 48.0 and sh.std[0, 1, 0] == 16.0 * ds.std[0, 1, 0] and sh.t[0, 1, 0] == ds.t[0, 1, 0]


def test_oracle_on_a_case_worked_by_hand():
    """T = 6, one cell, anchors at steps 1 and 4, before = after = 1, classes 0 and 1: the oracle itself"""
    ts = np.array([[1.0], [2.0], [np.nan], [4.0], [200.0], [0.5]])
    A = np.array([0, 1, 0, 0, 1, 0], bool)[:, None]
    r = co.composite_sums(ts, np.zeros((1, 1)), np.zeros(6, int), 0, A, np.array([0, 0, 0, 0, 1, 1]), 2, 1, 1)
    one = 1 << 16
    assert r["n"][:, :, 0].tolist() == [[1, 1, 0], [1, 0, 1]] and r["n_range"] == 1
    assert r["s"][:, :, 0].tolist() == [[one, 2 * one, 0], [4 * one, 0, one // 2]]
    assert r["ss"][1, 2, 0] == (one // 2) ** 2
    # the bitmap of the cases and the anchors of a table agree with each other
    B = cc.anchor_columns(200, 19, 30)
    words = cc.bitmap(B)
    assert words.shape == (4, 19) and words.dtype == np.uint64
    back = ((words[:, None, :] >> np.arange(64, dtype=np.uint64)[None, :, None]) & np.uint64(1)).reshape(256, 19)[:200].astype(bool)
    npt.assert_array_equal(back, B)
    npt.assert_array_equal(co.anchors_of_table(cc.table_of(B), np.arange(19), 200), B)


def test_c_entry_refusals_need_no_device_and_raise_the_exceptions_of_the_core_module():
    core = importlib.import_module("xmhw_amd._xmhw_hip")
    m = importlib.import_module("xmhw_amd._xmhw_hip_composite")
    assert not any(hasattr(m, n) for n in ("HipError", "Unsupported", "InvalidArgument", "CommError"))
    Tn = 10
    z = np.zeros(Tn, np.int32)

    def acc(T=Tn, C=4, ld=4, ldb=4, Dr=1, rows=z, shift=0, lda=4, classes=z, K=1, before=3, after=3, ldo=4, itemsize=4):
        m.composite_accumulate(0, itemsize, T, C, ld, 0, ldb, Dr, rows, shift, 0, lda, classes, K, before, after, 0, 0, 0, ldo, 0)

    def init(K=1, D=7, C=4, ldo=4):
        m.composite_init(K, D, C, 0, 0, 0, ldo, 0)

    long = (1 << 17)
    unsupported = [lambda: acc(K=0), lambda: acc(K=65), lambda: acc(before=64, after=64), lambda: acc(before=128, after=0),
                   lambda: acc(before=-1), lambda: acc(after=-1), lambda: acc(shift=25), lambda: acc(shift=-1),
                   lambda: acc(T=long, rows=np.zeros(long, np.int32), classes=np.zeros(long, np.int32)),
                   lambda: acc(C=1 << 31, ld=1 << 31, ldb=1 << 31, lda=1 << 31, ldo=1 << 31), lambda: init(K=0), lambda: init(K=65),
                   lambda: init(D=0), lambda: init(D=129)]
    for call in unsupported:
        with pytest.raises(core.Unsupported) as e:
            call()
        assert type(e.value) is core.Unsupported and isinstance(e.value, core.HipError) and "(code 3)" in str(e.value)
    # K is judged before D, D before shift, as the header says
    with pytest.raises(core.Unsupported, match="K must be in"):
        acc(K=0, before=100, after=100, shift=30)
    with pytest.raises(core.Unsupported, match="before \\+ after \\+ 1 must be in"):
        acc(before=100, after=100, shift=30)
    invalid = [(lambda: acc(classes=np.full(Tn, 1, np.int32)), r"class_of_t outside \[-1, K\)"),
               (lambda: acc(classes=np.full(Tn, -2, np.int32)), r"class_of_t outside"),
               (lambda: acc(rows=np.full(Tn, 1, np.int32)), r"row_of_t outside \[0, D\)"),
               (lambda: acc(ld=3), "bad T/C"), (lambda: acc(ldb=3), "bad T/C"), (lambda: acc(lda=3), "bad T/C"),
               (lambda: acc(ldo=3), "bad T/C"), (lambda: acc(Dr=0), "bad T/C"),
               (lambda: acc(rows=np.zeros(Tn + 1, np.int32)), "row_of_t length"),
               (lambda: acc(classes=np.zeros(Tn - 1, np.int32)), "class_of_t length"), (lambda: acc(itemsize=2), "itemsize"),
               (lambda: acc(), "NULL buffer"), (lambda: init(ldo=3), "bad C/ldo"), (lambda: init(), "NULL"),
               (lambda: m.set_composite_block(-1), "steps must be")]
    for call, text in invalid:
        with pytest.raises(core.InvalidArgument, match=text) as e:
            call()
        assert type(e.value) is core.InvalidArgument
    # the caps themselves are taken; nothing is launched for C == 0 or T == 0: no device is needed either
    acc(C=0, ld=0, ldb=0, lda=0, ldo=0, K=64, before=63, after=64, shift=24)
    acc(C=0, ld=0, ldb=0, lda=0, ldo=0, T=long - 1, rows=np.zeros(long - 1, np.int32), classes=np.zeros(long - 1, np.int32))
    acc(T=0, rows=np.zeros(0, np.int32), classes=np.zeros(0, np.int32))
    m.set_composite_block(0)
    assert (m.COMPOSITE_MAX_OFFSETS, m.COMPOSITE_MAX_CLASSES, m.COMPOSITE_MAX_STEPS, m.COMPOSITE_BITS, m.COMPOSITE_RANGE_BITS,
            m.COMPOSITE_MAX_SHIFT) == (128, 64, 1 << 17, 16, 7, 24)
    assert (cm.MAX_OFFSETS, cm.MAX_CLASSES, cm.MAX_STEPS, cm.BITS, cm.RANGE_BITS, cm.MAX_SHIFT) == (128, 64, 1 << 17, 16, 7, 24)
