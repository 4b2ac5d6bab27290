"""mhw_rank() on the device (csrc/kernels_rank.hip) against a numpy per-cell stable-argsort oracle, bit for
bit (ranks and return periods): the reference's fixture, the reference's own event tables, synthetic CSR
tables with ties, signed zeros, NaN and cells of every size around the 64-event work item, non-default
leading dimensions, and threshold() -> detect() -> mhw_rank() on the OISST grid."""
import os

import numpy as np
import numpy.testing as npt
import pytest

from test_host_rank import rank_oracle
from xmhw_amd.detect import EventDataset
from xmhw_amd.rank import RANKED

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
COLS = [EventDataset.columns.index(k) for k in RANKED]           # the 24 ranked table columns


@pytest.fixture(scope="module")
def gpu():
    from xmhw_amd._lib import require_gpu
    require_gpu()
    from xmhw_amd import rank
    return rank


def same(got, want):
    """bit-for-bit equality, NaN where NaN"""
    assert got.shape == want.shape
    npt.assert_array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    npt.assert_array_equal(got[ok].view(np.uint64), want[ok].view(np.uint64))


def check(gpu, table, offsets, columns, n_years):
    rank, rp = gpu.rank_device(table, offsets, columns, n_years)
    wr, wp = rank_oracle(table, np.asarray(offsets), columns, n_years)
    same(rank[:, 1:], wr[:, 1:])
    same(rp[:, 1:], wp[:, 1:])


def synth_table(sizes, seed, ncol=31):
    rng = np.random.default_rng(seed)
    n = int(sum(sizes))
    tab = rng.integers(0, 6, size=(n, ncol)).astype(np.float64)             # heavy ties
    tab[:, 6:14] = rng.normal(size=(n, 8))
    tab[:, 14:17] = np.round(rng.normal(size=(n, 3)), 1)
    z = rng.random((n, ncol)) < 0.1
    tab[z] = np.where(rng.random(int(z.sum())) < 0.5, -0.0, 0.0)             # -0.0 == 0.0
    tab[rng.random((n, ncol)) < 0.05] = np.nan
    tab[:, 0] = np.concatenate([np.arange(s) for s in sizes]) if n else []
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return tab, offsets


def test_reference_fixture(gpu):
    g = np.load(os.path.join(GOLD, "rank_cases.npz"))
    tab = np.zeros((5, 31))
    tab[:, 6] = g["values"]
    rank, rp = gpu.rank_device(tab, np.array([0, 5]), [6], 14245 / 365.25)
    npt.assert_array_equal(rank[:, 1], g["rank"])
    npt.assert_array_equal(rp[:, 1], (14245 / 365.25 + 1) / g["rank"])


def test_reference_event_tables(gpu):
    g = np.load(os.path.join(GOLD, "mhw_features_cases.npz"))
    table = g["table"]
    offsets = g["table_offsets"].astype(np.int64)
    check(gpu, table, offsets, COLS, 7.5)


@pytest.mark.parametrize("sizes", [
    [0],
    [1],
    [63],
    [64],
    [65],
    [256],
    [1024],
    [0, 1, 63, 64, 65, 0, 256, 1024, 2, 127, 128, 129, 0],
    [3, 5, 0, 7, 5003, 1, 60, 64, 4, 0, 9],
])
def test_synthetic_tables(gpu, sizes):
    tab, off = synth_table(sizes, seed=len(sizes) * 1000 + sum(sizes))
    check(gpu, tab, off, COLS, 40.0)


def test_many_cells(gpu):
    rng = np.random.default_rng(11)
    sizes = rng.poisson(30, size=3000)
    sizes[::97] = 0
    tab, off = synth_table(sizes, seed=12)
    check(gpu, tab, off, COLS, 41.0)


def test_leading_dimensions_and_column_lists(gpu):
    """ld_table 40, columns out of order, repeated and spread over more than one 16-column window;
    ld_out wider than ncols: the elements past ncols are left alone"""
    from xmhw_amd._lib import hip
    from xmhw_amd.device import DeviceBuffer
    h = hip()
    sizes = [5, 0, 70, 1, 130, 64]
    tab, off = synth_table(sizes, seed=3, ncol=40)
    cols = [39, 0, 7, 7, 22, 38, 1, 15, 16, 31, 30]
    ld_out = len(cols) + 3
    n = tab.shape[0]
    bufs = []
    try:
        d_tab = DeviceBuffer.from_array(tab); bufs.append(d_tab)
        d_off = DeviceBuffer.from_array(off); bufs.append(d_off)
        sentinel = np.full((n, ld_out), 12345.5)
        d_r = DeviceBuffer.from_array(sentinel); bufs.append(d_r)
        d_p = DeviceBuffer.from_array(sentinel); bufs.append(d_p)
        h.event_rank(d_tab.ptr, 40, d_off.ptr, len(sizes), cols, 3.25, d_r.ptr, d_p.ptr, ld_out)
        h.stream_sync(0)
        r = d_r.to_array((n, ld_out), np.float64)
        p = d_p.to_array((n, ld_out), np.float64)
    finally:
        for b in bufs:
            b.free()
    wr, wp = rank_oracle(tab, off, cols, 3.25)
    same(r[:, :len(cols)], wr[:, 1:])
    same(p[:, :len(cols)], wp[:, 1:])
    npt.assert_array_equal(r[:, len(cols):], 12345.5)
    npt.assert_array_equal(p[:, len(cols):], 12345.5)


def test_no_cells(gpu):
    from xmhw_amd._lib import hip
    hip().event_rank(0, 31, 0, 0, [6], 1.0, 0, 0, 1)            # C = 0: nothing is launched or touched
    rank, rp = gpu.rank_device(np.zeros((0, 31)), np.array([0]), [6, 7], 1.0)
    assert rank.shape == rp.shape == (0, 3)
    rank, rp = gpu.rank_device(np.zeros((0, 31)), np.array([0, 0, 0]), [6, 7], 1.0)
    assert rank.shape == (0, 3)


@pytest.mark.parametrize("cold", [False, True])
def test_oisst_end_to_end(gpu, cold):
    import xmhw_amd
    from xmhw_amd import GridSeries, climatology_series
    g = np.load(os.path.join(GOLD, "oisst_2003_2004.npz"))
    time = np.datetime64("2003-01-01") + g["time"].astype("timedelta64[D]")
    temp = GridSeries(g["sst"], ("time", "lat", "lon"), {"time": time, "lat": g["lat"], "lon": g["lon"]},
                      time_encoding={"calendar": "proleptic_gregorian"})
    clim = xmhw_amd.threshold(temp, pctile=80, coldSpells=cold)
    mhw = xmhw_amd.detect(temp, climatology_series(clim, "thresh"), climatology_series(clim, "seas"), coldSpells=cold)
    assert mhw.n_events > 20
    rank, rp = xmhw_amd.mhw_rank(mhw)
    n_years = time.shape[0] / 365.25
    cols = [mhw.columns.index(k) for k in RANKED]
    for c in range(mhw.n_cells):
        sl = slice(int(mhw.offsets[c]), int(mhw.offsets[c + 1]))
        wr, wp = rank_oracle(mhw.table[sl], np.array([0, sl.stop - sl.start]), cols, n_years)
        same(rank.table[sl, 1:], wr[:, 1:])
        same(rp.table[sl, 1:], wp[:, 1:])
        npt.assert_array_equal(rank.table[sl, 0], mhw.table[sl, 0])
    dims, coords, data = rank.to_dense()
    assert dims == ("events", "lat", "lon") and set(data) == {"event", *RANKED}
    if not cold:
        # a cell's longest event has duration rank 1 (ties: the latest of the longest)
        c = int(np.argmax(np.diff(mhw.offsets)))
        sl = slice(int(mhw.offsets[c]), int(mhw.offsets[c + 1]))
        d = mhw.table[sl, mhw.columns.index("duration")]
        best = np.nonzero(d == d.max())[0][-1]
        assert rank.table[sl, rank.columns.index("duration")][best] == 1


def test_point_series_with_the_reference_constant(gpu):
    """a single point: nYears = 14245 / 365.25 against the reference formula
    len(v) - v.argsort().argsort() (made stable, as documented), (nYears + 1) / rank"""
    import xmhw_amd
    from xmhw_amd import GridSeries, climatology_series
    g = np.load(os.path.join(GOLD, "oisst_2003_2004.npz"))
    time = np.datetime64("2003-01-01") + g["time"].astype("timedelta64[D]")
    sst = g["sst"].reshape(g["sst"].shape[0], -1)
    col = int(np.nonzero(~np.isnan(sst).any(axis=0))[0][0])
    temp = GridSeries(sst[:, col], ("time",), {"time": time}, time_encoding={"calendar": "proleptic_gregorian"})
    clim = xmhw_amd.threshold(temp, pctile=80)
    mhw = xmhw_amd.detect(temp, climatology_series(clim, "thresh"), climatology_series(clim, "seas"))
    assert mhw.point and mhw.n_events > 1
    ny = 14245 / 365.25
    rank, rp = xmhw_amd.mhw_rank(mhw, nYears=ny)
    for k in RANKED:
        v = mhw.table[:, mhw.columns.index(k)]
        if np.isnan(v).any():
            continue
        want = len(v) - v.argsort(kind="stable").argsort()
        j = rank.columns.index(k)
        npt.assert_array_equal(rank.table[:, j], want)
        npt.assert_array_equal(rp.table[:, j], (ny + 1) / want)
