"""mhw_objects() on the device (csrc/kernels_objects.hip) against the definition (tests/objects_oracle.py), with
assert_array_equal everywhere -- every output is an integer, a minimum or a maximum: the golden event tables,
synthetic CSR interval tables (no rows, one cell, cells of every size around a wave, a snake of one object, one
object of every row, a checkerboard in time, land and wrapping), canaries behind every output buffer, run-to-run
identity, a 12-million-row table, and threshold() -> detect() -> mhw_objects() on the OISST grid."""
import os

import numpy as np
import numpy.testing as npt
import pytest

import objects_cases as oc
import objects_oracle as oo
from xmhw_amd.objects import PER_OBJECT, _DTYPES, neighbour_table

pytestmark = pytest.mark.gpu
FIELDS = ("object", "root", "n_events", "n_cells", "time_start", "time_end", "duration", "cell_days", "area_days_q",
          "intensity_max", "peak_row", "time_peak", "peak_cell")


@pytest.fixture(scope="module")
def gpu():
    from xmhw_amd._lib import require_gpu
    require_gpu()
    from xmhw_amd import objects
    return objects


def check(gpu, args, oracle=oo.objects_graph):
    got = gpu.objects_device(*args)
    oo.same_result(got, oracle(*args))
    return got


def same_dataset(a, b):
    for k in FIELDS:
        npt.assert_array_equal(getattr(a, k), getattr(b, k), err_msg=k)
    assert (a.weight_bits, a.weight_unit) == (b.weight_bits, b.weight_unit)


def on_grid(keep, per_cell, connectivity=6, periodic_axis=None, seed=0):
    """stage arguments for ocean cells `keep` (2-D bool) with the interval lists per_cell (stacked order)"""
    rng = np.random.default_rng(seed)
    cell_index = np.nonzero(keep.reshape(-1))[0]
    start = np.array([r[0] for c in per_cell for r in c], dtype=np.int32)
    end = np.array([r[1] for c in per_cell for r in c], dtype=np.int32)
    offsets = np.concatenate([[0], np.cumsum([len(c) for c in per_cell])]).astype(np.int64)
    imax = np.round(rng.normal(size=start.shape[0]), 1)
    nbr = neighbour_table(cell_index, keep.shape, connectivity, periodic_axis)
    wq = rng.integers(0, 1 << 31, cell_index.shape[0], endpoint=True).astype(np.int64)
    return start, end, imax, offsets, nbr, (0 if connectivity == 6 else 1), wq


@pytest.mark.parametrize("key", list(oc.GOLDEN_COUNTS))
def test_golden_tables(gpu, key):
    connectivity, periodic = key
    ds = oc.golden_dataset()
    got = gpu.mhw_objects(ds, connectivity=connectivity, periodic=periodic, weights="coslat")
    want = gpu.mhw_objects(ds, connectivity=connectivity, periodic=periodic, weights="coslat", _compute=oo.objects_graph)
    same_dataset(got, want)
    assert (got.n_objects, int(got.n_events.max()), int((got.n_events == 1).sum())) == oc.GOLDEN_COUNTS[key]


def test_no_rows(gpu):
    from xmhw_amd._lib import hip
    hip().event_objects(0, 0, 0, 0, 0, 0, 4, 0, 0, 0)            # n = 0: nothing is launched or touched
    hip().object_reduce(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)
    got = gpu.objects_device(*oc.csr_case([0, 0, 0], 1))
    assert got["root"].shape == (0,) and all(got[k].shape == (0,) for k in PER_OBJECT)
    ob = gpu.mhw_objects(oc.dataset((2, 3), np.ones(6, bool), [[] for _ in range(6)], T=10))
    assert ob.n_objects == 0


@pytest.mark.parametrize("sizes", [[1], [63], [64], [65], [1000]])
def test_one_cell(gpu, sizes):
    got = check(gpu, oc.csr_case(sizes, seed=sizes[0]))
    npt.assert_array_equal(got["root"], np.arange(sizes[0]))     # the rows of one cell never link
    npt.assert_array_equal(got["n_cells"], 1)


@pytest.mark.parametrize("connectivity", [6, 26])
def test_cells_of_every_size(gpu, connectivity):
    sizes = [0, 1, 63, 64, 65, 1000, 0, 0, 64, 1, 1000, 65, 63, 2, 0, 129, 511, 513, 7, 0]
    check(gpu, oc.csr_case(sizes, seed=5, grid=(4, 5), connectivity=connectivity), oracle=oo.objects_edges)
    check(gpu, oc.csr_case(sizes, seed=6, grid=(1, 20), connectivity=connectivity, periodic_axis=1), oracle=oo.objects_edges)
    check(gpu, oc.csr_case(sizes, seed=7, T=300, grid=(5, 4), connectivity=connectivity, periodic_axis=0),
          oracle=oo.objects_edges)


@pytest.mark.parametrize("connectivity,periodic_axis", [(6, None), (26, None), (6, 1), (26, 0)])
def test_land_holes_and_wrapping(gpu, connectivity, periodic_axis):
    rng = np.random.default_rng(40 + connectivity)
    sizes = rng.poisson(12, size=700)
    sizes[::13] = 0
    check(gpu, oc.csr_case(sizes, seed=8, T=600, grid=(30, 31), land=1 - 700 / 930, connectivity=connectivity,
                           periodic_axis=periodic_axis), oracle=oo.objects_edges)
    check(gpu, oc.csr_case(sizes[:120], seed=9, T=200, grid=(12, 13), land=1 - 120 / 156, connectivity=connectivity,
                           periodic_axis=periodic_axis))


def test_snake_is_one_object(gpu):
    """a one-cell-wide path through a 64 x 64 grid, every cell one row on the same days: long union chains"""
    keep = np.zeros((64, 64), dtype=bool)
    keep[0::2] = True
    for k, i in enumerate(range(1, 64, 2)):
        keep[i, 63 if k % 2 == 0 else 0] = True
    n = int(keep.sum())
    args = on_grid(keep, [[(3, 12)]] * n)
    got = check(gpu, args, oracle=oo.objects_edges)
    npt.assert_array_equal(got["root"], 0)
    assert got["n_events"][0] == n == got["n_cells"][0] and got["cell_days"][0] == 10 * n
    # the same path with one cell cut out: two objects
    cut = keep.copy()
    cut[31, 63 if 15 % 2 == 0 else 0] = False
    got = check(gpu, on_grid(cut, [[(3, 12)]] * (n - 1)), oracle=oo.objects_edges)
    assert got["n_events"].shape == (2,)


def test_one_object_of_every_row(gpu):
    """one row per cell, all on overlapping days: every flush of the reduction goes to one slot"""
    keep = np.ones((300, 301), dtype=bool)
    rng = np.random.default_rng(3)
    s = rng.integers(0, 5, keep.size)
    args = on_grid(keep, [[(int(a), int(a) + 20)] for a in s], seed=4)
    got = check(gpu, args, oracle=oo.objects_edges)
    assert got["n_events"].tolist() == [keep.size] and got["n_cells"].tolist() == [keep.size]
    assert got["cell_days"][0] == 21 * keep.size
    assert got["area_days_q"][0] == 21 * int(args[6].sum()) > 2**40


def test_checkerboard_in_time(gpu):
    """cell (i, j) holds the days of the parity of i + j: no two voxels share a face, all share an edge"""
    ny, nx, days = 20, 21, 30
    keep = np.ones((ny, nx), dtype=bool)
    per_cell = [[(2 * k + (i + j) % 2,) * 2 for k in range(days)] for i in range(ny) for j in range(nx)]
    got = check(gpu, on_grid(keep, per_cell, 6), oracle=oo.objects_edges)
    npt.assert_array_equal(got["root"], np.arange(ny * nx * days))
    got = check(gpu, on_grid(keep, per_cell, 26), oracle=oo.objects_edges)
    npt.assert_array_equal(got["root"], 0)
    assert got["time_start"][0] == 0 and got["time_end"][0] == 2 * days - 1


def test_canaries_behind_every_output(gpu):
    """the entry points write n (or n_slots) elements of every output and nothing behind them; a row whose slot is
    outside [0, n_slots) is left out"""
    from xmhw_amd._lib import hip
    from xmhw_amd.device import DeviceBuffer
    h = hip()
    sizes = [5, 0, 70, 1, 130, 64, 3, 0, 9]
    start, end, imax, offsets, nbr, gap, wq = oc.csr_case(sizes, seed=21, T=300, grid=(3, 3), connectivity=26)
    n, C, pad = start.shape[0], len(sizes), 37
    want = oo.objects_graph(start, end, imax, offsets, nbr, gap, wq)
    bufs = []

    def up(a):
        bufs.append(DeviceBuffer.from_array(np.ascontiguousarray(a)))
        return bufs[-1]

    try:
        d_start, d_end, d_imax, d_off, d_nbr, d_wq = up(start), up(end), up(imax), up(offsets), up(nbr), up(wq)
        d_cell, d_root = up(np.full(n + pad, 0x5A5A5A5A, np.int32)), up(np.full(n + pad, 0x5A5A5A5A, np.int32))
        h.event_objects(d_start.ptr, d_end.ptr, n, d_off.ptr, C, d_nbr.ptr, nbr.shape[1], gap, d_cell.ptr, d_root.ptr)
        h.stream_sync(0)
        cell, root = d_cell.to_array((n + pad,), np.int32), d_root.to_array((n + pad,), np.int32)
        npt.assert_array_equal(root[:n], want["root"])
        npt.assert_array_equal(cell[:n], np.repeat(np.arange(C), sizes))
        npt.assert_array_equal(root[n:], 0x5A5A5A5A)
        npt.assert_array_equal(cell[n:], 0x5A5A5A5A)
        # slots = the roots themselves (n_slots = n), two rows pushed outside the range
        slot = root[:n].copy()
        loose = np.nonzero(slot == np.arange(n))[0][-2:]
        out_of_range = np.isin(slot, loose)
        slot[out_of_range] = np.where(np.arange(n)[out_of_range] % 2 == 0, -1, n)
        d_slot = up(slot)
        outs = {k: up(np.full(n + pad, 0x5A, np.int8).repeat(np.dtype(_DTYPES[k]).itemsize).view(_DTYPES[k])) for k in PER_OBJECT}
        h.object_reduce(d_start.ptr, d_end.ptr, d_imax.ptr, n, d_cell.ptr, d_off.ptr, d_wq.ptr, d_slot.ptr, n,
                        *[outs[k].ptr for k in PER_OBJECT])
        h.stream_sync(0)
        got = {k: outs[k].to_array((n + pad,), _DTYPES[k]) for k in PER_OBJECT}
    finally:
        for b in bufs:
            b.free()
    roots = np.unique(want["root"])
    kept = ~np.isin(roots, loose)
    empty = dict(n_events=0, n_cells=0, time_start=2**31 - 1, time_end=-1, cell_days=0, area_days_q=0,
                 intensity_max=np.nan, peak_row=-1)
    for k in PER_OBJECT:
        npt.assert_array_equal(got[k][n:].view(np.uint8), 0x5A, err_msg=k)
        npt.assert_array_equal(got[k][:n][roots[kept]], want[k][kept], err_msg=k)
        rest = np.ones(n, dtype=bool)
        rest[roots[kept]] = False
        npt.assert_array_equal(got[k][:n][rest], np.full(int(rest.sum()), empty[k], dtype=_DTYPES[k]), err_msg=k)


def test_two_runs_are_identical(gpu):
    rng = np.random.default_rng(2)
    args = oc.csr_case(rng.poisson(40, size=4096), seed=17, T=1500, grid=(64, 64), connectivity=26, periodic_axis=1)
    a, b = gpu.objects_device(*args), gpu.objects_device(*args)
    oo.same_result(a, b)
    oo.same_result(a, oo.objects_edges(*args))


def big_case(ny, nx, rows, seed):
    rng = np.random.default_rng(seed)
    C = ny * nx
    d = rng.integers(5, 40, (C, rows))
    g = rng.integers(2, 200, (C, rows))
    pos = np.cumsum(d + g, axis=1)
    start, end = (pos - d).reshape(-1).astype(np.int32), (pos - 1).reshape(-1).astype(np.int32)
    imax = rng.normal(size=C * rows).astype(np.float32).astype(np.float64)
    offsets = np.arange(C + 1, dtype=np.int64) * rows
    nbr = neighbour_table(np.arange(C), (ny, nx), 6, 1)
    wq = rng.integers(1, 1 << 20, C).astype(np.int64)
    return start, end, imax, offsets, nbr, 0, wq


def test_large_table(gpu):
    """448 x 448 = 200,704 cells x 60 rows = 12,042,240 rows, longitude wrapping.  The vectorised oracle
    (objects_edges: edge list, scipy's connected_components, sort-based reductions; one thread) takes 23 s on an
    8-core x86 host and finds 4,312,533 objects, the largest of 270 rows."""
    args = big_case(448, 448, 60, 99)
    got = gpu.objects_device(*args)
    oo.same_result(got, oo.objects_edges(*args))
    assert got["n_events"].sum() == 448 * 448 * 60


@pytest.mark.parametrize("cold", [False, True])
def test_oisst_end_to_end(gpu, cold):
    import xmhw_amd
    from xmhw_amd import GridSeries, climatology_series
    g = np.load(os.path.join(oc.GOLD, "oisst_2003_2004.npz"))
    time = np.datetime64("2003-01-01") + g["time"].astype("timedelta64[D]")
    temp = GridSeries(g["sst"], ("time", "lat", "lon"), {"time": time, "lat": g["lat"], "lon": g["lon"]},
                      time_encoding={"calendar": "proleptic_gregorian"})
    clim = xmhw_amd.threshold(temp, pctile=80, coldSpells=cold)
    mhw = xmhw_amd.detect(temp, climatology_series(clim, "thresh"), climatology_series(clim, "seas"), coldSpells=cold)
    assert mhw.n_events > 20
    for connectivity, periodic, weights in ((6, None, None), (26, None, "coslat"), (6, "lon", "coslat"), (26, "lat", None)):
        got = xmhw_amd.mhw_objects(mhw, connectivity=connectivity, periodic=periodic, weights=weights)
        want = xmhw_amd.mhw_objects(mhw, connectivity=connectivity, periodic=periodic, weights=weights,
                                    _compute=oo.objects_graph)
        same_dataset(got, want)
        assert 0 < got.n_objects <= mhw.n_events and got.n_events.sum() == mhw.n_events
        # the map of a day holds exactly the cells detect() has in an event on it
        pos = int(got.time_start[0])
        on = (mhw.table[:, 1] <= pos) & (mhw.table[:, 2] >= pos)
        cells = mhw.cell_index[np.repeat(np.arange(mhw.n_cells), np.diff(mhw.offsets))[on]]
        npt.assert_array_equal(np.nonzero(got.label_map(pos).reshape(-1) >= 0)[0], np.sort(cells))
