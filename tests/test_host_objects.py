"""Host side of mhw_objects() (xmhw_amd/objects.py) with the device stage replaced by the oracle
(tests/objects_oracle.py): the event graph against the rasterised voxels (own flood fill, and
scipy.ndimage.label where scipy imports), the golden event tables' object counts, hand cases for every rule of
the definition, the exceptions, the weights and the dataset's helpers."""
import math

import numpy as np
import numpy.testing as npt
import pytest

import objects_cases as oc
import objects_oracle as oo
from xmhw_amd import XmhwException, mhw_objects
from xmhw_amd.coverage import quantise_weights
from xmhw_amd.detect import EventDataset
from xmhw_amd.objects import neighbour_table, weight_bits

try:
    import scipy.ndimage as ndi
except ImportError:
    ndi = None

SEEDS = list(range(30))


def run(ds, **kw):
    return mhw_objects(ds, _compute=oo.objects_graph, **kw)


@pytest.mark.parametrize("connectivity", [6, 26])
@pytest.mark.parametrize("periodic", [None, "lon", "lat"])
def test_graph_is_the_voxel_volume(connectivity, periodic):
    for seed in SEEDS:
        ds = oc.random_grid(seed)
        start, end, imax, offsets, nbr, gap, flat, axis = oc.stage_inputs(ds, connectivity, periodic)
        wq = np.arange(ds.n_cells, dtype=np.int64) + 1
        g = oo.objects_graph(start, end, imax, offsets, nbr, gap, wq)
        T = ds.time.shape[0]
        vroot, label = oo.voxel_roots(start, end, flat, ds.sshape, T, connectivity, axis)
        npt.assert_array_equal(g["root"], vroot, err_msg=f"seed {seed}")
        # the object's numbers against the labelled volume itself
        for k, r in enumerate(np.unique(vroot)):
            vox = label == label[start[r], flat[r] // ds.sshape[1], flat[r] % ds.sshape[1]]
            assert g["cell_days"][k] == vox.sum()
            assert g["n_cells"][k] == vox.any(axis=0).sum()
            tt = np.nonzero(vox.any(axis=(1, 2)))[0]
            assert (g["time_start"][k], g["time_end"][k]) == (tt[0], tt[-1])
        oo.same_result(oo.objects_edges(start, end, imax, offsets, nbr, gap, wq), g)
        if periodic is None and ndi is not None:
            vol = oo.rasterise(start, end, flat, ds.sshape, T)
            st = ndi.generate_binary_structure(3, 1) if connectivity == 6 else np.ones((3, 3, 3))
            lab, _ = ndi.label(vol, structure=st)
            rows_lab = lab[start, flat // ds.sshape[1], flat % ds.sshape[1]]
            npt.assert_array_equal(oo.roots_from_labels(rows_lab), g["root"], err_msg=f"scipy, seed {seed}")


@pytest.mark.parametrize("key", list(oc.GOLDEN_COUNTS))
def test_golden_tables_object_counts(key):
    connectivity, periodic = key
    ds = oc.golden_dataset()
    assert ds.n_cells == 108 and ds.n_events == 1795
    ob = run(ds, connectivity=connectivity, periodic=periodic)
    assert (ob.n_objects, int(ob.n_events.max()), int((ob.n_events == 1).sum())) == oc.GOLDEN_COUNTS[key]
    assert ob.n_events.sum() == 1795 and ob.object.shape == (1795,)
    start, end, imax, offsets, nbr, gap, flat, axis = oc.stage_inputs(ds, connectivity, periodic)
    oo.same_result(oo.objects_edges(start, end, imax, offsets, nbr, gap, np.ones(108, np.int64)),
                   oo.objects_graph(start, end, imax, offsets, nbr, gap, np.ones(108, np.int64)))


def grid(ny, nx, cells, land=()):
    """cells: {(i, j): [(start, end[, imax]), ...]}; every other grid point is ocean without events, `land` is land"""
    keep = np.ones((ny, nx), dtype=bool)
    for p in land:
        keep[p] = False
    per_cell = [cells.get((i, j), []) for i in range(ny) for j in range(nx) if keep[i, j]]
    return oc.dataset((ny, nx), keep, per_cell, T=60)


def test_diagonal_pair():
    ds = grid(3, 3, {(0, 0): [(5, 9)], (1, 1): [(5, 9)]})
    assert run(ds, connectivity=6).n_objects == 2
    ob = run(ds, connectivity=26)
    assert ob.n_objects == 1 and ob.n_cells[0] == 2 and ob.cell_days[0] == 10


def test_end_to_start_in_neighbouring_cells():
    ds = grid(2, 3, {(0, 0): [(5, 9)], (0, 1): [(10, 14)], (1, 1): [(16, 20)]})
    assert run(ds, connectivity=6).n_objects == 3
    ob = run(ds, connectivity=26)                      # days 9 and 10 are a step apart; days 14 and 16 are not
    assert ob.n_objects == 2
    npt.assert_array_equal(ob.object, [0, 0, 1])
    npt.assert_array_equal(ob.duration, [10, 5])


def test_land_barrier():
    cells = {(0, 0): [(0, 9)], (0, 2): [(0, 9)], (1, 0): [(0, 9)], (1, 2): [(0, 9)]}
    ds = grid(2, 3, cells, land=[(0, 1), (1, 1)])
    for conn in (6, 26):
        ob = run(ds, connectivity=conn)
        assert ob.n_objects == 2
        npt.assert_array_equal(ob.n_cells, [2, 2])
    open_sea = grid(2, 3, {**cells, (0, 1): [(3, 4)]}, land=[(1, 1)])
    assert run(open_sea, connectivity=6).n_objects == 1


def test_wrap_only_link():
    ds = grid(2, 5, {(0, 0): [(10, 12)], (0, 4): [(12, 20)], (1, 2): [(0, 3)]})
    assert run(ds).n_objects == 3
    assert run(ds, periodic="lat").n_objects == 3
    ob = run(ds, periodic="lon")
    assert ob.n_objects == 2
    npt.assert_array_equal(ob.object, [1, 1, 0])       # ids by time_start: the (1, 2) event starts first
    npt.assert_array_equal(ob.root, [2, 0])
    # a cell is never its own neighbour, a wrapping line of two cells has one neighbour twice
    npt.assert_array_equal(neighbour_table(np.arange(2), (2, 1), 6, 1), [[-1, 1, -1, -1], [0, -1, -1, -1]])
    npt.assert_array_equal(neighbour_table(np.arange(2), (1, 2), 6, 1), [[-1, -1, 1, 1], [-1, -1, 0, 0]])


def test_rows_one_and_three_together_row_two_apart():
    # cell (0, 1): its rows 1 and 3 meet through cells (0, 0) and (1, 0), its row 2 touches nothing
    ds = grid(2, 2, {(0, 0): [(0, 8), (18, 30)], (1, 0): [(7, 19)], (0, 1): [(0, 5), (12, 14), (20, 25)],
                     (1, 1): [(40, 41)]})
    # rows: (0,0): 0 1 | (0,1): 2 3 4 | (1,0): 5 | (1,1): 6
    ob = run(ds)
    npt.assert_array_equal(ob.object, [0, 0, 0, 1, 0, 0, 2])
    assert ob.n_events[0] == 5 and ob.n_cells[0] == 3   # cell (0, 1) gives rows 2 and 4 and counts once
    assert ob.n_events[1] == 1 and ob.n_cells[1] == 1


def test_all_nan_object_and_peak_ties():
    nan = float("nan")
    ds = grid(1, 4, {(0, 0): [(0, 4, nan)], (0, 1): [(0, 4, nan)], (0, 3): [(0, 4, 2.0), (10, 14, 3.0), (20, 24, 3.0)],
                     (0, 2): [(12, 22, nan), (30, 31, -0.0)]})
    # rows: 0 | 1 | (0,2): 2 3 | (0,3): 4 5 6
    ob = run(ds)
    npt.assert_array_equal(ob.object, [0, 0, 2, 3, 1, 2, 2])
    assert np.isnan(ob.intensity_max[0]) and ob.peak_row[0] == -1 and np.isnan(ob.time_peak[0]) and ob.peak_cell[0] == -1
    assert ob.intensity_max[2] == 3.0 and ob.peak_row[2] == 5          # rows 5 and 6 tie: the smaller row; row 2 is NaN
    assert ob.time_peak[2] == 10 and ob.peak_cell[2] == 3
    assert ob.intensity_max[3] == 0.0 and not np.signbit(ob.intensity_max[3]) and ob.peak_row[3] == 3
    tie = grid(1, 2, {(0, 0): [(0, 4, -0.0)], (0, 1): [(0, 4, 0.0)]})
    assert run(tie).peak_row[0] == 0                                    # -0.0 == 0.0: the smaller row


def test_ids_follow_time_start_then_root():
    ds = grid(1, 5, {(0, 0): [(30, 35)], (0, 2): [(7, 9), (30, 31)], (0, 4): [(7, 8)]})
    ob = run(ds)
    npt.assert_array_equal(ob.time_start, [7, 7, 30, 30])
    npt.assert_array_equal(ob.root, [1, 3, 0, 2])
    npt.assert_array_equal(ob.object, [2, 0, 3, 1])
    npt.assert_array_equal(ob.time_stamps(ob.time_start), ds.time[[7, 7, 30, 30]])


def test_exceptions():
    ds = oc.random_grid(3)
    with pytest.raises(XmhwException, match="EventDataset"):
        mhw_objects({"table": ds.table}, _compute=oo.objects_graph)
    point = EventDataset(ds.table[:2], np.array([0, 2]), ds.time, np.array([0]), np.array([True]), (), (), {}, {}, {}, {}, True)
    with pytest.raises(XmhwException, match="grid"):
        run(point)
    for sdims, sshape in ((("x",), (ds.keep.size,)), (("a", "b", "c"), (1,) + ds.sshape)):
        other = EventDataset(ds.table, ds.offsets, ds.time, ds.cell_index, ds.keep, sdims, sshape, {}, {}, {}, {}, False)
        with pytest.raises(XmhwException, match="two spatial dims"):
            run(other)
    for conn in (4, 8, 18, "6", None):
        with pytest.raises(XmhwException, match="connectivity"):
            run(ds, connectivity=conn)
    with pytest.raises(XmhwException, match="periodic"):
        run(ds, periodic="time")
    with pytest.raises(XmhwException, match="weights should be None"):
        run(ds, weights="area")
    with pytest.raises(XmhwException, match="shape of the spatial grid"):
        run(ds, weights=np.ones(3))
    bad = np.ones(ds.sshape)
    bad[0, 0] = -1
    with pytest.raises(XmhwException, match=">= 0"):
        run(ds, weights=bad)
    with pytest.raises(XmhwException, match="all zero"):
        run(ds, weights=np.zeros(ds.sshape))
    bad[0, 0] = np.nan
    with pytest.raises(XmhwException, match="finite"):
        run(ds, weights=bad)
    touching = grid(1, 2, {(0, 0): [(0, 4), (5, 9)]})
    with pytest.raises(XmhwException, match="one step apart"):
        run(touching)
    # offsets that do not cover the table; the weights are looked at first
    broken = EventDataset(ds.table, ds.offsets[:-1], ds.time, ds.cell_index, ds.keep, ds.sdims, ds.sshape, ds.coords, {}, {}, {},
                          False)
    with pytest.raises(XmhwException, match="offsets and cell_index do not describe the table"):
        run(broken)
    with pytest.raises(XmhwException, match="weights should be None, 'coslat' or an array, got 'area'"):
        run(broken, weights="area")

    class Huge(EventDataset):
        n_events = 1 << 31
    huge = Huge(ds.table, ds.offsets, ds.time, ds.cell_index, ds.keep, ds.sdims, ds.sshape, ds.coords, {}, {}, {}, False)
    with pytest.raises(XmhwException, match=r"2\*\*31"):
        mhw_objects(huge, _compute=lambda *a: pytest.fail("device stage reached"))


def test_empty_table():
    ds = grid(2, 3, {})
    assert ds.n_events == 0
    ob = run(ds)
    assert ob.n_objects == 0 and ob.object.shape == (0,) and ob.root.shape == (0,)
    for k in ("n_events", "n_cells", "time_start", "time_end", "duration", "cell_days", "area_days_q", "intensity_max",
              "peak_row", "time_peak", "peak_cell"):
        assert getattr(ob, k).shape == (0,)
    assert ob.weight_bits == 31
    npt.assert_array_equal(ob.label_map(0), np.full((2, 3), -1))


@pytest.mark.parametrize("connectivity,periodic", [(6, None), (26, "lon")])
def test_label_map_is_the_rasterised_volume(connectivity, periodic):
    ds = oc.random_grid(11)
    ob = run(ds, connectivity=connectivity, periodic=periodic)
    start, end, imax, offsets, nbr, gap, flat, axis = oc.stage_inputs(ds, connectivity, periodic)
    _, label = oo.voxel_roots(start, end, flat, ds.sshape, ds.time.shape[0], connectivity, axis)
    for t in range(ds.time.shape[0]):
        m = ob.label_map(t)
        assert m.shape == ds.sshape and m.dtype == np.int32
        npt.assert_array_equal(m >= 0, label[t] >= 0)
        # one-to-one between the ids on the map and the flood fill's labels
        pairs = {(int(a), int(b)) for a, b in zip(m[m >= 0], label[t][m >= 0])}
        assert len(pairs) == len({a for a, _ in pairs}) == len({b for _, b in pairs})


def test_weight_bits_shrink_with_the_total_duration():
    assert weight_bits(0) == 31 and weight_bits(2**31 - 1) == 31 and weight_bits(2**31) == 30 and weight_bits(2**40) == 21
    # 3 cells x one event of 2**30 steps: the durations sum to 3 * 2**30 > 2**31
    d = 1 << 30
    ds = grid(1, 3, {(0, 0): [(0, d - 1)], (0, 1): [(5, d + 4)], (0, 2): [(9, d + 8)]})
    w = np.array([[0.3, 1.7, 0.9]])
    ob = run(ds, weights=w)
    assert ob.weight_bits == 30 and ob.weight_unit == 1.7 / 2**30
    assert ob.n_objects == 1 and ob.cell_days[0] == 3 * d
    wq = np.rint(w[0] / 1.7 * 2**30).astype(np.int64)
    assert ob.area_days_q[0] == int(wq.sum()) * d < 2**62


@pytest.mark.parametrize("weights", [None, "coslat", "array"])
def test_area_days_against_fsum(weights):
    ds = oc.random_grid(5)
    rng = np.random.default_rng(1)
    w_arg = rng.uniform(0.0, 3.0, ds.sshape) if weights == "array" else weights
    ob = run(ds, weights=w_arg, connectivity=26)
    if weights is None:
        w = np.ones(ds.sshape)
        assert ob.weight_unit == 2.0**-31
        npt.assert_array_equal(ob.area_days_q, ob.cell_days << 31)
    elif weights == "coslat":
        w = np.broadcast_to(np.cos(np.deg2rad(ds.coords["lat"]))[:, None], ds.sshape)
    else:
        w = w_arg
    w = w.reshape(-1)
    start, end, imax, offsets, nbr, gap, flat, axis = oc.stage_inputs(ds, 26, None)
    for k in range(ob.n_objects):
        rows = np.nonzero(ob.object == k)[0]
        want = math.fsum(float(w[flat[r]]) * (int(end[r]) - int(start[r]) + 1) for r in rows)
        assert abs(int(ob.area_days_q[k]) * ob.weight_unit - want) <= int(ob.cell_days[k]) * ob.weight_unit / 2


def test_quantise_weights_default_is_unchanged():
    w = np.array([0.25, 1.0, 3.0, 0.0, 2.999999])
    wq, unit = quantise_weights(w)
    npt.assert_array_equal(wq, np.rint(w / 3.0 * 2**31).astype(np.int64))
    assert unit == 3.0 / 2**31 and wq.max() == 1 << 31
    wq20, unit20 = quantise_weights(w, bits=20)
    npt.assert_array_equal(wq20, np.rint(w / 3.0 * 2**20).astype(np.int64))
    assert unit20 == 3.0 / 2**20
