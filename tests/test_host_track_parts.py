"""Host side of mhw_track_parts() (xmhw_amd/track_parts.py) with the device stage replaced by the flood-fill oracle
(tests/track_parts_oracle.stage_oracle): the alignment with mhw_tracks(), ``ids`` subsets and their order, the three
identities, the derived per-object fields, every refusal (the 2**31-voxel one on the arithmetic alone), and the
hand-drawn cases with their expected counts."""
import numpy as np
import numpy.testing as npt
import pytest

import objects_cases as oc
import objects_oracle as oo
import track_parts_cases as pc
import track_parts_oracle as po
import tracks_oracle as to
from xmhw_amd import TrackPartsDataset, XmhwException, mhw_objects, mhw_track_parts, mhw_tracks
from xmhw_amd.detect import EventDataset
from xmhw_amd.track_parts import voxel_offsets

SEEDS = list(range(6))


def objects(ds, **kw):
    return mhw_objects(ds, _compute=oo.objects_graph, **kw)


def tracks(ds, obj, **kw):
    return mhw_tracks(ds, obj, _compute=to.stage_voxels, **kw)


def parts(ds, obj, neighbours=None, **kw):
    return mhw_track_parts(ds, obj, neighbours=neighbours, _compute=po.stage_for(ds, obj, neighbours), **kw)


def identities(tp, tr):
    """the three identities of the module docstring, and the alignment"""
    for k in ("ids", "offsets", "time_start", "time_end", "duration", "pos"):
        npt.assert_array_equal(getattr(tp, k), getattr(tr, k), err_msg=k)
    assert (tp.n_parts >= 1).all()
    assert (tp.n_parts.astype(np.int64) + tp.cells_largest - 1 <= tr.n_cells).all()
    one = tp.n_parts == 1
    npt.assert_array_equal(tp.cells_largest[one], tr.n_cells[one])
    npt.assert_array_equal(tp.area_largest_q[one], tr.area_q[one])
    assert (tp.area_largest_q <= tr.area_q).all() and (tp.cells_largest >= 1).all()


@pytest.mark.parametrize("connectivity,periodic", [(6, None), (26, "lon")])
@pytest.mark.parametrize("weights", [None, "coslat"])
def test_random_grids_against_the_dense_oracle(connectivity, periodic, weights):
    for seed in SEEDS:
        ds = oc.random_grid(seed)
        obj = objects(ds, connectivity=connectivity, periodic=periodic, weights=weights)
        tp = parts(ds, obj, weights=weights)
        assert isinstance(tp, TrackPartsDataset) and tp.neighbours == (4 if connectivity == 6 else 8)
        po.same_as_dense(tp, po.parts_dense(ds, obj, None, weights))
        identities(tp, tracks(ds, obj, weights=weights))
        npt.assert_array_equal(tp.area_largest, tp.area_largest_q * obj.weight_unit)


@pytest.mark.parametrize("neighbours", [4, 8])
def test_neighbours_override_never_joins_two_objects(neighbours):
    """objects of connectivity 6, parts under 8 neighbours: a diagonal cell of ANOTHER object stays out"""
    for seed in SEEDS:
        ds = oc.random_grid(seed)
        obj = objects(ds, connectivity=6)
        tp = parts(ds, obj, neighbours=neighbours)
        assert tp.neighbours == neighbours
        po.same_as_dense(tp, po.parts_dense(ds, obj, None, None, neighbours))
        identities(tp, tracks(ds, obj))
    # two cells on a diagonal, connectivity 6: two objects, and 8 neighbours do not make one part of them
    ds = pc.grid(2, 2, {(0, 0): [(0, 2)], (1, 1): [(0, 2)]}, T=4)
    obj = objects(ds, connectivity=6)
    assert obj.n_objects == 2
    tp = parts(ds, obj, neighbours=8)
    assert tp.n_parts.tolist() == [1] * 6 and tp.cells_largest.tolist() == [1] * 6


@pytest.mark.parametrize("case", pc.hand_drawn(), ids=lambda c: c[0])
def test_hand_drawn(case):
    name, ds, kw, neighbours, n_parts, cells_largest = case
    obj = objects(ds, **kw)
    assert obj.n_objects == 1
    tp = parts(ds, obj, neighbours=neighbours)
    assert tp.n_parts.tolist() == n_parts and tp.cells_largest.tolist() == cells_largest
    assert tp.area_largest_q.tolist() == [c << obj.weight_bits for c in cells_largest]
    assert tp.days_split.tolist() == [sum(1 for v in n_parts if v > 1)]
    assert tp.n_parts_max.tolist() == [max(n_parts)]
    assert tp.pos_n_parts_max.tolist() == [int(obj.time_start[0]) + n_parts.index(max(n_parts))]
    po.same_as_dense(tp, po.parts_dense(ds, obj, None, None, neighbours))
    identities(tp, tracks(ds, obj))


def test_broken_bar_is_split_for_three_days():
    ds = pc.broken_bar()
    tp = parts(ds, objects(ds))
    assert tp.n_parts.tolist() == [1, 1, 1, 2, 2, 2, 1, 1, 1] and tp.days_split.tolist() == [3]
    assert tp.n_parts_max.tolist() == [2] and tp.pos_n_parts_max.tolist() == [3]
    s = tp.series(0)
    npt.assert_array_equal(s["pos"], np.arange(9))
    npt.assert_array_equal(s["time"], ds.time[:9])


def test_the_two_maxima_are_independent():
    """3 light cells in one part, 2 heavy cells in another: cells_largest from the first, area_largest_q from the second"""
    ds = pc.grid(3, 7, {(1, 0): [(0, 1)], (1, 1): [(0, 1)], (1, 2): [(0, 1)], (1, 4): [(0, 1)], (1, 5): [(0, 1)],
                        (1, 3): [(2, 3)]}, T=5)
    w = np.ones((3, 7))
    w[1, 4:6] = 4.0
    obj = objects(ds, connectivity=26, weights=w)                 # the middle cell, a day later, ties them into one object
    assert obj.n_objects == 1
    tp = parts(ds, obj, neighbours=4, weights=w)
    unit = 1 << obj.weight_bits
    assert tp.n_parts.tolist() == [2, 2, 1, 1]
    assert tp.cells_largest.tolist() == [3, 3, 1, 1]
    assert tp.area_largest_q.tolist() == [2 * unit, 2 * unit, unit // 4, unit // 4]
    identities(tp, tracks(ds, obj, weights=w))


def test_ids_order_and_alignment_with_tracks():
    ds = oc.random_grid(5)
    obj = objects(ds, connectivity=26)
    assert obj.n_objects >= 4
    full = parts(ds, obj)
    npt.assert_array_equal(full.ids, np.arange(obj.n_objects))
    npt.assert_array_equal(full.offsets, np.concatenate([[0], np.cumsum(obj.duration)]))
    ids = np.arange(obj.n_objects)[::-1][::2]                     # a subset, in reverse order
    tp = parts(ds, obj, ids=ids)
    identities(tp, tracks(ds, obj, ids=ids))
    npt.assert_array_equal(tp.ids, ids)
    for i, o in enumerate(ids):                                   # the subset holds the slices of the full result
        a, b = tp.series(i), full.series(int(o))
        for k in a:
            npt.assert_array_equal(a[k], b[k], err_msg=k)
    for k in ("n_parts_max", "pos_n_parts_max", "days_split"):
        npt.assert_array_equal(getattr(tp, k), getattr(full, k)[ids], err_msg=k)
    assert tp.n_voxels == int(obj.cell_days[ids].sum()) and full.n_voxels == int(obj.cell_days.sum())
    empty = parts(ds, obj, ids=[])
    assert empty.n_selected == 0 and empty.n_parts.shape == (0,) and empty.offsets.tolist() == [0] and empty.n_voxels == 0
    assert empty.days_split.shape == (0,)
    with pytest.raises(XmhwException):
        tp.series(len(ids))


def test_stage_arguments():
    """what the host hands to the stage: the voxel numbering of the issue, the neighbour table of the override"""
    ds = oc.random_grid(2)
    obj = objects(ds, connectivity=6, periodic="lon")
    ids = np.arange(obj.n_objects)[1::2]
    seen = {}

    def stage(start, end, slot, cell, row_offsets, nbr, wq, vox_off, time_start, offsets):
        seen.update(locals())
        return po.stage_for(ds, obj, 8)(start, end, slot, cell, row_offsets, nbr, wq, vox_off, time_start, offsets)

    tp = mhw_track_parts(ds, obj, ids=ids, neighbours=8, _compute=stage)
    from xmhw_amd.objects import neighbour_table
    npt.assert_array_equal(seen["nbr"], neighbour_table(ds.cell_index, ds.sshape, 26, 1))
    sel = np.isin(obj.object, ids)
    npt.assert_array_equal(seen["slot"] >= 0, sel)
    days = np.where(sel, seen["end"].astype(np.int64) - seen["start"] + 1, 0)
    npt.assert_array_equal(seen["vox_off"], np.concatenate([[0], np.cumsum(days)]))
    assert seen["vox_off"].dtype == np.int64 and tp.n_voxels == days.sum()
    npt.assert_array_equal(seen["row_offsets"], ds.offsets)
    npt.assert_array_equal(seen["wq"], np.full(ds.n_cells, 1 << obj.weight_bits))


def test_refusals():
    ds = oc.random_grid(1)
    obj = objects(ds)
    with pytest.raises(XmhwException, match="mhw_track_parts expects the EventDataset"):
        mhw_track_parts("x", obj)
    with pytest.raises(XmhwException, match="mhw_track_parts expects the ObjectDataset"):
        mhw_track_parts(ds, "x")
    other = objects(oc.random_grid(2))
    with pytest.raises(XmhwException, match="one entry per table row|does not belong"):
        parts(ds, other)
    point = EventDataset(ds.table[:0], np.zeros(2, np.int64), ds.time, np.zeros(1, np.int64), np.ones(1, bool), (), (), {}, {}, {},
                         {}, True)
    with pytest.raises(XmhwException, match="grid"):
        mhw_track_parts(point, obj)
    one_dim = EventDataset(ds.table, ds.offsets, ds.time, ds.cell_index, ds.keep, ("cell",), (int(np.prod(ds.sshape)),), {}, {},
                           {}, {}, False)
    with pytest.raises(XmhwException, match="two spatial dims"):
        mhw_track_parts(one_dim, obj)
    for bad, what in (([0, 0], "distinct"), ([obj.n_objects], r"in \[0"), ([-1], r"in \[0"), ([[0]], "1-D"), ([0.5], "integer")):
        with pytest.raises(XmhwException, match=what):
            parts(ds, obj, ids=bad)
    for bad in (6, 26, 0, "8", 4.5):
        with pytest.raises(XmhwException, match="neighbours should be None, 4 or 8"):
            mhw_track_parts(ds, obj, neighbours=bad, _compute=po.stage_for(ds, obj))
    with pytest.raises(XmhwException, match="weights should be None, 'coslat' or an array, got 'area'"):
        parts(ds, obj, weights="area")
    broken = EventDataset(ds.table, ds.offsets[:-1], ds.time, ds.cell_index, ds.keep, ds.sdims, ds.sshape, ds.coords, {}, {}, {},
                          False)
    with pytest.raises(XmhwException, match="offsets and cell_index do not describe the table"):
        parts(broken, obj)
    with pytest.raises(XmhwException, match="do not fit"):
        mhw_track_parts(ds, obj, _compute=lambda *a: dict(n_parts=np.ones(3, np.int32), cells_largest=np.ones(3, np.int32),
                                                          area_largest_q=np.ones(3, np.int64)))
    # a table row outside the days of its object: the refusal of mhw_tracks()
    moved = EventDataset(ds.table.copy(), ds.offsets, ds.time, ds.cell_index, ds.keep, ds.sdims, ds.sshape, ds.coords, {}, {}, {},
                         False)
    first = int(np.nonzero(ds.table[:, oc.COL["index_start"]] == obj.time_start[obj.object])[0][0])    # opens its object
    moved.table[first, oc.COL["index_start"]] -= 1
    with pytest.raises(XmhwException, match="outside the days of its object: obj does not belong to mhw"):
        parts(moved, obj)
    # a stage that reports an empty day
    L = int(obj.duration.sum())
    with pytest.raises(XmhwException, match="hold no cell"):
        mhw_track_parts(ds, obj, _compute=lambda *a: dict(n_parts=np.zeros(L, np.int32), cells_largest=np.zeros(L, np.int32),
                                                          area_largest_q=np.zeros(L, np.int64)))


def test_two_to_the_31_voxels_are_refused_on_the_arithmetic():
    """three rows of 2**30 days: L fits, V = 3 * 2**30 does not; nothing of that size is ever made"""
    big = 1 << 30
    with pytest.raises(XmhwException, match="ids="):
        voxel_offsets(np.zeros(3, np.int32), np.full(3, big - 1, np.int32), np.zeros(3, np.int32))
    with pytest.raises(XmhwException, match="ids="):                 # 2**31 itself is refused ...
        voxel_offsets(np.zeros(3, np.int32), np.full(3, big - 1, np.int32), np.array([0, -1, 0], np.int32))
    off = voxel_offsets(np.zeros(3, np.int32), np.array([big - 1, big - 1, big - 2], np.int32), np.array([0, -1, 0], np.int32))
    assert off.tolist() == [0, big, big, 2 * big - 1]             # ... one less is not; an unselected row counts 0
    ds = pc.grid(1, 3, {(0, 0): [(0, big - 1)], (0, 1): [(0, big - 1)], (0, 2): [(0, big - 1)]}, T=4)
    obj = objects(ds)
    assert obj.n_objects == 1 and int(obj.duration[0]) == big
    called = []
    with pytest.raises(XmhwException, match=r"2\*\*31 and more.*ids="):
        mhw_track_parts(ds, obj, _compute=lambda *a: called.append(1))
    assert not called


def test_empty_table():
    ds = oc.dataset((2, 3), np.ones(6, bool), [[] for _ in range(6)], T=10)
    called = []
    tp = mhw_track_parts(ds, objects(ds), _compute=lambda *a: called.append(1))
    assert tp.n_selected == 0 and tp.offsets.tolist() == [0] and not called
    assert tp.n_parts.shape == tp.area_largest.shape == tp.n_parts_max.shape == (0,)


def test_to_xarray():
    xr = pytest.importorskip("xarray")
    ds = oc.random_grid(4)
    obj = objects(ds)
    x = parts(ds, obj).to_xarray()
    assert isinstance(x, xr.Dataset) and x.sizes["obs"] == x["offsets"].values[-1] and x.attrs["neighbours"] == 4
