"""Host side of mhw_track_genealogy() (xmhw_amd/track_genealogy.py) with the device stage replaced by the flood-fill
oracle (tests/track_genealogy_oracle.stage_oracle): the alignment with mhw_tracks() and mhw_track_parts(), the derived
per-object fields, the sorting of the edges and edge_offsets, ``ids`` subsets and their order, every refusal (the
2**31-voxel one on the arithmetic alone), stages that return wrong shapes, the hash-set sizing, the turning of the
device's root voxels into edges, and the hand-drawn cases with every count and edge written out."""
import numpy as np
import numpy.testing as npt
import pytest

import objects_cases as oc
import objects_oracle as oo
import track_genealogy_cases as gc
import track_genealogy_oracle as go
import track_parts_cases as pc
import track_parts_oracle as po
import tracks_oracle as to
from xmhw_amd import (TrackGenealogyDataset, XmhwException, mhw_objects, mhw_track_genealogy, mhw_track_parts, mhw_tracks)
from xmhw_amd import track_genealogy as tgm

SEEDS = list(range(6))


def objects(ds, **kw):
    return mhw_objects(ds, _compute=oo.objects_graph, **kw)


def genealogy(ds, obj, neighbours=None, **kw):
    return mhw_track_genealogy(ds, obj, neighbours=neighbours, _compute=go.stage_for(ds, obj, neighbours), **kw)


def identities(tg, connected):
    """the identities of the module docstring that need nothing but the result itself"""
    first, last = tg.offsets[:-1], tg.offsets[1:] - 1
    assert (tg.n_links[first] == 0).all() and (tg.n_born[first] == tg.n_parts[first]).all()
    assert (tg.n_ended[last] == tg.n_parts[last]).all()
    assert (tg.n_links >= tg.n_parts - tg.n_born).all()
    L = int(tg.offsets[-1])
    entry = tg.offsets[tg.edge_track] + (tg.edge_pos - tg.time_start[tg.edge_track])
    npt.assert_array_equal(np.bincount(entry, minlength=L), tg.n_links)
    # the out-degrees recomputed from the edge list: a node is (entry of the earlier day, label)
    nodes, outdeg = np.unique(np.stack([entry - 1, tg.edge_from], axis=1), axis=0, return_counts=True)
    npt.assert_array_equal(np.bincount(nodes[outdeg >= 2, 0], minlength=L), tg.n_split)
    npt.assert_array_equal(tg.n_parts - np.bincount(nodes[:, 0], minlength=L), tg.n_ended)
    order = np.lexsort((tg.edge_to, tg.edge_from, tg.edge_pos, tg.edge_track))
    npt.assert_array_equal(order, np.arange(order.shape[0]))
    npt.assert_array_equal(tg.edge_offsets, np.searchsorted(tg.edge_track, np.arange(tg.n_selected + 1)))
    npt.assert_array_equal(tg.n_edges, np.diff(tg.edge_offsets))
    npt.assert_array_equal(tg.n_nodes, np.add.reduceat(tg.n_parts.astype(np.int64), first) if tg.n_selected else [])
    if connected:
        assert (tg.n_edges >= tg.n_nodes - 1).all()


@pytest.mark.parametrize("connectivity,periodic", [(6, None), (26, "lon"), (6, "lon"), (26, None)])
def test_random_grids_against_the_dense_oracle(connectivity, periodic):
    for seed in SEEDS:
        ds = oc.random_grid(seed)
        obj = objects(ds, connectivity=connectivity, periodic=periodic)
        tg = genealogy(ds, obj)
        assert isinstance(tg, TrackGenealogyDataset) and tg.neighbours == (4 if connectivity == 6 else 8)
        go.same_as_dense(tg, go.genealogy_dense(ds, obj))
        identities(tg, connected=connectivity == 6)
        tr = mhw_tracks(ds, obj, _compute=to.stage_voxels)
        tp = mhw_track_parts(ds, obj, _compute=po.stage_for(ds, obj))
        for k in ("ids", "offsets", "time_start", "time_end", "duration", "pos"):
            npt.assert_array_equal(getattr(tg, k), getattr(tr, k), err_msg=k)
            npt.assert_array_equal(getattr(tg, k), getattr(tp, k), err_msg=k)
        npt.assert_array_equal(tg.n_parts, tp.n_parts)
        assert tg.n_voxels == tp.n_voxels


@pytest.mark.parametrize("neighbours", [4, 8])
def test_neighbours_override_on_objects_of_connectivity_6(neighbours):
    for seed in SEEDS:
        ds = oc.random_grid(seed)
        obj = objects(ds, connectivity=6)
        tg = genealogy(ds, obj, neighbours=neighbours)
        assert tg.neighbours == neighbours
        go.same_as_dense(tg, go.genealogy_dense(ds, obj, None, neighbours))
        identities(tg, connected=True)
        npt.assert_array_equal(tg.n_parts, mhw_track_parts(ds, obj, neighbours=neighbours, _compute=po.stage_for(ds, obj, neighbours)).n_parts)


@pytest.mark.parametrize("case", gc.hand_drawn(), ids=lambda c: c[0])
def test_hand_drawn(case):
    name, ds, want = case
    obj = objects(ds, connectivity=6)
    assert obj.n_objects == 1
    tg = genealogy(ds, obj)
    gc.check_hand_drawn(tg, want)
    go.same_as_dense(tg, go.genealogy_dense(ds, obj))
    identities(tg, connected=True)


def test_broken_bar_splits_once_and_merges_once():
    ds = pc.broken_bar()
    tg = genealogy(ds, objects(ds))
    assert tg.n_splits.tolist() == [1] and tg.n_merges.tolist() == [1] and tg.n_births.tolist() == [0] and tg.n_ends.tolist() == [0]
    s = tg.series(0)
    npt.assert_array_equal(s["pos"], np.arange(9))
    npt.assert_array_equal(s["time"], ds.time[:9])
    assert s["n_split"].tolist().index(1) == 2 and s["n_merged"].tolist().index(1) == 6
    e = tg.edges(0)
    assert e["edge_pos"].shape == (12,) and e["edge_from"].dtype == np.int64
    npt.assert_array_equal(e["time"], ds.time[e["edge_pos"]])
    assert [(int(a), int(b)) for p, a, b in zip(e["edge_pos"], e["edge_from"], e["edge_to"]) if p == 3] == [(5, 5), (5, 8)]
    with pytest.raises(XmhwException):
        tg.edges(1)
    with pytest.raises(XmhwException):
        tg.series(-1)


def test_births_and_ends_within_a_life():
    """a cell that joins an object a day late through a diagonal (connectivity 26, parts under 4 neighbours) is born
    within the life of its object, and one that leaves early ends within it"""
    ds = pc.grid(3, 3, {(0, 0): [(0, 5)], (1, 1): [(2, 3)]}, T=7)
    obj = objects(ds, connectivity=26)
    assert obj.n_objects == 1
    tg = genealogy(ds, obj, neighbours=4)
    assert tg.n_parts.tolist() == [1, 1, 2, 2, 1, 1] and tg.n_born.tolist() == [1, 0, 1, 0, 0, 0]
    assert tg.n_ended.tolist() == [0, 0, 0, 1, 0, 1] and tg.n_births.tolist() == [1] and tg.n_ends.tolist() == [1]
    assert tg.n_edges.tolist() == [6] and tg.n_nodes.tolist() == [8]       # not connected: 6 < 8 - 1
    eight = genealogy(ds, obj)
    assert eight.n_parts.tolist() == [1] * 6 and eight.n_births.tolist() == [0] and eight.n_edges.tolist() == [5]


def test_ids_reversed_and_partial():
    ds = oc.random_grid(5)
    obj = objects(ds, connectivity=26)
    assert obj.n_objects >= 4
    full = genealogy(ds, obj)
    npt.assert_array_equal(full.ids, np.arange(obj.n_objects))
    ids = np.arange(obj.n_objects)[::-1][::2]                     # a subset, in reverse order
    tg = genealogy(ds, obj, ids=ids)
    go.same_as_dense(tg, go.genealogy_dense(ds, obj, ids))
    identities(tg, connected=False)
    tr = mhw_tracks(ds, obj, ids=ids, _compute=to.stage_voxels)
    for k in ("ids", "offsets", "time_start", "time_end", "duration", "pos"):
        npt.assert_array_equal(getattr(tg, k), getattr(tr, k), err_msg=k)
    for i, o in enumerate(ids):                                   # the subset holds the slices of the full result
        a, b = tg.series(i), full.series(int(o))
        for k in a:
            npt.assert_array_equal(a[k], b[k], err_msg=k)
        a, b = tg.edges(i), full.edges(int(o))
        assert (a["edge_track"] == i).all() and (b["edge_track"] == o).all()
        for k in ("edge_pos", "edge_from", "edge_to"):
            npt.assert_array_equal(a[k], b[k], err_msg=k)
    for k in go.PER_OBJECT:
        npt.assert_array_equal(getattr(tg, k), getattr(full, k)[ids], err_msg=k)
    empty = genealogy(ds, obj, ids=[])
    assert empty.n_selected == 0 and empty.n_parts.shape == (0,) and empty.offsets.tolist() == [0] and empty.n_voxels == 0
    assert empty.edge_offsets.tolist() == [0] and empty.edge_from.shape == (0,) and empty.n_splits.shape == (0,)


def test_edges_are_sorted_whatever_the_stage_returns():
    ds = oc.random_grid(3)
    obj = objects(ds, connectivity=6)
    stage = go.stage_for(ds, obj)

    def shuffled(*args):
        got = stage(*args)
        order = np.random.default_rng(0).permutation(got["edge_track"].shape[0])
        for k in go.EDGES:
            got[k] = got[k][order]
        return got

    tg = mhw_track_genealogy(ds, obj, _compute=shuffled)
    assert tg.edge_track.shape[0] > 10
    go.same_as_dense(tg, go.genealogy_dense(ds, obj))


def test_stage_arguments_and_edge_capacity():
    ds = oc.random_grid(2)
    obj = objects(ds, connectivity=6, periodic="lon")
    ids = np.arange(obj.n_objects)[1::2]
    seen = {}

    def stage(start, end, slot, cell, row_offsets, nbr, vox_off, time_start, offsets):
        seen.update(locals())
        return go.stage_for(ds, obj, 8)(start, end, slot, cell, row_offsets, nbr, vox_off, time_start, offsets)

    tg = mhw_track_genealogy(ds, obj, ids=ids, neighbours=8, _compute=stage)
    from xmhw_amd.objects import neighbour_table
    npt.assert_array_equal(seen["nbr"], neighbour_table(ds.cell_index, ds.sshape, 26, 1))
    sel = np.isin(obj.object, ids)
    npt.assert_array_equal(seen["slot"] >= 0, sel)
    days = np.where(sel, seen["end"].astype(np.int64) - seen["start"] + 1, 0)
    npt.assert_array_equal(seen["vox_off"], np.concatenate([[0], np.cumsum(days)]))
    assert tg.n_voxels == days.sum()
    npt.assert_array_equal(seen["row_offsets"], ds.offsets)
    # one key per selected row and day but the last: an upper bound of the edges, the rows of detect() never touching
    cap = tgm.edge_capacity(seen["start"], seen["end"], seen["slot"], seen["cell"])
    assert cap == int((days - 1)[sel].sum()) >= tg.edge_track.shape[0]
    # two touching rows of one cell count one key more where their slots agree
    s, e, c = np.array([0, 4, 9, 0]), np.array([3, 8, 9, 5]), np.array([0, 0, 0, 1])
    assert tgm.edge_capacity(s, e, np.array([0, 0, 0, 0]), c) == 3 + 4 + 0 + 5 + 2
    assert tgm.edge_capacity(s, e, np.array([0, 1, 0, 0]), c) == 3 + 4 + 0 + 5
    assert tgm.edge_capacity(s, e, np.array([0, -1, -1, 0]), c) == 3 + 5
    assert tgm.edge_capacity(s[:0], e[:0], s[:0], c[:0]) == 0
    assert [tgm.table_slots(k) for k in (0, 1, 2, 3, 4, 5, 1024, 1025)] == [2, 2, 4, 8, 8, 16, 2048, 4096]
    assert tgm.VOXEL_BYTES == 12 and tgm.SLOT_BYTES == 8


@pytest.mark.parametrize("neighbours", [4, 8])
def test_root_voxels_become_edges(neighbours):
    """what track_genealogy_device() does with the device's keys: roots numbered as the device numbers them (the smallest
    voxel of a part, voxels in row order) are turned into the stage oracle's edges, unselected rows lying between"""
    ds = oc.random_grid(4)
    obj = objects(ds, connectivity=6)
    ids = np.arange(obj.n_objects)[::2]
    seen = {}

    def stage(*args):
        seen["args"] = args
        seen["got"] = go.stage_for(ds, obj, neighbours)(*args)
        return seen["got"]

    mhw_track_genealogy(ds, obj, ids=ids, neighbours=neighbours, _compute=stage)
    start, end, slot, cell, _, _, vox_off, _, _ = seen["args"]
    ny, nx = ds.sshape
    flat = np.asarray(ds.cell_index)[cell]
    keys = set()
    for i in range(ids.shape[0]):
        member = np.nonzero(slot == i)[0]
        roots = {}                                                # day -> {cell label map value -> smallest voxel}
        for t in range(int(start[member].min()), int(end[member].max()) + 1):
            on = np.zeros((ny, nx), dtype=bool)
            live = [r for r in member if start[r] <= t <= end[r]]
            for r in live:
                on[flat[r] // nx, flat[r] % nx] = True
            lab = go.label_map(on, neighbours)
            root = {}
            for r in live:
                name, v = int(lab[flat[r] // nx, flat[r] % nx]), int(vox_off[r] + t - start[r])
                root[name] = min(root.get(name, v), v)
            roots[t] = (lab, root)
        for r in member:
            for t in range(int(start[r]), int(end[r])):
                i0, j0 = flat[r] // nx, flat[r] % nx
                a, b = roots[t][1][int(roots[t][0][i0, j0])], roots[t + 1][1][int(roots[t + 1][0][i0, j0])]
                keys.add((a << 32) | b)
    keys = np.array(sorted(keys, reverse=True), dtype=np.uint64)
    got = tgm.edges_of_keys(keys, start, slot, cell, vox_off)
    assert keys.shape[0] > 10
    for k, a in zip(go.EDGES, got):
        assert a.dtype == np.int32
        npt.assert_array_equal(a, seen["got"][k], err_msg=k)


def test_refusals():
    ds = oc.random_grid(1)
    obj = objects(ds)
    with pytest.raises(XmhwException, match="mhw_track_genealogy expects the EventDataset"):
        mhw_track_genealogy("x", obj)
    with pytest.raises(XmhwException, match="mhw_track_genealogy expects the ObjectDataset"):
        mhw_track_genealogy(ds, "x")
    other = objects(oc.random_grid(2))                            # a foreign obj
    with pytest.raises(XmhwException, match="one entry per table row|does not belong"):
        genealogy(ds, other)
    for bad, what in (([0, 0], "distinct"), ([obj.n_objects], r"in \[0"), ([-1], r"in \[0"), ([[0]], "1-D"), ([0.5], "integer")):
        with pytest.raises(XmhwException, match=what):
            genealogy(ds, obj, ids=bad)
    for bad in (6, 26, 0, "8", 4.5):
        with pytest.raises(XmhwException, match="neighbours should be None, 4 or 8"):
            mhw_track_genealogy(ds, obj, neighbours=bad, _compute=go.stage_for(ds, obj))


def test_stages_that_return_wrong_shapes():
    ds = oc.random_grid(1)
    obj = objects(ds)
    good = go.stage_for(ds, obj)
    L = int(obj.duration.sum())

    def broken(**change):
        def stage(*args):
            got = good(*args)
            got.update({k: f(got[k]) for k, f in change.items()})
            return got
        return stage

    with pytest.raises(XmhwException, match=f"do not fit {L} entries"):
        mhw_track_genealogy(ds, obj, _compute=broken(n_split=lambda a: a[:-1]))
    with pytest.raises(XmhwException, match="edge arrays of different lengths"):
        mhw_track_genealogy(ds, obj, _compute=broken(edge_to=lambda a: a[:-1]))
    with pytest.raises(XmhwException, match="hold no cell"):
        mhw_track_genealogy(ds, obj, _compute=broken(n_parts=lambda a: a * 0))
    with pytest.raises(XmhwException, match="outside the selection or the cells"):
        mhw_track_genealogy(ds, obj, _compute=broken(edge_from=lambda a: a + ds.n_cells))
    with pytest.raises(XmhwException, match="outside the selection or the cells"):
        mhw_track_genealogy(ds, obj, _compute=broken(edge_track=lambda a: a - 1))
    with pytest.raises(XmhwException, match="do not fit its n_links"):
        mhw_track_genealogy(ds, obj, _compute=broken(n_links=lambda a: a + 1))
    with pytest.raises(XmhwException, match="do not fit its n_links"):            # an edge on the first day of its object
        mhw_track_genealogy(ds, obj, _compute=broken(edge_pos=lambda a: a - 1000))
    with pytest.raises(XmhwException, match="do not fit its n_links"):
        mhw_track_genealogy(ds, obj, _compute=broken(**{k: (lambda a: a[:-1]) for k in go.EDGES}))


def test_two_to_the_31_voxels_are_refused_on_the_arithmetic():
    """three rows of 2**30 days: L fits, V = 3 * 2**30 does not; nothing of that size is ever made"""
    big = 1 << 30
    ds = pc.grid(1, 3, {(0, 0): [(0, big - 1)], (0, 1): [(0, big - 1)], (0, 2): [(0, big - 1)]}, T=4)
    obj = objects(ds)
    assert obj.n_objects == 1 and int(obj.duration[0]) == big
    called = []
    with pytest.raises(XmhwException, match=r"2\*\*31 and more.*ids="):
        mhw_track_genealogy(ds, obj, _compute=lambda *a: called.append(1))
    assert not called


def test_empty_table():
    ds = oc.dataset((2, 3), np.ones(6, bool), [[] for _ in range(6)], T=10)
    called = []
    tg = mhw_track_genealogy(ds, objects(ds), _compute=lambda *a: called.append(1))
    assert tg.n_selected == 0 and tg.offsets.tolist() == [0] and tg.edge_offsets.tolist() == [0] and not called
    assert tg.n_parts.shape == tg.edge_track.shape == tg.n_edges.shape == (0,)


def test_to_xarray():
    xr = pytest.importorskip("xarray")
    ds = oc.random_grid(4)
    obj = objects(ds)
    tg = genealogy(ds, obj)
    x = tg.to_xarray()
    assert isinstance(x, xr.Dataset) and x.sizes["obs"] == x["offsets"].values[-1] and x.attrs["neighbours"] == 4
    assert x.sizes["edge"] == x["edge_offsets"].values[-1] == tg.edge_track.shape[0]
