"""mhw_track_genealogy() on the device (csrc/kernels_genealogy.hip): the stage against the flood-fill stage oracle and
the public function against the dense oracle (tests/track_genealogy_oracle.py), every integer and every edge equal.

The pair kernel runs one lane per table row in workgroups of 256 rows and deduplicates (part, part) pairs in a hash set
of 2 slots and more: the random grids work tables of a few slots, where probing runs past the table's end and wraps;
the full grid sends 16 workgroups to one key; the checkerboard and the land grids put hundreds to thousands of
distinct keys in, from one to more than ten workgroups of rows, next to rows of other and of unselected objects."""
import numpy as np
import numpy.testing as npt
import pytest

import objects_cases as oc
import track_genealogy_cases as gc
import track_genealogy_oracle as go
import track_parts_cases as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    from xmhw_amd._lib import hip, require_gpu
    require_gpu()
    from xmhw_amd import track_genealogy
    h = hip()
    assert h.GENEALOGY_VOXEL_BYTES == track_genealogy.VOXEL_BYTES == 12
    assert h.GENEALOGY_SLOT_BYTES == track_genealogy.SLOT_BYTES == 8
    assert h.GENEALOGY_FIELDS == len(track_genealogy.COUNT_FIELDS) == 6
    return track_genealogy


def identities(tg, tp, connected):
    """the identities of the issue, with == and <="""
    for k in ("ids", "offsets", "time_start", "time_end", "duration", "pos"):
        npt.assert_array_equal(getattr(tg, k), getattr(tp, k), err_msg=k)
    npt.assert_array_equal(tg.n_parts, tp.n_parts)
    first, last = tg.offsets[:-1], tg.offsets[1:] - 1
    assert (tg.n_links[first] == 0).all() and (tg.n_born[first] == tg.n_parts[first]).all()
    assert (tg.n_ended[last] == tg.n_parts[last]).all()
    assert (tg.n_links >= tg.n_parts - tg.n_born).all()
    L = int(tg.offsets[-1])
    entry = tg.offsets[tg.edge_track] + (tg.edge_pos - tg.time_start[tg.edge_track])
    npt.assert_array_equal(np.bincount(entry, minlength=L), tg.n_links)
    nodes, outdeg = np.unique(np.stack([entry - 1, tg.edge_from], axis=1), axis=0, return_counts=True)
    npt.assert_array_equal(np.bincount(nodes[outdeg >= 2, 0], minlength=L), tg.n_split)
    npt.assert_array_equal(tg.n_parts - np.bincount(nodes[:, 0], minlength=L), tg.n_ended)
    if connected:
        assert (tg.n_edges >= tg.n_nodes - 1).all()


def run(gpu, ds, obj, ids=None, neighbours=None, dense=True):
    """mhw_track_genealogy() with its device stage checked against the stage oracle on the way, then against the dense
    oracle, the public route itself and the identities (n_parts against mhw_track_parts() on the device)"""
    import xmhw_amd
    oracle = go.stage_for(ds, obj, neighbours)

    def stage(*args):
        got, want = gpu.track_genealogy_device(*args), oracle(*args)
        for k in gpu.STAGE_FIELDS:
            assert got[k].dtype == want[k].dtype == np.int32, k
            npt.assert_array_equal(got[k], want[k], err_msg=k)
        return got

    tg = xmhw_amd.mhw_track_genealogy(ds, obj, ids=ids, neighbours=neighbours, _compute=stage)
    if dense:
        go.same_as_dense(tg, go.genealogy_dense(ds, obj, ids, neighbours))
    plain = xmhw_amd.mhw_track_genealogy(ds, obj, ids=ids, neighbours=neighbours)                   # the public route itself
    for k in gpu.STAGE_FIELDS + ("edge_offsets",) + go.PER_OBJECT:
        npt.assert_array_equal(getattr(plain, k), getattr(tg, k), err_msg=k)
    identities(tg, xmhw_amd.mhw_track_parts(ds, obj, ids=ids, neighbours=neighbours), connected=obj.connectivity == 6)
    return tg


@pytest.mark.parametrize("seed", range(30))
def test_random_grids(gpu, seed):
    import xmhw_amd
    ds = oc.random_grid(seed, T=40)
    for connectivity in (6, 26):
        for periodic in (None, "lon"):
            obj = xmhw_amd.mhw_objects(ds, connectivity=connectivity, periodic=periodic)
            run(gpu, ds, obj)
            if connectivity == 6:
                for neighbours in (4, 8):
                    run(gpu, ds, obj, neighbours=neighbours)


@pytest.mark.parametrize("seed", [0, 11, 23])
def test_one_object_at_a_time_in_tables_of_a_few_slots(gpu, seed):
    """every object selected alone: hash sets of 2, 4, 8 ... slots, half full, where linear probing wraps"""
    import xmhw_amd
    ds = oc.random_grid(seed, T=40)
    obj = xmhw_amd.mhw_objects(ds, connectivity=6)
    full = run(gpu, ds, obj)
    slots = set()
    for o in range(obj.n_objects):
        tg = run(gpu, ds, obj, ids=[o], dense=False)
        slots.add(gpu.table_slots(int(obj.cell_days[o] - obj.n_events[o])))
        for k, v in full.series(o).items():
            npt.assert_array_equal(tg.series(0)[k], v, err_msg=k)
        for k in ("edge_pos", "edge_from", "edge_to"):
            npt.assert_array_equal(tg.edges(0)[k], full.edges(o)[k], err_msg=k)
    assert min(slots) <= 8 and len(slots) >= 3


@pytest.mark.parametrize("key", list(oc.GOLDEN_COUNTS))
def test_golden_tables(gpu, key):
    import xmhw_amd
    connectivity, periodic = key
    ds = oc.golden_dataset()
    obj = xmhw_amd.mhw_objects(ds, connectivity=connectivity, periodic=periodic)
    assert obj.n_objects == oc.GOLDEN_COUNTS[key][0]
    tg = run(gpu, ds, obj)
    assert tg.n_voxels == int(obj.cell_days.sum())


@pytest.mark.parametrize("case", gc.hand_drawn(), ids=lambda c: c[0])
def test_hand_drawn(gpu, case):
    import xmhw_amd
    name, ds, want = case
    obj = xmhw_amd.mhw_objects(ds, connectivity=6)
    assert obj.n_objects == 1
    gc.check_hand_drawn(run(gpu, ds, obj), want)


@pytest.mark.parametrize("days", [2, 6])
def test_dedup_under_contention(gpu, days):
    """a 64 x 64 full grid over the same days: 4,096 pairs a day step from 16 workgroups of rows, ONE distinct edge"""
    import xmhw_amd
    ds = gc.full_grid(64, days)
    obj = xmhw_amd.mhw_objects(ds)
    assert obj.n_objects == 1 and obj.n_events[0] == 4096
    tg = run(gpu, ds, obj)
    assert tg.n_parts.tolist() == [1] * days and tg.n_links.tolist() == [0] + [1] * (days - 1)
    assert tg.n_born.tolist() == [1] + [0] * (days - 1) and tg.n_ended.tolist() == [0] * (days - 1) + [1]
    assert tg.n_merged.tolist() == tg.n_split.tolist() == [0] * days
    assert tg.edge_pos.tolist() == list(range(2, days + 1)) and tg.edge_from.tolist() == tg.edge_to.tolist() == [0] * (days - 1)


def test_many_distinct_keys_on_the_checkerboard(gpu):
    import xmhw_amd
    ds = pc.checkerboard(16, 5)
    obj = xmhw_amd.mhw_objects(ds, connectivity=26)
    assert obj.n_objects == 1
    four = run(gpu, ds, obj, neighbours=4)
    assert four.n_parts.tolist() == [128] * 5 and four.n_links.tolist() == [0] + [128] * 4
    assert four.n_split.tolist() == four.n_merged.tolist() == [0] * 5 and four.n_edges.tolist() == [512]
    assert four.n_born.tolist() == [128, 0, 0, 0, 0] and four.n_ended.tolist() == [0, 0, 0, 0, 128]
    npt.assert_array_equal(four.edge_from, four.edge_to)
    eight = run(gpu, ds, obj)
    assert eight.neighbours == 8 and eight.n_parts.tolist() == [1] * 5 and eight.n_links.tolist() == [0, 1, 1, 1, 1]
    assert eight.n_edges.tolist() == [4]


@pytest.mark.parametrize("rows", [None, (2, 3)], ids=["one-event", "2-3-rows"])
def test_land_grid_of_ten_workgroups(gpu, rows):
    import xmhw_amd
    ds = pc.land_grid(seed=4, rows=rows)
    assert 2300 < ds.n_cells < 2620
    # objects under 8 neighbours (at 40 % land nearly every ocean cell is in one of them), parts under 4: many parts a day
    obj = xmhw_amd.mhw_objects(ds, connectivity=26)
    big = int(np.argmax(obj.n_events))
    assert obj.n_events[big] > (2000 if rows is None else 4000)   # ten workgroups of 256 rows and more, one object
    tg = run(gpu, ds, obj, neighbours=4)
    if rows is None:                                              # ten days of the same footprint: every part goes on
        assert tg.n_splits.sum() == tg.n_merges.sum() == 0 and tg.n_parts[tg.offsets[:-1]].sum() > 50
        assert tg.edge_track.shape[0] == 9 * tg.n_parts[tg.offsets[:-1]].sum()
        run(gpu, ds, obj)                                          # under 8 neighbours
    else:
        assert tg.n_splits[big] > 10 and tg.n_merges[big] > 10    # the footprint changes from day to day
        assert tg.edge_track.shape[0] > 4000
        ids = np.argsort(obj.n_events)[::-1][:5][::-1]            # the five largest, unselected neighbours among them
        part = run(gpu, ds, obj, ids=ids, neighbours=4)
        for i, o in enumerate(ids):
            for k, v in tg.series(int(o)).items():
                npt.assert_array_equal(part.series(i)[k], v, err_msg=k)


def stage_args(ds, obj):
    """what mhw_track_genealogy() hands to its stage"""
    import xmhw_amd
    seen = {}
    xmhw_amd.mhw_track_genealogy(ds, obj, _compute=lambda *a: seen.setdefault("args", a) and go.stage_for(ds, obj)(*a))
    return [np.array(a) for a in seen["args"]]


def test_touching_rows_of_one_cell(gpu):
    """stage level only (detect() joins or separates such rows): two rows of one cell, the second starting the day after
    the first ends, link the two days where their slots agree and do not where they differ"""
    from xmhw_amd.objects import neighbour_table
    cell_index, sshape = np.arange(2), (1, 2)                     # two ocean cells, every row in the first
    start, end, cell = np.array([1, 4], np.int32), np.array([3, 6], np.int32), np.array([0, 0], np.int32)
    row_offsets, vox_off = np.array([0, 2, 2], np.int64), np.array([0, 3, 6], np.int64)
    nbr = neighbour_table(cell_index, sshape, 6, None)
    oracle = go.stage_oracle(cell_index, sshape, 4)
    # one object over the days 1..6: the only link from day 3 to day 4 is the one across the two rows
    args = (start, end, np.array([0, 0], np.int32), cell, row_offsets, nbr, vox_off, np.array([1], np.int32), np.array([0, 6], np.int64))
    assert gpu.edge_capacity(start, end, args[2], cell) == 2 + 2 + 1
    got, want = gpu.track_genealogy_device(*args), oracle(*args)
    for k in gpu.STAGE_FIELDS:
        npt.assert_array_equal(got[k], want[k], err_msg=k)
    assert got["n_parts"].tolist() == [1] * 6 and got["n_links"].tolist() == [0, 1, 1, 1, 1, 1]
    assert got["n_born"].tolist() == [1, 0, 0, 0, 0, 0] and got["n_ended"].tolist() == [0, 0, 0, 0, 0, 1]
    assert got["edge_pos"].tolist() == [2, 3, 4, 5, 6] and got["edge_track"].tolist() == [0] * 5
    # the same two rows in two objects, days 1..3 and 4..6: no key across them
    args = (start, end, np.array([0, 1], np.int32), cell, row_offsets, nbr, vox_off, np.array([1, 4], np.int32),
            np.array([0, 3, 6], np.int64))
    assert gpu.edge_capacity(start, end, args[2], cell) == 2 + 2
    got, want = gpu.track_genealogy_device(*args), oracle(*args)
    for k in gpu.STAGE_FIELDS:
        npt.assert_array_equal(got[k], want[k], err_msg=k)
    assert got["n_parts"].tolist() == [1] * 6 and got["n_links"].tolist() == [0, 1, 1, 0, 1, 1]
    assert got["n_born"].tolist() == [1, 0, 0, 1, 0, 0] and got["n_ended"].tolist() == [0, 0, 1, 0, 0, 1]
    assert got["edge_pos"].tolist() == [2, 3, 5, 6] and got["edge_track"].tolist() == [0, 0, 1, 1]


def test_unselected_neighbours_and_reversed_ids(gpu):
    import xmhw_amd
    ds = oc.random_grid(7, T=40)
    obj = xmhw_amd.mhw_objects(ds, connectivity=6)
    assert obj.n_objects >= 6
    ids = np.arange(obj.n_objects)[::-1][::2]                     # every other object, last first: the rest lie between them
    tg = run(gpu, ds, obj, ids=ids, neighbours=8)
    full = run(gpu, ds, obj, neighbours=8)
    for i, o in enumerate(ids):
        for k in gpu.COUNT_FIELDS:
            npt.assert_array_equal(tg.series(i)[k], full.series(int(o))[k], err_msg=k)
        for k in ("edge_pos", "edge_from", "edge_to"):
            npt.assert_array_equal(tg.edges(i)[k], full.edges(int(o))[k], err_msg=k)


def test_twice_the_same(gpu):
    import xmhw_amd
    ds = pc.land_grid(seed=9, rows=(2, 3))
    obj = xmhw_amd.mhw_objects(ds, connectivity=26, periodic="lon")
    a = xmhw_amd.mhw_track_genealogy(ds, obj, neighbours=4)
    b = xmhw_amd.mhw_track_genealogy(ds, obj, neighbours=4)
    assert a.edge_track.shape[0] > 4000
    for k in gpu.STAGE_FIELDS + ("edge_offsets", "offsets", "pos") + go.PER_OBJECT:
        npt.assert_array_equal(getattr(a, k), getattr(b, k), err_msg=k)


def test_rows_that_do_not_fit_are_counted_not_written(gpu):
    """a selected row whose days are not those of its voxel numbers is left out of every kernel and reported"""
    import xmhw_amd
    ds = oc.random_grid(3, T=40)
    obj = xmhw_amd.mhw_objects(ds)
    args = stage_args(ds, obj)
    row = int(np.argmax(args[1] - args[0]))
    args[0][row] -= 10_000                                         # starts long before its object
    with pytest.raises(gpu.XmhwException, match="do not lie within"):
        gpu.track_genealogy_device(*args)


def test_a_capacity_too_small_is_reported_not_overrun(gpu):
    """the C ABI with edge_capacity = 1 on a table that forms many distinct keys: the 2-slot set fills, the overflow flag
    is raised, and nothing is written beyond the one edge of the buffer"""
    import xmhw_amd.device as dev
    from xmhw_amd._lib import hip
    ds = pc.checkerboard(16, 5)
    import xmhw_amd
    obj = xmhw_amd.mhw_objects(ds, connectivity=26)
    start, end, slot, cell, row_offsets, nbr, vox_off, time_start, offsets = stage_args(ds, obj)
    nbr = np.ascontiguousarray(nbr[:, :4])                        # 4 neighbours: 128 parts a day, 512 distinct keys
    h = hip()
    n, C, V, L = start.shape[0], row_offsets.shape[0] - 1, int(vox_off[-1]), int(offsets[-1])
    guard = np.full(8, 0x5555555555555555, dtype=np.uint64)
    with dev.DeviceScope() as s:
        d = [s.upload(np.ascontiguousarray(a)) for a in (start, end, slot, cell, row_offsets, nbr, vox_off, time_start, offsets)]
        d_counts, d_edges = s.alloc(4 * 6 * L), s.upload(guard)
        d_ne, d_bad, d_over = s.alloc(8), s.alloc(4), s.alloc(4)
        h.object_genealogy(d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, n, d[4].ptr, C, d[5].ptr, 4, d[6].ptr, V, d[7].ptr, d[8].ptr, 1, L,
                           d_counts.ptr, d_edges.ptr, 1, d_ne.ptr, d_bad.ptr, d_over.ptr)
        h.stream_sync(0)
        edges = d_edges.to_array((8,), np.uint64)
        assert int(d_over.to_array((1,), np.int32)[0]) != 0 and int(d_bad.to_array((1,), np.int32)[0]) == 0
        assert int(d_ne.to_array((1,), np.int64)[0]) == 2          # the two slots of the set
    npt.assert_array_equal(edges[1:], guard[1:])
    assert edges[0] != guard[0]


def test_refused_without_a_launch(gpu):
    from xmhw_amd._lib import hip
    h = hip()
    big = 1 << 31
    base = dict(n=1, C=1, V=1, n_slots=1, L=1, cap=1)

    def call(a):
        h.object_genealogy(0, 0, 0, 0, a["n"], 0, a["C"], 0, 4, 0, a["V"], 0, 0, a["n_slots"], a["L"], 0, 0, a["cap"], 0, 0, 0)

    for k in base:                                                # XMHW_ERR_UNSUPPORTED
        with pytest.raises(h.HipError, match=r"\(code 3\)"):
            call(dict(base, **{k: big}))
    for k in base:
        with pytest.raises(h.InvalidArgument):
            call(dict(base, **{k: -1}))
    with pytest.raises(h.InvalidArgument):                        # null buffers
        call(base)


def test_no_events_touches_nothing(gpu):
    import xmhw_amd
    ds = oc.dataset((2, 3), np.ones(6, bool), [[] for _ in range(6)], T=10)
    tg = xmhw_amd.mhw_track_genealogy(ds, xmhw_amd.mhw_objects(ds))
    assert tg.n_selected == 0 and tg.n_parts.shape == (0,) and tg.edge_track.shape == (0,)
