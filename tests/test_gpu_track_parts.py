"""mhw_track_parts() on the device (csrc/kernels_parts.hip): the stage against the flood-fill stage oracle and the public
function against the dense oracle (tests/track_parts_oracle.py), every integer equal.

The kernels run one lane per table row in workgroups of 256 rows and one lane per voxel in the init and flatten
kernels; the cases put one, a few and ten workgroups of rows to work, parts of 1 to 4,096 cells, chains of several
hundred unions, and rows of other objects and of unselected objects next to the ones that are united."""
import numpy as np
import numpy.testing as npt
import pytest

import objects_cases as oc
import track_parts_cases as pc
import track_parts_oracle as po

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    from xmhw_amd._lib import hip, require_gpu
    require_gpu()
    from xmhw_amd import track_parts
    assert hip().PARTS_VOXEL_BYTES == track_parts.VOXEL_BYTES == 16
    return track_parts


def run(gpu, ds, obj, ids=None, weights=None, neighbours=None, tracks=True):
    """mhw_track_parts() with its device stage checked against the stage oracle on the way, then against the dense oracle
    and, with ``tracks``, the identities against mhw_tracks()"""
    import xmhw_amd
    oracle = po.stage_for(ds, obj, neighbours)

    def stage(*args):
        got, want = gpu.track_parts_device(*args), oracle(*args)
        for k in gpu.STAGE_FIELDS:
            assert got[k].dtype == want[k].dtype, k
            npt.assert_array_equal(got[k], want[k], err_msg=k)
        return got

    tp = xmhw_amd.mhw_track_parts(ds, obj, ids=ids, weights=weights, neighbours=neighbours, _compute=stage)
    po.same_as_dense(tp, po.parts_dense(ds, obj, ids, weights, neighbours))
    plain = xmhw_amd.mhw_track_parts(ds, obj, ids=ids, weights=weights, neighbours=neighbours)       # the public route itself
    for k in gpu.STAGE_FIELDS:
        npt.assert_array_equal(getattr(plain, k), getattr(tp, k), err_msg=k)
    if tracks:
        identities(tp, xmhw_amd.mhw_tracks(ds, obj, ids=ids, weights=weights))
    return tp


def identities(tp, tr):
    for k in ("ids", "offsets", "time_start", "pos"):
        npt.assert_array_equal(getattr(tp, k), getattr(tr, k), err_msg=k)
    assert (tp.n_parts >= 1).all()
    assert (tp.n_parts.astype(np.int64) + tp.cells_largest - 1 <= tr.n_cells).all()
    one = tp.n_parts == 1
    npt.assert_array_equal(tp.cells_largest[one], tr.n_cells[one])
    npt.assert_array_equal(tp.area_largest_q[one], tr.area_q[one])


@pytest.mark.parametrize("seed", range(30))
def test_random_grids(gpu, seed):
    import xmhw_amd
    ds = oc.random_grid(seed, T=40)
    for connectivity in (6, 26):
        for periodic in (None, "lon"):
            weights = "coslat" if seed % 2 else None
            obj = xmhw_amd.mhw_objects(ds, connectivity=connectivity, periodic=periodic, weights=weights)
            run(gpu, ds, obj, weights=weights)
            if connectivity == 6:                                 # parts under both neighbourhoods on objects of 6: the
                for neighbours in (4, 8):                         # equal-slot rule keeps a diagonal cell of another object out
                    run(gpu, ds, obj, weights=weights, neighbours=neighbours)


@pytest.mark.parametrize("key", list(oc.GOLDEN_COUNTS))
def test_golden_tables(gpu, key):
    import xmhw_amd
    connectivity, periodic = key
    ds = oc.golden_dataset()
    obj = xmhw_amd.mhw_objects(ds, connectivity=connectivity, periodic=periodic, weights="coslat")
    assert obj.n_objects == oc.GOLDEN_COUNTS[key][0]
    tp = run(gpu, ds, obj, weights="coslat")
    assert tp.n_voxels == int(obj.cell_days.sum())


@pytest.mark.parametrize("case", pc.hand_drawn(), ids=lambda c: c[0])
def test_hand_drawn(gpu, case):
    import xmhw_amd
    name, ds, kw, neighbours, n_parts, cells_largest = case
    obj = xmhw_amd.mhw_objects(ds, **kw)
    assert obj.n_objects == 1
    tp = run(gpu, ds, obj, neighbours=neighbours)
    assert tp.n_parts.tolist() == n_parts and tp.cells_largest.tolist() == cells_largest
    assert tp.days_split.tolist() == [sum(1 for v in n_parts if v > 1)]


def test_checkerboard(gpu):
    import xmhw_amd
    ds = pc.checkerboard(16, 5)
    obj = xmhw_amd.mhw_objects(ds, connectivity=26)
    assert obj.n_objects == 1
    four = run(gpu, ds, obj, neighbours=4)
    assert four.n_parts.tolist() == [128] * 5 and four.cells_largest.tolist() == [1] * 5 and four.days_split.tolist() == [5]
    eight = run(gpu, ds, obj)
    assert eight.neighbours == 8 and eight.n_parts.tolist() == [1] * 5 and eight.cells_largest.tolist() == [128] * 5


def test_spiral_is_one_part_through_a_long_chain(gpu):
    import xmhw_amd
    ds, cells = pc.spiral(33, 3)
    assert cells > 500
    obj = xmhw_amd.mhw_objects(ds, connectivity=6)
    assert obj.n_objects == 1
    tp = run(gpu, ds, obj)
    assert tp.n_parts.tolist() == [1] * 3 and tp.cells_largest.tolist() == [cells] * 3


@pytest.mark.parametrize("rows", [None, (2, 3)], ids=["one-event", "2-3-rows"])
def test_land_grid_of_ten_workgroups(gpu, rows):
    import xmhw_amd
    ds = pc.land_grid(seed=4, rows=rows)
    assert 2300 < ds.n_cells < 2620
    rng = np.random.default_rng(1)
    w = rng.uniform(0.0, 3.0, ds.sshape)
    # objects under 8 neighbours (at 40 % land nearly every ocean cell is in one of them), parts under 4: many parts a day
    obj = xmhw_amd.mhw_objects(ds, connectivity=26, weights=w)
    tp = run(gpu, ds, obj, weights=w, neighbours=4)
    big = int(np.argmax(obj.n_events))
    s = tp.series(big)
    assert obj.n_events[big] > (2000 if rows is None else 4000)   # ten workgroups of 256 rows and more, one object
    if rows is None:
        assert len(set(s["n_parts"].tolist())) == 1 and s["n_parts"][0] > 20 and s["cells_largest"][0] > 100
        whole = run(gpu, ds, obj, weights=w, tracks=False).series(big)             # under 8 neighbours: one part
        assert whole["n_parts"].tolist() == [1] * 10 and whole["cells_largest"][0] == obj.n_cells[big]
    else:
        assert len(set(s["n_parts"].tolist())) > 3                # the parts change from day to day
    assert tp.n_voxels > 20_000


def test_two_rows_of_one_object_in_one_cell(gpu):
    import xmhw_amd
    ds = pc.grid(1, 5, {(0, 2): [(0, 3), (8, 11)], (0, 1): [(2, 9)], (0, 3): [(2, 9)]}, T=14)
    obj = xmhw_amd.mhw_objects(ds)
    assert obj.n_objects == 1
    tp = run(gpu, ds, obj)
    assert tp.n_parts.tolist() == [1, 1, 1, 1, 2, 2, 2, 2, 1, 1, 1, 1]
    assert tp.cells_largest.tolist() == [1, 1, 3, 3, 1, 1, 1, 1, 3, 3, 1, 1]


def test_unselected_neighbours_and_reversed_ids(gpu):
    import xmhw_amd
    ds = oc.random_grid(7, T=40)
    obj = xmhw_amd.mhw_objects(ds, connectivity=6)
    assert obj.n_objects >= 6
    ids = np.arange(obj.n_objects)[::-1][::2]                     # every other object, last first: the rest lie between them
    tp = run(gpu, ds, obj, ids=ids, neighbours=8)
    full = run(gpu, ds, obj, neighbours=8)
    for i, o in enumerate(ids):
        for k in ("n_parts", "cells_largest", "area_largest_q"):
            npt.assert_array_equal(tp.series(i)[k], full.series(int(o))[k], err_msg=k)


def test_twice_the_same(gpu):
    import xmhw_amd
    ds = pc.land_grid(seed=9, rows=(2, 3))
    obj = xmhw_amd.mhw_objects(ds, connectivity=26, periodic="lon")
    a = xmhw_amd.mhw_track_parts(ds, obj, weights="coslat")
    b = xmhw_amd.mhw_track_parts(ds, obj, weights="coslat")
    for k in gpu.STAGE_FIELDS:
        npt.assert_array_equal(getattr(a, k), getattr(b, k), err_msg=k)


def test_extreme_weights(gpu):
    """weight_bits = 31 and one part of 4,096 cells: area_largest_q = 4096 * 2**31 = 2**43"""
    import xmhw_amd
    ds = pc.grid(64, 64, {(i, j): [(1, 2)] for i in range(64) for j in range(64)}, T=4)
    obj = xmhw_amd.mhw_objects(ds)
    assert obj.n_objects == 1 and obj.weight_bits == 31
    tp = run(gpu, ds, obj)
    assert tp.n_parts.tolist() == [1, 1] and tp.cells_largest.tolist() == [4096, 4096]
    assert tp.area_largest_q.tolist() == [4096 << 31] * 2


def test_rows_that_do_not_fit_are_counted_not_written(gpu):
    """a selected row whose days are not those of its voxel numbers is left out of every kernel and reported"""
    import xmhw_amd
    ds = oc.random_grid(3, T=40)
    obj = xmhw_amd.mhw_objects(ds)
    seen = {}

    def stage(*args):
        seen["args"] = args
        return gpu.track_parts_device(*args)

    xmhw_amd.mhw_track_parts(ds, obj, _compute=stage)
    args = [np.array(a) for a in seen["args"]]
    row = int(np.argmax(args[1] - args[0]))
    args[0][row] -= 10_000                                         # starts long before its object
    with pytest.raises(gpu.XmhwException, match="do not lie within"):
        gpu.track_parts_device(*args)


def test_refused_without_a_launch(gpu):
    from xmhw_amd._lib import hip
    h = hip()
    big = 1 << 31
    base = dict(n=1, C=1, V=1, n_slots=1, L=1)
    for kw in (dict(n=big), dict(C=big), dict(V=big), dict(n_slots=big), dict(L=big)):      # XMHW_ERR_UNSUPPORTED
        a = dict(base, **kw)
        with pytest.raises(h.HipError, match=r"\(code 3\)"):
            h.object_parts(0, 0, 0, 0, a["n"], 0, a["C"], 0, 4, 0, 0, a["V"], 0, 0, a["n_slots"], a["L"], 0, 0, 0, 0)
    for kw in (dict(n=-1), dict(C=-1), dict(V=-1), dict(n_slots=-1), dict(L=-1)):
        a = dict(base, **kw)
        with pytest.raises(h.InvalidArgument):
            h.object_parts(0, 0, 0, 0, a["n"], 0, a["C"], 0, 4, 0, 0, a["V"], 0, 0, a["n_slots"], a["L"], 0, 0, 0, 0)
    with pytest.raises(h.InvalidArgument):                        # null buffers
        h.object_parts(0, 0, 0, 0, 1, 0, 1, 0, 4, 0, 0, 1, 0, 0, 1, 1, 0, 0, 0, 0)


def test_no_events_touches_nothing(gpu):
    import xmhw_amd
    ds = oc.dataset((2, 3), np.ones(6, bool), [[] for _ in range(6)], T=10)
    tp = xmhw_amd.mhw_track_parts(ds, xmhw_amd.mhw_objects(ds))
    assert tp.n_selected == 0 and tp.n_parts.shape == (0,)
