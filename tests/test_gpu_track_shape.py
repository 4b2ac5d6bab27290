"""mhw_track_shape() on the device (csrc/kernels_shape.hip): the stage against the shifted-map stage oracle and the public
function against the dense oracle (tests/track_shape_oracle.py), every integer equal.

The kernel runs one lane per table row in workgroups of 256 rows; the cases put one, a few and sixteen workgroups to
work, rows whose neighbour cells hold rows of the same object with gaps, rows of other objects and of unselected
objects, land, the edge of the grid, and both wraps (a dim of length 1 and of length 2 among them)."""
import numpy as np
import numpy.testing as npt
import pytest

import object_chain_raw as ocr
import objects_cases as oc
import track_parts_cases as pc
import track_shape_cases as sc
import track_shape_oracle as so
from object_chain_raw import raw_shape as raw_stage

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    from xmhw_amd._lib import hip, require_gpu
    require_gpu()
    from xmhw_amd import track_shape
    h = hip()
    assert h.SHAPE_CLASSES == len(track_shape.CLASSES) == 3
    assert (h.SHAPE_FACE_COAST, h.SHAPE_FACE_BORDER, h.SHAPE_FACE_FOLDED) == (track_shape.FACE_COAST, track_shape.FACE_BORDER,
                                                                               track_shape.FACE_FOLDED)
    return track_shape


def identities(sh, tr, periodic):
    for k in ("ids", "offsets", "time_start", "pos"):
        npt.assert_array_equal(getattr(sh, k), getattr(tr, k), err_msg=k)
    exposed = sh.edges_exposed.astype(np.int64)
    assert (sh.cells_edge <= tr.n_cells).all()
    assert (sh.cells_edge <= exposed).all() and (exposed <= 4 * sh.cells_edge.astype(np.int64)).all()
    assert (exposed <= 4 * tr.n_cells.astype(np.int64)).all()
    assert (exposed >= (4 if periodic is None else 2)).all()
    if sh.attrs["lengths"] == "none":
        for c in ("open", "coast", "border"):
            npt.assert_array_equal(getattr(sh, f"perimeter_{c}_q"), getattr(sh, f"edges_{c}").astype(np.int64) << sh.length_bits)


def run(gpu, ds, obj, ids=None, lengths=None, tracks=True):
    """mhw_track_shape() with its device stage checked against the stage oracle on the way, then against the dense oracle
    and, with ``tracks``, the identities against a real mhw_tracks()"""
    import xmhw_amd
    oracle = so.stage_for(ds, obj)

    def stage(*args):
        got, want = gpu.track_shape_device(*args), oracle(*args)
        for k in gpu.STAGE_FIELDS:
            assert got[k].dtype == want[k].dtype, k
            npt.assert_array_equal(got[k], want[k], err_msg=k)
        return got

    sh = xmhw_amd.mhw_track_shape(ds, obj, ids=ids, lengths=lengths, _compute=stage)
    so.same_as_dense(sh, so.shape_dense(ds, obj, ids, lengths))
    plain = xmhw_amd.mhw_track_shape(ds, obj, ids=ids, lengths=lengths)             # the public route itself
    for k in gpu.STAGE_FIELDS:
        npt.assert_array_equal(getattr(plain, k), getattr(sh, k), err_msg=k)
    if tracks:
        identities(sh, xmhw_amd.mhw_tracks(ds, obj, ids=ids), obj.periodic)
    return sh


def random_lengths(ds, seed):
    rng = np.random.default_rng(1000 + seed)
    ln = rng.uniform(0.0, 5.0, tuple(ds.sshape) + (4,))
    ln[rng.random(ln.shape) < 0.1] = 0.0
    return ln


@pytest.mark.parametrize("seed", range(30))
def test_random_grids(gpu, seed):
    import xmhw_amd
    ds = oc.random_grid(seed, T=40)
    for connectivity in (6, 26):
        for periodic in (None, "lon"):
            obj = xmhw_amd.mhw_objects(ds, connectivity=connectivity, periodic=periodic)
            for lengths in (None, "sphere", random_lengths(ds, seed)):
                run(gpu, ds, obj, lengths=lengths, tracks=lengths is None)


@pytest.mark.parametrize("seed", [3, 7, 12])
def test_every_object_alone(gpu, seed):
    import xmhw_amd
    ds = oc.random_grid(seed, T=40)
    obj = xmhw_amd.mhw_objects(ds, connectivity=6, periodic="lon")
    full = run(gpu, ds, obj, lengths="sphere", tracks=False)
    oracle = so.stage_for(ds, obj)
    for o in range(obj.n_objects):                                # the others lie around it, unselected

        def stage(*args):
            got, want = gpu.track_shape_device(*args), oracle(*args)
            for k in gpu.STAGE_FIELDS:
                npt.assert_array_equal(got[k], want[k], err_msg=k)
            return got

        alone = xmhw_amd.mhw_track_shape(ds, obj, ids=[o], lengths="sphere", _compute=stage)
        for k in gpu.STAGE_FIELDS:
            npt.assert_array_equal(alone.series(0)[k], full.series(o)[k], err_msg=k)


@pytest.mark.parametrize("case", sc.hand_drawn(), ids=lambda c: c["name"])
def test_hand_drawn(gpu, case):
    import xmhw_amd
    ds = case["ds"]
    obj = xmhw_amd.mhw_objects(ds, **case["kw"])
    assert obj.n_objects == 1
    sh = run(gpu, ds, obj)
    for k in ("edges_open", "edges_coast", "edges_border", "cells_edge"):
        assert getattr(sh, k).tolist() == case[k], k


def test_wrap_of_two_counts_each_face_with_its_own_length(gpu):
    import xmhw_amd
    ds = sc.wrap_of_two()
    ln = np.zeros((1, 2, 4))
    ln[0, 0] = [1.0, 2.0, 4.0, 8.0]
    ln[0, 1] = [16.0, 32.0, 64.0, 128.0]
    sh = run(gpu, ds, xmhw_amd.mhw_objects(ds, periodic="lon"), lengths=ln)
    assert sh.perimeter_open.tolist() == [12.0, 12.0, 0.0, 0.0] and sh.perimeter_border.tolist() == [3.0, 3.0, 51.0, 51.0]


@pytest.mark.parametrize("days", [2, 6])
@pytest.mark.parametrize("periodic", [None, "lon"])
def test_full_grid_of_sixteen_workgroups(gpu, days, periodic):
    """4,096 rows, one object: only the edge of the grid is exposed -- 4 * 64 faces, or the 2 * 64 of the dim that does not
    wrap"""
    import xmhw_amd
    ds = sc.full_grid(64, days)
    obj = xmhw_amd.mhw_objects(ds, periodic=periodic)
    assert obj.n_objects == 1 and ds.n_events == 4096
    sh = run(gpu, ds, obj, lengths="sphere")
    border, cells = (256, 252) if periodic is None else (128, 128)
    assert sh.edges_border.tolist() == [border] * days and sh.cells_edge.tolist() == [cells] * days
    assert not sh.edges_open.any() and not sh.edges_coast.any()


def test_checkerboard_shares_no_face(gpu):
    import xmhw_amd
    ds = pc.checkerboard(16, 5)
    obj = xmhw_amd.mhw_objects(ds, connectivity=26)
    assert obj.n_objects == 1
    sh = run(gpu, ds, obj)
    # 128 cells, 512 faces; on each side of the board 8 black squares
    assert sh.edges_open.tolist() == [480] * 5 and sh.edges_border.tolist() == [32] * 5 and sh.cells_edge.tolist() == [128] * 5


@pytest.fixture(scope="module")
def land(gpu):
    """the 64 x 64 grid with 40 % land and 2-3 rows per cell, its objects under 8 neighbours, random lengths"""
    import xmhw_amd
    ds = pc.land_grid(seed=4, rows=(2, 3))
    assert 2300 < ds.n_cells < 2620
    obj = xmhw_amd.mhw_objects(ds, connectivity=26)
    return ds, obj, random_lengths(ds, 4)


def test_land_grid_every_object(gpu, land):
    ds, obj, ln = land
    sh = run(gpu, ds, obj, lengths=ln)
    big = int(np.argmax(obj.n_events))
    assert obj.n_events[big] > 4000                               # sixteen workgroups of 256 rows and more, one object
    s = sh.series(big)
    assert s["edges_coast"].max() > 100 and s["edges_open"].max() > 100 and s["edges_border"].max() > 10
    assert len(set(s["edges_open"].tolist())) > 3                 # the outline changes from day to day


def test_land_grid_the_largest_object_alone(gpu, land):
    """the rows of every other object lie between its rows, unselected"""
    ds, obj, ln = land
    big = int(np.argmax(obj.n_events))
    assert obj.n_objects > 1
    run(gpu, ds, obj, ids=[big], lengths=ln, tracks=False)


def captured_arguments(ds, obj, **kw):
    return ocr.captured_arguments("shape", ds, obj, **kw)


@pytest.mark.parametrize("which", ["both", "one"])
def test_two_objects_side_by_side(gpu, which):
    ds, both, one = sc.two_objects_side_by_side()
    args = sc.stage_arguments(ds, both, [0, 0], [3, 3]) if which == "both" else sc.stage_arguments(ds, one, [0], [3])
    got, want = gpu.track_shape_device(*args), so.stage_oracle(ds.cell_index, ds.sshape)(*args)
    for k in gpu.STAGE_FIELDS:
        npt.assert_array_equal(got[k], want[k], err_msg=k)
    assert got["edges_open"].tolist() == [4] * (6 if which == "both" else 3) and set(got["cells_edge"].tolist()) == {1}


def test_rows_that_do_not_fit_are_counted_not_written(gpu):
    """a selected row whose days leave its object's entries neither adds nor covers: the result is that of the table with
    the row unselected, and n_bad says 1"""
    import xmhw_amd
    ds = oc.random_grid(3, T=40)
    obj = xmhw_amd.mhw_objects(ds)
    args = captured_arguments(ds, obj, lengths="sphere")
    oracle = so.stage_for(ds, obj)
    good, bad = raw_stage(args)
    assert bad == 0
    for k in gpu.STAGE_FIELDS:
        npt.assert_array_equal(good[k], oracle(*args)[k], err_msg=k)
    row = int(np.argmax(args[1] - args[0]))
    for change in ("starts-early", "ends-late", "cell"):
        broken = [a.copy() for a in args]
        if change == "starts-early":
            broken[0][row] -= 10_000
        elif change == "ends-late":                              # the last row of its cell: the ends stay in order
            row = int(args[4][args[3][row] + 1]) - 1
            broken[1][row] += 10_000
        else:
            broken[3][row] = args[5].shape[0]
        with pytest.raises(gpu.XmhwException, match="do not lie within"):
            gpu.track_shape_device(*broken)
        got, bad = raw_stage(broken)
        assert bad == 1
        without = [a.copy() for a in args]
        without[2][row] = -1
        want = oracle(*without)
        for k in gpu.STAGE_FIELDS:
            npt.assert_array_equal(got[k], want[k], err_msg=f"{change} {k}")
    # a face that names no cell is passed over and the row reported
    broken = [a.copy() for a in args]
    c = int(args[3][row])
    k = int(np.argmax(args[5][c] >= 0))
    assert args[5][c, k] >= 0
    broken[5][c, k] = args[5].shape[0] + 7
    got, bad = raw_stage(broken)
    assert bad == int((args[3][args[2] >= 0] == c).sum()) >= 1
    assert got["edges_open"].sum() <= good["edges_open"].sum()


def test_row_offsets_that_do_not_describe_the_rows(gpu):
    """whatever row_offsets holds, no row outside [0, n) is read; offsets that place every cell's rows outside the table
    find no neighbour row at all: every face towards a cell comes out open"""
    import xmhw_amd
    ds = oc.random_grid(5, T=40)
    obj = xmhw_amd.mhw_objects(ds, periodic="lon")
    args = captured_arguments(ds, obj, lengths="sphere")
    start, end, slot, cell, row_offsets, faces, lq, time_start, offsets = args
    n, L = start.shape[0], int(offsets[-1])
    want = {k: np.zeros(L, np.int64) for k in gpu.STAGE_FIELDS}
    for r in range(n):
        f, q = faces[cell[r]], lq[cell[r]]
        at = offsets[slot[r]] + np.arange(start[r], end[r] + 1) - time_start[slot[r]]
        want["edges_open"][at] += int((f >= 0).sum())
        want["edges_coast"][at] += int((f == -1).sum())
        want["edges_border"][at] += int((f == -2).sum())
        want["perimeter_open_q"][at] += int(q[f >= 0].sum())
        want["perimeter_coast_q"][at] += int(q[f == -1].sum())
        want["perimeter_border_q"][at] += int(q[f == -2].sum())
        want["cells_edge"][at] += int((f != -3).any())
    for moved in (row_offsets + n, row_offsets - n - 5, row_offsets + (1 << 40), row_offsets - (1 << 40),
                  np.where(np.arange(row_offsets.shape[0]) % 2, 1 << 40, -(1 << 40))):
        got, bad = raw_stage([start, end, slot, cell, moved, faces, lq, time_start, offsets])
        assert bad == 0
        if moved[0] < 0 and moved[1] > 0:                        # [0, n) for every other cell: some rows are found
            assert (got["edges_open"] <= want["edges_open"]).all()
            continue
        for k in gpu.STAGE_FIELDS:
            npt.assert_array_equal(got[k], want[k], err_msg=k)


def test_twice_the_same(gpu, land):
    import xmhw_amd
    ds, _, ln = land
    obj = xmhw_amd.mhw_objects(ds, connectivity=26, periodic="lon")
    a = xmhw_amd.mhw_track_shape(ds, obj, lengths=ln)
    b = xmhw_amd.mhw_track_shape(ds, obj, lengths=ln)
    for k in gpu.STAGE_FIELDS:
        npt.assert_array_equal(getattr(a, k), getattr(b, k), err_msg=k)


def test_refused_without_a_launch(gpu):
    from xmhw_amd._lib import hip
    h = hip()
    big = 1 << 31
    base = dict(n=1, C=1, K=4, n_slots=1, L=1)

    def call(**kw):
        a = dict(base, **kw)
        h.object_shape(0, 0, 0, 0, a["n"], 0, a["C"], 0, a["K"], 0, 0, 0, a["n_slots"], a["L"], 0, 0, 0, 0)

    for kw in (dict(n=big), dict(C=big), dict(n_slots=big), dict(L=big), dict(K=8), dict(K=3), dict(K=0)):      # XMHW_ERR_UNSUPPORTED
        with pytest.raises(h.HipError, match=r"\(code 3\)"):
            call(**kw)
    for kw in (dict(n=-1), dict(C=-1), dict(n_slots=-1), dict(L=-1)):
        with pytest.raises(h.InvalidArgument):
            call(**kw)
    with pytest.raises(h.InvalidArgument):                        # null buffers
        call()


def test_no_events_touches_nothing(gpu):
    import xmhw_amd
    ds = oc.dataset((2, 3), np.ones(6, bool), [[] for _ in range(6)], T=10)
    sh = xmhw_amd.mhw_track_shape(ds, xmhw_amd.mhw_objects(ds))
    assert sh.n_selected == 0 and sh.edges_open.shape == (0,)
