"""Host side of mhw_track_shape() (xmhw_amd/track_shape.py) with the device stage replaced by the shifted-map oracle
(tests/track_shape_oracle.stage_oracle): the alignment with mhw_tracks(), ``ids`` subsets and their order, the
identities, the derived fields, the face table against a loop, the "sphere" lengths against closed forms, the
quantisation, every refusal, and the hand-drawn cases with their expected counts."""
import math

import numpy as np
import numpy.testing as npt
import pytest

import objects_cases as oc
import objects_oracle as oo
import track_shape_cases as sc
import track_shape_oracle as so
import tracks_oracle as to
from xmhw_amd import TrackShapeDataset, XmhwException, compactness, mhw_objects, mhw_track_shape, mhw_tracks
from xmhw_amd import track_shape as ts
from xmhw_amd.detect import EventDataset

SEEDS = list(range(6))


def objects(ds, **kw):
    return mhw_objects(ds, _compute=oo.objects_graph, **kw)


def tracks(ds, obj, **kw):
    return mhw_tracks(ds, obj, _compute=to.stage_voxels, **kw)


def shape(ds, obj, **kw):
    return mhw_track_shape(ds, obj, _compute=so.stage_for(ds, obj), **kw)


def identities(sh, tr, periodic):
    """the identities of the module docstring, and the alignment"""
    for k in ("ids", "offsets", "time_start", "time_end", "duration", "pos"):
        npt.assert_array_equal(getattr(sh, k), getattr(tr, k), err_msg=k)
    exposed = sh.edges_exposed.astype(np.int64)
    npt.assert_array_equal(exposed, sh.edges_open.astype(np.int64) + sh.edges_coast + sh.edges_border)
    assert (sh.cells_edge <= tr.n_cells).all()
    assert (sh.cells_edge <= exposed).all() and (exposed <= 4 * sh.cells_edge.astype(np.int64)).all()
    assert (exposed <= 4 * tr.n_cells.astype(np.int64)).all()
    assert (exposed >= (4 if periodic is None else 2)).all()


def random_lengths(ds, seed):
    rng = np.random.default_rng(seed)
    ln = rng.uniform(0.0, 5.0, tuple(ds.sshape) + (4,))
    ln[rng.random(ln.shape) < 0.1] = 0.0
    return ln


@pytest.mark.parametrize("connectivity,periodic", [(6, None), (26, "lon"), (6, "lat")])
@pytest.mark.parametrize("lengths", [None, "sphere", "random"])
def test_random_grids_against_the_dense_oracle(connectivity, periodic, lengths):
    for seed in SEEDS:
        ds = oc.random_grid(seed)
        ln = random_lengths(ds, seed) if lengths == "random" else lengths
        obj = objects(ds, connectivity=connectivity, periodic=periodic)
        sh = shape(ds, obj, lengths=ln)
        assert isinstance(sh, TrackShapeDataset) and sh.periodic == periodic
        so.same_as_dense(sh, so.shape_dense(ds, obj, None, ln))
        identities(sh, tracks(ds, obj), periodic)
        if lengths is None:
            for c in ts.CLASSES:
                npt.assert_array_equal(getattr(sh, f"perimeter_{c}_q"), getattr(sh, f"edges_{c}").astype(np.int64) << sh.length_bits)


def test_derived_fields():
    ds = oc.random_grid(3)
    obj = objects(ds, connectivity=26)
    ln = random_lengths(ds, 11)
    sh = shape(ds, obj, lengths=ln)
    unit = float(ln.max()) / 2.0 ** sh.length_bits
    assert sh.length_unit == unit and sh.length_bits == 31 and sh.attrs["lengths"] == "array"
    total = sh.perimeter_open_q + sh.perimeter_coast_q + sh.perimeter_border_q
    npt.assert_array_equal(sh.perimeter_q, total)
    for c in ts.CLASSES:
        npt.assert_array_equal(getattr(sh, f"perimeter_{c}"), getattr(sh, f"perimeter_{c}_q") * unit)
    npt.assert_array_equal(sh.perimeter, total * unit)
    assert (sh.edges_coast > 0).any() and (sh.edges_border > 0).any() and (sh.edges_open > 0).any()
    for i in range(sh.n_selected):
        s = sh.series(i)
        q = s["perimeter_q"].tolist()
        assert sh.perimeter_max[i] == max(q) * unit
        assert sh.pos_perimeter_max[i] == obj.time_start[i] + q.index(max(q))
        assert sh.days_coastal[i] == sum(1 for v in s["edges_coast"] if v > 0)
        npt.assert_array_equal(s["pos"], np.arange(obj.time_start[i], obj.time_end[i] + 1))
        npt.assert_array_equal(s["time"], ds.time[s["pos"]])
        for a, b, frac in zip(s["perimeter_open_q"].tolist(), s["perimeter_coast_q"].tolist(), s["coast_fraction"].tolist()):
            assert (math.isnan(frac) and a + b == 0) or frac == b / (a + b)
    # a cell in the corner of a 1 x 1 ocean: only border faces -> 0 / 0
    one = sc.grid(1, 1, {(0, 0): [(0, 1)]}, T=3)
    sh1 = shape(one, objects(one))
    assert sh1.edges_border.tolist() == [4, 4] and np.isnan(sh1.coast_fraction).all() and sh1.perimeter.tolist() == [4.0, 4.0]


def test_compactness():
    ds = sc.full_grid(4, 2)                                       # a square of 4 x 4 cells: area 16, perimeter 16
    obj = objects(ds)
    sh, tr = shape(ds, obj), tracks(ds, obj)
    npt.assert_allclose(compactness(sh, tr), [math.pi / 4] * 2, rtol=1e-15)
    ds = oc.random_grid(2)
    obj = objects(ds)
    sh, tr = shape(ds, obj), tracks(ds, obj)
    npt.assert_array_equal(compactness(sh, tr), 4.0 * np.pi * tr.area / sh.perimeter ** 2)
    ids = np.arange(obj.n_objects)[::-1]
    with pytest.raises(XmhwException, match="same ids"):
        compactness(shape(ds, obj, ids=ids), tr)
    with pytest.raises(XmhwException, match="expects"):
        compactness(tr, sh)


def brute_face_table(cell_index, sshape, axis):
    ny, nx = sshape
    number = {int(p): c for c, p in enumerate(cell_index)}
    out = []
    for p in cell_index:
        i, j = divmod(int(p), nx)
        row = []
        for di, dj in ((-1, 0), (1, 0), (0, -1), (0, 1)):
            a = 0 if di else 1
            ii, jj = i + di, j + dj
            if axis == a:
                if sshape[a] == 1:
                    row.append(-3)
                    continue
                ii, jj = ii % ny, jj % nx
            if not (0 <= ii < ny and 0 <= jj < nx):
                row.append(-2)
            else:
                row.append(number.get(ii * nx + jj, -1))
        out.append(row)
    return np.array(out, dtype=np.int32).reshape(len(cell_index), 4)


@pytest.mark.parametrize("axis", [None, 0, 1])
def test_face_table_against_a_loop(axis):
    rng = np.random.default_rng(0)
    for sshape in ((5, 7), (1, 6), (6, 1), (2, 2), (1, 1), (2, 5), (4, 2)):
        keep = rng.random(sshape[0] * sshape[1]) >= 0.3
        keep[0] = True
        cell_index = np.nonzero(keep)[0]
        got = ts.face_table(cell_index, sshape, axis)
        assert got.dtype == np.int32
        npt.assert_array_equal(got, brute_face_table(cell_index, sshape, axis), err_msg=str(sshape))
    assert (ts.FACE_COAST, ts.FACE_BORDER, ts.FACE_FOLDED) == (-1, -2, -3)
    # what objects.neighbour_table keeps apart from -1 only by being >= 0 is the same here
    from xmhw_amd.objects import neighbour_table
    cell_index = np.nonzero(rng.random(35) >= 0.3)[0]
    a, b = ts.face_table(cell_index, (5, 7), axis), neighbour_table(cell_index, (5, 7), 6, axis)
    npt.assert_array_equal(np.where(a < 0, -1, a), b)


def test_sphere_lengths_closed_forms():
    R = 6371.0088
    lat = np.arange(-87.5, 90, 5.0)                               # 36 rows, the outer faces at the poles
    lon = np.arange(0.0, 360, 10.0)
    ln = ts.sphere_lengths({"lat": lat, "lon": lon}, ("lat", "lon"), (36, 36))
    assert ln.shape == (36, 36, 4) and ln.dtype == np.float64
    npt.assert_array_equal(ln[..., 2], ln[..., 3])                # the west and the east face of a cell
    npt.assert_allclose(ln[..., 2], R * math.radians(5.0), rtol=1e-13)
    assert (ln[0, :, 0] == 0.0).all() and (ln[-1, :, 1] == 0.0).all()       # the faces at the two poles, exactly
    npt.assert_array_equal(ln[1:, :, 0], ln[:-1, :, 1])           # one face seen from its two cells
    npt.assert_allclose(ln[:, :, 0], ln[::-1, :, 1], rtol=1e-12)  # cells at +-lat mirror each other
    for i in (0, 7, 18, 35):
        npt.assert_allclose(ln[i, :, 1], R * math.cos(math.radians(-90 + 5.0 * (i + 1))) * math.radians(10.0) if i < 35 else 0.0,
                            rtol=1e-12, atol=0)
    # the dims the other way round and a descending latitude: the same numbers where they belong
    ln2 = ts.sphere_lengths({"lat": lat[::-1], "lon": lon}, ("lon", "lat"), (36, 36))
    npt.assert_array_equal(ln2[..., 0], ln2[..., 1])              # dim 0 is the longitude
    npt.assert_allclose(ln2[:, :, 2].T, ln[::-1, :, 1], rtol=1e-12)         # towards the smaller index = towards the north
    # uneven spacing: faces half way, the ends extended by half the adjacent spacing, latitude clipped
    ln3 = ts.sphere_lengths({"lat": np.array([0.0, 10.0, 30.0, 85.0]), "lon": np.array([0.0, 2.0, 6.0])}, ("lat", "lon"), (4, 3))
    edges = [-5.0, 5.0, 20.0, 57.5, 90.0]
    npt.assert_allclose(ln3[:, 0, 2], [R * math.radians(b - a) for a, b in zip(edges[:-1], edges[1:])], rtol=1e-13)
    npt.assert_allclose(ln3[1, :, 0], [R * math.cos(math.radians(5.0)) * math.radians(w) for w in (2.0, 3.0, 4.0)], rtol=1e-13)
    assert (ln3[3, :, 1] == 0.0).all()
    npt.assert_array_equal(so.sphere_lengths(oc.random_grid(0)), ts.sphere_lengths(oc.random_grid(0).coords, ("lat", "lon"),
                                                                                   oc.random_grid(0).sshape))


def test_quantisation_and_length_bits():
    assert [ts.length_bits(c) for c in (1, 2**20, 2**29 - 1, 2**29, 2**30, 2**31 - 1)] == [31, 31, 31, 30, 29, 29]
    for c in (1, 1000, 2**29, 2**31 - 1):
        assert 4 * c * 2 ** ts.length_bits(c) < 2**63
    ln = np.array([[[0.0, 1.0, 2.5, 10.0]]])
    lq, unit = ts.quantise_lengths(ln, 31)
    assert lq.dtype == np.int64 and lq.tolist() == [[[0, 214748365, 536870912, 2147483648]]]
    assert unit == 10.0 / 2**31
    lq, _ = ts.quantise_lengths(np.array([0.5, 1.5, 2.5, 4.0]), 2)        # half to even
    assert lq.tolist() == [0, 2, 2, 4]
    # what the stage is handed
    ds = oc.random_grid(2)
    obj = objects(ds, periodic="lon")
    ln = random_lengths(ds, 5)
    seen = {}

    def stage(start, end, slot, cell, row_offsets, faces, lq, time_start, offsets):
        seen.update(locals())
        return so.stage_for(ds, obj)(start, end, slot, cell, row_offsets, faces, lq, time_start, offsets)

    ids = np.arange(obj.n_objects)[1::2]
    sh = mhw_track_shape(ds, obj, ids=ids, lengths=ln, _compute=stage)
    want = np.rint(ln / ln.max() * 2.0 ** 31).astype(np.int64).reshape(-1, 4)[ds.cell_index]
    npt.assert_array_equal(seen["lq"], want)
    assert seen["lq"].dtype == np.int64 and seen["faces"].dtype == np.int32
    npt.assert_array_equal(seen["faces"], ts.face_table(ds.cell_index, ds.sshape, 1))
    npt.assert_array_equal(seen["slot"] >= 0, np.isin(obj.object, ids))
    npt.assert_array_equal(seen["row_offsets"], ds.offsets)
    npt.assert_array_equal(seen["time_start"], obj.time_start[ids])
    assert sh.length_bits == 31


def test_ids_order_and_alignment_with_tracks():
    ds = oc.random_grid(5)
    obj = objects(ds, connectivity=26)
    assert obj.n_objects >= 4
    full = shape(ds, obj, lengths="sphere")
    npt.assert_array_equal(full.ids, np.arange(obj.n_objects))
    npt.assert_array_equal(full.offsets, np.concatenate([[0], np.cumsum(obj.duration)]))
    for ids in (np.arange(obj.n_objects)[::-1], np.arange(obj.n_objects)[::-1][::2], np.arange(obj.n_objects)[1:3]):
        sh = shape(ds, obj, ids=ids, lengths="sphere")            # the unselected objects lie beside the selected ones
        identities(sh, tracks(ds, obj, ids=ids), None)
        npt.assert_array_equal(sh.ids, ids)
        for i, o in enumerate(ids):                               # the subset holds the slices of the full result
            a, b = sh.series(i), full.series(int(o))
            for k in a:
                npt.assert_array_equal(a[k], b[k], err_msg=k)
        for k in ("perimeter_max", "pos_perimeter_max", "days_coastal"):
            npt.assert_array_equal(getattr(sh, k), getattr(full, k)[ids], err_msg=k)
    empty = shape(ds, obj, ids=[])
    assert empty.n_selected == 0 and empty.edges_open.shape == (0,) and empty.offsets.tolist() == [0]
    assert empty.days_coastal.shape == empty.perimeter_max.shape == empty.coast_fraction.shape == (0,)
    with pytest.raises(XmhwException):
        full.series(obj.n_objects)


@pytest.mark.parametrize("case", sc.hand_drawn(), ids=lambda c: c["name"])
def test_hand_drawn(case):
    ds = case["ds"]
    obj = objects(ds, **case["kw"])
    assert obj.n_objects == 1
    sh = shape(ds, obj)
    for k in ("edges_open", "edges_coast", "edges_border", "cells_edge"):
        assert getattr(sh, k).tolist() == case[k], k
    for c in ts.CLASSES:
        assert getattr(sh, f"perimeter_{c}_q").tolist() == [v << sh.length_bits for v in case[f"edges_{c}"]]
    assert sh.perimeter.tolist() == [float(a + b + c) for a, b, c in zip(case["edges_open"], case["edges_coast"], case["edges_border"])]
    assert sh.days_coastal.tolist() == [sum(1 for v in case["edges_coast"] if v > 0)]
    so.same_as_dense(sh, so.shape_dense(ds, obj))
    identities(sh, tracks(ds, obj), obj.periodic)


def test_broken_bar_changes_its_perimeter():
    """the faces across lon twice as long as those across lat: whole, the bar has 10 + 2 * 2; broken, 8 + 2 * 2 + 2 * 2"""
    import track_parts_cases as pc
    ds = pc.broken_bar()
    ln = np.ones((3, 5, 4))
    ln[..., 2:] = 2.0
    sh = shape(ds, objects(ds), lengths=ln)
    assert sh.length_unit == 2.0 / 2**31
    assert sh.perimeter_open.tolist() == [10.0] * 3 + [12.0] * 3 + [10.0] * 3 and sh.perimeter_border.tolist() == [4.0] * 9
    assert sh.perimeter.tolist() == [14.0] * 3 + [16.0] * 3 + [14.0] * 3
    assert sh.perimeter_max.tolist() == [16.0] and sh.pos_perimeter_max.tolist() == [3]


def test_wrap_of_two_counts_each_face_with_its_own_length():
    ds = sc.wrap_of_two()
    ln = np.zeros((1, 2, 4))
    ln[0, 0] = [1.0, 2.0, 4.0, 8.0]
    ln[0, 1] = [16.0, 32.0, 64.0, 128.0]
    sh = shape(ds, objects(ds, periodic="lon"), lengths=ln)
    assert sh.perimeter_open.tolist() == [12.0, 12.0, 0.0, 0.0]
    assert sh.perimeter_border.tolist() == [3.0, 3.0, 51.0, 51.0]


def test_coast_ring_fraction():
    sh = shape(sc.coast_ring(), objects(sc.coast_ring()))
    assert sh.coast_fraction.tolist() == [5 / 16] * 4 and sh.days_coastal.tolist() == [4]


@pytest.mark.parametrize("which", ["both", "one"])
def test_two_objects_side_by_side_at_stage_level(which):
    ds, both, one = sc.two_objects_side_by_side()
    stage = so.stage_oracle(ds.cell_index, ds.sshape)
    if which == "both":
        got = stage(*sc.stage_arguments(ds, both, [0, 0], [3, 3]))
        assert got["edges_open"].tolist() == [4] * 6 and got["cells_edge"].tolist() == [1] * 6
    else:
        got = stage(*sc.stage_arguments(ds, one, [0], [3]))       # the neighbour is not selected: open all the same
        assert got["edges_open"].tolist() == [4] * 3 and got["cells_edge"].tolist() == [1] * 3
    assert not got["edges_coast"].any() and not got["edges_border"].any()


def test_refusals():
    ds = oc.random_grid(1)
    obj = objects(ds)
    with pytest.raises(XmhwException, match="mhw_track_shape expects the EventDataset"):
        mhw_track_shape("x", obj)
    with pytest.raises(XmhwException, match="mhw_track_shape expects the ObjectDataset"):
        mhw_track_shape(ds, "x")
    other = objects(oc.random_grid(2))
    with pytest.raises(XmhwException, match="one entry per table row|does not belong"):
        shape(ds, other)
    point = EventDataset(ds.table[:0], np.zeros(2, np.int64), ds.time, np.zeros(1, np.int64), np.ones(1, bool), (), (), {}, {}, {},
                         {}, True)
    with pytest.raises(XmhwException, match="grid"):
        mhw_track_shape(point, obj)
    one_dim = EventDataset(ds.table, ds.offsets, ds.time, ds.cell_index, ds.keep, ("cell",), (int(np.prod(ds.sshape)),), {}, {},
                           {}, {}, False)
    with pytest.raises(XmhwException, match="two spatial dims"):
        mhw_track_shape(one_dim, obj)
    for bad, what in (([0, 0], "distinct"), ([obj.n_objects], r"in \[0"), ([-1], r"in \[0"), ([[0]], "1-D"), ([0.5], "integer")):
        with pytest.raises(XmhwException, match=what):
            shape(ds, obj, ids=bad)
    called = []
    count = lambda *a: called.append(1)                          # noqa: E731
    renamed = EventDataset(ds.table, ds.offsets, ds.time, ds.cell_index, ds.keep, ("y", "x"), ds.sshape, {}, {}, {}, {}, False)
    with pytest.raises(XmhwException, match="obj.periodic should be None or one of"):
        mhw_track_shape(renamed, objects(ds, periodic="lon"), _compute=count)
    # lengths=: refused before the stage is called
    with pytest.raises(XmhwException, match="lengths should be None, 'sphere' or an array, got 'km'"):
        mhw_track_shape(ds, obj, lengths="km", _compute=count)
    with pytest.raises(XmhwException, match="needs latitude and longitude coordinates"):
        mhw_track_shape(renamed, obj, lengths="sphere", _compute=count)
    for coords, what in (({"lat": np.zeros((2, 2)), "lon": ds.coords["lon"]}, "1-D along their dims"),
                         ({"lat": ds.coords["lat"] * 2, "lon": ds.coords["lon"]}, r"within \[-90, 90\]"),
                         ({"lat": ds.coords["lat"], "lon": ds.coords["lon"] * np.nan}, "finite")):
        odd = EventDataset(ds.table, ds.offsets, ds.time, ds.cell_index, ds.keep, ds.sdims, ds.sshape, coords, {}, {}, {}, False)
        with pytest.raises(XmhwException, match=what):
            mhw_track_shape(odd, obj, lengths="sphere", _compute=count)
    thin = sc.folded()
    with pytest.raises(XmhwException, match="at least 2 values"):
        mhw_track_shape(thin, objects(thin), lengths="sphere", _compute=count)
    good = np.ones(tuple(ds.sshape) + (4,))
    for bad, what in ((good[..., :3], "should have the shape"), (good.reshape(-1, 4), "should have the shape"),
                      (np.where(np.arange(4) == 1, np.nan, good), "finite and >= 0"),
                      (np.where(np.arange(4) == 2, np.inf, good), "finite and >= 0"), (-good, "finite and >= 0"),
                      (good * 0.0, "at least one value > 0"), (object(), "got object|should have the shape")):
        with pytest.raises(XmhwException, match=what):
            mhw_track_shape(ds, obj, lengths=bad, _compute=count)
    assert not called
    broken = EventDataset(ds.table, ds.offsets[:-1], ds.time, ds.cell_index, ds.keep, ds.sdims, ds.sshape, ds.coords, {}, {}, {},
                          False)
    with pytest.raises(XmhwException, match="offsets and cell_index do not describe the table"):
        shape(broken, obj)
    # a table row outside the days of its object: the refusal of mhw_tracks()
    moved = EventDataset(ds.table.copy(), ds.offsets, ds.time, ds.cell_index, ds.keep, ds.sdims, ds.sshape, ds.coords, {}, {}, {},
                         False)
    first = int(np.nonzero(ds.table[:, oc.COL["index_start"]] == obj.time_start[obj.object])[0][0])    # opens its object
    moved.table[first, oc.COL["index_start"]] -= 1
    with pytest.raises(XmhwException, match="outside the days of its object: obj does not belong to mhw"):
        shape(moved, obj)


def test_stand_ins_that_return_the_wrong_thing():
    ds = oc.random_grid(1)
    obj = objects(ds)
    L = int(obj.duration.sum())
    right = so.stage_for(ds, obj)

    def changed(**kw):
        def stage(*a):
            got = right(*a)
            got.update(kw)
            return got
        return stage

    for k in ts.STAGE_FIELDS:
        with pytest.raises(XmhwException, match="do not fit"):
            mhw_track_shape(ds, obj, _compute=changed(**{k: np.ones(L + 1, np.int64)}))
        with pytest.raises(XmhwException, match="do not fit"):
            mhw_track_shape(ds, obj, _compute=changed(**{k: np.ones((L, 1), np.int64)}))
    with pytest.raises(XmhwException, match="should return the arrays"):
        mhw_track_shape(ds, obj, _compute=lambda *a: dict(edges_open=np.ones(L, np.int32)))
    with pytest.raises(XmhwException, match="should return the arrays"):
        mhw_track_shape(ds, obj, _compute=lambda *a: None)
    # a stage that reports a day without a cell, or with fewer faces than any footprint has
    zeros = {k: np.zeros(L, np.int64) for k in ts.STAGE_FIELDS}
    with pytest.raises(XmhwException, match=f"{L} days of the selected objects hold no cell"):
        mhw_track_shape(ds, obj, _compute=lambda *a: zeros)
    three = dict(zeros, edges_open=np.full(L, 3), cells_edge=np.ones(L, np.int64))
    with pytest.raises(XmhwException, match="hold no cell: obj does not belong to mhw"):
        mhw_track_shape(ds, obj, _compute=lambda *a: three)
    wrapped = objects(ds, periodic="lon")
    Lw = int(wrapped.duration.sum())
    two = {k: np.zeros(Lw, np.int64) for k in ts.STAGE_FIELDS}
    two.update(edges_border=np.full(Lw, 2), cells_edge=np.ones(Lw, np.int64))
    assert mhw_track_shape(ds, wrapped, _compute=lambda *a: two).edges_exposed.tolist() == [2] * Lw


def test_empty_table():
    ds = oc.dataset((2, 3), np.ones(6, bool), [[] for _ in range(6)], T=10)
    called = []
    sh = mhw_track_shape(ds, objects(ds), _compute=lambda *a: called.append(1))
    assert sh.n_selected == 0 and sh.offsets.tolist() == [0] and not called
    assert sh.edges_open.shape == sh.perimeter.shape == sh.perimeter_max.shape == (0,)
    # and the device stage itself hands back zeros for nothing to do, without a device
    z = ts.track_shape_device(np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32),
                              np.zeros(7, np.int64), np.zeros((6, 4), np.int32), np.ones((6, 4), np.int64), np.zeros(1, np.int32),
                              np.array([0, 3]))
    assert set(z) == set(ts.STAGE_FIELDS) and all(v.shape == (3,) and not v.any() for v in z.values())


def test_to_xarray():
    xr = pytest.importorskip("xarray")
    ds = oc.random_grid(4)
    obj = objects(ds)
    x = shape(ds, obj, lengths="sphere").to_xarray()
    assert isinstance(x, xr.Dataset) and x.sizes["obs"] == x["offsets"].values[-1] and x.attrs["lengths"] == "sphere"
    assert x.attrs["length_bits"] == 31 and "coast_fraction" in x and "days_coastal" in x
