"""Host side of mhw_tracks() (xmhw_amd/tracks.py) with the device stage replaced by a numpy stand-in that follows the
stage contract (tests/tracks_oracle.stage_voxels): the refusals, the CSR layout and the order of ``ids``, the two
identities that tie the series to mhw_objects(), the dense brute-force oracle on random grids and the golden
tables, and hand-built cases with known answers."""
import numpy as np
import numpy.testing as npt
import pytest

import objects_cases as oc
import objects_oracle as oo
import tracks_oracle as to
from xmhw_amd import TrackDataset, XmhwException, mhw_objects, mhw_tracks
from xmhw_amd.detect import EventDataset
from xmhw_amd.tracks import moment_bits

SEEDS = list(range(12))


def objects(ds, **kw):
    return mhw_objects(ds, _compute=oo.objects_graph, **kw)


def tracks(ds, obj, **kw):
    return mhw_tracks(ds, obj, _compute=to.stage_voxels, **kw)


def identities(tr, obj, same_weights=True):
    ids = tr.ids
    npt.assert_array_equal(np.add.reduceat(tr.n_cells.astype(np.int64), tr.offsets[:-1]) if len(ids) else [], obj.cell_days[ids])
    if same_weights:
        npt.assert_array_equal(np.add.reduceat(tr.area_q, tr.offsets[:-1]) if len(ids) else [], obj.area_days_q[ids])
    npt.assert_array_equal(np.diff(tr.offsets), obj.duration[ids])


def grid(ny, nx, cells, T=60, lat=None, lon=None):
    per_cell = [cells.get((i, j), []) for i in range(ny) for j in range(nx)]
    ds = oc.dataset((ny, nx), np.ones((ny, nx), bool), per_cell, T=T)
    if lat is not None:
        ds.coords["lat"] = np.asarray(lat, dtype=np.float64)
    if lon is not None:
        ds.coords["lon"] = np.asarray(lon, dtype=np.float64)
    return ds


def without_latlon(ds):
    coords = {"time": ds.coords["time"]}
    return EventDataset(ds.table, ds.offsets, ds.time, ds.cell_index, ds.keep, ("j", "i"), ds.sshape, coords, {}, {}, {}, False)


@pytest.mark.parametrize("connectivity,periodic", [(6, None), (26, "lon")])
@pytest.mark.parametrize("weights", [None, "coslat"])
def test_random_grids_against_the_dense_oracle(connectivity, periodic, weights):
    for seed in SEEDS:
        ds = oc.random_grid(seed)
        obj = objects(ds, connectivity=connectivity, periodic=periodic, weights=weights)
        tr = tracks(ds, obj, weights=weights)
        assert isinstance(tr, TrackDataset) and tr.mode == "sphere"
        identities(tr, obj)
        to.same_as_dense(tr, to.tracks_dense(ds, obj, None, weights))


@pytest.mark.parametrize("key", list(oc.GOLDEN_COUNTS))
def test_golden_tables(key):
    connectivity, periodic = key
    ds = oc.golden_dataset()
    obj = objects(ds, connectivity=connectivity, periodic=periodic, weights="coslat")
    tr = tracks(ds, obj, weights="coslat")
    identities(tr, obj)
    assert tr.n_selected == oc.GOLDEN_COUNTS[key][0]
    big = np.argsort(obj.n_events)[::-1][:5]
    sub = tracks(ds, obj, ids=big, weights="coslat")
    identities(sub, obj)
    to.same_as_dense(sub, to.tracks_dense(ds, obj, big, "coslat"))
    for i, o in enumerate(big):                                   # the subset holds the slices of the full result
        a, b = sub.series(i), tr.series(int(o))
        for k in a:
            npt.assert_array_equal(a[k], b[k], err_msg=k)


def test_array_weights_and_other_weights_than_the_objects():
    ds = oc.random_grid(3)
    rng = np.random.default_rng(0)
    w = rng.uniform(0, 5, ds.sshape)
    obj = objects(ds, weights=w)
    tr = tracks(ds, obj, weights=w)
    identities(tr, obj)
    to.same_as_dense(tr, to.tracks_dense(ds, obj, None, w))
    other = tracks(ds, obj, weights=None)                         # other weights: the cell identity still holds
    identities(other, obj, same_weights=False)
    npt.assert_array_equal(other.area_q, other.n_cells.astype(np.int64) << obj.weight_bits)


def test_refusals():
    ds = oc.random_grid(1)
    obj = objects(ds)
    with pytest.raises(XmhwException, match="EventDataset"):
        mhw_tracks("x", obj)
    with pytest.raises(XmhwException, match="ObjectDataset"):
        mhw_tracks(ds, "x")
    other = objects(oc.random_grid(2))
    with pytest.raises(XmhwException, match="one entry per table row|does not belong"):
        tracks(ds, other)
    point = EventDataset(ds.table[:0], np.zeros(2, np.int64), ds.time, np.zeros(1, np.int64), np.ones(1, bool), (), (), {}, {}, {},
                         {}, True)
    with pytest.raises(XmhwException, match="grid"):
        tracks(point, obj)
    one_dim = EventDataset(ds.table, ds.offsets, ds.time, ds.cell_index, ds.keep, ("cell",), (int(np.prod(ds.sshape)),), {}, {},
                           {}, {}, False)
    with pytest.raises(XmhwException, match="two spatial dims"):
        tracks(one_dim, obj)
    for bad, what in (([0, 0], "distinct"), ([obj.n_objects], r"in \[0"), ([-1], r"in \[0"), ([[0]], "1-D"), ([0.5], "integer")):
        with pytest.raises(XmhwException, match=what):
            tracks(ds, obj, ids=bad)
    with pytest.raises(XmhwException, match="weights"):
        tracks(ds, obj, weights="area")
    with pytest.raises(XmhwException, match="weights should be None, 'coslat' or an array, got 'area'"):
        tracks(ds, obj, weights="area")
    # offsets that do not cover the table; the weights are looked at first
    broken = EventDataset(ds.table, ds.offsets[:-1], ds.time, ds.cell_index, ds.keep, ds.sdims, ds.sshape, ds.coords, {}, {}, {},
                          False)
    with pytest.raises(XmhwException, match="offsets and cell_index do not describe the table"):
        tracks(broken, obj)
    with pytest.raises(XmhwException, match="weights should be None, 'coslat' or an array, got 'area'"):
        tracks(broken, obj, weights="area")
    with pytest.raises(XmhwException, match="shape"):
        tracks(ds, obj, weights=np.ones((2, 2, 2)))
    with pytest.raises(XmhwException, match="wrap"):                # index mode on a wrapping grid
        plain = without_latlon(ds)
        tracks(plain, mhw_objects(plain, periodic="i", _compute=oo.objects_graph))
    with pytest.raises(XmhwException, match="do not fit"):
        mhw_tracks(ds, obj, _compute=lambda *a: dict(n_cells=np.zeros(3, np.int32), sums=np.zeros((4, 3), np.int64)))


def test_ids_order_and_csr_layout():
    ds = oc.random_grid(5)
    obj = objects(ds, connectivity=26)
    assert obj.n_objects >= 4
    full = tracks(ds, obj)
    npt.assert_array_equal(full.ids, np.arange(obj.n_objects))
    npt.assert_array_equal(full.offsets, np.concatenate([[0], np.cumsum(obj.duration)]))
    ids = np.arange(obj.n_objects)[::-1][::2]                     # a subset, in reverse order
    tr = tracks(ds, obj, ids=ids)
    npt.assert_array_equal(tr.ids, ids)
    assert tr.offsets[-1] == obj.duration[ids].sum() == tr.n_cells.shape[0]
    for i, o in enumerate(ids):
        s = tr.series(i)
        npt.assert_array_equal(s["pos"], np.arange(obj.time_start[o], obj.time_end[o] + 1))
        npt.assert_array_equal(s["time"], ds.time[s["pos"]])
        for k in ("n_cells", "area_q", "mx", "my", "mz", "lat", "lon"):
            npt.assert_array_equal(s[k], full.series(int(o))[k], err_msg=k)
        for t, nc in zip(s["pos"], s["n_cells"]):
            assert nc == (obj.label_map(t) == o).sum()
    identities(tr, obj)
    empty = tracks(ds, obj, ids=[])
    assert empty.n_selected == 0 and empty.n_cells.shape == (0,) and empty.offsets.tolist() == [0]
    with pytest.raises(XmhwException):
        tr.series(len(ids))


def test_empty_table():
    ds = oc.dataset((2, 3), np.ones(6, bool), [[] for _ in range(6)], T=10)
    called = []
    tr = mhw_tracks(ds, objects(ds), _compute=lambda *a: called.append(1))
    assert tr.n_selected == 0 and tr.offsets.tolist() == [0] and not called
    assert tr.lat.shape == tr.area.shape == tr.path_km.shape == tr.area_max_q.shape == (0,)


def test_single_cell():
    ds = grid(3, 4, {(1, 2): [(5, 9)]}, lat=[-30, 0, 30], lon=[0, 90, 180, 270])
    obj = objects(ds)
    tr = tracks(ds, obj)
    assert tr.n_cells.tolist() == [1] * 5 and tr.area_q.tolist() == [1 << obj.weight_bits] * 5
    npt.assert_allclose(tr.lat, 0.0, atol=1e-9)
    npt.assert_allclose(tr.lon, 180.0, atol=1e-9)
    assert tr.mx.tolist() == [-(1 << tr.moment_bits) * (1 << 20)] * 5 and not tr.mz.any()
    assert tr.path_km.tolist() == [0.0] and tr.pos_area_max.tolist() == [5] and tr.area_max_q.tolist() == [1 << obj.weight_bits]
    assert tr.moment_bits == moment_bits(obj.weight_bits, 12) == min(obj.weight_bits, 61 - 20 - 4)
    assert tr.area.tolist() == [1.0] * 5


def test_symmetric_about_the_equator():
    ds = grid(4, 3, {(0, 1): [(2, 6)], (1, 1): [(2, 6)], (2, 1): [(2, 6)], (3, 1): [(2, 6)]}, lat=[-45, -15, 15, 45],
              lon=[10, 20, 30])
    tr = tracks(ds, objects(ds), weights="coslat")
    assert tr.n_selected == 1 and tr.n_cells.tolist() == [4] * 5
    assert not tr.mz.any()                                        # exactly: sin is odd and rint is symmetric
    npt.assert_array_equal(tr.lat, 0.0)
    npt.assert_allclose(tr.lon, 20.0, atol=1e-4)


def test_astride_the_date_line():
    lon = np.arange(12) * 30.0 + 15.0                             # 15 .. 345: cells 5 and 6 sit at 165 and 195
    ds = grid(3, 12, {(1, 5): [(3, 8)], (1, 6): [(3, 8)]}, lat=[-10, 0, 10], lon=lon)
    tr = tracks(ds, objects(ds, periodic="lon"))
    npt.assert_allclose(tr.lon, 180.0, atol=1e-4)
    west = np.where(lon > 180, lon - 360, lon)                    # the same grid written -180 .. 180, first and last column
    order = np.argsort(west)
    ds2 = grid(3, 12, {(1, 0): [(3, 8)], (1, 11): [(3, 8)]}, lat=[-10, 0, 10], lon=west[order])
    obj2 = objects(ds2, periodic="lon")
    assert obj2.n_objects == 1
    tr2 = tracks(ds2, obj2)
    npt.assert_allclose(np.abs(tr2.lon), 180.0, atol=1e-4)         # on the date line, not at longitude 0
    npt.assert_allclose(tr2.lat, 0.0, atol=1e-9)
    to.same_as_dense(tr2, to.tracks_dense(ds2, obj2))


def test_split_and_merge():
    """one cell all along, two arms that leave it and come back: the cells of the day go 3, 2, 3"""
    ds = grid(1, 5, {(0, 2): [(0, 3), (8, 11)], (0, 1): [(2, 9)], (0, 3): [(2, 9)]}, T=20, lat=[0.0], lon=[0, 1, 2, 3, 4])
    obj = objects(ds)
    assert obj.n_objects == 1
    tr = tracks(ds, obj)
    assert tr.n_cells.tolist() == [1, 1, 3, 3, 2, 2, 2, 2, 3, 3, 1, 1]
    npt.assert_allclose(tr.lon, 2.0, atol=1e-4)
    assert tr.pos_area_max.tolist() == [2] and tr.area_max_q[0] == 3 << obj.weight_bits
    identities(tr, obj)


def test_neighbours_in_the_array_and_a_row_that_ends_on_the_last_day():
    """object 0's only row ends on its last day: its negative term lands on the first entry of object 1"""
    ds = grid(1, 5, {(0, 0): [(1, 4)], (0, 3): [(2, 6)], (0, 4): [(5, 6)]}, T=10, lat=[0.0], lon=[0, 10, 20, 30, 40])
    obj = objects(ds)
    assert obj.n_objects == 2 and obj.time_end.tolist() == [4, 6]
    tr = tracks(ds, obj)
    assert tr.offsets.tolist() == [0, 4, 9]
    assert tr.n_cells.tolist() == [1, 1, 1, 1, 1, 1, 1, 2, 2]
    rev = tracks(ds, obj, ids=[1, 0])
    assert rev.n_cells.tolist() == [1, 1, 1, 2, 2, 1, 1, 1, 1]
    npt.assert_allclose(rev.lon[[0, 3, 5]], [30.0, 35.0, 0.0], atol=1e-3)
    assert rev.path_km[1] == 0.0 and 500 < rev.path_km[0] < 600      # 5 degrees of the equator: 556 km
    to.same_as_dense(rev, to.tracks_dense(ds, obj, [1, 0]))


def test_index_mode():
    ds = without_latlon(grid(4, 6, {(1, 1): [(0, 4)], (1, 2): [(2, 4)], (2, 2): [(3, 6)]}, T=10))
    obj = mhw_objects(ds, _compute=oo.objects_graph)
    tr = tracks(ds, obj)
    assert tr.mode == "index" and tr.lat is None and tr.path_km is None and not tr.mz.any()
    assert tr.moment_bits == min(obj.weight_bits, 61 - 3 - 5)
    assert tr.n_cells.tolist() == [1, 1, 2, 3, 3, 1, 1]
    npt.assert_array_equal(tr.ci, [1, 1, 1, 4 / 3, 4 / 3, 2, 2])
    npt.assert_array_equal(tr.cj, [1, 1, 1.5, 5 / 3, 5 / 3, 2, 2])
    rng = np.random.default_rng(1)
    w = rng.uniform(0.1, 1, ds.sshape)
    trw = tracks(ds, obj, weights=w)
    to.same_as_dense(trw, to.tracks_dense(ds, obj, None, w))
    assert (trw.quantisation_bound() < 1e-6).all()


def test_quantisation_bound_is_small_on_a_real_grid_and_says_so_when_it_cannot_be():
    ds = oc.golden_dataset()
    obj = objects(ds, weights="coslat")
    tr = tracks(ds, obj, weights="coslat")
    b = tr.quantisation_bound()
    assert np.nanmax(b[tr.n_cells < 20]) < 1e-3                    # 20 bits: a micro-radian or so per unit vector
    # two opposite cells of equal weight: the vectors cancel, the centre is undefined or unbounded
    ds2 = grid(1, 2, {(0, 0): [(0, 1)], (0, 1): [(0, 1)]}, T=4, lat=[0.0], lon=[0.0, 180.0])
    obj2 = objects(ds2, periodic="lon")
    tr2 = tracks(ds2, obj2)
    assert tr2.n_cells.tolist() == [2, 2] and np.isnan(tr2.lon).all() and np.isnan(tr2.quantisation_bound()).all()


def test_to_xarray():
    xr = pytest.importorskip("xarray")
    ds = oc.random_grid(4)
    x = tracks(ds, objects(ds)).to_xarray()
    assert isinstance(x, xr.Dataset) and x.sizes["obs"] == x["offsets"].values[-1]
