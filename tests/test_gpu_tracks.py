"""mhw_tracks() on the device (csrc/kernels_tracks.hip): the C ABI entry against the voxel-by-voxel stage oracle and
the public function against the dense oracle (tests/tracks_oracle.py), every integer equal.

The scan works on tiles of TILE = 1024 entries (XMHW_TRACKS_TILE; 256 threads x 4 entries), and the tile sums are
scanned by the same kernels one level up, so a second level of tiles starts at 1024 tiles = 1,048,576 entries.  The
synthetic cases put L + 1 (the entries plus the sentinel) on both sides of each boundary."""
import numpy as np
import numpy.testing as npt
import pytest

import objects_cases as oc
import objects_oracle as oo
import tracks_oracle as to

pytestmark = pytest.mark.gpu
TILE = 1024


@pytest.fixture(scope="module")
def gpu():
    from xmhw_amd._lib import hip, require_gpu
    require_gpu()
    from xmhw_amd import tracks
    assert hip().TRACKS_TILE == TILE
    return tracks


def stage_case(L, seed, m, C=500, rows_per_object=6, vmax=(1 << 20, 1 << 30, 1 << 30, 1 << 30), same_sign=False):
    """stage arguments: m objects whose durations sum to L, each with a row from its first day, a row to its last day
    and random rows between; a few rows with a slot outside the selection"""
    rng = np.random.default_rng(seed)
    cuts = np.sort(rng.choice(np.arange(1, L), m - 1, replace=False)) if m > 1 else np.zeros(0, np.int64)
    offsets = np.concatenate([[0], cuts, [L]]).astype(np.int64)
    dur = np.diff(offsets)
    t0 = rng.integers(0, 3000, m).astype(np.int64)
    k = rows_per_object
    slot = np.repeat(np.arange(m), k)
    d = np.repeat(dur, k)
    s = (rng.random(m * k) * d).astype(np.int64)
    e = np.minimum(s + rng.integers(0, 40, m * k), d - 1)
    s[0::k] = 0                                                   # a row from the first day
    s[1::k] = np.maximum(d[1::k] - 1 - rng.integers(0, 5, m), 0)
    e[1::k] = d[1::k] - 1                                         # a row to the last day: its -term is the neighbour's entry 0
    e = np.maximum(e, s)
    start, end = (s + np.repeat(t0, k)).astype(np.int32), (e + np.repeat(t0, k)).astype(np.int32)
    slot = slot.astype(np.int32)
    out = rng.random(m * k) < 0.02
    slot[out] = np.where(rng.random(int(out.sum())) < 0.5, -1, m)
    cell = rng.integers(0, C, m * k).astype(np.int32)
    vec = np.stack([rng.integers(0, v, C, endpoint=True) * (1 if (same_sign or i == 0) else rng.choice([-1, 1], C))
                    for i, v in enumerate(vmax)]).astype(np.int64)
    order = rng.permutation(m * k)
    return start[order], end[order], slot[order], cell[order], vec, t0.astype(np.int32), offsets


def check_stage(gpu, args):
    got, want = gpu.tracks_device(*args), to.stage_voxels(*args)
    assert got["n_cells"].dtype == np.int32 and got["sums"].dtype == np.int64
    npt.assert_array_equal(got["n_cells"], want["n_cells"])
    npt.assert_array_equal(got["sums"], want["sums"])
    return got


@pytest.mark.parametrize("L1", [2, TILE - 1, TILE, TILE + 1, 3 * TILE + 17, TILE * TILE - 1, TILE * TILE, TILE * TILE + 1,
                                2 * TILE * TILE + 12345])
def test_scan_tile_boundaries(gpu, L1):
    L = L1 - 1
    m = max(1, min(L // 3, 40_000))
    check_stage(gpu, stage_case(L, seed=L1 % 1000, m=m))
    check_stage(gpu, stage_case(L, seed=7, m=1, rows_per_object=min(4 * L, 50_000)))     # one object over every tile


def test_one_giant_object(gpu):
    """65,536 cells, four rows each, all in one object of 200 days: every atomic of the scatter lands on 201 entries"""
    C, k, D = 65_536, 4, 200
    rng = np.random.default_rng(11)
    s = rng.integers(0, D, (C, k))
    e = np.minimum(s + rng.integers(0, 60, (C, k)), D - 1)
    s[:, 0], e[:, 1] = 0, D - 1
    start, end = (s.reshape(-1) + 77).astype(np.int32), (e.reshape(-1) + 77).astype(np.int32)
    slot = np.zeros(C * k, dtype=np.int32)
    cell = np.repeat(np.arange(C, dtype=np.int32), k)
    # the extremes of mhw_tracks(): weights of 2**31 - 1 and moments of 2**(mb + 20) with mb = 61 - 20 - bit_length(C),
    # one sign: with every cell present the sums reach C * 2**(mb + 20) = 2**60
    mb = 61 - 20 - C.bit_length()
    vec = np.stack([np.full(C, (1 << 31) - 1), np.full(C, 1 << (mb + 20)), np.full(C, -(1 << (mb + 20))),
                    np.full(C, (1 << (mb + 20)) - 1)]).astype(np.int64)
    args = (start, end, slot, cell, vec, np.array([77], np.int32), np.array([0, D], np.int64))
    got = check_stage(gpu, args)
    assert got["n_cells"].max() > C // 2 and np.abs(got["sums"]).max() > 1 << 58
    again = gpu.tracks_device(*args)
    npt.assert_array_equal(again["n_cells"], got["n_cells"])
    npt.assert_array_equal(again["sums"], got["sums"])


def test_extreme_values_on_the_largest_case(gpu):
    """the no-overflow claim where the scan is deepest: 2**31 - 1 area weights and moments of 2**(mb + 20) of one sign,
    mb = 61 - 20 - bit_length(C)"""
    C = 500
    top = 1 << (61 - C.bit_length())
    L = 2 * TILE * TILE + 999
    args = stage_case(L, seed=3, m=30_000, C=C, vmax=((1 << 31) - 1, top, top, top), same_sign=True)
    args[4][:, :] = np.array([(1 << 31) - 1, top, -top, top - 1])[:, None]
    got = check_stage(gpu, args)
    again = gpu.tracks_device(*args)                              # a second run: bit-identical
    npt.assert_array_equal(again["n_cells"], got["n_cells"])
    npt.assert_array_equal(again["sums"], got["sums"])


def test_refused_without_a_launch(gpu):
    from xmhw_amd._lib import hip
    h = hip()
    big = 1 << 31
    for kw in (dict(n=big), dict(n_slots=big), dict(L=big - 1)):                   # XMHW_ERR_UNSUPPORTED, null pointers and all
        a = dict(n=1, n_slots=1, L=1)
        a.update(kw)
        with pytest.raises(h.HipError, match=r"\(code 3\)"):
            h.object_tracks(0, 0, a["n"], 0, 0, 1, 0, 1, 0, 0, a["n_slots"], a["L"], 0, 0, a["L"] + 1, 0)
    for kw in (dict(n=-1), dict(n_slots=-1), dict(L=-1), dict(C=-1)):
        a = dict(n=1, n_slots=1, L=1, C=1)
        a.update(kw)
        with pytest.raises(h.InvalidArgument):
            h.object_tracks(0, 0, a["n"], 0, 0, a["C"], 0, 1, 0, 0, a["n_slots"], a["L"], 0, 0, 2, 0)
    with pytest.raises(h.InvalidArgument):                        # null buffers
        h.object_tracks(0, 0, 1, 0, 0, 1, 0, 1, 0, 0, 1, 1, 0, 0, 2, 0)
    from xmhw_amd.device import DeviceBuffer
    bufs = [DeviceBuffer(64) for _ in range(3)]
    try:
        with pytest.raises(h.InvalidArgument):                    # outputs given, inputs null
            h.object_tracks(0, 0, 1, 0, 0, 1, 0, 1, 0, 0, 1, 1, bufs[0].ptr, bufs[1].ptr, 2, bufs[2].ptr)
        with pytest.raises(h.InvalidArgument):                    # ld < L + 1
            h.object_tracks(0, 0, 1, 0, 0, 1, 0, 1, 0, 0, 1, 1, bufs[0].ptr, bufs[1].ptr, 1, bufs[2].ptr)
    finally:
        for b in bufs:
            b.free()
    with pytest.raises(gpu.XmhwException, match="ids="):
        gpu.tracks_device(np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(1, np.int32),
                          np.zeros((4, 1), np.int64), np.zeros(1, np.int32), np.array([0, (1 << 31) - 1], np.int64))


def test_rows_that_do_not_fit_are_counted_not_written(gpu):
    args = list(stage_case(5000, seed=1, m=20))
    args[0] = args[0].copy()
    row = int(np.nonzero(args[2] == 3)[0][0])
    args[0][row] -= 10_000                                        # starts long before its object
    with pytest.raises(gpu.XmhwException, match="do not lie within"):
        gpu.tracks_device(*args)


@pytest.mark.parametrize("seed", range(8))
def test_random_grids(gpu, seed):
    import xmhw_amd
    ds = oc.random_grid(seed)
    for connectivity, periodic, weights in ((6, None, "coslat"), (26, "lon", None)):
        obj = xmhw_amd.mhw_objects(ds, connectivity=connectivity, periodic=periodic, weights=weights)
        tr = xmhw_amd.mhw_tracks(ds, obj, weights=weights)
        to.same_as_dense(tr, to.tracks_dense(ds, obj, None, weights))
        npt.assert_array_equal(np.add.reduceat(tr.n_cells.astype(np.int64), tr.offsets[:-1]), obj.cell_days)
        npt.assert_array_equal(np.add.reduceat(tr.area_q, tr.offsets[:-1]), obj.area_days_q)
        ids = np.arange(obj.n_objects)[::-1][::3]
        to.same_as_dense(xmhw_amd.mhw_tracks(ds, obj, ids=ids, weights=weights), to.tracks_dense(ds, obj, ids, weights))


@pytest.mark.parametrize("key", list(oc.GOLDEN_COUNTS))
def test_golden_tables(gpu, key):
    import xmhw_amd
    connectivity, periodic = key
    ds = oc.golden_dataset()
    obj = xmhw_amd.mhw_objects(ds, connectivity=connectivity, periodic=periodic, weights="coslat")
    tr = xmhw_amd.mhw_tracks(ds, obj, weights="coslat")
    npt.assert_array_equal(np.add.reduceat(tr.n_cells.astype(np.int64), tr.offsets[:-1]), obj.cell_days)
    npt.assert_array_equal(np.add.reduceat(tr.area_q, tr.offsets[:-1]), obj.area_days_q)
    host = xmhw_amd.mhw_tracks(ds, obj, weights="coslat", _compute=to.stage_voxels)
    for k in ("n_cells", "area_q", "mx", "my", "mz", "lat", "lon", "area_max_q", "pos_area_max", "path_km"):
        npt.assert_array_equal(getattr(tr, k), getattr(host, k), err_msg=k)
    big = np.argsort(obj.n_events)[::-1][:6]
    to.same_as_dense(xmhw_amd.mhw_tracks(ds, obj, ids=big, weights="coslat"), to.tracks_dense(ds, obj, big, "coslat"))


def test_no_events_touches_nothing(gpu):
    import xmhw_amd
    ds = oc.dataset((2, 3), np.ones(6, bool), [[] for _ in range(6)], T=10)
    tr = xmhw_amd.mhw_tracks(ds, xmhw_amd.mhw_objects(ds))
    assert tr.n_selected == 0 and tr.n_cells.shape == (0,)
