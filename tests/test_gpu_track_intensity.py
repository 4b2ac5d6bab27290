"""mhw_track_intensity() on the device (csrc/kernels_track_intensity.hip): the stage against the voxel-by-voxel oracle
(tests/track_intensity_oracle.py) and the public function against the same oracle on compact arrays; every integer and
every maximum compared with assert_array_equal.

The kernel works on blocks of 256 cells (waves of 64) x chunks of CHUNK = 64 steps (XMHW_TRACK_INTENSITY_CHUNK); the
geometry cases put T on both sides of a chunk boundary, use a cell count that is no multiple of 64 and rows that start on
a chunk's first step and end on its last."""
import math

import numpy as np
import numpy.testing as npt
import pytest

import coverage_cases as cc
import objects_cases as oc
import track_intensity_cases as tc
import track_intensity_oracle as tio

pytestmark = pytest.mark.gpu
CHUNK = 64


@pytest.fixture(scope="module")
def gpu():
    from xmhw_amd._lib import hip, require_gpu
    require_gpu()
    from xmhw_amd import track_intensity
    assert hip().TRACK_INTENSITY_CHUNK == CHUNK and hip().TRACK_INTENSITY_BITS == track_intensity.INTENSITY_BITS == 16
    return track_intensity


def random_wi(C, ib, seed=5):
    rng = np.random.default_rng(seed)
    wi = rng.integers(0, (1 << ib) + 1, C).astype(np.int64)
    wi[rng.random(C) < 0.05] = 0
    wi[rng.random(C) < 0.05] = 1 << ib
    return wi


def detected(d, ny, nx, joinGaps=True, cold=False):
    """the device detection of a coverage_cases.synthetic() series as an EventDataset on a (ny, nx) grid"""
    from xmhw_amd.detect_front import detect_cells
    r = detect_cells(d["ts"], d["seas"], d["thresh"], d["doy"], d["doys"], 5, joinGaps, 2, cold)
    return tc.event_dataset(r["table"], r["offsets"], d["ts"].shape[0], ny, nx)


def check_stage(gpu, d, rows, wi, cold=False, **kw):
    args = (d["ts"], d["seas"], d["thresh"], d["doy"], d["doys"], rows, wi, cold)
    got, want = gpu.track_intensity_cells(*args, **kw), tio.stage_voxels(*args)
    assert got["n_range"] == 0 and got["n_bad"] == 0 and want["n_range"] == 0
    tio.same_integers(got, want)
    return got


STAGE_CASES = {"f32": dict(), "f64_366_rows": dict(dtype=np.float64, D=366), "nan": dict(nan_frac=0.05),
               "cold": dict(cold=True), "no_join": dict(joinGaps=False)}


@pytest.mark.parametrize("name", list(STAGE_CASES))
def test_stage_against_the_oracle(gpu, name):
    kw = dict(STAGE_CASES[name])
    joinGaps = kw.pop("joinGaps", True)
    ny, nx, T = 40, 50, 1500
    d = cc.synthetic(T, ny * nx, **{"dtype": np.float32, "seed": 21, **kw})
    cold = kw.get("cold", False)
    mhw = detected(d, ny, nx, joinGaps, cold)
    rng = np.random.default_rng(1)
    obj, tr, rows = tc.selection(mhw)
    ids = rng.permutation(obj.n_objects)[: max(1, (2 * obj.n_objects) // 3)]       # a shuffled part: some rows unselected
    obj, tr, rows = tc.selection(mhw, ids=ids)
    assert mhw.n_events > 2000 and (rows.slot < 0).any()
    got = check_stage(gpu, d, rows, random_wi(ny * nx, gpu.intensity_bits(obj.weight_bits, ny * nx)), cold)
    assert (got["cat_cells"].sum(axis=1) > 0).all() and got["n_valid"].sum() > 50_000
    # the identities that tie the series to mhw_tracks()
    assert (got["n_valid"] <= tr.n_cells).all() and (got["cat_cells"].sum(axis=0) <= got["n_valid"]).all()
    if name == "nan":
        assert (got["n_valid"] < tr.n_cells).any()
    if name == "no_join":                                          # no NaN and no joined gap: every voxel has a value
        npt.assert_array_equal(got["n_valid"], tr.n_cells)
    if name == "f32":                                              # one set of atomics per voxel: the same bits
        from xmhw_amd._lib import hip
        hip().set_track_intensity_combine(0)
        try:
            tio.same_integers(gpu.track_intensity_cells(d["ts"], d["seas"], d["thresh"], d["doy"], d["doys"], rows,
                                                        random_wi(ny * nx, gpu.intensity_bits(obj.weight_bits, ny * nx))), got)
        finally:
            hip().set_track_intensity_combine(1)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_peak_equals_the_objects_maximum_and_cumulative_within_the_rounding(gpu, dtype):
    """intensity_peak and obj.intensity_max are maxima of the same float64 expression, x - seas: equal bit for bit.  With
    unit weights and no NaN, sum_t isum_q / 2**(16 + ib) of an object is the sum of rint(a * 2**16) / 2**16 over its
    voxels and the sum of its rows' intensity_cumulative is the sum of a: every voxel differs by at most 2**-17, hence
    cell_days * 2**-17; a row's own float64 running sum of d terms below 2**7 adds at most d * d * 2**7 * 2**-53."""
    ny, nx, T = 20, 30, 800
    d = cc.synthetic(T, ny * nx, dtype, seed=4)
    mhw = detected(d, ny, nx)
    obj, tr, rows = tc.selection(mhw)
    ib = gpu.intensity_bits(obj.weight_bits, ny * nx)
    got = check_stage(gpu, d, rows, np.full(ny * nx, 1 << ib, dtype=np.int64))
    first = tr.offsets[:-1]
    peak = np.fmax.reduceat(got["intensity_max"], first)
    npt.assert_array_equal(peak, obj.intensity_max)
    cum = mhw.table[:, mhw.columns.index("intensity_cumulative")]
    dur = mhw.table[:, mhw.columns.index("duration")]
    for o in range(obj.n_objects):
        mine = np.asarray(obj.object) == o
        total = sum(int(v) for v in got["isum_q"][tr.offsets[o]:tr.offsets[o + 1]])
        tol = int(obj.cell_days[o]) * 2.0 ** -17 + float((dur[mine] ** 2).sum()) * 2.0 ** -46
        assert abs(total / 2.0 ** (16 + ib) - math.fsum(cum[mine])) <= tol, o


def geometry_case(T, seed):
    """150 cells (10 x 15: two whole waves and a part), T steps: random rows, rows that fill a chunk exactly, a cell
    without rows (0) and an isolated cell (32) whose rows belong to objects that are left out"""
    rng = np.random.default_rng(seed)
    ny, nx = 10, 15
    C = ny * nx
    per_cell = [oc.random_intervals(rng, T, 6) for _ in range(C)]
    for c in range(3, C, 7):                                       # rows from a chunk's first step to its last
        k = int(rng.integers(0, max(1, T // CHUNK)))
        per_cell[c] = [(k * CHUNK, min((k + 1) * CHUNK, T) - 1)]
    lonely = 2 * nx + 2
    for c in (0, lonely - 1, lonely + 1, lonely - nx, lonely + nx):
        per_cell[c] = []
    per_cell[lonely] = [(1, min(5, T - 1))] + ([(CHUNK - 2, min(CHUNK + 3, T - 1))] if T > CHUNK else [])
    mhw = oc.dataset((ny, nx), np.ones(C, bool), per_cell, T=T)
    seas = 10.0 + rng.normal(size=(37, C))
    thresh = seas + rng.uniform(0.2, 0.9, size=(37, C))
    doys = np.arange(1, 38)
    doy = doys[np.arange(T) % 37]
    ts = (seas[np.arange(T) % 37] + rng.normal(scale=1.5, size=(T, C))).astype(np.float32)
    ts[rng.random((T, C)) < 0.03] = np.nan
    return mhw, dict(ts=ts, seas=seas, thresh=thresh, doy=doy, doys=doys), lonely


@pytest.mark.parametrize("T", [CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 17])
def test_chunk_geometry(gpu, T):
    import xmhw_amd
    mhw, d, lonely = geometry_case(T, seed=T)
    obj = xmhw_amd.mhw_objects(mhw)
    r0, r1 = int(mhw.offsets[lonely]), int(mhw.offsets[lonely + 1])
    out = np.unique(np.asarray(obj.object)[r0:r1])
    ids = np.setdiff1d(np.arange(obj.n_objects), out)[::-1]
    obj, tr, rows = tc.selection(mhw, ids=ids)
    assert r1 > r0 and (rows.slot[r0:r1] < 0).all() and mhw.offsets[1] == 0
    got = check_stage(gpu, d, rows, random_wi(150, gpu.intensity_bits(obj.weight_bits, 150)))
    assert got["n_valid"].sum() > 100
    tio.same_integers(check_stage(gpu, d, rows, random_wi(150, gpu.intensity_bits(obj.weight_bits, 150)),
                                  max_batch_bytes=70 * (T * 4 + 2 * 37 * 8 + 64)), got)        # three batches of cells


def test_one_giant_object(gpu):
    """every row of 16,384 cells x 200 days in one object at the extreme weights (wi = 2**ib) and anomalies just under
    2**7: every atomic lands on 200 entries and the sums reach 2**60"""
    import xmhw_amd
    ny = nx = 128
    C, T = ny * nx, 200
    mhw = oc.dataset((ny, nx), np.ones(C, bool), [[(0, T - 1)] for _ in range(C)], T=T)
    obj, tr, rows = tc.selection(mhw)
    assert obj.n_objects == 1 and tr.offsets[-1] == T
    ib = gpu.intensity_bits(obj.weight_bits, C)
    assert ib == 61 - 16 - 7 - C.bit_length()
    rng = np.random.default_rng(0)
    seas = rng.normal(size=(1, C))
    ts = 127.99 - rng.random((T, C)) * 0.01
    ts[:, ::2] *= -1.0                                             # half of the cells at the other end: both signs meet
    ts += seas
    ts[rng.random((T, C)) < 0.001] = np.nan
    ts[5] = seas[0] + 127.9                                        # one sign on a few days
    ts[6] = seas[0] - 127.9
    d = dict(ts=ts, seas=seas, thresh=seas + 1.0, doy=np.zeros(T, np.int64), doys=np.zeros(1, np.int64))
    got = check_stage(gpu, d, rows, np.full(C, 1 << ib, dtype=np.int64))
    assert np.abs(got["isum_q"]).max() > 1 << 57
    again = gpu.track_intensity_cells(d["ts"], d["seas"], d["thresh"], d["doy"], d["doys"], rows, np.full(C, 1 << ib, np.int64))
    tio.same_integers(again, got)


def public_case(T=800, ny=12, nx=17, seed=2, **kw):
    import xmhw_amd
    g = tc.calendar_grid(T, ny, nx, seed=seed, nan_frac=0.02, **kw)
    mhw = xmhw_amd.detect(g["temp"], g["th"], g["se"])
    return g, mhw


def oracle_of(g, mhw, obj, tr, weights):
    """the dense oracle on the compact arrays of the grid, with weights quantised here"""
    import tracks_oracle as to
    from xmhw_amd.track_intensity import selection_rows
    keep = g["keep"]
    C = int(keep.sum())
    ib = min(int(obj.weight_bits), 61 - 16 - 7 - C.bit_length())
    w = to.grid_weights(mhw, weights)
    wi = np.rint(w / w.max() * 2.0 ** ib).astype(np.int64)[keep]
    return tio.stage_voxels(g["ts"][:, keep], g["seas"][:, keep], g["thresh"][:, keep], g["doy"], g["doys"],
                            selection_rows(mhw, obj, tr), wi)


def test_public_function_with_land_and_shuffled_ids(gpu):
    import xmhw_amd
    g, mhw = public_case()
    npt.assert_array_equal(mhw.keep, g["keep"])
    obj = xmhw_amd.mhw_objects(mhw, weights="coslat")
    ids = np.random.default_rng(9).permutation(obj.n_objects)[: obj.n_objects - 3]
    tr = xmhw_amd.mhw_tracks(mhw, obj, ids=ids, weights="coslat")
    got = xmhw_amd.mhw_track_intensity(g["temp"], g["th"], g["se"], mhw, obj, tr, weights="coslat")
    assert got.ids is tr.ids and got.offsets is tr.offsets and obj.n_objects > 10
    tio.same_integers(got, oracle_of(g, mhw, obj, tr, "coslat"))
    assert (got.n_valid <= tr.n_cells).all() and (got.cat_cells.sum(axis=0) <= got.n_valid).all()
    # refusals that need the device path
    with pytest.raises(xmhw_amd.XmhwException, match="weights"):
        xmhw_amd.mhw_track_intensity(g["temp"], g["th"], g["se"], mhw, obj, xmhw_amd.mhw_tracks(mhw, obj), weights="coslat")
    hot = g["temp"].values.copy()
    row = int(np.nonzero(np.asarray(obj.object) == ids[0])[0][0])
    cell = int(np.searchsorted(mhw.offsets, row, side="right") - 1)
    hot.reshape(hot.shape[0], -1)[int(mhw.table[row, 1]), mhw.cell_index[cell]] += 200.0
    with pytest.raises(xmhw_amd.XmhwException, match="anomaly"):
        xmhw_amd.mhw_track_intensity(xmhw_amd.GridSeries(hot, g["temp"].dims, g["temp"].coords), g["th"], g["se"], mhw, obj, tr,
                                     weights="coslat")


def test_slabs_do_not_change_a_bit(gpu, monkeypatch):
    import xmhw_amd
    g, mhw = public_case(seed=5)
    obj = xmhw_amd.mhw_objects(mhw)
    tr = xmhw_amd.mhw_tracks(mhw, obj)
    calls = []
    add_slab = gpu._Accumulators.add_slab
    monkeypatch.setattr(gpu._Accumulators, "add_slab", lambda self, *a, **k: (calls.append(a[0].n), add_slab(self, *a, **k))[1])
    one = xmhw_amd.mhw_track_intensity(g["temp"], g["th"], g["se"], mhw, obj, tr)
    assert len(calls) == 1
    many = xmhw_amd.mhw_track_intensity(g["temp"], g["th"], g["se"], mhw, obj, tr, max_batch_bytes=2_000_000)
    assert len(calls) - 1 >= 3 and sum(calls[1:]) == calls[0]
    tio.same_integers(many, one)
    tio.same_integers(xmhw_amd.mhw_track_intensity(g["temp"], g["th"], g["se"], mhw, obj, tr), one)
    tio.same_integers(one, oracle_of(g, mhw, obj, tr, None))
    for k in ("intensity_mean", "intensity_cumulative", "intensity_peak", "pos_peak"):
        npt.assert_array_equal(getattr(many, k), getattr(one, k), err_msg=k)


def test_golden_tables(gpu):
    """the 108 reference series on the 9 x 12 grid of objects_cases.golden_dataset().  Their climatologies are expanded
    along time (one row per step) and their lengths differ, which the doy-labelled public function cannot take: the
    series are padded with NaN to the longest and go through the stage entry with one climatology row per step."""
    mhw = oc.golden_dataset()
    series = [(x, se, th) for x, se, th, _, _, _ in cc.golden_series()]
    T = max(x.shape[0] for x, _, _ in series)                      # the series run past the last event's end
    assert len(series) == 108 and T >= np.asarray(mhw.time).shape[0]
    ts, seas, thresh = (np.full((T, 108), np.nan) for _ in range(3))
    for c, (x, se, th) in enumerate(series):
        ts[:x.shape[0], c], seas[:x.shape[0], c], thresh[:x.shape[0], c] = x, se, th
    d = dict(ts=ts, seas=seas, thresh=thresh, doy=np.arange(T), doys=np.arange(T))
    obj, tr, rows = tc.selection(mhw, weights="coslat")
    ids = np.random.default_rng(3).permutation(obj.n_objects)
    obj, tr, rows = tc.selection(mhw, ids=ids, weights="coslat")
    got = check_stage(gpu, d, rows, random_wi(108, gpu.intensity_bits(obj.weight_bits, 108)))
    npt.assert_array_equal(np.fmax.reduceat(got["intensity_max"], tr.offsets[:-1]), obj.intensity_max[ids])
    assert (got["n_valid"] <= tr.n_cells).all() and got["n_valid"].sum() > 10_000


def test_refused_without_a_launch(gpu):
    from xmhw_amd._lib import hip
    h = hip()
    big = 1 << 31
    with pytest.raises(h.HipError, match=r"\(code 3\)"):
        h.track_intensity_init(big, 0, 0, 0, 0, 0, big, 0, 0)
    with pytest.raises(h.HipError, match=r"\(code 3\)"):
        h.track_intensity_finish(big, 0)
    for kw in (dict(n=big), dict(n_rows=big), dict(n_slots=big), dict(L=big)):
        a = dict(n=1, n_rows=1, n_slots=1, L=1)
        a.update(kw)
        with pytest.raises(h.HipError, match=r"\(code 3\)"):
            h.track_intensity_accumulate(0, 4, 1, a["n"], a["n"], 0, 0, a["n"], 1, np.zeros(1, np.int32), 0, 0, 0, 0, a["n_rows"],
                                         0, 0, 0, 0, a["n_slots"], a["L"], 0, 0, 0, 0, 0, a["L"], 0, 0)
    with pytest.raises(h.InvalidArgument):                        # null buffers
        h.track_intensity_accumulate(0, 4, 1, 1, 1, 0, 0, 1, 1, np.zeros(1, np.int32), 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 1, 0, 0, 0,
                                     0, 0, 1, 0, 0)
    with pytest.raises(h.InvalidArgument):
        h.set_track_intensity_combine(2)
