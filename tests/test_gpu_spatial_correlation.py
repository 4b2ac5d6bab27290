"""spatial_correlation() on the device against tests/spatial_correlation_oracle.py: exact equality of the six arrays and
the counter.  The C entries are called raw, on pitched inputs (ld, ldb and ldo larger than ny * nx; the columns past the
grid hold valid samples in range) and outputs pre-filled with a bit pattern that must be gone inside the grid and intact
beyond it; every forced block length, both tile shapes and every offset grouping must give the same bits.  Then the
public function on a small periodic grid against the oracle, e-folding lengths included."""
import functools

import numpy as np
import numpy.testing as npt
import pytest

import spatial_correlation_cases as sc
import spatial_correlation_oracle as so

pytestmark = pytest.mark.gpu

EXTRA = 5                       # columns past ny * nx in every pitched array (ldb: one more, ldo: two more)
FILL32, FILL64 = -0x5A5A5A5B, -0x5A5A5A5A5A5A5A5B
FIELDS = so.FIELDS
DTYPES = {k: np.int32 if k == "n" else np.int64 for k in FIELDS}
GRIDS = ((1, 1), (1, 64), (3, 65), (5, 70), (9, 130), (37, 33))


@pytest.fixture(scope="module")
def dev():
    from xmhw_amd._lib import require_gpu
    require_gpu()
    import xmhw_amd.device as d
    return d


@pytest.fixture(autouse=True)
def automatic_afterwards():
    yield
    from xmhw_amd._lib import hip_spatialcorr
    hip_spatialcorr().set_spatial_corr_block(0)
    hip_spatialcorr().set_spatial_corr_tile(0)


@functools.lru_cache(maxsize=None)
def _case(T, ny, nx, dtype, seed, Dr=1, land="none"):
    ts, base, rows, sea = sc.field(T, ny, nx, np.dtype(dtype).type, seed, Dr=Dr, land=land)
    return {"ts": ts, "base": base, "rows": rows, "sea": sea, "ny": ny, "nx": nx}


def _offsets(D, nx, periodic):
    """sc.offsets(D); on a periodic grid the entries with |di| >= nx are folded into it (the entry refuses them)"""
    off = sc.offsets(D).copy()
    if periodic:
        wide = np.abs(off[:, 1]) >= nx
        off[wide, 1] = np.sign(off[wide, 1]) * (nx - 1)
    return off


@functools.lru_cache(maxsize=None)
def _want(T, ny, nx, dtype, seed, Dr, land, pattern, D, periodic, shift=0):
    d = _case(T, ny, nx, dtype, seed, Dr, land)
    classes, K = pattern(T)
    return so.spatial_corr_sums(d["ts"], d["base"], d["rows"], shift, classes, K, _offsets(D, nx, periodic), ny, nx, periodic)


def _pitched(a, ld, fill):
    out = np.full(a.shape[:-1] + (ld,), fill, dtype=a.dtype)
    out[..., :a.shape[-1]] = a
    return out


def buffers(dev, K, D, ny, nx):
    from xmhw_amd._lib import hip_spatialcorr
    ldo = ny * nx + EXTRA + 2
    b = {k: dev.DeviceBuffer.from_array(np.full((K, D, ldo), FILL32 if dt is np.int32 else FILL64, dt)) for k, dt in DTYPES.items()}
    b.update(cnt=dev.DeviceBuffer.from_array(np.full(1, 123, np.int64)), ldo=ldo, K=K, D=D, N=ny * nx)
    hip_spatialcorr().spatial_corr_init(K, D, ny, nx, *(b[k].ptr for k in FIELDS), ldo, b["cnt"].ptr)
    return b


def raw_accumulate(dev, d, classes, K, offsets, periodic, out, shift=0, block=0, tile=0, parts=None):
    """xmhw_spatial_corr_accumulate_* on the case into the buffers ``out``: the whole series in one call, or the
    consecutive blocks ``parts`` = [(t0, nt), ...] in one call each, one after the other on the stream without a
    read-back; the inputs are pitched by columns of valid samples in range"""
    from xmhw_amd._lib import hip, hip_spatialcorr
    m = hip_spatialcorr()
    ts = d["ts"]
    T, N = ts.shape
    ld, ldb = N + EXTRA, N + EXTRA + 1
    m.set_spatial_corr_block(block)
    m.set_spatial_corr_tile(tile)
    held = [dev.DeviceBuffer.from_array(_pitched(ts, ld, 21.0)), dev.DeviceBuffer.from_array(_pitched(d["base"], ldb, 20.0))]
    try:
        for t0, nt in parts or [(0, T)]:
            m.spatial_corr_accumulate(held[0].ptr + ts.dtype.itemsize * ld * t0, ts.dtype.itemsize, ld, t0, nt, T, d["ny"],
                                      d["nx"], int(periodic), held[1].ptr, ldb, d["base"].shape[0], d["rows"], shift, classes,
                                      K, offsets, *(out[k].ptr for k in FIELDS), out["ldo"], out["cnt"].ptr)
        hip().stream_sync(0)
    finally:
        for b in held:
            b.free()


def result(b):
    """read back, check the columns past the grid, free"""
    K, D, N, ldo = b["K"], b["D"], b["N"], b["ldo"]
    try:
        got = {k: b[k].to_array((K, D, ldo), dt) for k, dt in DTYPES.items()}
        cnt = b["cnt"].to_array((1,), np.int64)
    finally:
        for v in b.values():
            if hasattr(v, "free"):
                v.free()
    for k, a in got.items():
        assert (a[..., N:] == (FILL32 if a.dtype == np.int32 else FILL64)).all(), f"{k}: a column past the grid was touched"
    out = {k: a[..., :N] for k, a in got.items()}
    out["n_range"] = int(cnt[0])
    return out


def run_whole(dev, d, classes, K, offsets, periodic, **kw):
    b = buffers(dev, K, len(offsets), d["ny"], d["nx"])
    raw_accumulate(dev, d, classes, K, offsets, periodic, b, **kw)
    return result(b)


def same(got, want):
    for k in FIELDS:
        assert got[k].dtype == want[k].dtype, k
        npt.assert_array_equal(got[k], want[k], err_msg=k)
    assert got["n_range"] == want["n_range"]


@pytest.mark.parametrize("periodic", [False, True])
@pytest.mark.parametrize("grid", GRIDS)
def test_grids_that_cross_a_wave_a_tile_and_the_seam(dev, grid, periodic):
    """1 x 1, one wave, one point past a wave, more than two waves per row, rows past a tile with fewer than 64
    longitudes: 17 offsets of both signs with the cap (+-32, +-32), which is wider than most of these grids, under both
    tile shapes and two block settings"""
    ny, nx = grid
    T, dtype = 37, ("float32", "float64")[(ny + nx) % 2]
    d = _case(T, ny, nx, dtype, 100 + ny, land="island" if ny * nx > 9 else "none")
    classes, K = sc.every_step(T)
    off = _offsets(17, nx, periodic)
    want = _want(T, ny, nx, dtype, 100 + ny, 1, "island" if ny * nx > 9 else "none", sc.every_step, 17, periodic)
    assert want["n"][:, 0].sum() > 0 and (ny * nx == 1 or want["n_range"] > 0)
    if ny * nx > 64:
        assert all((want[k][:, 1:] != 0).any() for k in FIELDS)
    for tile in (4, 8):
        for block in (0, 7):
            same(run_whole(dev, d, classes, K, off, periodic, block=block, tile=tile), want)


def test_a_grid_narrower_than_the_offsets_and_a_seam_one_column_wider(dev):
    """without a seam nx = 20 lies below |di| = 32: those partners are off the grid, n = 0; with a seam nx = 33 = |di| + 1:
    the partner at +32 is the neighbour at -1"""
    classes, K = sc.one_class(37)
    d = _case(37, 4, 20, "float32", 5)
    off = sc.offsets(17)
    want = so.spatial_corr_sums(d["ts"], d["base"], d["rows"], 0, classes, K, off, 4, 20, False)
    wide = np.abs(off[:, 1]) == 32
    assert wide.sum() >= 6 and (want["n"][:, wide] == 0).all() and (want["n"][:, ~wide] > 0).any()
    same(run_whole(dev, d, classes, K, off, False), want)
    d = _case(37, 3, 33, "float64", 6)
    off = np.array([(0, 0), (0, 32), (0, -1), (0, -32), (0, 1), (2, 32), (-2, -32)], np.int32)
    want = so.spatial_corr_sums(d["ts"], d["base"], d["rows"], 0, classes, K, off, 3, 33, True)
    for k in FIELDS:
        npt.assert_array_equal(want[k][:, 1], want[k][:, 2])            # +32 is -1 across the seam, -32 is +1
        npt.assert_array_equal(want[k][:, 3], want[k][:, 4])
    assert want["n"][:, 5].sum() > 0
    for tile in (4, 8):
        same(run_whole(dev, d, classes, K, off, True, tile=tile), want)


@pytest.mark.parametrize("periodic", [False, True])
@pytest.mark.parametrize("land", sc.LANDS)
def test_land(dev, land, periodic):
    """none, an island, a whole land row and a whole land column on the seam, all land; 5 % scattered NaN on top"""
    T, ny, nx = 37, 9, 130
    d = _case(T, ny, nx, "float32", 21, land=land)
    classes, K = sc.with_minus_one(T)
    want = _want(T, ny, nx, "float32", 21, 1, land, sc.with_minus_one, 9, periodic)
    assert (want["n"][..., ~d["sea"]] == 0).all() and (np.isnan(d["ts"]).mean() > 0.04)
    if land == "all":
        assert all((want[k] == 0).all() for k in FIELDS) and want["n_range"] == 0
    else:
        assert all((want[k] != 0).any() for k in FIELDS) and want["n_range"] > 0
    same(run_whole(dev, d, classes, K, _offsets(9, nx, periodic), periodic), want)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("T", [1, 37, 300])
def test_steps_and_forced_blocks_give_identical_bits(dev, T, dtype):
    """blocks of 1, 7 and 64 steps, longer than the series, and automatic: nothing is counted twice, n_range included"""
    ny, nx = 5, 70
    d = _case(T, ny, nx, dtype, 7)
    off = _offsets(9, nx, True)
    for pattern in (sc.one_class, sc.with_minus_one):
        classes, K = pattern(T)
        want = _want(T, ny, nx, dtype, 7, 1, "none", pattern, 9, True)
        if (classes >= 0).any():
            assert want["n"].sum() > 0
        if T > 1 and pattern is sc.one_class:
            assert want["n_range"] >= 4
        for block in (1, 7, 64, 10 ** 6, 0):
            same(run_whole(dev, d, classes, K, off, True, block=block), want)


@pytest.mark.parametrize("pattern", sc.PATTERNS)
def test_classes(dev, pattern):
    """one class; labels that change every step; labels with -1; K = 64"""
    T, ny, nx = 300, 3, 65
    d = _case(T, ny, nx, "float32", 31)
    classes, K = pattern(T)
    want = _want(T, ny, nx, "float32", 31, 1, "none", pattern, 8, False)
    assert (want["n"][:, 0].reshape(K, -1).sum(axis=1) > 0).all()
    for block in (0, 64):
        same(run_whole(dev, d, classes, K, _offsets(8, nx, False), False, block=block), want)


@pytest.mark.parametrize("D", [1, 8, 9, 17, 64])
def test_offset_counts_across_the_group_boundaries(dev, D):
    """only (0, 0); one group of 8; nine offsets in one group of 16; 17 in two; 64 in four -- n_range is that of the grid
    under every list"""
    T, ny, nx = 37, 37, 70
    d = _case(T, ny, nx, "float64", 41, land="island")
    classes, K = sc.every_step(T)
    for periodic in (False, True):
        want = _want(T, ny, nx, "float64", 41, 1, "island", sc.every_step, D, periodic)
        assert want["n_range"] == _want(T, ny, nx, "float64", 41, 1, "island", sc.every_step, 1, periodic)["n_range"] > 0
        if D >= 9:
            assert (want["n"][:, 8] > 0).any()                           # the cap (32, 32) has partners on 37 x 70, with a seam or without
        if D >= 8:
            npt.assert_array_equal(want["sxy"][:, 7], want["sxy"][:, 1])  # the duplicate
        for tile in (4, 8):
            same(run_whole(dev, d, classes, K, _offsets(D, nx, periodic), periodic, tile=tile, block=(0, 7)[tile == 8]), want)


@pytest.mark.parametrize("Dr", [1, 366])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_types_and_base_rows(dev, dtype, Dr):
    T, ny, nx = 300, 5, 70
    d = _case(T, ny, nx, dtype, 51, Dr=Dr, land="lines")
    assert d["base"].shape[0] == Dr and (Dr == 1 or (np.diff(d["rows"]) < 0).any())
    classes, K = sc.with_minus_one(T)
    for periodic in (False, True):
        want = _want(T, ny, nx, dtype, 51, Dr, "lines", sc.with_minus_one, 17, periodic)
        assert all((want[k] != 0).any() for k in FIELDS)
        same(run_whole(dev, d, classes, K, _offsets(17, nx, periodic), periodic, block=(0, 64)[periodic]), want)


def test_a_shift_brings_large_samples_into_range(dev):
    """out-of-range and infinite samples are counted once, by their own point, and are no partner either: with shift 3
    the finite ones of them are samples"""
    T, ny, nx = 37, 5, 70
    d = _case(T, ny, nx, "float64", 61)
    classes, K = sc.one_class(T)
    off = _offsets(9, nx, False)
    w0, w3 = (so.spatial_corr_sums(d["ts"], d["base"], d["rows"], s, classes, K, off, ny, nx, False) for s in (0, 3))
    assert w0["n_range"] == 5 and w3["n_range"] == 2                    # what the case spoils; the two infinities stay
    p = 2                                                               # the point exactly 2**7 above its base ...
    t = 2
    assert w3["n"][0, 0, p] == w0["n"][0, 0, p] + 1
    q = p + 1                                                           # ... is the partner at (0, -1) of its neighbour
    e = [tuple(v) for v in off.tolist()].index((0, -1))
    assert w3["n"][0, e, q] == w0["n"][0, e, q] + (1 if not np.isnan(d["ts"][t, q]) else 0)
    for shift, want in ((0, w0), (3, w3)):
        for block in (0, 1):
            same(run_whole(dev, d, classes, K, off, False, shift=shift, block=block), want)


@pytest.mark.parametrize("periodic", [False, True])
def test_mirror_identity(dev, periodic):
    """e and -e in one call: the sums of -e at p are those of +e at p - e with x and y exchanged"""
    from xmhw_amd.spatial_correlation import shift_back
    T, ny, nx = 37, 9, 130
    d = _case(T, ny, nx, "float32", 71, land="lines")
    classes, K = sc.every_step(T)
    es = [(0, 1), (1, 0), (2, -3), (8, 8), (32, 32), (8, -32), (0, 32), (1, -1)]      # (32, 32) leaves 9 rows: zeros both ways
    off = np.array([v for e in es for v in (e, (-e[0], -e[1]))], np.int32)
    got = run_whole(dev, d, classes, K, off, periodic)
    grid = {k: got[k].reshape(K, len(off), ny, nx) for k in FIELDS}
    for i, (dj, di) in enumerate(es):
        assert (grid["n"][:, 2 * i].sum() > 0) == (dj < ny)
        for k, other in zip(FIELDS, ("n", "sy", "sx", "syy", "sxx", "sxy")):
            npt.assert_array_equal(grid[k][:, 2 * i + 1], shift_back(grid[other][:, 2 * i], dj, di, periodic), err_msg=f"{k} {dj} {di}")
    same(got, so.spatial_corr_sums(d["ts"], d["base"], d["rows"], 0, classes, K, off, ny, nx, periodic))


def test_two_accumulate_calls_on_consecutive_blocks_equal_one(dev):
    T, ny, nx = 300, 5, 70
    d = _case(T, ny, nx, "float32", 81, Dr=366)
    classes, K = sc.with_minus_one(T)
    off = _offsets(17, nx, True)
    want = _want(T, ny, nx, "float32", 81, 366, "none", sc.with_minus_one, 17, True)
    for parts in ([(0, 113), (113, 187)], [(0, 1), (1, 298), (299, 1)]):
        b = buffers(dev, K, len(off), ny, nx)
        raw_accumulate(dev, d, classes, K, off, True, b, parts=parts, block=64)
        same(result(b), want)


def test_public_function_on_a_small_periodic_grid(dev):
    """spatial_correlation() end to end: the device runs (0, 0) and the half-plane in time blocks of 50 steps, the host
    fills the mirror; the integers equal the oracle run on the whole request, and so do the lengths derived from them"""
    import xmhw_amd
    from xmhw_amd import GridSeries
    T, ny, nx = 120, 6, 40
    ts, base, rows, sea = sc.field(T, ny, nx, np.float32, 91, land="island", spoil=False)
    time = np.datetime64("2003-01-01") + np.arange(T).astype("timedelta64[D]")
    coords = {"time": time, "lat": -3.0 + 1.0 * np.arange(ny), "lon": 9.0 * np.arange(nx)}
    x = GridSeries(ts.reshape(T, ny, nx), ("time", "lat", "lon"), coords)
    got = xmhw_amd.spatial_correlation(x, base=base.reshape(ny, nx), classes="month", periodic="lon", block_steps=50)
    request = got.offset
    assert request.shape == (25, 2) and got.klass.tolist() == [1, 2, 3, 4]
    kid = (time.astype("datetime64[M]").astype(int) % 12).astype(np.int32)
    want = so.spatial_corr_sums(ts, base, rows, 0, kid, 4, request, ny, nx, True)
    for k in FIELDS:
        npt.assert_array_equal(getattr(got, k).reshape(4, 25, ny * nx), want[k], err_msg=k)
    ref = xmhw_amd.SpatialCorrelationDataset(got.klass, request, *(want[k].reshape(4, 25, ny, nx) for k in FIELDS),
                                             sea.reshape(ny, nx), ("lat", "lon"), coords, coords["lat"], 9.0, 0, True)
    for axis in ("zonal", "meridional"):
        L = got.efolding_length(axis)
        npt.assert_array_equal(L, ref.efolding_length(axis))
        assert np.isfinite(L[:, sea.reshape(ny, nx)]).any() and np.isnan(L[:, ~sea.reshape(ny, nx)]).all()
    npt.assert_array_equal(got.r, ref.r)
    # a sample out of range is refused in the words of the pattern
    ts[5, 7] = 500.0
    with pytest.raises(xmhw_amd.XmhwException, match=r"^1 samples of x lie 2\*\*\(7 \+ shift\) and more .* shift = 0"):
        xmhw_amd.spatial_correlation(GridSeries(ts.reshape(T, ny, nx), ("time", "lat", "lon"), coords), base=base.reshape(ny, nx),
                                     reach=(1, 1))
