"""regrid() on the device against tests/regrid_oracle.py, bit for bit: the output as unsigned views with NaN positions
equal, wsum, n and n_range as integers.  The C entries are called raw, on pitched inputs (ld and ldo larger than the
grids; the columns past the destination grid pre-filled with a bit pattern that must be intact afterwards), over every
case of tests/regrid_cases.py; then a subset under both paths and three step chunks with identical bits (the path each
call took read back from xmhw_regrid_class), the nested cross-check against coarsen() on the device, the corners (the
range edge, infinities, the share threshold to the unit, the 2^59 corner, an all-empty table, no steps) and the public
function in time blocks."""
import functools

import numpy as np
import numpy.testing as npt
import pytest

import regrid_cases as rc
import regrid_oracle as ro

pytestmark = pytest.mark.gpu

FILL32, FILL64 = -0x5A5A5A5B, -0x5A5A5A5A5A5A5A5B
EXTRA = 5                       # columns of the outputs past my * mx
CASES = rc.listed()
SUBSET = rc.invariance_subset(CASES)
DIRECT, STAGED = 1, 2


@pytest.fixture(scope="module")
def dev():
    from xmhw_amd._lib import require_gpu
    require_gpu()
    import xmhw_amd.device as d
    return d


@pytest.fixture(autouse=True)
def automatic_afterwards():
    yield
    from xmhw_amd._lib import hip_regrid
    hip_regrid().set_regrid_variant(0)
    hip_regrid().set_regrid_chunk(0)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same_floats(got, want):
    """bit for bit, every NaN standing for every other"""
    npt.assert_array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    npt.assert_array_equal(bits(got)[ok], bits(want)[ok])


def raw(dev, field, ny, nx, rows, cols, periodic, x0, a, variant=0, chunk=0, want_sums=True):
    """xmhw_regrid_* on the host arrays: ``field`` (T, ld) pitched as it is.  Returns (out, wsum, n, n_range, the path
    the call took); the columns past my * mx of the outputs are checked to be untouched."""
    from xmhw_amd._lib import hip, hip_regrid
    m = hip_regrid()
    T, ld = field.shape
    isz = field.dtype.itemsize
    my, mx = len(rows[0]), len(cols[0])
    cells = my * mx
    ldo = cells + EXTRA
    d_ts = dev.DeviceBuffer.from_array(field.reshape(-1) if T else np.zeros(1, field.dtype))
    fill = np.float32(-7.25) if isz == 4 else np.float64(-7.25)
    rows_out = max(T, 1)
    d_out = dev.DeviceBuffer.from_array(np.full((rows_out, ldo), fill, field.dtype))
    d_ws = dev.DeviceBuffer.from_array(np.full((rows_out, ldo), FILL64, np.int64))
    d_n = dev.DeviceBuffer.from_array(np.full((rows_out, ldo), FILL32, np.int32))
    d_cnt = dev.DeviceBuffer.from_array(np.full(1, 123, np.int64))
    try:
        m.set_regrid_variant(variant)
        m.set_regrid_chunk(chunk)
        klass = m.regrid_class(nx, rows[1], cols[0], cols[1], periodic)
        m.regrid(d_ts.ptr, isz, T, ld, ny, nx, *rows, *cols, periodic, x0, a, d_out.ptr, ldo,
                 d_ws.ptr if want_sums else 0, d_n.ptr if want_sums else 0, d_cnt.ptr)
        hip().stream_sync(0)
        out, ws = d_out.to_array((rows_out, ldo), field.dtype), d_ws.to_array((rows_out, ldo), np.int64)
        n = d_n.to_array((rows_out, ldo), np.int32)
        cnt = int(d_cnt.to_array((1,), np.int64)[0]) - 123           # the counter is ADDED to
    finally:
        for b in (d_ts, d_out, d_ws, d_n, d_cnt):
            b.free()
    npt.assert_array_equal(out[:, cells:], fill)
    npt.assert_array_equal(ws[:, cells:], FILL64)
    npt.assert_array_equal(n[:, cells:], FILL32)
    if not want_sums:
        npt.assert_array_equal(ws, FILL64)
        npt.assert_array_equal(n, FILL32)
    if T == 0:
        npt.assert_array_equal(out, fill)
    return out[:T, :cells], ws[:T, :cells], n[:T, :cells], cnt, klass


def check(got, want):
    same_floats(got[0], want[0])
    npt.assert_array_equal(got[1], want[1])
    npt.assert_array_equal(got[2], want[2])
    assert got[3] == want[3]


@functools.lru_cache(maxsize=None)
def _inputs(c):
    return rc.tables(c) + (rc.make_data(c),)


@functools.lru_cache(maxsize=None)
def _want(c):
    ny, nx, rows, cols, field = _inputs(c)
    return ro.regrid_oracle(field, ny, nx, rows, cols, c.periodic, 0.0, c.a)


@pytest.mark.parametrize("c", CASES, ids=rc.case_id)
def test_raw_entry_equals_the_oracle(dev, c):
    ny, nx, rows, cols, field = _inputs(c)
    check(raw(dev, field, ny, nx, rows, cols, c.periodic, 0.0, c.a), _want(c))


def test_the_cases_bite():
    """what the list above compares is not trivial: invalid cells beside valid ones, cells without a sample, empty runs,
    runs that cross the seam, a run as long as the grid, weights of 0 and 4096"""
    invalid = empty = valid = seam = whole = zero = full = 0
    for c in CASES:
        ny, nx, rows, cols, _ = _inputs(c)
        out, _, n, n_range = _want(c)
        invalid += int(np.isnan(out).sum())
        valid += int((~np.isnan(out)).sum())
        empty += int((n == 0).sum())
        assert n_range == 0
        cnt = np.diff(cols[1])
        if c.periodic:
            seam += int((cols[0] + cnt > nx).sum())
            whole += int((cnt == nx).sum())
        zero += int((rows[2] == 0).sum() + (cols[2] == 0).sum())
        full += int((rows[2] == 4096).sum() + (cols[2] == 4096).sum())
    assert invalid > 1000 and valid > invalid and 100 < empty < invalid
    assert seam > 50 and whole >= 2 and zero > 1000 and full > 1000
    assert any((np.diff(_inputs(c)[3][1]) == 0).any() and (np.diff(_inputs(c)[3][1]) == 64).any() for c in CASES)


def test_optional_outputs_may_be_null(dev):
    c = next(k for k in CASES if (k.mx, k.my, k.kind) == (130, 3, "shift") and k.dtype is np.float32)
    ny, nx, rows, cols, field = _inputs(c)
    got = raw(dev, field, ny, nx, rows, cols, c.periodic, 0.0, c.a, want_sums=False)
    same_floats(got[0], _want(c)[0])
    assert got[3] == _want(c)[3]


# ---- both paths, every chunk: the same bits ----------------------------------------------------------

def test_both_paths_and_every_chunk_give_identical_bits(dev):
    took = {1: [], 2: []}
    for c in SUBSET:
        ny, nx, rows, cols, field = _inputs(c)
        for variant in (1, 2):
            for chunk in (1, 4, 0):
                got = raw(dev, field, ny, nx, rows, cols, c.periodic, 0.0, c.a, variant=variant, chunk=chunk)
                check(got, _want(c))
                took[variant].append((c, got[4]))
    # the paths that actually ran, as the entry itself says: variant 1 is always direct; variant 2 is staged for every
    # kind, both sample types, both periodic settings and every width of the subset at least once
    assert all(k == DIRECT for _, k in took[1])
    staged = {c for c, k in took[2] if k == STAGED}
    assert {c.kind for c in staged} == set(rc.KINDS) and {c.mx for c in staged} == set(rc.WIDTHS)
    assert {c.periodic for c in staged} == {0, 1} and {c.dtype for c in staged} == set(rc.DTYPES)
    assert any(k == DIRECT for _, k in took[2])                  # and a footprint that does not fit fell back


# ---- nested blocks: regrid() == coarsen() on the device ----------------------------------------------

@pytest.mark.parametrize("ny,nx", [(8, 130), (13, 257)])
@pytest.mark.parametrize("fy,fx", [(2, 2), (3, 2), (4, 4)])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_nested_blocks_equal_coarsen_on_the_device(dev, ny, nx, fy, fx, dtype):
    from xmhw_amd._lib import hip, hip_coarsen
    rng = np.random.default_rng(ny * 1000 + nx + 7 * fy + fx)
    T, a = 9, 30000
    ncy, ncx = -(-ny // fy), -(-nx // fx)
    ay_of_row = rng.integers(0, 4097, ny).astype(np.int32)
    field = rng.normal(0.0, 8.0, (T, ny * nx)).astype(dtype)
    field[rng.random(field.shape) < 0.2] = np.nan
    # the tables of the integer blocks: ax all 4096, ay arbitrary; a block that hangs over the grid holds its in-grid part
    rcount = np.minimum(fy, ny - np.arange(ncy) * fy)
    ccount = np.minimum(fx, nx - np.arange(ncx) * fx)
    rp = np.concatenate([[0], np.cumsum(rcount)]).astype(np.int32)
    cp = np.concatenate([[0], np.cumsum(ccount)]).astype(np.int32)
    wy = np.add.reduceat(ay_of_row.astype(np.int64), rp[:-1]).astype(np.int32)
    rows = ((np.arange(ncy) * fy).astype(np.int32), rp, ay_of_row, wy)
    cols = ((np.arange(ncx) * fx).astype(np.int32), cp, np.full(nx, 4096, np.int32), (ccount * 4096).astype(np.int32))
    got = raw(dev, field, ny, nx, rows, cols, 0, 0.0, a)
    # coarsen() with wi[j, i] = ay[j] * 4096 on the same series
    isz, cells = field.dtype.itemsize, ncy * ncx
    wi = np.repeat(ay_of_row.astype(np.int64) * 4096, nx).astype(np.int32)
    d_ts, d_wi = dev.DeviceBuffer.from_array(field), dev.DeviceBuffer.from_array(wi)
    d_out, d_ws, d_n = dev.DeviceBuffer(T * cells * isz), dev.DeviceBuffer(T * cells * 8), dev.DeviceBuffer(T * cells * 4)
    d_cnt = dev.DeviceBuffer.from_array(np.zeros(1, np.int64))
    try:
        hip_coarsen().coarsen(d_ts.ptr, isz, T, ny * nx, ny, nx, fy, fx, ncy, ncx, d_wi.ptr, 0.0, a,
                              np.arange(T + 1, dtype=np.int32), d_out.ptr, cells, d_ws.ptr, d_n.ptr, d_cnt.ptr)
        hip().stream_sync(0)
        want = (d_out.to_array((T, cells), dtype), d_ws.to_array((T, cells), np.int64), d_n.to_array((T, cells), np.int32),
                int(d_cnt.to_array((1,), np.int64)[0]))
    finally:
        for b in (d_ts, d_wi, d_out, d_ws, d_n, d_cnt):
            b.free()
    check(got, want)
    assert np.isnan(want[0]).any() and (~np.isnan(want[0])).any()


# ---- corners -----------------------------------------------------------------------------------------

def one_cell(ay=(4096,), ax=(4096,), wy=None, wx=None, copies=1):
    """tables of `copies` destination columns that all read the same len(ay) x len(ax) source cells from (0, 0)"""
    ay, ax = np.asarray(ay, np.int32), np.asarray(ax, np.int32)
    rows = (np.zeros(1, np.int32), np.array([0, ay.size], np.int32), ay, np.array([ay.sum() if wy is None else wy], np.int32))
    cols = (np.zeros(copies, np.int32), (np.arange(copies + 1) * ax.size).astype(np.int32), np.tile(ax, copies),
            np.full(copies, ax.sum() if wx is None else wx, np.int32))
    return rows, cols


@pytest.mark.parametrize("variant", [1, 2])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_range_edge_and_infinities_are_counted_per_pair(dev, dtype, variant):
    x0 = 0.0
    inside = np.nextafter(dtype(128.0), dtype(0.0))              # one ulp inside: |x - x0| < 2^7
    steps = [inside, -inside, 128.0, -128.0, np.inf, -np.inf, np.nan, 1.5]
    field = np.array(steps, dtype=dtype).reshape(-1, 1)
    rows, cols = one_cell(copies=3)                              # three destination cells share the one sample
    want = ro.regrid_oracle(field, 1, 1, rows, cols, 0, x0, 0)
    d = field[:, 0].astype(np.float64) - x0
    n_out = int(((np.abs(d) >= 128.0) & ~np.isnan(d)).sum())
    assert want[3] == 3 * n_out and n_out >= 4                   # (destination, source) pairs, not samples
    assert not np.isnan(want[0][0]).any() and np.isnan(want[0][2]).all() and (want[2][4] == 0).all()
    got = raw(dev, field, 1, 1, rows, cols, 0, x0, 0, variant=variant)
    check(got, want)
    assert got[4] == variant


@pytest.mark.parametrize("variant", [1, 2])
def test_the_share_threshold_to_the_unit(dev, variant):
    # wsum = 2048 * 4096 = 2^23 of wy * wx = 4096 * 4096 = 2^24: the share is exactly a = 32768 of 65536
    rows, cols = one_cell(ay=(2048,), wy=4096)
    field = np.array([[1.25]], np.float32)
    for a, valid in ((32768, True), (32769, False), (0, True), (65536, False)):
        want = ro.regrid_oracle(field, 1, 1, rows, cols, 0, 0.0, a)
        assert (not np.isnan(want[0][0, 0])) == valid and want[1][0, 0] == 1 << 23
        check(raw(dev, field, 1, 1, rows, cols, 0, 0.0, a, variant=variant), want)


@pytest.mark.parametrize("variant", [1, 2])
@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_the_corner_of_the_64_bits(dev, sign, variant):
    """a 64 x 64 run, all weights 4096, every xq = +-2^23: |xsum| = 2^59, wsum * 65536 = 2^52, wy = wx = 2^18"""
    x = sign * np.nextafter(128.0, 0.0)                          # rint(x * 65536) = +-2^23
    field = np.full((2, 64 * 64), x, np.float64)
    rows, cols = one_cell(ay=(4096,) * 64, ax=(4096,) * 64)
    want = ro.regrid_oracle(field, 64, 64, rows, cols, 0, 0.0, 65536, exact=True)
    assert want[1][0, 0] == 1 << 36 and want[2][0, 0] == 4096 and not np.isnan(want[0]).any()
    got = raw(dev, field, 64, 64, rows, cols, 0, 0.0, 65536, variant=variant)
    check(got, want)
    assert got[4] == variant


def test_an_all_empty_table_and_no_steps(dev):
    my, mx = 2, 70
    rows = (np.zeros(my, np.int32), np.zeros(my + 1, np.int32), np.zeros(0, np.int32), np.full(my, 5, np.int32))
    cols = (np.zeros(mx, np.int32), np.zeros(mx + 1, np.int32), np.zeros(0, np.int32), np.full(mx, 5, np.int32))
    field = np.ones((3, 12), np.float32)
    got = raw(dev, field, 3, 4, rows, cols, 1, 0.0, 0)
    assert np.isnan(got[0]).all() and (got[1] == 0).all() and (got[2] == 0).all() and got[3] == 0 and got[4] == DIRECT
    c = SUBSET[0]
    ny, nx, rows, cols, field = _inputs(c)
    got = raw(dev, field[:0], ny, nx, rows, cols, c.periodic, 0.0, c.a)   # nt = 0: nothing is written
    assert got[0].shape[0] == 0 and got[3] == 0


# ---- the public function -----------------------------------------------------------------------------

def test_public_function_in_time_blocks(dev):
    from xmhw_amd import GridSeries, regrid
    rng = np.random.default_rng(11)
    T, lat, lon = 11, np.arange(-19.875, 20, 0.25), np.arange(0.125, 360, 0.25)[:200]
    x = rng.normal(15.0, 5.0, (T, lat.size, lon.size)).astype(np.float32)
    x[rng.random(x.shape) < 0.1] = np.nan
    temp = GridSeries(x, ("time", "lat", "lon"), {"time": np.arange(T), "lat": lat, "lon": lon}, attrs={"units": "degC"})
    like = {"lat": np.arange(19.5, -20, -1.0), "lon": np.arange(0.5, 50, 1.0)}
    import regrid_oracle
    want, winfo = regrid(temp, like=like, coverage=True, _compute=regrid_oracle.as_stage)
    assert (~np.isnan(want.values)).sum() > 1000
    for block in (1, 5, None):
        got, info = regrid(temp, like=like, coverage=True, block_steps=block)
        same_floats(got.values, want.values)
        npt.assert_array_equal(info.wsum, winfo.wsum)
        npt.assert_array_equal(info.n, winfo.n)
        npt.assert_array_equal(bits(info.coverage), bits(winfo.coverage))
        assert got.dims == temp.dims and got.values.dtype == np.float32 and got.attrs == temp.attrs
