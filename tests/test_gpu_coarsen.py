"""coarsen() on the device against tests/coarsen_oracle.py, bit for bit: the output as unsigned views with NaN positions
equal, wsum, n and n_range as integers.  The C entries are called raw first, on pitched inputs (ld and ldo larger than
the grids; the columns past the coarse grid pre-filled with a bit pattern that must be intact afterwards), over the
grids, factors, coarse grids, windows and shares of tests/coarsen_cases.py; every instantiation (fx 1, 2, 4, the column
loop; wide and one-sample loads) must be reached and give the same bits where more than one is legal, every window chunk
and every time block likewise.  Then the validity threshold to the unit, the range edge, the 64-bit corner, the refusals
and the public function."""
import functools

import numpy as np
import numpy.testing as npt
import pytest

import coarsen_cases as cc
import coarsen_oracle as co

pytestmark = pytest.mark.gpu

FILL32, FILL64 = -0x5A5A5A5B, -0x5A5A5A5A5A5A5A5B
EXTRA = 5                       # columns of the outputs past ncy * ncx
CASES = cc.listed()


@pytest.fixture(scope="module")
def dev():
    from xmhw_amd._lib import require_gpu
    require_gpu()
    import xmhw_amd.device as d
    return d


@pytest.fixture(autouse=True)
def automatic_afterwards():
    yield
    from xmhw_amd._lib import hip_coarsen
    hip_coarsen().set_coarsen_variant(0)
    hip_coarsen().set_coarsen_chunk(0)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same_floats(got, want):
    """bit for bit, every NaN standing for every other"""
    npt.assert_array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    npt.assert_array_equal(bits(got)[ok], bits(want)[ok])


def raw(dev, field, wi, ny, nx, fy, fx, ncy, ncx, x0, a, win, variant=0, chunk=0, shift=0, want_sums=True):
    """xmhw_coarsen_* on the host arrays: ``field`` (T, ld) pitched as it is, the series pointer advanced by ``shift``
    samples (the rows then start ``shift`` samples later: the buffer holds them).  Returns (out, wsum, n, n_range, the
    class the call took); the columns past ncy * ncx of the outputs are checked to be untouched."""
    from xmhw_amd._lib import hip, hip_coarsen
    m = hip_coarsen()
    T, ld = field.shape
    isz = field.dtype.itemsize
    S, cells = len(win) - 1, ncy * ncx
    ldo = cells + EXTRA
    pad = np.zeros(shift, field.dtype)
    d_ts = dev.DeviceBuffer.from_array(np.concatenate([pad, field.reshape(-1), pad]))
    d_wi = dev.DeviceBuffer.from_array(wi.astype(np.int32))
    fill = np.float32(-7.25) if isz == 4 else np.float64(-7.25)
    d_out = dev.DeviceBuffer.from_array(np.full((S, ldo), fill, field.dtype))
    d_ws = dev.DeviceBuffer.from_array(np.full((S, ldo), FILL64, np.int64))
    d_n = dev.DeviceBuffer.from_array(np.full((S, ldo), FILL32, np.int32))
    d_cnt = dev.DeviceBuffer.from_array(np.full(1, 123, np.int64))
    try:
        m.set_coarsen_variant(variant)
        m.set_coarsen_chunk(chunk)
        ts_ptr = d_ts.ptr + shift * isz
        klass = m.coarsen_class(ts_ptr, d_wi.ptr, ld, nx, isz, fx)
        m.coarsen(ts_ptr, isz, T, ld, ny, nx, fy, fx, ncy, ncx, d_wi.ptr, x0, a, np.asarray(win, np.int32), d_out.ptr, ldo,
                  d_ws.ptr if want_sums else 0, d_n.ptr if want_sums else 0, d_cnt.ptr)
        hip().stream_sync(0)
        out, ws, n = d_out.to_array((S, ldo), field.dtype), d_ws.to_array((S, ldo), np.int64), d_n.to_array((S, ldo), np.int32)
        cnt = int(d_cnt.to_array((1,), np.int64)[0]) - 123           # the counter is ADDED to
    finally:
        for b in (d_ts, d_wi, d_out, d_ws, d_n, d_cnt):
            b.free()
    npt.assert_array_equal(out[:, cells:], fill)
    npt.assert_array_equal(ws[:, cells:], FILL64)
    npt.assert_array_equal(n[:, cells:], FILL32)
    if not want_sums:
        npt.assert_array_equal(ws, FILL64)
        npt.assert_array_equal(n, FILL32)
    return out[:, :cells], ws[:, :cells], n[:, :cells], cnt, klass


def check(got, want):
    same_floats(got[0], want[0])
    npt.assert_array_equal(got[1], want[1])
    npt.assert_array_equal(got[2], want[2])
    assert got[3] == want[3]


@functools.lru_cache(maxsize=None)
def _data(c):
    return cc.make_data(c)


@functools.lru_cache(maxsize=None)
def _want(c):
    field, wi = _data(c)
    return co.coarsen_oracle(field, c.ny, c.nx, c.fy, c.fx, c.ncy, c.ncx, wi, 0.0, c.a, cc.windows(c.window, cc.T_STEPS))


@pytest.mark.parametrize("c", CASES, ids=cc.case_id)
def test_raw_entry_equals_the_oracle(dev, c):
    field, wi = _data(c)
    got = raw(dev, field, wi, c.ny, c.nx, c.fy, c.fx, c.ncy, c.ncx, 0.0, c.a, cc.windows(c.window, cc.T_STEPS))
    check(got, _want(c))


def test_the_cases_bite():
    """what the list above compares is not trivial: invalid entries beside valid ones, blocks without a sample, blocks
    that hang over the grid, samples under a zero weight"""
    invalid = empty = valid = 0
    for c in CASES:
        out, _, n, n_range = _want(c)
        invalid += int(np.isnan(out).sum())
        valid += int((~np.isnan(out)).sum())
        empty += int((n == 0).sum())
        assert n_range == 0
    assert invalid > 1000 and valid > 2 * invalid and 100 < empty < invalid
    assert any(c.ny % c.fy or c.nx % c.fx for c in CASES if c.ncy * c.fy > c.ny or c.ncx * c.fx > c.nx)


def test_optional_outputs_may_be_null(dev):
    c = next(k for k in CASES if (k.ny, k.nx, k.fy, k.fx) == (8, 130, 2, 2) and k.dtype is np.float32)
    field, wi = _data(c)
    got = raw(dev, field, wi, c.ny, c.nx, c.fy, c.fx, c.ncy, c.ncx, 0.0, c.a, cc.windows(c.window, cc.T_STEPS), want_sums=False)
    same_floats(got[0], _want(c)[0])
    assert got[3] == _want(c)[3]


# ---- every instantiation, and the same bits from each ------------------------------------------------

def _aligned_case(ny, nx, fy, fx, dtype, ld_extra, seed):
    """a case whose pitch is ny * nx + ld_extra (make_data pitches by 3: re-pitched here)"""
    c = cc.Case(ny, nx, fy, fx, -(-ny // fy), -(-nx // fx), dtype, "5", 20000, seed)
    field, wi = cc.make_data(c)
    out = np.full((field.shape[0], ny * nx + ld_extra), np.nan, dtype)
    out[:, :ny * nx] = field[:, :ny * nx]
    return c, out, wi


def test_every_instantiation_is_reached_with_identical_bits(dev):
    """nx odd with fx = 2 and fx = 4, a series pointer advanced by one sample, pitches that keep the rows 16-byte aligned
    or not: the class of every call is recorded, all twelve (six per sample type) must turn up, and wherever more than
    one instantiation is legal (the narrow loads and the column loop always are) they return the same bits"""
    reached = set()
    win = cc.windows("5", cc.T_STEPS)
    k = 0
    for dtype in cc.DTYPES:
        for fx in (1, 2, 3, 4):
            for nx in (130, 131, 132):
                for ld_extra in (0, 1, 2, 4):
                    for shift in (0, 1):
                        k += 1
                        if (k + fx) % 3 and not (fx in (2, 4) and shift == 0 and ld_extra in (0, 4) and nx != 131):
                            continue                                  # a third of the unaligned ones do
                        c, field, wi = _aligned_case(4, nx, 2, fx, dtype, ld_extra, 300 + k)
                        want = co.coarsen_oracle(field, c.ny, c.nx, c.fy, c.fx, c.ncy, c.ncx, wi, 0.0, c.a, win)
                        for variant in (0, 1, 2):
                            got = raw(dev, field, wi, c.ny, c.nx, c.fy, c.fx, c.ncy, c.ncx, 0.0, c.a, win, variant=variant,
                                      shift=shift)
                            check(got, want)
                            reached.add((np.dtype(dtype).name, got[4]))
                            if variant == 2:
                                assert got[4] == 0
                            if variant == 1:
                                assert got[4] in (0, 1, 2, 4)
    assert reached == {(np.dtype(d).name, k) for d in cc.DTYPES for k in range(6)}, reached


@pytest.mark.parametrize("chunk", (1, 3, 1000))
def test_window_chunks_do_not_change_a_bit(dev, chunk):
    for c in CASES:
        if (c.ny, c.nx) == (13, 257) and (c.fy, c.fx) in ((2, 2), (5, 8)) and c.dtype is np.float32:
            field, wi = _data(c)
            got = raw(dev, field, wi, c.ny, c.nx, c.fy, c.fx, c.ncy, c.ncx, 0.0, c.a, cc.windows(c.window, cc.T_STEPS), chunk=chunk)
            check(got, _want(c))


# ---- the device stage: time blocks, gaps -------------------------------------------------------------

@pytest.mark.parametrize("dtype", cc.DTYPES)
def test_time_blocks_and_gaps_do_not_change_a_bit(dev, dtype):
    from xmhw_amd.coarsen import coarsen_grid, window_blocks, check_windows
    c = cc.Case(13, 257, 3, 2, 5, 129, dtype, "gaps", 32768, 77)
    field, wi = cc.make_data(c, T=128)
    field = np.ascontiguousarray(field[:, :c.ny * c.nx])
    for win in (cc.windows("5", 128), cc.windows("31", 128), cc.gap_pairs(128), cc.windows("gaps", 128)):
        want = co.coarsen_oracle(field, c.ny, c.nx, c.fy, c.fx, c.ncy, c.ncx, wi, 0.0, c.a, win)
        one = coarsen_grid(field, c.ny, c.nx, c.fy, c.fx, c.ncy, c.ncx, wi, 0.0, c.a, win, want=True)
        check(one, want)
        pairs = check_windows(128, windows=win)
        longest = int((pairs[:, 1] - pairs[:, 0]).max())
        for steps in (max(40, longest), max(64, longest)):
            assert len(window_blocks(pairs, 1, 0, block_steps=steps)) >= 2
            got = coarsen_grid(field, c.ny, c.nx, c.fy, c.fx, c.ncy, c.ncx, wi, 0.0, c.a, win, want=True, block_steps=steps)
            check(got, want)
            same_floats(got[0], one[0])
    # exactly 2 and 5 blocks of whole windows
    win = cc.windows("2", 128)
    assert len(window_blocks(check_windows(128, windows=win), 1, 0, block_steps=64)) == 2
    assert len(window_blocks(check_windows(128, windows=win), 1, 0, block_steps=26)) == 5
    want = co.coarsen_oracle(field, c.ny, c.nx, c.fy, c.fx, c.ncy, c.ncx, wi, 0.0, c.a, win)
    for steps in (None, 64, 26):
        check(coarsen_grid(field, c.ny, c.nx, c.fy, c.fx, c.ncy, c.ncx, wi, 0.0, c.a, win, want=True, block_steps=steps), want)
    without = coarsen_grid(field, c.ny, c.nx, c.fy, c.fx, c.ncy, c.ncx, wi, 0.0, c.a, win)
    assert without[1] is None and without[2] is None
    same_floats(without[0], want[0])


# ---- validity to the unit ----------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", cc.DTYPES)
def test_validity_threshold_to_the_unit(dev, dtype):
    """blocks of 2 x 2 over windows of 3 steps: W = 65536, a = 49152, so a * len * W / 65536 = 3 * 49152.  Block 0 has
    exactly that valid weight (valid); block 1 one weight unit less (NaN); block 2 is all land (n = 0); block 3 has
    zero weights only; block 4 is whole"""
    ny, nx, T = 2, 10, 6
    wi = np.full((ny, nx), 16384, np.int32)
    x = np.full((T, ny, nx), 20.0, dtype) + np.arange(ny * nx, dtype=dtype).reshape(ny, nx)
    x[:, 1, 1] = np.nan                                          # block 0: three points of 16384 at every step
    wi[:, 2:4] = [[16384, 16384], [16383, 16385]]                # block 1: W is 65536 still
    x[:, 1, 3] = np.nan                                          #   the point of 16385 is missing: 49151 a step
    x[:, :, 4:6] = np.nan                                        # block 2
    wi[:, 6:8] = 0                                               # block 3
    win = np.array([0, 3, 6], np.int32)
    for a, valid01 in ((49152, (True, False)), (49151, (True, True)), (49153, (False, False)), (0, (True, True)),
                       (65536, (False, False))):
        got = raw(dev, x.reshape(T, -1), wi.reshape(-1), ny, nx, 2, 2, 1, 5, 0.0, a, win)
        check(got, co.coarsen_oracle(x.reshape(T, -1), ny, nx, 2, 2, 1, 5, wi.reshape(-1), 0.0, a, win))
        out, ws, n = got[0], got[1], got[2]
        assert tuple(~np.isnan(out[0, :2])) == valid01
        npt.assert_array_equal(ws[0], [3 * 49152, 3 * 49151, 0, 0, 3 * 65536])
        npt.assert_array_equal(n[0], [9, 9, 0, 0, 12])
        assert np.isnan(out[:, 2:4]).all() and not np.isnan(out[:, 4]).any()


# ---- the range edge ----------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,x0", [(np.float32, 0.0), (np.float64, 0.0), (np.float64, 273.15), (np.float32, 16.0)])
def test_range_edge_counts_exactly(dev, dtype, x0):
    from xmhw_amd import GridSeries, coarsen
    from xmhw_amd.exception import XmhwException
    ny, nx, T = 2, 8, 4
    edge = dtype(x0 + 128.0)
    lo_edge = dtype(x0 - 128.0)
    inside, lo_inside = np.nextafter(edge, dtype(0)), np.nextafter(lo_edge, dtype(0) if x0 == 0 else dtype(1e9))
    assert abs(float(inside) - x0) < 128.0 and abs(float(lo_inside) - x0) < 128.0
    x = np.full((T, ny, nx), dtype(x0 + 1.5), dtype)
    x[0, 0, 0], x[0, 0, 1] = inside, lo_inside                   # in range: they count
    x[1, 0, 2], x[1, 1, 2] = edge, lo_edge                       # out of range: left out and counted
    x[2, 0, 4], x[2, 1, 5] = np.inf, -np.inf
    x[3, 0, 6] = dtype(-0.0) if x0 == 0 else dtype(x0)          # -0.0 (or d = 0): an ordinary sample
    x[3, 1, 7] = edge                                            # under a zero weight: no sample, not counted
    wi = np.full((ny, nx), 1 << 20, np.int32)
    wi[1, 7] = 0
    win = np.array([0, 1, 2, 4], np.int32)
    want = co.coarsen_oracle(x.reshape(T, -1), ny, nx, 2, 2, 1, 4, wi.reshape(-1), x0, 0, win)
    assert want[3] == 4
    got = raw(dev, x.reshape(T, -1), wi.reshape(-1), ny, nx, 2, 2, 1, 4, x0, 0, win)
    check(got, want)                                             # the raw call counts and continues
    assert got[2][1, 1] == 2 and got[2][0, 0] == 4 and not np.isnan(got[0]).any()
    g = GridSeries(x, ("time", "lat", "lon"), {"time": np.arange(T), "lat": np.arange(2.0), "lon": np.arange(8.0)})
    # under uniform weights the sample at [3, 1, 7] is one as well: five are out of range, and the public call raises
    with pytest.raises(XmhwException, match="5 samples lie 2\\*\\*7 and more from offset=.*offset=273.15"):
        coarsen(g, space=2, offset=x0, min_fraction=0.0)


# ---- the 64-bit corner -------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", cc.DTYPES)
@pytest.mark.parametrize("sign", (1.0, -1.0))
def test_overflow_corner(dev, dtype, sign):
    """a volume of exactly 4096 (8 x 8 x 64), every weight 2**24, every sample at the range edge: |xsum| reaches
    2**12 * 2**24 * 2**23 = 2**59, checked against Python integers by the oracle"""
    ny, nx, T = 8, 16, 64
    x = np.full((T, ny, nx), np.nextafter(dtype(sign * 128.0), dtype(0)), dtype)      # xq = +-2**23 (rint of 2**23 - 1/2 or nearer)
    x[:, :, 8:] = dtype(sign * 127.99)                           # the second block: a little inside
    x = x.reshape(T, -1)
    wi = np.full(ny * nx, 1 << 24, np.int32)
    win = np.array([0, 64], np.int32)
    want = co.coarsen_oracle(x, ny, nx, 8, 8, 1, 2, wi, 0.0, 65536, win, exact=True)
    assert want[1][0, 0] == 4096 << 24 and not np.isnan(want[0]).any()
    for variant in (0, 2):
        check(raw(dev, x, wi, ny, nx, 8, 8, 1, 2, 0.0, 65536, win, variant=variant), want)


# ---- refusals leave the outputs alone ----------------------------------------------------------------

def test_refusals_leave_the_outputs_untouched(dev):
    from xmhw_amd._lib import hip, hip_coarsen
    core, m = hip(), hip_coarsen()
    T, ny, nx = 8, 4, 6
    x = np.full((T, ny * nx), 1.0, np.float32)
    d_ts, d_wi = dev.DeviceBuffer.from_array(x), dev.DeviceBuffer.from_array(np.ones(ny * nx, np.int32))
    d_out = dev.DeviceBuffer.from_array(np.full((4, 6), -7.25, np.float32))
    d_ws = dev.DeviceBuffer.from_array(np.full((4, 6), FILL64, np.int64))
    d_n = dev.DeviceBuffer.from_array(np.full((4, 6), FILL32, np.int32))
    d_cnt = dev.DeviceBuffer.from_array(np.full(1, 123, np.int64))
    w = np.array([0, 4, 8], np.int32)

    def call(nt=T, fy=2, fx=2, ncy=2, ncx=3, a=100, win=w):
        m.coarsen(d_ts.ptr, 4, nt, ny * nx, ny, nx, fy, fx, ncy, ncx, d_wi.ptr, 0.0, a, win, d_out.ptr, 6, d_ws.ptr, d_n.ptr,
                  d_cnt.ptr)

    try:
        with pytest.raises(core.Unsupported):                    # a volume of 4097
            call(nt=4097, fy=1, fx=1, ncy=4, ncx=6, win=np.array([0, 4097], np.int32))
        with pytest.raises(core.Unsupported):
            call(fy=17, fx=241, ncy=1, ncx=1, win=np.array([0, 1], np.int32))
        for bad in (dict(fy=0), dict(fx=0), dict(win=np.array([0, 4, 4], np.int32)), dict(win=np.array([0, 5, 3], np.int32)),
                    dict(win=np.array([0, 4, 9], np.int32)), dict(a=65537), dict(ncy=3)):
            with pytest.raises(core.InvalidArgument):
                call(**bad)
        hip().stream_sync(0)
        npt.assert_array_equal(d_out.to_array((4, 6), np.float32), np.float32(-7.25))
        npt.assert_array_equal(d_ws.to_array((4, 6), np.int64), FILL64)
        npt.assert_array_equal(d_n.to_array((4, 6), np.int32), FILL32)
        assert int(d_cnt.to_array((1,), np.int64)[0]) == 123
        call()                                                   # ... and the same buffers take a good call
        hip().stream_sync(0)
        npt.assert_array_equal(d_out.to_array((4, 6), np.float32)[:2], np.float32(1.0))
    finally:
        for b in (d_ts, d_wi, d_out, d_ws, d_n, d_cnt):
            b.free()


# ---- the public function -----------------------------------------------------------------------------

def _public_grid(dtype=np.float32, ny=12, nx=22, T=40, seed=5):
    from xmhw_amd import GridSeries
    rng = np.random.default_rng(seed)
    tt = np.arange(T)[:, None, None]
    x = (15.0 + 3.0 * np.sin(2 * np.pi * tt / 20.0 + rng.uniform(0, 6, (ny, nx))) + rng.normal(0, 1.0, (T, ny, nx))).astype(dtype)
    x[rng.random(x.shape) < 0.05] = np.nan
    x[:, 3:7, 4:9] = np.nan                                      # land
    time = np.datetime64("2001-01-01") + np.arange(T).astype("timedelta64[D]")
    lat, lon = -60.0 + 10.0 * np.arange(ny), 0.25 * np.arange(nx)
    return GridSeries(x, ("time", "lat", "lon"), {"time": time, "lat": lat, "lon": lon})


@pytest.mark.parametrize("boundary", ("trim", "pad"))
@pytest.mark.parametrize("dtype", cc.DTYPES)
def test_public_function_equals_the_oracle(dev, boundary, dtype):
    from xmhw_amd import coarsen
    g = _public_grid(dtype)
    kw = dict(space=(4, 4), time=7, weights="coslat", min_fraction=0.6, boundary=boundary, coverage=True)
    got, info = coarsen(g, **kw)
    want, winfo = coarsen(g, _compute=co.as_stage, **kw)
    assert got.values.shape == ((5, 3, 5) if boundary == "trim" else (6, 3, 6)) and got.values.dtype == dtype
    same_floats(got.values, want.values)
    npt.assert_array_equal(info.wsum, winfo.wsum)
    npt.assert_array_equal(info.n, winfo.n)
    npt.assert_array_equal(bits(info.coverage), bits(winfo.coverage))
    assert info.coverage.dtype == np.float32 and info.n_range == 0
    assert np.isnan(got.values).any() and not np.isnan(got.values).all()
    for k in ("time", "lat", "lon"):
        npt.assert_array_equal(got.coords[k], want.coords[k])
    blocked, _ = coarsen(g, block_steps=14, **kw)
    same_floats(blocked.values, got.values)


def test_coarse_series_feeds_spatial_correlation(dev):
    from xmhw_amd import coarsen, spatial_correlation
    g = _public_grid(np.float32, ny=16, nx=40, T=60, seed=8)
    coarse, _ = coarsen(g, space=4)
    oracle_coarse, _ = coarsen(g, space=4, _compute=co.as_stage)
    assert coarse.values.shape == (60, 4, 10)
    got = spatial_correlation(coarse, reach=(2, 2))
    want = spatial_correlation(oracle_coarse, reach=(2, 2))
    for k in ("n", "sx", "sy", "sxx", "syy", "sxy"):
        npt.assert_array_equal(getattr(got, k), getattr(want, k))
    same_floats(got.r, want.r)
    assert (got.n > 0).any()
