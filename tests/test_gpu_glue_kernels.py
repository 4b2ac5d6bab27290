"""The glue kernels between file and threshold() / detect() (csrc/kernels_generic.hip: land_mask, gather_cells,
scatter_cells; csrc/kernels_ingest.hip: decode, encode_i16, pad_gaps) one by one through their bindings: leading
dimensions wider than the grid, poisoned pad columns, 0xFF canaries behind the outputs, the shapes at which the
kernels change path (quarters of the time axis, the 8-row unroll and its tail, clamped lanes, the second trip of the
row-strided loops).  Every reference is numpy, every comparison exact."""
import numpy as np
import numpy.testing as npt
import pytest

import pad_oracle as po
from test_gpu_padding import _random_gappy

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def h():
    from xmhw_amd._lib import hip, require_gpu
    require_gpu()
    return hip()


class _Bufs:
    def __init__(self, h):
        from xmhw_amd.device import DeviceBuffer
        self.h, self._new, self.bufs = h, DeviceBuffer, []

    def up(self, a):
        b = self._new.from_array(a)
        self.bufs.append(b)
        return b

    def canary(self, shape, dtype):
        """a buffer of ``shape`` elements, every byte 0xFF"""
        b = self._new(int(np.prod(shape)) * np.dtype(dtype).itemsize)
        self.bufs.append(b)
        self.h.memset(b.ptr, 0xFF, b.nbytes)
        return b

    def free(self):
        for b in self.bufs:
            b.free()
        self.bufs = []


def _untouched(a):
    return (np.ascontiguousarray(a).view(np.uint8) == 0xFF).all()


# ---- land_mask ------------------------------------------------------------------------------------------------
MASK_TS = (1, 2, 3, 4, 7, 8, 9, 37, 100)
MASK_CS = (1, 63, 64, 65, 130)


def _mask_runs(T, C, rng):
    """two missing-sample masks (T, C + 5) of one shape, planted columns first (as many as C holds):
    all missing; none missing; exactly one missing sample in each quarter [T p / 4, T (p + 1) / 4) in turn; all
    missing but one sample in each quarter in turn; the other columns: none missing, or missing at random.
    Run 0: the last column all missing, the pad columns valid; run 1: the reverse -- a lane clamped onto column
    C - 1 must not write, and a lane that read the pad must not count it."""
    base = np.zeros((T, C + 5), dtype=bool)
    cols = iter(range(C))
    plants = [("all", None), ("none", None)] + [("one", p) for p in range(4)] + [("but one", p) for p in range(4)]
    for (kind, p), c in zip(plants, cols):
        if kind == "all":
            base[:, c] = True
        elif kind in ("one", "but one"):
            t0, t1 = T * p // 4, T * (p + 1) // 4
            if t1 == t0:
                continue                         # T < 4: this quarter has no step
            t = int(rng.integers(t0, t1))
            base[:, c] = kind == "but one"
            base[t, c] = kind == "one"
    for c in cols:
        if rng.random() < 0.4:
            base[:, c] = rng.random(T) < 0.3
    runs = []
    for last_missing in (True, False):
        m = base.copy()
        m[:, C - 1] = last_missing
        m[:, C:] = not last_missing
        runs.append(m)
    return runs


def _check_mask(h, bufs, call, data, missing, C):
    d = bufs.up(data)
    for anynans in (0, 1):
        keep = bufs.canary((C + 8,), np.uint8)
        call(d.ptr, anynans, keep.ptr)
        h.stream_sync(0)
        got = keep.to_array((C + 8,), np.uint8)
        want = ~missing[:, :C].any(axis=0) if anynans else ~missing[:, :C].all(axis=0)
        npt.assert_array_equal(got[:C], want.astype(np.uint8), err_msg=f"T {data.shape[0]} C {C} anynans {anynans}")
        assert _untouched(got[C:])
    bufs.free()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_land_mask_quarters_tails_and_clamped_lanes(h, dtype):
    rng = np.random.default_rng(41)
    bufs = _Bufs(h)
    isz = np.dtype(dtype).itemsize
    try:
        for T in MASK_TS:
            for C in MASK_CS:
                for missing in _mask_runs(T, C, rng):
                    data = rng.normal(size=missing.shape).astype(dtype)
                    data[missing] = np.nan
                    _check_mask(h, bufs, lambda p, anynans, keep: h.land_mask(p, isz, T, C, C + 5, anynans, keep),
                                data, missing, C)
    finally:
        bufs.free()


@pytest.mark.parametrize("big", [False, True])
@pytest.mark.parametrize("fill", [-32768, 7])
def test_land_mask_i16_quarters_tails_and_clamped_lanes(h, big, fill):
    """the fill code as stored; the code whose bytes are the fill code's bytes swapped is an ordinary sample"""
    rng = np.random.default_rng(43 + (fill & 0xFFFF))
    bufs = _Bufs(h)
    swapped = int(np.array([fill], dtype=np.int16).byteswap()[0])
    try:
        for T in MASK_TS:
            for C in MASK_CS:
                for k, missing in enumerate(_mask_runs(T, C, rng)):
                    codes = rng.integers(-32767, 32767, size=missing.shape).astype(np.int16)
                    codes[codes == fill] = 11
                    codes[rng.random(missing.shape) < 0.1] = swapped
                    codes[missing] = fill
                    stored = codes.astype(">i2" if big else "<i2").view(np.int16)
                    _check_mask(h, bufs, lambda p, anynans, keep: h.land_mask_i16(p, T, C, C + 5, int(big), 1, fill,
                                                                                 anynans, keep), stored, missing, C)
                    if k == 0:                  # no fill code: nothing is missing, whatever the codes are
                        _check_mask(h, bufs, lambda p, anynans, keep: h.land_mask_i16(p, T, C, C + 5, int(big), 0, fill,
                                                                                     anynans, keep),
                                    stored, np.zeros_like(missing), C)
    finally:
        bufs.free()


# ---- gather_cells / scatter_cells: the row axis strides over a grid of at most 1024 rows -----------------------
STRIDED_ROWS = (1, 1023, 1024, 1025, 2500)


@pytest.mark.parametrize("dtype", [np.int16, np.float32, np.float64])
def test_gather_cells_every_row_and_pitch(h, dtype):
    rng = np.random.default_rng(47)
    bufs = _Bufs(h)
    ld_in = 70
    try:
        for rows in STRIDED_ROWS:
            src = (rng.normal(size=(rows, ld_in)) * 1000).astype(dtype)
            d_src = bufs.up(src)
            for n in (1, 37, 300):
                index = rng.integers(0, ld_in, size=n).astype(np.int64)          # with repeats, unsorted
                d_idx = bufs.up(index)
                d_out = bufs.canary((rows + 1, n + 3), dtype)
                h.gather_cells(d_src.ptr, np.dtype(dtype).itemsize, rows, ld_in, d_idx.ptr, n, d_out.ptr, n + 3)
                h.stream_sync(0)
                got = d_out.to_array((rows + 1, n + 3), dtype)
                npt.assert_array_equal(got[:rows, :n], src[:, index], err_msg=f"rows {rows} n {n}")
                assert _untouched(got[:rows, n:]) and _untouched(got[rows])
            bufs.free()
    finally:
        bufs.free()


def test_scatter_cells_every_row_and_pitch(h):
    """every element of out[rows][ld_out] that no index addresses is NaN (include/xmhw_amd.h); nothing behind it"""
    rng = np.random.default_rng(53)
    bufs = _Bufs(h)
    ld_out = 90
    try:
        for rows in STRIDED_ROWS:
            for n in (1, 37, 89):
                src = np.full((rows, n + 2), 1e30)
                src[:, :n] = rng.normal(size=(rows, n))
                index = np.sort(rng.choice(ld_out, size=n, replace=False)).astype(np.int64)
                d_src, d_idx = bufs.up(src), bufs.up(index)
                d_out = bufs.canary((rows + 1, ld_out), np.float64)
                h.scatter_cells(d_src.ptr, rows, n + 2, d_idx.ptr, n, d_out.ptr, ld_out)
                h.stream_sync(0)
                got = d_out.to_array((rows + 1, ld_out), np.float64)
                want = np.full((rows, ld_out), np.nan)
                want[:, index] = src[:, :n]
                npt.assert_array_equal(got[:rows], want, err_msg=f"rows {rows} n {n}")
                assert _untouched(got[rows])
                bufs.free()
            # the all-land call of device.py: no cell at all, the whole result is NaN
            d_out = bufs.canary((rows + 1, ld_out), np.float64)
            h.scatter_cells(0, rows, 1, 0, 0, d_out.ptr, ld_out)
            h.stream_sync(0)
            got = d_out.to_array((rows + 1, ld_out), np.float64)
            assert np.isnan(got[:rows]).all() and _untouched(got[rows])
            bufs.free()
    finally:
        bufs.free()


# ---- decode / encode_i16: the row axis strides over a grid of at most 2048 rows --------------------------------
CODEC_ROWS = (2047, 2048, 2049, 4100)
DECODE_PAIRS = [(">i2", np.float32, 0.01, 3.5, -32768), ("<i2", np.float32, 0.25, -1.0, 7),
                (">i2", np.float64, 0.001, 20.0, -1), (">f4", np.float32, None, None, None),
                ("<f4", np.float32, 2.0, 1.0, -999.0), (">f8", np.float64, None, None, -999.0)]


@pytest.mark.parametrize("pair", DECODE_PAIRS, ids=lambda p: f"{p[0]}-{np.dtype(p[1]).name}")
def test_decode_every_row_and_pitch(h, pair):
    raw_dt, out_dt, scale, offset, fill = pair
    dt = np.dtype(raw_dt)
    osz = np.dtype(out_dt).itemsize
    rng = np.random.default_rng(59)
    bufs = _Bufs(h)
    cols, ld_raw, ld_out = 65, 68, 70
    try:
        for rows in CODEC_ROWS:
            if dt.kind == "i":
                raw = rng.integers(-32768, 32767, size=(rows, ld_raw)).astype(dt)
            else:
                raw = rng.normal(0, 50, size=(rows, ld_raw)).astype(dt)
            if fill is not None:
                raw[::5, ::7] = fill
                raw[:, cols:] = fill                     # the pad columns: missing
            want = raw[:, :cols].astype(out_dt)
            if scale is not None:
                want = want * out_dt(scale) + out_dt(offset)
            if fill is not None:
                want[raw[:, :cols] == dt.type(fill)] = np.nan
            d_in, d_out = bufs.up(raw), bufs.canary((rows + 1, ld_out), out_dt)
            h.decode(d_in.ptr, dt.itemsize, int(dt.byteorder == ">"), rows, cols, ld_raw, d_out.ptr, osz, ld_out,
                     scale is not None, float(scale or 1.0), float(offset or 0.0), fill is not None, float(fill or 0.0))
            h.stream_sync(0)
            got = d_out.to_array((rows + 1, ld_out), out_dt)
            npt.assert_array_equal(got[:rows, :cols], want, err_msg=f"rows {rows}")
            assert np.isnan(want).any() == (fill is not None)
            assert _untouched(got[:rows, cols:]) and _untouched(got[rows])
            bufs.free()
    finally:
        bufs.free()


@pytest.mark.parametrize("scale,offset,fill", [(0.5, 1.0, -32768), (0.01, 10.0, 7), (-0.25, 3.0, -32768)])
def test_encode_i16_every_row_and_pitch(h, scale, offset, fill):
    """code = clip(rint((float64(x) - add_offset) / scale_factor), -32767, 32767), NaN -> fill: ties go to the even
    code, infinities and everything beyond the range clamp, the lowest code is never written"""
    rng = np.random.default_rng(61)
    bufs = _Bufs(h)
    cols, ld_in, ld_out = 65, 68, 70
    # exact .5 ties of both parities in float32 (scale and offset are dyadic in the first and third parameter set)
    k = np.arange(-40, 40)
    special = np.concatenate([(offset + scale * (k + 0.5)), [np.inf, -np.inf, np.nan, -0.0, 0.0, 1e9, -1e9, 3.0e38, -3.0e38],
                              offset + scale * np.array([32766.5, 32767.0, 32767.5, 32768.0, 40000.0]),
                              offset - scale * np.array([32766.5, 32767.0, 32767.5, 32768.0, 40000.0])]).astype(np.float32)
    try:
        for rows in CODEC_ROWS:
            x = (offset + scale * rng.normal(0, 9000, size=(rows, ld_in))).astype(np.float32)
            where = rng.random(x.shape) < 0.3
            x[where] = rng.choice(special, size=int(where.sum()))
            x[:, cols:] = 1e30
            with np.errstate(invalid="ignore"):
                code = np.clip(np.rint((x[:, :cols].astype(np.float64) - offset) / scale), -32767, 32767)
            want = np.where(np.isnan(x[:, :cols]), fill, code).astype(np.int16)
            d_in, d_out = bufs.up(x), bufs.canary((rows + 1, ld_out), np.int16)
            h.encode_i16(d_in.ptr, rows, cols, ld_in, d_out.ptr, ld_out, scale, offset, fill)
            h.stream_sync(0)
            got = d_out.to_array((rows + 1, ld_out), np.int16)
            npt.assert_array_equal(got[:rows, :cols], want, err_msg=f"rows {rows}")
            assert _untouched(got[:rows, cols:]) and _untouched(got[rows])
            bufs.free()
            # the inputs hold what the docstring names
            if scale in (0.5, -0.25):
                with np.errstate(invalid="ignore"):
                    exact = (x[:, :cols].astype(np.float64) - offset) / scale
                    tie = (np.abs(exact) % 1.0 == 0.5) & (np.abs(exact) < 32767)
                assert tie.sum() > 100 and (code[tie] % 2 == 0).all()
                assert (code[tie] > exact[tie]).any() and (code[tie] < exact[tie]).any()
            assert (want == 32767).any() and (want == -32767).any() and np.isnan(x[:, :cols]).any()
            assert np.isinf(x[:, :cols]).any() and (np.signbit(x[:, :cols]) & (x[:, :cols] == 0)).any()
            if fill != -32768:
                assert not (got[:rows, :cols] == -32768).any()
    finally:
        bufs.free()


# ---- pad_gaps --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("T,C", [(9, 64), (731, 300)])
def test_pad_gaps_on_a_pitched_series(h, dtype, T, C):
    """ld = C + 4: the pad columns hold a NaN run between valid samples, which the kernel must leave alone"""
    if T < 40:
        rng = np.random.default_rng(T)
        y = rng.normal(size=(T, C)).astype(dtype)
        y[rng.random((T, C)) < 0.4] = np.nan
        t = np.datetime64("2000-01-01", "D") + np.arange(T).astype("timedelta64[D]")
    else:
        y, t = _random_gappy(T, C, dtype, seed=T + C)
    x = po.interp_index(t)
    pitched = np.empty((T, C + 4), dtype=dtype)
    pitched[:, :C] = y
    pitched[:, C:] = np.arange(T, dtype=dtype)[:, None]
    pitched[3:5, C:] = np.nan
    bufs = _Bufs(h)
    try:
        d_x = bufs.up(np.ascontiguousarray(x, dtype=np.float64))
        for days in (1, 2, 3.5, 1000):
            g = days * 86400e9
            with np.errstate(invalid="ignore"):
                ref = po.interpolate_na(y, x, g)
            d_y = bufs.up(pitched)
            h.pad_gaps(d_y.ptr, y.dtype.itemsize, T, C, C + 4, d_x.ptr, float(g))
            h.stream_sync(0)
            got = d_y.to_array(pitched.shape, dtype)
            npt.assert_array_equal(got[:, :C], ref, err_msg=f"max_gap {days} days")
            npt.assert_array_equal(got[:, C:], pitched[:, C:])
            assert np.isnan(got[3:5, C:]).all()
        assert np.isnan(y).sum() > np.isnan(ref).sum()
    finally:
        bufs.free()
