"""The per-row bookkeeping of the sorted-list kernel (kernels_sorted.hip, step 3 and the register-rank check 4c) is done with
mask bit operations, a count taken from the sorted run (sorted_count.h) and one "is any own list saturated" test instead of
selects, a compare per key and a compare per list.  None of it may change a result: thresh is compared BIT FOR BIT, and
seas to the rounding of another summation order, with `clim_generic` (an independent algorithm) on the same device
buffers, as tests/test_gpu_sorted.py does.

Shapes: 96 cells (three waves: the last one full, the middle of a strip) and 33 (a wave with 31 padded cells).  Records: 37,
39 and 40 years (odd and even track counts on the K = 16 / KL = 14 body, the padded last track), 12 years (6 tracks per lane:
three waves per SIMD), 43 years (K = 18 / KL = 16).  Calendars: daily with leap years, without, a record that starts on
Feb 29.  Data in one field: white noise on a seasonal cycle, a third of the cells quantised to 0.01 (ties and the tie branch),
a constant cell (saturated lists: the register-rank check and the capacity path), a +inf and a -inf in cells of their own;
and a field with 5 % NaN.  Quantiles 0.9, 0.1 (mirrored), 0.85 and 1.0.  int16 codes read in place in modes 1 (float32
decode) and 2 (float64 decode: the kernel selects on the codes) at 40 years: the body is shared.
"""
import numpy as np
import numpy.testing as npt
import pytest

import xmhw_oracle as ora

pytestmark = pytest.mark.gpu

SORTED = 40
FILL = -32768


@pytest.fixture(scope="module")
def dev():
    from xmhw_amd._lib import require_gpu
    require_gpu()
    import xmhw_amd.device as d
    return d


def _doy(calendar, years):
    if calendar == "leap":
        return ora.add_doy(np.arange("1982-01-01", f"{1982 + years}-01-01", dtype="datetime64[D]"))
    if calendar == "feb29":       # the record starts on a Feb 29 and ends with a February
        return ora.add_doy(np.arange("1984-02-29", f"{1984 + years}-03-01", dtype="datetime64[D]"))
    assert calendar == "noleap"   # a 365-day calendar: doy 60 never occurs
    d = (np.arange(years * 365) % 365 + 1).astype(np.int64)
    return np.where(d >= 60, d + 1, d)


def _field(T, C, seed, kind):
    rng = np.random.default_rng(seed)
    t = np.arange(T)[:, None]
    x = 15.0 + rng.uniform(2, 10, C) * np.sin(2 * np.pi * (t - rng.uniform(0, 365, C)) / 365.25) + rng.normal(size=(T, C))
    x[:, C // 3:2 * C // 3] = np.round(x[:, C // 3:2 * C // 3] / 0.01) * 0.01
    x = x.astype(np.float32)
    if kind == "nan5":
        x[rng.random((T, C)) < 0.05] = np.nan
    else:
        assert kind == "mixed"
        x[:, 1] = 7.0
        x[T // 3, 2] = np.inf
        x[T // 2, 3] = -np.inf
    return x


def _run(dev, doy, C, fn, **plan_kw):
    plan = dev.Plan(doy, 5, **plan_kw)
    th, se = dev.DeviceBuffer(8 * plan.D * C), dev.DeviceBuffer(8 * plan.D * C)
    try:
        use = plan.layout_in_use()
        fn(plan, th, se)
        dev.hip().stream_sync(0)
        return th.to_array((plan.D, C), np.float64), se.to_array((plan.D, C), np.float64), use
    finally:
        th.free()
        se.free()
        plan.destroy()


def _check_f32(dev, x, doy, q):
    C = x.shape[1]
    d_ts = dev.DeviceBuffer.from_array(x)
    try:
        def clim(plan, th, se):
            dev.clim_raw(plan, d_ts, 4, C, q, False, th, se)
        tg, sg, _ = _run(dev, doy, C, clim, kernel="generic")
        t1, s1, use = _run(dev, doy, C, clim, layout="sorted")
    finally:
        d_ts.free()
    assert use == SORTED
    with np.errstate(invalid="ignore"):
        npt.assert_array_equal(t1, tg)
        npt.assert_allclose(s1, sg, rtol=1e-12, atol=1e-300, equal_nan=True)
    return t1


@pytest.mark.parametrize("C", [96, 33])
@pytest.mark.parametrize("years", [37, 39, 40, 12, 43])
def test_mixed_field_every_body(dev, years, C):
    doy = _doy("leap", years)
    t1 = _check_f32(dev, _field(doy.shape[0], C, 1000 + years + C, "mixed"), doy, 0.9)
    assert (t1[:, 1] == 7.0).all()            # the constant cell
    assert np.isfinite(t1[:, 0]).all()


@pytest.mark.parametrize("years,C", [(39, 96), (40, 96), (40, 33), (12, 96), (43, 96)])
def test_five_per_cent_nan(dev, years, C):
    doy = _doy("leap", years)
    _check_f32(dev, _field(doy.shape[0], C, 2000 + years + C, "nan5"), doy, 0.9)


@pytest.mark.parametrize("q", [0.1, 0.85, 1.0])
@pytest.mark.parametrize("years", [39, 40, 12, 43])
def test_quantiles(dev, years, q):
    doy = _doy("leap", years)
    _check_f32(dev, _field(doy.shape[0], 96, 3000 + years, "mixed"), doy, q)


def test_mirrored_quantile_with_nan(dev):
    doy = _doy("leap", 40)
    _check_f32(dev, _field(doy.shape[0], 33, 3100, "nan5"), doy, 0.1)


@pytest.mark.parametrize("calendar", ["noleap", "feb29"])
@pytest.mark.parametrize("years", [37, 40, 12])
def test_calendars(dev, years, calendar):
    doy = _doy(calendar, years)
    _check_f32(dev, _field(doy.shape[0], 33, 4000 + years, "mixed"), doy, 0.9)


@pytest.mark.parametrize("C", [96, 33])
@pytest.mark.parametrize("q", [0.9, 0.1])
@pytest.mark.parametrize("decoded", ["float32", "float64"])
def test_int16_codes_in_place(dev, decoded, q, C):
    """mode 1 (float32 attributes: the samples are float32(code) * sf + of) and mode 2 (float64 attributes: the kernel selects
    on the codes and decodes the two selected ones) against the generic kernel on the series xmhw_decode makes of the codes;
    a third of the cells on a coarse grid of codes (ties), a constant cell, 1 % fill codes"""
    doy = _doy("leap", 40)
    T = doy.shape[0]
    out = np.float32 if decoded == "float32" else np.float64
    scale, offset = (float(np.float32(0.01)), float(np.float32(10.0))) if decoded == "float32" else (0.01, 10.0)
    x = _field(T, C, 5000 + C, "nan5" if q == 0.1 else "mixed")
    x[:, 1] = 7.0
    with np.errstate(invalid="ignore"):
        codes = np.where(np.isfinite(x), np.clip(np.rint((x.astype(np.float64) - 10.0) / 0.01), -32767, 32767), FILL).astype(np.int16)
    codes[:, C // 3:C // 2] = codes[:, C // 3:C // 2] // 50 * 50
    rng = np.random.default_rng(C)
    codes[rng.random((T, C)) < 0.01] = FILL
    h = dev.hip()
    d_codes = dev.DeviceBuffer.from_array(codes)
    isz = np.dtype(out).itemsize
    d_ts = dev.DeviceBuffer(isz * T * C)
    try:
        h.decode(d_codes.ptr, 2, 0, T, C, C, d_ts.ptr, isz, C, True, scale, offset, True, float(FILL), 0)
        h.stream_sync(0)
        tg, sg, _ = _run(dev, doy, C, lambda plan, th, se: dev.clim_raw(plan, d_ts, isz, C, q, False, th, se), kernel="generic")
        tp, sp, use = _run(dev, doy, C, lambda plan, th, se: dev.clim_raw_packed(
            plan, d_codes, C, q, False, th, se, scale_factor=scale, add_offset=offset, fill=FILL, decoded=decoded))
    finally:
        d_codes.free()
        d_ts.free()
    assert use == SORTED
    npt.assert_array_equal(tp, tg)
    npt.assert_allclose(sp, sg, rtol=1e-12, atol=1e-12, equal_nan=True)

