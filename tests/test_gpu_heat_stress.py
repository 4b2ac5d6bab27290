"""heat_stress() and the class sums on the device against tests/heat_stress_oracle.py: exact equality of every array.
The C entries are called raw, on pitched inputs and outputs pre-filled with a bit pattern that must be gone inside
[0, C) and intact beyond it; every forced block length must give the same bits."""
import functools

import numpy as np
import numpy.testing as npt
import pytest

import heat_stress_cases as hc
import heat_stress_oracle as ho

pytestmark = pytest.mark.gpu

EXTRA = 5                       # columns past C in every pitched array
FILL32, FILL64 = -0x5A5A5A5B, -0x5A5A5A5A5A5A5A5B


@pytest.fixture(scope="module")
def dev():
    from xmhw_amd._lib import require_gpu
    require_gpu()
    import xmhw_amd.device as d
    return d


@pytest.fixture(autouse=True)
def automatic_block_afterwards():
    yield
    from xmhw_amd._lib import hip_stress
    hip_stress().set_heat_stress_block(0)


@functools.lru_cache(maxsize=None)
def _case(T, C, dtype, seed, W, D=1, cold=False, marks=(64,)):
    d = hc.synthetic(T, C, np.dtype(dtype).type, seed, W, D=D, cold=cold, marks=marks)
    return d, ho.step_fields(d["ts"], d["base"], d["rows"], W, 1.0, cold)


def _pitched(a, ld, fill):
    out = np.full(a.shape[:-1] + (ld,), fill, dtype=a.dtype)
    out[..., :a.shape[-1]] = a
    return out


def raw_stress(dev, d, W, classes, K, level_q, at, negate=False, h0=1.0, block=0, c0=0, n=None, out=None):
    """xmhw_heat_stress_accumulate_* on the columns c0 .. c0 + n - 1 of the case (all of them by default) into the
    buffers ``out`` of stress_buffers(); the inputs are pitched by EXTRA columns that would be extreme heat if a kernel
    read them."""
    from xmhw_amd._lib import hip, hip_stress
    h, hs = hip(), hip_stress()
    ts, base = d["ts"], d["base"]
    T, C = ts.shape
    n = C - c0 if n is None else n
    D, J = base.shape[0], len(at)
    ld = n + EXTRA
    hs.set_heat_stress_block(block)
    d_ts = dev.DeviceBuffer.from_array(_pitched(ts[:, c0:c0 + n], ld, 1e6))
    d_base = dev.DeviceBuffer.from_array(_pitched(base[:, c0:c0 + n], ld, -1e3 if not negate else 1e3))
    at32, lq = np.asarray(at, np.int32), np.asarray(level_q, np.int64)
    try:
        hs.heat_stress_accumulate(d_ts.ptr, ts.dtype.itemsize, T, n, ld, d_base.ptr, ld, D, d["rows"], int(negate), W, h0, classes, K,
                                  lq, at32, out["counts"].ptr + 4 * c0, out["hsum"].ptr + 8 * c0, out["key"].ptr + 8 * c0,
                                  out["snap"].ptr + 4 * c0, out["ldo"], out["cnt"].ptr)
        h.stream_sync(0)
    finally:
        d_ts.free()
        d_base.free()


def stress_buffers(dev, K, J, C):
    from xmhw_amd._lib import hip_stress
    ldo = C + EXTRA
    b = {"counts": dev.DeviceBuffer.from_array(np.full((K, 8, ldo), FILL32, np.int32)),
         "hsum": dev.DeviceBuffer.from_array(np.full((K, ldo), FILL64, np.int64)),
         "key": dev.DeviceBuffer.from_array(np.full((K, ldo), FILL64, np.int64)),
         "snap": dev.DeviceBuffer.from_array(np.full((max(J, 1), ldo), FILL32, np.int32)),
         "pq": dev.DeviceBuffer.from_array(np.full((K, ldo), FILL32, np.int32)),
         "pt": dev.DeviceBuffer.from_array(np.full((K, ldo), FILL32, np.int32)),
         "cnt": dev.DeviceBuffer.from_array(np.full(1, 123, np.int64)), "ldo": ldo, "K": K, "J": J, "C": C}
    hip_stress().heat_stress_init(K, C, b["counts"].ptr, b["hsum"].ptr, b["key"].ptr, ldo, b["cnt"].ptr)
    return b


def stress_result(b):
    """finish, read back, check the columns past C, free"""
    from xmhw_amd._lib import hip, hip_stress
    K, J, C, ldo = b["K"], b["J"], b["C"], b["ldo"]
    try:
        hip_stress().heat_stress_finish(K, C, b["key"].ptr, b["pq"].ptr, b["pt"].ptr, ldo)
        hip().stream_sync(0)
        counts, hsum = b["counts"].to_array((K, 8, ldo), np.int32), b["hsum"].to_array((K, ldo), np.int64)
        key, snap = b["key"].to_array((K, ldo), np.int64), b["snap"].to_array((max(J, 1), ldo), np.int32)
        pq, pt = b["pq"].to_array((K, ldo), np.int32), b["pt"].to_array((K, ldo), np.int32)
        cnt = b["cnt"].to_array((1,), np.int64)
    finally:
        for v in b.values():
            if hasattr(v, "free"):
                v.free()
    for a, fill in ((counts, FILL32), (hsum, FILL64), (key, FILL64), (snap, FILL32), (pq, FILL32), (pt, FILL32)):
        assert (a[..., C:] == fill).all(), "a column past C was touched"
    if J == 0:
        assert (snap == FILL32).all()
    return {"counts": counts[..., :C], "hsum_q": hsum[:, :C], "peak_q": pq[:, :C], "peak_t": pt[:, :C],
            "snap_q": snap[:J, :C], "n_range": int(cnt[0])}


def run_whole(dev, d, W, classes, K, level_q, at, negate=False, block=0):
    b = stress_buffers(dev, K, len(at), d["ts"].shape[1])
    raw_stress(dev, d, W, classes, K, level_q, at, negate, block=block, out=b)
    return stress_result(b)


def same(got, want):
    for k in ("counts", "hsum_q", "peak_q", "peak_t", "snap_q"):
        assert got[k].dtype == want[k].dtype, k
        npt.assert_array_equal(got[k], want[k], err_msg=k)
    assert got["n_range"] == want["n_range"]


def boundary_steps(T, *marks):
    at = {0, T - 1}
    for m in marks:
        for s in range(m, T, max(m, 1)):
            at.update(t for t in (s - 1, s) if 0 <= t < T)
    return sorted(at)[:64]


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("C", [1, 63, 64, 65, 255, 256, 257, 600])
def test_cell_counts_around_a_wave_and_a_workgroup(dev, dtype, C):
    T, W = 400, 84
    d, f = _case(T, C, dtype, 1000 + C, W)
    at = boundary_steps(T, 64, 100)
    for pattern in hc.PATTERNS:
        classes, K = pattern(T)
        want = ho.reduce_by_class(f, classes, K, hc.levels(3), at)
        if C >= 63:
            hc.check_case(want)
        for block in (0, 64):
            same(run_whole(dev, d, W, classes, K, hc.levels(3), at, block=block), want)


@pytest.mark.parametrize("W", [1, 2, 7, 84, 255])
def test_windows_lengths_and_forced_blocks_give_the_same_bits(dev, W):
    C = 65
    for T in sorted({1, W - 1, W, W + 1, 2 * W + 3, 400} - {0}):
        blocks = {1, W - 1, W, W + 1, 64, 0}                      # (W - 1 = 0 is the automatic block again)
        d, f = _case(T, C, "float32", 7 * W + T, W, marks=tuple(sorted({64, max(W, 2)})))
        classes, K = hc.per_year(T)
        at = boundary_steps(T, 64, max(W, 2), W + 1)
        want = ho.reduce_by_class(f, classes, K, hc.levels(2), at)
        for block in sorted(blocks):
            same(run_whole(dev, d, W, classes, K, hc.levels(2), at, block=block), want)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_a_climatology_base_with_its_rows(dev, dtype):
    T, C, W = 400, 257, 84
    d, f = _case(T, C, dtype, 44, W, D=366)
    assert d["rows"].max() == 365 and (np.diff(d["rows"]) < 0).any()
    at = boundary_steps(T, 64)
    for pattern in (hc.per_year, hc.every_step):
        classes, K = pattern(T)
        want = ho.reduce_by_class(f, classes, K, hc.levels(6), at)
        hc.check_case(want)
        for block in (0, 1, 83, 85):
            same(run_whole(dev, d, W, classes, K, hc.levels(6), at, block=block), want)


def test_level_counts_for_no_one_and_six_levels(dev):
    T, C, W = 400, 130, 84
    d, f = _case(T, C, "float32", 9, W)
    classes, K = hc.per_year(T)
    for L in (0, 1, 6):
        want = ho.reduce_by_class(f, classes, K, hc.levels(L), [])
        got = run_whole(dev, d, W, classes, K, hc.levels(L), [])
        same(got, want)
        assert (got["counts"][:, 2 + L:] == 0).all()
        if L:
            assert got["counts"][:, 2].sum() > 0
    assert ho.reduce_by_class(f, classes, K, hc.levels(6), [])["counts"][:, 7].sum() == 0     # 400 weeks: never


def test_cold_spells_negate_series_and_base(dev):
    T, C, W = 300, 100, 30
    d, f = _case(T, C, "float64", 21, W, 366, True)
    classes, K = hc.runs_of_minus_one(T)
    want = ho.reduce_by_class(f, classes, K, hc.levels(2), [0, T - 1])
    hc.check_case(want)
    same(run_whole(dev, d, W, classes, K, hc.levels(2), [0, T - 1], negate=True), want)
    warm = run_whole(dev, d, W, classes, K, hc.levels(2), [0, T - 1])
    assert (warm["hsum_q"] != want["hsum_q"]).any()


def test_out_of_range_samples_are_counted_and_move_nothing_else(dev):
    T, C, W = 200, 70, 20
    d, f = _case(T, C, "float32", 5, W)
    classes, K = hc.every_step(T)
    clean = ho.reduce_by_class(f, classes, K, hc.levels(2), [T - 1])
    bad = {k: (v.copy() if hasattr(v, "copy") else v) for k, v in d.items()}
    bad["ts"][10, 0], bad["ts"][11, 5], bad["ts"][150, 64], bad["ts"][199, 69] = 500.0, np.inf, -np.inf, 160.0
    fb = ho.step_fields(bad["ts"], bad["base"], bad["rows"], W, 1.0)
    assert fb["n_range"] == 4
    want = ho.reduce_by_class(fb, classes, K, hc.levels(2), [T - 1])
    got = run_whole(dev, bad, W, classes, K, hc.levels(2), [T - 1])
    same(got, want)
    untouched = np.ones(C, bool)
    untouched[[0, 5, 64, 69]] = False
    for k in ("hsum_q", "peak_q", "peak_t"):
        npt.assert_array_equal(got[k][:, untouched], clean[k][:, untouched])


def test_slabs_add_up_to_the_whole(dev):
    T, C, W = 300, 330, 84
    d, f = _case(T, C, "float32", 77, W)
    classes, K = hc.per_year(T)
    at = boundary_steps(T, 100)
    want = ho.reduce_by_class(f, classes, K, hc.levels(3), at)
    for cuts in ((0, 129, C), (0, 1, 257, C), (0, 64, 65, C)):
        b = stress_buffers(dev, K, len(at), C)
        for c0, c1 in zip(cuts[:-1], cuts[1:]):
            raw_stress(dev, d, W, classes, K, hc.levels(3), at, c0=c0, n=c1 - c0, out=b)
        same(stress_result(b), want)
    # a single-cell slab alone: the other columns keep the zeros of init
    b = stress_buffers(dev, K, len(at), C)
    raw_stress(dev, d, W, classes, K, hc.levels(3), at, c0=200, n=1, out=b)
    got = stress_result(b)
    for k in ("counts", "hsum_q", "peak_q", "peak_t", "snap_q"):
        npt.assert_array_equal(got[k][..., 200], want[k][..., 200])
    assert (got["counts"][..., :200] == 0).all() and (got["peak_t"][:, 201:] == -1).all() and (got["peak_q"][:, :200] == 0).all()


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_class_sums_raw(dev, dtype):
    from xmhw_amd._lib import hip, hip_stress
    h, hs = hip(), hip_stress()
    T = 400
    for C in (1, 65, 257, 600):
        d, _ = _case(T, C, dtype, 300 + C, 84)
        ts = d["ts"].copy()
        ts[7, 0] = 500.0                                          # out of range: counted, left out
        ld = ldo = C + EXTRA
        for pattern in hc.PATTERNS:
            classes, K = pattern(T)
            want = ho.class_sums(ts, 20.0, classes, K)
            assert want["n_range"] == (1 if classes[7] >= 0 else 0) and want["n_valid"].sum() > 0
            for block in (0, 1, 7, 64):
                hs.set_heat_stress_block(block)
                bufs = [dev.DeviceBuffer.from_array(a) for a in (_pitched(ts, ld, 1e6), np.full((K, ldo), FILL32, np.int32),
                                                                 np.full((K, ldo), FILL64, np.int64), np.full(1, 9, np.int64))]
                d_ts, d_n, d_s, d_c = bufs
                try:
                    hs.class_sums_init(K, C, d_n.ptr, d_s.ptr, ldo, d_c.ptr)
                    hs.class_sums_accumulate(d_ts.ptr, ts.dtype.itemsize, T, C, ld, 20.0, classes, K, d_n.ptr, d_s.ptr, ldo, d_c.ptr)
                    h.stream_sync(0)
                    n, s, cnt = d_n.to_array((K, ldo), np.int32), d_s.to_array((K, ldo), np.int64), d_c.to_array((1,), np.int64)
                finally:
                    for b in bufs:
                        b.free()
                npt.assert_array_equal(n[:, :C], want["n_valid"])
                npt.assert_array_equal(s[:, :C], want["sum_q"])
                assert cnt[0] == want["n_range"] and (n[:, C:] == FILL32).all() and (s[:, C:] == FILL64).all()


def _grid(T, ny, nx, seed):
    rng = np.random.default_rng(seed)
    time = np.datetime64("2001-01-01") + np.arange(T).astype("timedelta64[D]")
    x = (20.0 + 3.0 * np.sin(2 * np.pi * np.arange(T) / 365.25)[:, None, None] + rng.normal(0, 1.2, (T, ny, nx))).astype(np.float32)
    x[:, rng.random((ny, nx)) < 0.3] = np.nan
    x[:, 2, :] = np.nan                                              # a dead grid line
    x[rng.random(x.shape) < 0.01] = np.nan
    from xmhw_amd import GridSeries
    return GridSeries(x, ("time", "lat", "lon"), {"time": time, "lat": np.arange(ny) * 0.25, "lon": np.arange(nx) * 0.25})


def _same_dataset(a, b, names):
    for k in names:
        npt.assert_array_equal(getattr(a, k), getattr(b, k), err_msg=k)


STRESS_FIELDS = ("klass", "n_steps", "n_valid", "n_hot", "n_level", "hsum_q", "peak_q", "peak_t", "snap_q", "keep", "dhw_peak",
                 "dhw_at", "degree_days")
MMM_FIELDS = ("n_valid", "sum_q", "monthly_mean", "mmm", "keep")


def test_public_functions_equal_the_host_path_with_the_oracle(dev, oisst):
    from xmhw_amd import GridSeries, degree_heating_weeks, heat_stress, maximum_monthly_mean
    temp = GridSeries(oisst["sst"], ("time", "lat", "lon"), {"time": oisst["time64"], "lat": oisst["lat"], "lon": oisst["lon"]})
    for series, kw in ((temp, dict(levels=(1, 2), at=[0, 590, 730])), (_grid(800, 9, 14, 4), dict(at=[83, 799], window=60))):
        mm = maximum_monthly_mean(series)
        mm_host = maximum_monthly_mean(series, _compute=ho.class_sums_cells)
        _same_dataset(mm, mm_host, MMM_FIELDS)
        for extra in (dict(), dict(max_batch_bytes=1 << 14), dict(classes="month", coldSpells=True)):
            got = heat_stress(series, mm, **kw, **extra)
            host = heat_stress(series, mm_host, _compute=ho.heat_stress_cells, **kw, **{k: v for k, v in extra.items() if k != "max_batch_bytes"})
            _same_dataset(got, host, STRESS_FIELDS)
        assert got.keep.sum() == mm.keep.sum() > 0
        _same_dataset(degree_heating_weeks(series, **kw), heat_stress(series, mm_host, _compute=ho.heat_stress_cells, **kw), STRESS_FIELDS)
    # a point series
    p = GridSeries(oisst["sst"][:, 2, 2], ("time",), {"time": oisst["time64"]})
    _same_dataset(heat_stress(p, 27.0, levels=(1, 2)), heat_stress(p, 27.0, levels=(1, 2), _compute=ho.heat_stress_cells), STRESS_FIELDS)
