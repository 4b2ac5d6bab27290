"""mhw_displacement() on the device against tests/displacement_oracle.py (a brute force over all grid points that uses no
candidate list): exact equality of every integer field and of n_visited."""
import functools

import numpy as np
import numpy.testing as npt
import pytest

import days_by_cases as dbc
import displacement_cases as dc
import displacement_oracle as ora

pytestmark = pytest.mark.gpu

GRIDS = ((1, 1), (1, 70), (3, 64), (5, 65), (7, 130), (12, 200))
TS = (1, 63, 64, 65, 130)


@pytest.fixture(scope="module")
def dev():
    from xmhw_amd._lib import require_gpu
    require_gpu()
    import xmhw_amd.device as d
    return d


@pytest.fixture(scope="module")
def stage(dev):
    from xmhw_amd.displacement import displacement_grid
    return displacement_grid


@functools.lru_cache(maxsize=None)
def _case(ny, nx, T, **kw):
    kw = dict(kw)
    if "pattern" in kw:
        kw["classes"] = dbc.PATTERNS[kw.pop("pattern")]
    case = dc.stage_case(ny, nx, T, **kw)
    return case, dc.run_stage(ora.displacement_grid, case)


def _variant(gi, ti):
    """what varies over the matrix of grids and lengths: dtype, wrap, class pattern, reach"""
    n = gi * len(TS) + ti
    return dict(seed=n, dtype=(np.float32, np.float64)[n % 2], periodic=bool((n // 2) % 2), pattern=n % 3,
                max_distance=(400.0, 900.0, 2500.0)[n % 3])


@pytest.mark.parametrize("ti", range(len(TS)))
@pytest.mark.parametrize("gi", range(len(GRIDS)))
def test_grids_and_lengths(stage, gi, ti):
    """30 % land with a fully land row, NaN holes, a NaN target, float32 / float64, wrap on and off, every class pattern"""
    (ny, nx), T = GRIDS[gi], TS[ti]
    case, want = _case(ny, nx, T, **_variant(gi, ti))
    if ny * nx > 1 and T > 1:
        dc.check_case(want, far=nx * ny > 64, unreached=False)
    dc.assert_same(dc.run_stage(stage, case), want)


def test_the_matrix_covers_what_it_claims():
    seen = {"found": 0, "unreached": 0, "far": 0, "classes": set()}
    for gi, (ny, nx) in enumerate(GRIDS):
        for ti, T in enumerate(TS):
            v = _variant(gi, ti)
            case, want = _case(ny, nx, T, **v)
            seen["found"] += int(want["n_found"].sum())
            seen["unreached"] += int((want["n_days"] - want["n_found"]).sum())
            seen["far"] += int((want["max_m"] > 300000).sum())
            seen["classes"].add(v["pattern"])
            assert ny < 3 or not case["keep"][1].any(), "the fully land row"
    assert min(seen["found"], seen["unreached"], seen["far"]) > 100 and seen["classes"] == {0, 1, 2}


@pytest.mark.parametrize("pattern", range(len(dbc.PATTERNS)))
@pytest.mark.parametrize("periodic", [False, True])
def test_class_patterns(stage, pattern, periodic):
    case, want = _case(7, 130, 210, seed=40 + pattern, periodic=periodic, pattern=pattern, max_distance=1200.0,
                       dlon=360.0 / 130 if periodic else 1.0)
    dc.check_case(want)
    assert (want["n_days"].sum(axis=1) > 0).all(), "a class without sources"
    dc.assert_same(dc.run_stage(stage, case), want)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_two_basins_and_excluded_points(stage, dtype):
    case, want = _case(5, 65, 65, seed=5, dtype=dtype, basin=True, max_distance=5000.0, pattern=1)
    open_case, open_want = _case(5, 65, 65, seed=5, dtype=dtype, basin=False, max_distance=5000.0, pattern=1)
    dc.check_case(want)
    excluded = case["basin"][case["cell_index"]] < 0
    assert excluded.any() and (want["n_days"][:, excluded] == 0).all()
    assert want["sum_m"].sum() > 0 and open_want["n_found"].sum() != want["n_found"].sum()
    dc.assert_same(dc.run_stage(stage, case), want)


@pytest.mark.parametrize("periodic", [False, True])
def test_cold_spells(stage, periodic):
    case, want = _case(5, 65, 64, seed=8, cold=True, periodic=periodic, pattern=2, max_distance=1500.0)
    dc.check_case(want)
    dc.assert_same(dc.run_stage(stage, case), want)


@pytest.mark.parametrize("nx", [64, 65, 130])
def test_only_the_source_is_listed(stage, nx):
    case, want = _case(3, nx, 65, seed=9, max_distance=0.0)
    assert case["table"].n_entries == 3
    dc.check_case(want, far=False)
    assert want["n_visited"] == want["n_days"].sum() and want["max_m"].max() == 0
    dc.assert_same(dc.run_stage(stage, case), want)


@pytest.mark.parametrize("periodic", [False, True])
def test_lists_reach_past_every_grid_edge(stage, periodic):
    case, want = _case(5, 65, 63, seed=10, max_distance=20016.0, periodic=periodic, dtype=np.float64)
    per_row = 5 * (65 if periodic else 129)
    npt.assert_array_equal(np.diff(case["table"].row_offsets), per_row)
    dc.check_case(want, unreached=False)
    dc.assert_same(dc.run_stage(stage, case), want)


def test_uniformly_warm_field_no_source_finds_anything(stage):
    case, want = _case(7, 130, 64, seed=11, field="warm", holes=0.0, max_distance=5000.0)     # lists of some 600 entries
    assert want["n_days"].sum() > 1000 and want["n_found"].sum() == 0 and want["sum_m"].sum() == 0
    n = np.diff(case["table"].row_offsets)
    rows = case["cell_index"] // 130
    assert want["n_visited"] == int((want["n_days"][0] * n[rows]).sum())        # every source walks its whole list
    dc.assert_same(dc.run_stage(stage, case), want)


def test_every_source_finds_itself(stage):
    case, want = _case(7, 130, 64, seed=12, field="cool", holes=0.0, max_distance=700.0)
    nan_target = 1                                      # stage_case() plants one NaN target: that source finds nothing
    assert want["n_days"].sum() - want["n_found"].sum() <= nan_target and want["max_m"].max() == 0
    dc.assert_same(dc.run_stage(stage, case), want)


@pytest.mark.parametrize("steps", [1, 7, 64, 65])
def test_time_blocks_do_not_change_a_bit(stage, steps):
    case, want = _case(7, 130, 130, seed=13, pattern=1, periodic=True, max_distance=900.0)
    one = dc.run_stage(stage, case)
    dc.assert_same(one, want)
    dc.assert_same(dc.run_stage(stage, case, block_steps=steps), one)


def test_time_blocks_from_the_budget(stage):
    """max_batch_bytes below one step still moves one step at a time"""
    case, want = _case(3, 64, 65, seed=14, pattern=2)
    dc.assert_same(dc.run_stage(stage, case, max_batch_bytes=1), want)


@pytest.mark.parametrize("steps", [1, 5, 64])
def test_blocks_inside_the_kernel_do_not_change_a_bit(dev, stage, steps):
    case, want = _case(5, 65, 130, seed=15, pattern=2, max_distance=900.0)
    h = dev.hip()
    h.set_displacement_block(steps)
    try:
        got = dc.run_stage(stage, case)
    finally:
        h.set_displacement_block(0)
    dc.assert_same(got, want)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_pitched_series_with_canary_columns(dev, dtype):
    """The block is read with its leading dimension: the columns between the rows hold a value that would qualify for
    every source, so reading one changes the result; they come back untouched."""
    from xmhw_amd import displacement as dp
    case, want = _case(5, 65, 64, seed=16, dtype=dtype, pattern=1, max_distance=900.0)
    field = case["field"]
    T, N = field.shape
    ld = N + 7
    pitched = np.full((T, ld), -1.0e6, dtype=dtype)
    pitched[:, :N] = field
    _, rows, cop, classes, K, basin = dp.check_stage_inputs(field, case["seas"], case["rows"], case["view"], case["cell_index"],
                                                            case["table"], case["classes"], case["K"], None)
    acc = dp._Accumulators(case["view"], cop, case["table"], classes, K, basin, False, T, rows)
    try:
        with dev.DeviceScope() as s:
            d_ts, d_se = s.upload(pitched), s.upload(case["seas"])
            for t0, nt in ((0, 10), (10, 54)):
                acc.add_block(d_ts.ptr + t0 * ld * pitched.itemsize, pitched.itemsize, ld, t0, nt, d_se.ptr,
                              case["seas"].shape[1], case["seas"].shape[0])
            got = acc.result()
            back = d_ts.to_array((T, ld), dtype)
    finally:
        acc.free()
    dc.assert_same(got, want)
    npt.assert_array_equal(back, pitched)


def test_c_abi_refusals(dev):
    """before anything is touched: every pointer is 0"""
    h = dev.hip()
    rows, cls = np.zeros(4, np.int32), np.zeros(4, np.int32)

    def accumulate(K=1, T=4, ny=2, nx=2, C=4, classes=cls, row_of_t=rows, t0=0, nt=4):
        h.displacement_accumulate(0, 4, ny * nx, t0, nt, T, ny, nx, 0, 0, C, 1, row_of_t, 0, 0, C, 0, C, 0, 0, 0, 0, 0, 0, 0,
                                  classes, K, 0, 0, 0, 0, 0, 0, C, 0)

    for K in (0, 1025):
        with pytest.raises(h.Unsupported, match=r"K must be in \[1, 1024\]"):
            h.displacement_init(K, 4, 0, 0, 0, 0, 0, 0, 4, 0)
        with pytest.raises(h.Unsupported, match=r"K must be in \[1, 1024\]"):
            accumulate(K=K)
    with pytest.raises(h.Unsupported, match="2\\^31 cells"):
        h.displacement_init(1, 1 << 31, 0, 0, 0, 0, 0, 0, 1 << 31, 0)
    with pytest.raises(h.Unsupported, match="2\\^31 cells"):
        accumulate(C=1 << 31)
    with pytest.raises(h.Unsupported, match="2\\^15"):
        accumulate(nx=1 << 15)
    with pytest.raises(h.InvalidArgument, match=r"class_of_t outside \[-1, K\)"):
        accumulate(classes=np.array([0, 1, 0, 0], np.int32))
    with pytest.raises(h.InvalidArgument, match=r"class_of_t outside \[-1, K\)"):
        accumulate(classes=np.array([0, -2, 0, 0], np.int32))
    with pytest.raises(h.InvalidArgument, match=r"row_of_t outside \[0, D\)"):
        accumulate(row_of_t=np.array([0, 0, 1, 0], np.int32))
    with pytest.raises(h.InvalidArgument, match="bad T/t0/nt"):
        accumulate(t0=2, nt=3)
    with pytest.raises(h.InvalidArgument, match="NULL"):
        accumulate()


@functools.lru_cache(maxsize=None)
def _blob_inputs():
    """Twelve years on an 8 x 12 grid, one degree apart: a seasonal cycle that is the same everywhere, noise, and a warm
    blob of four degrees centred on (4, 6) for forty days of the last year (twelve years: the blob's eleven samples per
    window stay below the top tenth of 132, so the threshold does not climb into it).  Two land points."""
    from xmhw_amd import GridSeries
    ny, nx = 8, 12
    time = np.arange("2001-01-01", "2013-01-01", dtype="datetime64[D]")
    T = time.shape[0]
    rng = np.random.default_rng(3)
    jj, ii = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    x = 15.0 + 5.0 * np.sin(2 * np.pi * np.arange(T) / 365.25)[:, None, None] + 0.3 * rng.standard_normal((T, ny, nx))
    r2 = (jj - 4) ** 2 + (ii - 6) ** 2
    x[4100:4140] += 4.0 * np.exp(-r2 / 6.0)[None]
    x[:, 0, 0] = np.nan
    x[:, 7, 3] = np.nan
    lat, lon = 10.0 + np.arange(ny), 200.0 + np.arange(nx)
    return GridSeries(x.astype(np.float32), ("time", "lat", "lon"), {"time": time, "lat": lat, "lon": lon},
                      time_encoding={"calendar": "proleptic_gregorian"})


def test_threshold_detect_displacement_end_to_end(dev):
    from xmhw_amd import add_doy, climatology_series, detect, displacement_offsets, mhw_displacement, threshold
    temp = _blob_inputs()
    clim = threshold(temp)
    th, se = climatology_series(clim, "thresh"), climatology_series(clim, "seas")
    mhw = detect(temp, th, se)
    res = mhw_displacement(temp, th, se, mhw, classes="year", max_distance=1500.0)
    again = mhw_displacement(temp, th, se, mhw, classes="year", max_distance=1500.0, max_batch_bytes=1 << 20)     # two time blocks
    ny, nx = 8, 12
    T = temp.values.shape[0]
    keep = np.asarray(mhw.keep).reshape(-1)
    assert keep.sum() == ny * nx - 2
    time = temp.coords["time"]
    year = time.astype("datetime64[Y]").astype(int) + 1970
    rows = np.searchsorted(np.asarray(se.coords["doy"]), add_doy(time)).astype(np.int32)
    seas = np.asarray(se.values).reshape(len(se.coords["doy"]), -1)[:, keep]
    table = displacement_offsets(temp.coords["lat"], nx, 1.0, 1500.0)
    want = ora.displacement_grid(temp.values.reshape(T, -1), seas, rows, mhw.compact_view(), np.nonzero(keep)[0], table,
                                 year - 2001, 12)
    dc.check_case(want, unreached=False)
    npt.assert_array_equal(res.klass, np.arange(2001, 2013))
    for name in dc_fields():
        full = np.zeros((12, ny * nx), dtype=want[name].dtype)
        full[:, keep] = want[name]
        npt.assert_array_equal(getattr(res, name), full.reshape(12, ny, nx), err_msg=name)
        npt.assert_array_equal(getattr(again, name), getattr(res, name), err_msg=name)
    assert res.attrs["n_visited"] == again.attrs["n_visited"] == want["n_visited"]
    # the blob: its days are sources in its year, and the way out is the longer the nearer the centre
    mean = res.displacement_mean_km[11]
    assert res.n_days[11, 4, 6] >= 35 and res.n_found[11, 4, 6] >= 35
    assert mean[4, 6] > mean[4, 8] > 0.0 and mean[4, 6] > mean[2, 6] > 0.0 and mean[4, 6] > 200.0


def dc_fields():
    from xmhw_amd.displacement import STAGE_FIELDS
    return STAGE_FIELDS
