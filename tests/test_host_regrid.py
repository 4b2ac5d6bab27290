"""The host side of regrid() without a device: bounds and overlap tables against a brute-force float64 overlap, the
mirror and the longitude conventions, exact constants, the identity, conservation and the quantisation bound with the
numpy oracle (tests/regrid_oracle.py) standing in for the device stage, the refusals of the C entries in their stated
order, and the frame of the result."""
import importlib

import numpy as np
import numpy.testing as npt
import pytest

import regrid_cases as rc
import regrid_oracle as ro
from xmhw_amd import GridSeries, XmhwException, axis_bounds, overlap_table, regrid

STAGE = ro.as_stage
rg = importlib.import_module("xmhw_amd.regrid")            # (xmhw_amd.regrid itself is the function)


def brute_overlap(src, dst, measure, period=None):
    """(m, n) float64: the overlap of every destination cell with every source cell, pair by pair (a periodic source
    is met two periods to either side as well)"""
    f = (lambda v: np.sin(np.deg2rad(v))) if measure == "sphere" else (lambda v: v)
    s, d = f(np.asarray(src, np.float64)), f(np.asarray(dst, np.float64))
    slo, shi = np.minimum(s[:-1], s[1:])[None], np.maximum(s[:-1], s[1:])[None]
    dlo, dhi = np.minimum(d[:-1], d[1:])[:, None], np.maximum(d[:-1], d[1:])[:, None]
    out = np.zeros((len(dst) - 1, len(src) - 1))
    for k in ((-2, -1, 0, 1, 2) if period else (0,)):
        shift = k * (period or 0.0)
        out += np.clip(np.minimum(dhi, shi + shift) - np.maximum(dlo, slo + shift), 0.0, None)
    return out


def dense(table, n):
    """(m, n) int64 weights of a CSR table"""
    first, ptr, w, _ = table
    out = np.zeros((len(first), n), np.int64)
    for J in range(len(first)):
        for k in range(ptr[J + 1] - ptr[J]):
            out[J, (first[J] + k) % n] += w[ptr[J] + k]
    return out


GEOMETRIES = [
    # (source bounds, destination bounds, measure, period)
    (np.linspace(-90, 90, 37), np.linspace(-90, 90, 10), "sphere", None),                     # 5 -> 20 degrees, nested
    (np.linspace(-90, 90, 37), axis_bounds(np.linspace(90, -90, 37), (-90, 90)), "sphere", None),   # shifted, descending
    (np.linspace(90, -90, 19), np.linspace(-80, 80, 65), "sphere", None),                     # descending source, refining
    (np.linspace(-30, 30, 25), np.array([-45.0, -31, -29.5, 0.3, 7, 29, 40, 50]), "plane", None),   # uneven, partly outside
    (np.linspace(0, 360, 73), np.linspace(-180, 180, 31), "plane", 360.0),                    # the other longitude convention
    (np.linspace(0, 360, 73), np.linspace(-2.5, 357.5, 73), "plane", 360.0),                  # shifted across the seam
    (np.linspace(0, 360, 13), np.linspace(355, -5, 41), "plane", 360.0),                      # descending destination, refining
    (np.linspace(100, 200, 21), np.linspace(90, 210, 13), "plane", None),                     # a regional longitude
]


def test_axis_bounds():
    npt.assert_array_equal(axis_bounds([0.125, 0.375, 0.625]), [0.0, 0.25, 0.5, 0.75])
    npt.assert_array_equal(axis_bounds([90.0, 0.0, -90.0], (-90, 90)), [90.0, 45.0, -45.0, -90.0])
    npt.assert_array_equal(axis_bounds([1.0, 2.0, 4.0]), [0.5, 1.5, 3.0, 5.0])
    npt.assert_array_equal(axis_bounds([5.0], (0, 10)), [0.0, 10.0])
    for bad in ([1.0, 1.0], [1.0, 3.0, 2.0], [], [[1.0, 2.0]], [np.nan, 1.0]):
        with pytest.raises(XmhwException):
            axis_bounds(bad)
    with pytest.raises(XmhwException, match="limits"):
        axis_bounds([5.0])


@pytest.mark.parametrize("g", range(len(GEOMETRIES)))
def test_overlap_tables_equal_brute_force(g):
    src, dst, measure, period = GEOMETRIES[g]
    first, ptr, w, full = overlap_table(src, dst, measure, period)
    n, m = len(src) - 1, len(dst) - 1
    cnt = np.diff(ptr)
    assert first.dtype == ptr.dtype == w.dtype == full.dtype == np.int32 and ptr[0] == 0 and len(w) == ptr[-1]
    assert (cnt <= 64).all() and (w >= 0).all() and (w <= 4096).all() and (full <= 1 << 18).all()
    brute = brute_overlap(src, dst, measure, period)
    got = dense((first, ptr, w, full), n)
    f = (lambda v: np.sin(np.deg2rad(v))) if measure == "sphere" else (lambda v: v)
    extent = np.abs(np.diff(f(np.asarray(dst, float))))
    for J in range(m):
        if brute[J].max() <= 0:
            assert cnt[J] == 0
            continue
        unit = 4096 / brute[J].max()
        # every weight is the overlap in the run's unit, rounded once; a dropped end cell rounded to 0
        npt.assert_array_less(np.abs(got[J] - brute[J] * unit), 0.5 + 1e-6)
        assert w[ptr[J]:ptr[J + 1]].max() == 4096 and w[ptr[J]] > 0 and w[ptr[J + 1] - 1] > 0
        # the weights of a run sum to the extent at most; to the extent (within the roundings) where the cell is inside
        assert w[ptr[J]:ptr[J + 1]].sum() <= full[J] and abs(full[J] - extent[J] * unit) <= 0.5 * cnt[J] + 0.5 + 1e-6
        if abs(brute[J].sum() - extent[J]) < 1e-12:
            assert w[ptr[J]:ptr[J + 1]].sum() == full[J]         # inside the source: the run sums to the extent
        else:
            assert w[ptr[J]:ptr[J + 1]].sum() < full[J]
        assert period is not None or first[J] + cnt[J] <= n


def test_ascending_and_descending_axes_give_mirrored_tables():
    src, dst = np.linspace(-90, 90, 37), axis_bounds(np.linspace(-87.5, 87.5, 15), (-90, 90))
    up = overlap_table(src, dst, "sphere")
    n, m = len(src) - 1, len(dst) - 1
    # the destination reversed: the runs in reverse order
    down_dst = overlap_table(src, dst[::-1], "sphere")
    npt.assert_array_equal(dense(down_dst, n), dense(up, n)[::-1])
    npt.assert_array_equal(down_dst[3], up[3][::-1])
    # the source reversed: every run mirrored in memory order
    down_src = overlap_table(src[::-1], dst, "sphere")
    npt.assert_array_equal(dense(down_src, n), dense(up, n)[:, ::-1])
    npt.assert_array_equal(down_src[0], n - (up[0] + np.diff(up[1])))
    both = overlap_table(src[::-1], dst[::-1], "sphere")
    npt.assert_array_equal(dense(both, n), dense(up, n)[::-1, ::-1])
    assert m == 15


def field_on(lat, lon, T=3, seed=0, dtype=np.float32, land=False):
    rng = np.random.default_rng(seed)
    x = (12.0 + 6.0 * np.cos(np.deg2rad(lat))[None, :, None] + rng.normal(0, 1.5, (T, lat.size, lon.size))).astype(dtype)
    if land:
        x[:, lat.size // 3:lat.size // 3 + 3, lon.size // 4:lon.size // 4 + 5] = np.nan
        x[rng.random(x.shape) < 0.03] = np.nan
    return GridSeries(x, ("time", "lat", "lon"), {"time": np.arange(T), "lat": lat, "lon": lon}, attrs={"units": "degC"})


def test_both_longitude_conventions_give_the_same_result():
    lat, lon = np.arange(-58.75, 60, 2.5), np.arange(1.25, 360, 2.5)
    temp = field_on(lat, lon, land=True)
    dlat = np.arange(-55.0, 56, 5.0)
    a, ia = regrid(temp, lat=dlat, lon=np.arange(0.0, 360, 5.0), _compute=STAGE)
    b, ib = regrid(temp, lat=dlat, lon=np.arange(-180.0, 180, 5.0), _compute=STAGE)
    assert ia.periodic and ib.periodic
    # 0 .. 355 against -180 .. 175: the same cells, rotated by half the circle
    npt.assert_array_equal(np.roll(a.values, 36, axis=2).view(np.uint32), b.values.view(np.uint32))
    assert (~np.isnan(a.values)).sum() > 1000 and np.isnan(a.values).sum() > 0
    # the source in the other convention as well: -178.75 .. 178.75
    lon2 = np.where(lon > 180, lon - 360, lon)
    order = np.argsort(lon2)
    temp2 = GridSeries(temp.values[:, :, order], temp.dims, {"time": np.arange(3), "lat": lat, "lon": lon2[order]})
    c, _ = regrid(temp2, lat=dlat, lon=np.arange(0.0, 360, 5.0), _compute=STAGE)
    npt.assert_array_equal(c.values.view(np.uint32), a.values.view(np.uint32))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_constant_field_stays_constant_exactly(dtype):
    lat, lon = np.arange(-89.5, 90, 1.0), np.arange(0.5, 360, 1.0)
    for value in (17.3, -1.8, 0.0):
        x = np.full((2, lat.size, lon.size), value, dtype)
        temp = GridSeries(x, ("time", "lat", "lon"), {"time": np.arange(2), "lat": lat, "lon": lon})
        out, _ = regrid(temp, lat=np.linspace(88.59375, -88.59375, 127), lon=np.arange(0.0, 360, 1.40625), _compute=STAGE)
        # the fixed point of the constant, to the output type: every cell, whatever its weights
        want = dtype(np.rint(np.float64(dtype(value)) * 65536.0) / 65536.0)
        npt.assert_array_equal(out.values, np.full(out.values.shape, want, dtype))


def test_a_destination_equal_to_the_source_returns_its_fixed_point():
    lat, lon = np.arange(-29.875, 30, 0.25)[::-1].copy(), np.arange(0.125, 90, 0.25)
    temp = field_on(lat, lon, land=True, dtype=np.float64)
    out, info = regrid(temp, like=temp, coverage=True, _compute=STAGE)
    assert not info.periodic and (np.diff(info.rows[1]) == 1).all() and (np.diff(info.cols[1]) == 1).all()
    want = np.rint(temp.values * 65536.0) / 65536.0
    npt.assert_array_equal(out.values, want)
    npt.assert_array_equal(info.n, ~np.isnan(temp.values))
    npt.assert_array_equal(info.coverage[~np.isnan(want)], 1.0)


def exact_mean(temp, info, src_bounds, dst_bounds, measure, periodic):
    """(the float64 mean under the unquantised overlaps over the samples the result used, the spread of the samples of
    each footprint) for the geometry of a regrid() call"""
    oy = brute_overlap(src_bounds[0], dst_bounds[0], measure)
    ox = brute_overlap(src_bounds[1], dst_bounds[1], "plane", 360.0 if periodic else None)
    x = temp.values.astype(np.float64)
    ok = ~np.isnan(x)
    num = np.einsum("Jj,tji,Ii->tJI", oy, np.where(ok, x, 0.0), ox)
    den = np.einsum("Jj,tji,Ii->tJI", oy, ok.astype(np.float64), ox)
    hi = np.full(num.shape, -np.inf)
    lo = np.full(num.shape, np.inf)
    top, bottom = np.where(ok, x, -np.inf), np.where(ok, x, np.inf)
    for J in range(oy.shape[0]):
        for I in range(ox.shape[0]):
            jj, ii = np.nonzero(oy[J] > 0)[0], np.nonzero(ox[I] > 0)[0]
            if jj.size and ii.size:
                hi[:, J, I] = top[:, jj][:, :, ii].max(axis=(1, 2))
                lo[:, J, I] = bottom[:, jj][:, :, ii].min(axis=(1, 2))
    with np.errstate(divide="ignore", invalid="ignore"):
        return num / den, np.where(hi >= lo, hi - lo, 0.0)


CALLS = [
    # (source lat, lon centres, destination lat, lon centres, measure)
    (np.arange(-59.0, 60, 2.0), np.arange(1.0, 360, 2.0), np.arange(-57.5, 58, 5.0), np.arange(2.5, 360, 5.0), "sphere"),
    (np.arange(-4.875, 5, 0.25), np.arange(0.125, 10, 0.25), np.arange(5.0, -5.1, -0.25), np.arange(0.0, 10.1, 0.25), "sphere"),
    (np.arange(-22.5, 23, 1.0), np.arange(0.5, 90, 1.0), np.linspace(21.09375, -21.09375, 31), np.arange(0.703125, 90, 1.40625), "sphere"),
    (np.arange(-4.5, 5, 1.0), np.arange(100.5, 112, 1.0), np.arange(-4.875, 5, 0.25), np.arange(100.125, 112, 0.25), "plane"),
]


@pytest.mark.parametrize("k", range(len(CALLS)))
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_quantisation_bound_holds_against_unquantised_overlaps(k, dtype):
    slat, slon, dlat, dlon, measure = CALLS[k]
    temp = field_on(slat, slon, seed=k, dtype=dtype, land=True)
    out, info = regrid(temp, lat=dlat, lon=dlon, measure=measure, min_fraction=0.0, coverage=True, _compute=STAGE)
    limits = (-90.0, 90.0) if measure == "sphere" else None
    src_b = (axis_bounds(slat, limits), axis_bounds(slon))
    dst_b = (axis_bounds(dlat, limits), axis_bounds(dlon))
    want, spread = exact_mean(temp, info, src_b, dst_b, measure, info.periodic)
    bound = info.quantisation_bound(out.values, spread)
    ok = ~np.isnan(out.values)
    assert ok.sum() > 400 and (info.n[ok] >= 1).all()
    err = np.abs(out.values.astype(np.float64) - want)
    assert (err[ok] <= bound[ok]).all(), float((err[ok] / bound[ok]).max())
    assert np.isnan(bound[~ok]).all()
    # the bound is no blanket: the weight term stays a small share of the spread, and some error is a real share of it
    assert np.median(bound[ok] / np.maximum(spread[ok], 1e-3)) < 0.05
    if k != 3:                                                   # (1 x 1 footprints have no weight error to speak of)
        assert (err[ok] / bound[ok]).max() > 0.02


def test_conservation_on_a_land_free_field():
    slat, slon, dlat, dlon, measure = CALLS[0]
    slat, dlat = np.arange(-89.5, 90, 1.0), np.arange(-88.75, 90, 2.5)      # the whole sphere on both grids
    temp = field_on(slat, slon, seed=5, dtype=np.float64)
    out, info = regrid(temp, lat=dlat, lon=dlon, min_fraction=1.0, coverage=True, _compute=STAGE)
    assert not np.isnan(out.values).any()
    sa = np.abs(np.diff(np.sin(np.deg2rad(axis_bounds(slat, (-90, 90))))))[:, None] * np.abs(np.diff(axis_bounds(slon)))[None]
    da = np.abs(np.diff(np.sin(np.deg2rad(axis_bounds(dlat, (-90, 90))))))[:, None] * np.abs(np.diff(axis_bounds(dlon)))[None]
    assert abs(sa.sum() - da.sum()) < 1e-9 * sa.sum()
    _, spread = exact_mean(temp, info, (axis_bounds(slat, (-90, 90)), axis_bounds(slon)),
                           (axis_bounds(dlat, (-90, 90)), axis_bounds(dlon)), "sphere", True)
    bound = info.quantisation_bound(out.values, spread)
    # the extents of the definition are per run (each in the unit of its largest overlap), so the sums are weighted by
    # the cells' areas themselves: wy * wx in one common unit
    for t in range(out.values.shape[0]):
        src_total, dst_total = (sa * temp.values[t]).sum(), (da * out.values[t]).sum()
        assert abs(dst_total - src_total) <= (da * bound[t]).sum() + 1e-12 * abs(src_total)
        assert abs(dst_total - src_total) < 1e-4 * da.sum()


def test_a_span_above_64_raises_and_names_coarsen():
    with pytest.raises(XmhwException, match=r"coarsen\(\) first"):
        overlap_table(np.linspace(0, 65, 66), np.array([0.0, 65.0]), "plane")
    overlap_table(np.linspace(0, 64, 65), np.array([0.0, 64.0]), "plane")
    lat, lon = np.arange(-44.95, 45, 0.1), np.arange(0.05, 20, 0.1)
    with pytest.raises(XmhwException, match=r"coarsen\(\) first"):
        regrid(field_on(lat, lon, T=1), lat=np.arange(-40.0, 41, 10.0), lon=np.arange(2.5, 20, 5.0), _compute=STAGE)
    for bad in (dict(measure="cube"), dict(period=360.0, measure="sphere")):
        with pytest.raises(XmhwException):
            overlap_table(np.linspace(0, 10, 11), np.linspace(0, 10, 6), **bad)
    with pytest.raises(XmhwException, match="period"):
        overlap_table(np.linspace(0, 400, 11), np.linspace(0, 10, 6), "plane", 360.0)


def test_c_entry_refusals_in_their_stated_order_need_no_device():
    core = importlib.import_module("xmhw_amd._xmhw_hip")
    m = importlib.import_module("xmhw_amd._xmhw_hip_regrid")
    assert not any(hasattr(m, n) for n in ("HipError", "Unsupported", "InvalidArgument", "CommError"))
    assert (m.REGRID_MAX_RUN, m.REGRID_MAX_WEIGHT, m.REGRID_MAX_EXTENT, m.REGRID_BITS) == (rg.MAX_RUN, rg.MAX_WEIGHT, rg.MAX_EXTENT, rg.BITS)
    i32 = lambda *v: np.array(v, np.int32)                                                     # noqa: E731
    ok_rows = dict(row_first=i32(0, 1), row_ptr=i32(0, 2, 3), ay=i32(5, 4096, 7), wy=i32(5000, 7))
    ok_cols = dict(col_first=i32(0, 3, 2), col_ptr=i32(0, 1, 3, 3), ax=i32(1, 2, 3), wx=i32(1, 6, 0))

    def call(nt=10, ld=12, ny=3, nx=4, periodic=1, x0=0.0, a=0, ldo=6, itemsize=4, **tables):
        t = dict(ok_rows, **ok_cols)
        t.update(tables)
        m.regrid(0, itemsize, nt, ld, ny, nx, t["row_first"], t["row_ptr"], t["ay"], t["wy"], t["col_first"], t["col_ptr"],
                 t["ax"], t["wx"], periodic, x0, a, 0, ldo, 0, 0, 0)

    # the caps first: they win over everything that is invalid as well
    long_run = dict(col_first=i32(0), col_ptr=i32(0, 65), ax=np.ones(65, np.int32), wx=i32(65))
    with pytest.raises(core.Unsupported, match="more than 64"):
        call(a=65537, ld=1, ldo=0, **long_run)
    with pytest.raises(core.Unsupported, match="weight above"):
        call(ay=i32(5, 4097, 7), x0=np.nan)
    with pytest.raises(core.Unsupported, match="extent above"):
        call(wx=i32(1, (1 << 18) + 1, 0), nt=-1)
    with pytest.raises(core.Unsupported, match="2\\^31"):
        call(ny=65536, nx=32768, ld=1 << 31)
    for bad in (dict(nt=-1), dict(ny=-1), dict(nx=-1), dict(ld=11), dict(ldo=5),
                dict(row_ptr=i32(1, 2, 3)), dict(row_ptr=i32(0, 2, 1)),                         # not from 0, decreasing
                dict(ay=i32(5, -1, 7)), dict(ax=i32(1, 4, 3)),                                  # negative; above the extent
                dict(row_first=i32(0, 3)), dict(row_first=i32(-1, 1)), dict(row_first=i32(2, 1)),   # rows leave the grid
                dict(col_first=i32(0, 4, 2)), dict(col_first=i32(0, 3, 2), periodic=0),         # columns: periodic or not
                dict(a=65537), dict(a=-1), dict(x0=np.inf), dict(x0=np.nan)):
        with pytest.raises(core.InvalidArgument):
            call(**bad)
    with pytest.raises(core.InvalidArgument, match="tables must be"):
        call(wy=i32(5000))                                       # the lengths of the host tables, in the binding
    with pytest.raises(core.InvalidArgument, match="itemsize"):
        call(itemsize=2)
    call(nt=0)                                                   # no step: nothing is launched, before any NULL check
    empty = dict(row_first=i32(), row_ptr=i32(0), ay=i32(), wy=i32())
    call(ldo=0, **empty)                                         # an empty destination grid likewise
    with pytest.raises(core.InvalidArgument, match="NULL"):
        call()
    for bad in (-1, 3):
        with pytest.raises(core.InvalidArgument):
            m.set_regrid_variant(bad)
    with pytest.raises(core.InvalidArgument):
        m.set_regrid_chunk(-1)
    m.set_regrid_variant(0)
    m.set_regrid_chunk(0)


def test_the_path_of_a_call_needs_no_device():
    m = importlib.import_module("xmhw_amd._xmhw_hip_regrid")
    i32 = lambda v: np.asarray(v, np.int32)                                                     # noqa: E731
    first, ptr = i32(np.arange(300) * 4), i32(np.arange(301) * 4)
    try:
        assert m.regrid_class(1200, i32([0, 4]), first, ptr, 0) == 2                            # 4 x 1024 dwords
        assert m.regrid_class(1200, i32([0, 17]), first, ptr, 0) == 1                           # 17 x 1024 > 16384
        assert m.regrid_class(1200, i32([0, 0]), first, ptr, 0) == 1                            # nothing to stage
        assert m.regrid_class(1199, i32([0, 4]), first, ptr, 0) == 0                            # a run leaves the grid
        assert m.regrid_class(1199, i32([0, 4]), first, ptr, 1) == 2                            # ... unless it wraps
        assert m.regrid_class(1200, i32([0, 65]), first, ptr, 0) == 0
        # the automatic choice stages small tiles of strided runs only: not a larger tile, not overlapping 2 x 2 footprints
        assert m.regrid_class(1200, i32([0, 5]), first, ptr, 0) == 1                            # 5 x 1024 > 4096
        shifted, two = i32(np.arange(300)), i32(np.arange(301) * 2)
        assert m.regrid_class(301, i32([0, 2]), shifted, two, 0) == 1
        m.set_regrid_variant(1)
        assert m.regrid_class(1200, i32([0, 4]), first, ptr, 0) == 1
        m.set_regrid_variant(2)
        assert m.regrid_class(1200, i32([0, 4]), first, ptr, 0) == 2 and m.regrid_class(1200, i32([0, 17]), first, ptr, 0) == 1
        assert m.regrid_class(1200, i32([0, 5]), first, ptr, 0) == 2 and m.regrid_class(301, i32([0, 2]), shifted, two, 0) == 2
    finally:
        m.set_regrid_variant(0)


def test_the_listed_cases_are_the_full_product_and_valid_tables():
    cases = rc.listed()
    assert len(cases) == 160 and len(set(cases)) == 160 and len({rc.case_id(c) for c in cases}) == 160
    runs = set()
    for c in cases:
        ny, nx, rows, cols = rc.tables(c)
        rg.check_table(rows, c.my, ny, False, "row")
        rg.check_table(cols, c.mx, nx, bool(c.periodic), "column")
        runs |= set(np.diff(rows[1]).tolist()) | set(np.diff(cols[1]).tolist())
        assert rc.make_data(c).shape == (rc.T_STEPS, ny * nx + 3)
    assert set(rc.RUNS) <= runs
    assert len(rc.invariance_subset(cases)) == 40


def test_stage_checks_and_oracle_agree_on_a_listed_case():
    c = next(k for k in rc.listed() if (k.mx, k.my, k.kind, k.periodic) == (130, 3, "random", 1) and k.dtype is np.float64)
    ny, nx, rows, cols = rc.tables(c)
    field = rc.make_data(c)[:, :ny * nx]
    got = rg.check_stage_inputs(field, ny, nx, c.my, c.mx, rows, cols, 1, 0.0, c.a)
    assert got[0].dtype == np.float64 and all(v.dtype == np.int32 for v in got[5] + got[6])
    out, wsum, n, n_range = ro.regrid_oracle(field, ny, nx, rows, cols, 1, 0.0, c.a, exact=True)
    # the separable order the kernel uses gives the same integers
    first, ptr, ax, _ = cols
    J = 1
    for I in (0, 57, 129):
        xs = ws = 0
        for r in range(rows[1][J + 1] - rows[1][J]):
            sx = sw = 0
            for k in range(ptr[I + 1] - ptr[I]):
                x = field[3, (rows[0][J] + r) * nx + (first[I] + k) % nx]
                if ax[ptr[I] + k] > 0 and not np.isnan(x):
                    sw += int(ax[ptr[I] + k])
                    sx += int(ax[ptr[I] + k]) * int(np.rint(x * 65536.0))
            ay = int(rows[2][rows[1][J] + r])
            xs, ws = xs + ay * sx, ws + ay * sw
        assert ws == wsum[3, J * c.mx + I]
        if ws and not np.isnan(out[3, J * c.mx + I]):
            assert out[3, J * c.mx + I] == 0.0 + (float(xs) / float(ws)) / 65536.0
    for bad in (dict(a=-1), dict(a=65537), dict(x0=np.nan)):
        kw = dict(x0=0.0, a=0)
        kw.update(bad)
        with pytest.raises(XmhwException):
            rg.check_stage_inputs(field, ny, nx, c.my, c.mx, rows, cols, 1, kw["x0"], kw["a"])
    with pytest.raises(XmhwException, match="leaves"):
        rg.check_stage_inputs(field, ny, nx, c.my, c.mx, rows, cols, 0, 0.0, 0)


def test_types_dims_attrs_and_coordinates_of_the_result():
    lat, lon = np.arange(-9.5, 10, 1.0), np.arange(0.5, 30, 1.0)
    temp = field_on(lat, lon, T=4, land=True)
    like = {"lat": np.arange(8.0, -9, -2.0), "lon": np.arange(1.0, 30, 2.0)}
    out, info = regrid(temp, like=like, coverage=True, _compute=STAGE)
    assert isinstance(out, GridSeries) and out.dims == temp.dims and out.values.dtype == np.float32
    assert out.values.shape == (4, 9, 15) and out.attrs == {"units": "degC"}
    npt.assert_array_equal(out.coords["lat"], like["lat"])
    npt.assert_array_equal(out.coords["lon"], like["lon"])
    npt.assert_array_equal(out.coords["time"], temp.coords["time"])
    assert info.coverage.dtype == np.float32 and info.coverage.shape == (4, 9, 15) and info.wsum.dtype == np.int64
    assert info.n.dtype == np.int32 and info.n_range == 0 and info.a == 32768 and not info.periodic
    assert np.nanmax(info.coverage) == 1.0 and np.nanmin(info.coverage) < 0.5
    npt.assert_array_equal(np.isnan(out.values), ~((info.n >= 1) & (info.wsum * 65536 >= info.a * (info.rows[3][:, None].astype(np.int64) * info.cols[3][None]))[...]))
    plain, pinfo = regrid(temp, like=GridSeries(np.zeros((1, 9, 15)), ("time", "lat", "lon"), dict(like, time=np.arange(1))), _compute=STAGE)
    npt.assert_array_equal(plain.values.view(np.uint32), out.values.view(np.uint32))
    assert pinfo.coverage is None and pinfo.wsum is None and pinfo.n is None
    # another order of dims goes in and comes out
    turned = GridSeries(np.transpose(temp.values, (2, 0, 1)), ("lon", "time", "lat"), temp.coords, attrs=temp.attrs)
    tout, _ = regrid(turned, like=like, _compute=STAGE)
    assert tout.dims == ("lon", "time", "lat")
    npt.assert_array_equal(np.transpose(tout.values, (1, 2, 0)).view(np.uint32), out.values.view(np.uint32))
    # explicit bounds replace the derived ones; a series in kelvin needs its offset
    b, _ = regrid(temp, lat_bounds=np.arange(9.0, -10, -2.0), lon_bounds=np.arange(0.0, 31, 2.0), _compute=STAGE)
    npt.assert_array_equal(b.values.view(np.uint32), out.values.view(np.uint32))
    npt.assert_array_equal(b.coords["lat"], like["lat"])
    kelvin = GridSeries(temp.values + np.float32(273.15), temp.dims, temp.coords)
    with pytest.raises(XmhwException, match="offset=273.15"):
        regrid(kelvin, like=like, _compute=STAGE)
    regrid(kelvin, like=like, offset=273.15, _compute=STAGE)
    for bad in (dict(like=like, lat=lat), dict(), dict(lat=lat), dict(like={"lat": lat}), dict(like=like, min_fraction=1.5),
                dict(like=like, measure="flat"), dict(like=like, offset=np.inf), dict(like=3)):
        with pytest.raises(XmhwException):
            regrid(temp, _compute=STAGE, **bad)
    from xmhw_amd.device import PackedArray
    packed = GridSeries(np.zeros((4, 20, 30), np.int16), temp.dims, temp.coords)
    packed.values = PackedArray(packed.values, dict(scale=0.01, offset=0.0, fill=-32768, out="float32"))      # as open_series() does
    with pytest.raises(XmhwException, match="regrid does not read packed int16 views: pass decoded floats"):
        regrid(packed, like=like, _compute=STAGE)
    with pytest.raises(XmhwException, match="two spatial dims"):
        regrid(GridSeries(np.zeros((4, 20)), ("time", "lat"), {"time": np.arange(4), "lat": lat}), like=like, _compute=STAGE)


def test_dataarray_in_dataarray_out():
    xr = pytest.importorskip("xarray")
    lat, lon = np.arange(-9.5, 10, 1.0), np.arange(0.5, 30, 1.0)
    g = field_on(lat, lon, T=4, land=True)
    time = np.arange("2001-01-01", "2001-01-05", dtype="datetime64[D]")
    da = xr.DataArray(g.values, dims=g.dims, coords={"time": time, "lat": ("lat", lat, {"units": "degrees_north"}), "lon": lon},
                      attrs={"units": "degC"}, name="sst")
    like = xr.DataArray(np.zeros((9, 15)), dims=("lat", "lon"), coords={"lat": np.arange(8.0, -9, -2.0), "lon": np.arange(1.0, 30, 2.0)})
    out, info = regrid(da, like=like, coverage=True, _compute=STAGE)
    want, _ = regrid(g, like={"lat": like["lat"].values, "lon": like["lon"].values}, _compute=STAGE)
    assert isinstance(out, xr.DataArray) and out.dims == da.dims and out.name == "sst" and out.attrs == da.attrs
    npt.assert_array_equal(out.values.view(np.uint32), want.values.view(np.uint32))
    npt.assert_array_equal(out["lat"].values, like["lat"].values)
    npt.assert_array_equal(out["time"].values, time)
    assert out["lat"].attrs == {"units": "degrees_north"}
    ds = info.to_xarray()
    assert ds["coverage"].dims == ("time", "lat", "lon") and ds.attrs["min_share_65536ths"] == 32768
