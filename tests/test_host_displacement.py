"""mhw_displacement() without a GPU: the candidate lists, a hand-drawn case, the refusals, the dataset and the public call
with the brute-force oracle as the stage."""
import numpy as np
import pytest

import cooccurrence_cases as coc
import displacement_cases as dc
import displacement_oracle as ora
import track_intensity_cases as tic
from xmhw_amd import (DisplacementDataset, DisplacementTable, GridSeries, XmhwException, displacement_offsets,
                      mhw_displacement)
from xmhw_amd import displacement as dp
from xmhw_amd.device import PackedArray

LATS = {"regular": np.linspace(-50.0, 50.0, 11), "irregular": np.array([-61.0, -33.5, -30.0, -2.0, 0.0, 7.5, 41.0, 80.0]),
        "one_row": np.array([37.0])}


def all_rows(table):
    return [table.row(j) for j in range(table.ny)]


@pytest.fixture(scope="module")
def tables():
    out = {}
    for name, lat in LATS.items():
        for nx in (1, 7, 8):
            for periodic in (False, True):
                for maxd in (0.0, 900.0, 20016.0):
                    out[name, nx, periodic, maxd] = displacement_offsets(lat, nx, 360.0 / 8 if periodic else 3.0, maxd, periodic)
    return out


def test_lists_are_sorted_start_at_the_source_and_hold_no_duplicate(tables):
    for key, table in tables.items():
        assert isinstance(table, DisplacementTable)
        assert table.row_offsets.dtype == np.int64 and table.djdi.dtype == np.int16
        assert all(a.dtype == np.int32 for a in (table.dist_m, table.north_m, table.east_m))
        for j, (dj, di, dist, north, east) in enumerate(all_rows(table)):
            assert (dj[0], di[0], dist[0], north[0], east[0]) == (0, 0, 0, 0, 0), key
            k = list(zip(dist.tolist(), dj.tolist(), di.tolist()))
            assert k == sorted(k), key
            assert len(set(zip(dj.tolist(), di.tolist()))) == len(k), key
            assert (j + dj >= 0).all() and (j + dj < table.ny).all()
            assert (dist <= table.max_m).all() and (dist < 1 << dp.DIST_BITS).all()


def test_lists_equal_the_exhaustive_evaluation(tables):
    """the pruning of displacement_offsets() drops nothing: every (dj, di) of the grid, evaluated and filtered"""
    for key, table in tables.items():
        for got, want in zip(all_rows(table), ora.brute_lists(table)):
            for g, w in zip(got, want):
                np.testing.assert_array_equal(g, w, err_msg=str(key))


def test_a_small_distance_lists_the_source_alone_and_a_large_one_the_whole_grid(tables):
    for (name, nx, periodic, maxd), table in tables.items():
        n = np.diff(table.row_offsets)
        if maxd == 0.0:
            assert (n == 1).all()
        if maxd > 19000.0:                               # half a great circle is 20015.09 km
            assert (n == table.ny * dp.di_range(nx, periodic).shape[0]).all()


def test_rows_mirrored_about_the_equator_have_mirrored_lists():
    lat = np.array([-40.0, -12.5, -3.0, 3.0, 12.5, 40.0])
    for periodic in (False, True):
        table = displacement_offsets(lat, 9, 40.0 if periodic else 5.0, 2500.0, periodic)
        for j in range(table.ny):
            dj, di, dist, north, east = table.row(j)
            mj, mi, mdist, mnorth, meast = table.row(table.ny - 1 - j)
            a = sorted(zip(dist.tolist(), (-dj).tolist(), di.tolist(), (-north).tolist(), east.tolist()))
            b = sorted(zip(mdist.tolist(), mj.tolist(), mi.tolist(), mnorth.tolist(), meast.tolist()))
            assert a == b


def test_distances_agree_with_the_vector_angle():
    """an independent formula on well-conditioned pairs (the angle between unit vectors through atan2): within 1 m"""
    lat = np.linspace(-70.0, 70.0, 15)
    table = displacement_offsets(lat, 24, 15.0, 9000.0, True)
    phi = np.deg2rad(lat)
    checked = 0
    for j in range(table.ny):
        dj, di, dist, north, _ = table.row(j)
        p1, p2, lam = phi[j], phi[j + dj], np.deg2rad(di * 15.0)
        a = np.stack([np.cos(p1) * np.ones_like(lam), np.zeros_like(lam), np.sin(p1) * np.ones_like(lam)])
        b = np.stack([np.cos(p2) * np.cos(lam), np.cos(p2) * np.sin(lam), np.sin(p2)])
        angle = np.arctan2(np.linalg.norm(np.cross(a, b, axis=0), axis=0), (a * b).sum(axis=0))
        well = dist > 100000
        assert np.abs(6371000.0 * angle - dist)[well].max() <= 1.0
        np.testing.assert_array_equal(north, np.rint(6371000.0 * (p2 - p1)))
        checked += int(well.sum())
    assert checked > 1000


@pytest.mark.parametrize("nx,lo,hi", [(8, -3, 4), (7, -3, 3), (1, 0, 0), (2, 0, 1)])
def test_the_periodic_di_range(nx, lo, hi):
    di = dp.di_range(nx, True)
    assert (di[0], di[-1], di.shape[0]) == (lo, hi, nx)
    i = np.arange(nx)
    d = dp.wrapped_di(i[:, None], i[None, :], nx, True)
    assert d.min() >= lo and d.max() <= hi
    assert ((i[:, None] + d) % nx == i[None, :]).all()
    for row in d:                                                          # every destination column exactly once
        assert sorted(row.tolist()) == di.tolist()
    table = displacement_offsets(np.array([0.0, 1.0]), nx, 360.0 / nx, 20016.0, True)
    for j in range(2):
        assert sorted(set(table.row(j)[1].tolist())) == di.tolist()
    plain = dp.di_range(nx, False)
    assert (plain[0], plain[-1]) == (-(nx - 1), nx - 1)


def walk_lists(case):
    """The device's algorithm in plain loops: the FIRST qualifying entry of the row's list, in list order."""
    table, field, view = case["table"], np.asarray(case["field"], dtype=np.float64), case["view"]
    ny, nx, K, C = table.ny, table.nx, case["K"], view["C"]
    T = field.shape[0]
    if case["cold"]:
        field = -field
    ev = ora.in_event(view, T)
    basin = case["basin"]
    out = {n: np.zeros((K, C), dt) for n, dt in dp._STAGE.items()}
    visited = 0
    for c, p in enumerate(case["cell_index"]):
        j, i = divmod(int(p), nx)
        if basin is not None and basin[p] < 0:
            continue
        dj, di, dist, north, east = table.row(j)
        for t in np.nonzero(ev[:, c])[0]:
            k = case["classes"][t]
            if k < 0:
                continue
            out["n_days"][k, c] += 1
            g = case["seas"][case["rows"][t], c]
            for e in range(dj.shape[0]):
                ii = i + int(di[e])
                if table.periodic:
                    ii %= nx
                if not 0 <= ii < nx:
                    continue
                pp = (j + int(dj[e])) * nx + ii
                if field[t, pp] <= g and (basin is None or basin[pp] == basin[p]):
                    out["n_found"][k, c] += 1
                    out["sum_m"][k, c] += dist[e]
                    out["sum_north_m"][k, c] += north[e]
                    out["sum_east_m"][k, c] += east[e]
                    out["max_m"][k, c] = max(out["max_m"][k, c], dist[e])
                    visited += e + 1
                    break
            else:
                visited += dj.shape[0]
    out["n_visited"] = visited
    return out


HAND = """
19 25 25 25 25 25 25 25
25 25 25 25 25 25 25 25
25 25 nan 25 25 25 25 25
25 25 25 25 25 25 25 25
25 25 25 25 25 18 25 25
"""
# source (j, i) -> the (dj, di) of its nearest point at or below 20 degrees, None: none within 400 km; one degree is
# 111.195 km, so 400 km are 3.597 degrees.  The cool points are (0, 0) and (4, 5).
HAND_PLAIN = {(0, 0): (0, 0),          # cool itself
              (2, 3): (2, 2),          # to (4, 5): 2.83 degrees; (0, 0) is 3.61 away
              (2, 1): (-2, -1),        # to (0, 0): 2.24 degrees; (4, 5) is 4.47 away
              (4, 0): None,            # (0, 0) is 4 degrees = 444.8 km away, (4, 5) 5 degrees
              (1, 7): None}            # (4, 5) is 3.61 degrees = 400.9 km away, (0, 0) 7.07 degrees
HAND_PERIODIC = dict(HAND_PLAIN)
HAND_PERIODIC.update({(4, 0): (0, -3),     # round the seam: (4, 5) is three columns to the west
                      (1, 7): (-1, 1)})    # round the seam: (0, 0) is the next column to the east


def hand_case(periodic):
    ny, nx = 5, 8
    field = np.array([[float(v) for v in line.split()] for line in HAND.strip().splitlines()]).reshape(1, ny * nx)
    keep = ~np.isnan(field[0])
    cell_index = np.nonzero(keep)[0]
    C = cell_index.shape[0]
    sources = sorted(j * nx + i for j, i in HAND_PLAIN)
    cells = np.searchsorted(cell_index, sources)
    offsets = np.zeros(C + 1, dtype=np.int64)
    offsets[cells + 1] = 1
    offsets = np.cumsum(offsets)
    view = dict(n=len(sources), C=C, offsets=offsets, start=np.zeros(len(sources), np.int32),
                end=np.zeros(len(sources), np.int32), cell_index=cell_index)
    lat = np.array([-2.0, -1.0, 0.0, 1.0, 2.0])
    table = displacement_offsets(lat, nx, 1.0, 400.0, periodic)
    return dict(field=field, seas=np.full((1, C), 20.0), rows=np.zeros(1, np.int32), view=view, cell_index=cell_index,
                table=table, classes=np.zeros(1, np.int32), K=1, basin=None, cold=False), lat


@pytest.mark.parametrize("periodic", [False, True])
def test_hand_drawn_case(periodic):
    # ``periodic`` wraps the column index, whatever the spacing: column 7 and column 0 are one degree apart
    case, lat = hand_case(periodic)
    expect = HAND_PERIODIC if periodic else HAND_PLAIN
    dlon = case["table"].dlon
    want = {n: np.zeros((1, case["view"]["C"]), dt) for n, dt in dp._STAGE.items()}
    for (j, i), hit in expect.items():
        c = int(np.searchsorted(case["cell_index"], j * 8 + i))
        want["n_days"][0, c] = 1
        if hit is not None:
            dist, north, east = dp.pair_metrics(np.deg2rad(lat[j]), np.deg2rad(lat[j + hit[0]]), np.deg2rad(hit[1] * dlon))
            want["n_found"][0, c], want["sum_m"][0, c], want["max_m"][0, c] = 1, dist, dist
            want["sum_north_m"][0, c], want["sum_east_m"][0, c] = north, east
    if not periodic:                                    # one degree on the sphere, to the metre
        c = int(np.searchsorted(case["cell_index"], 2 * 8 + 1))
        assert abs(int(want["sum_m"][0, c]) - 111195 * np.sqrt(5.0)) < 100
        assert int(want["sum_north_m"][0, c]) == -2 * 111195 + 0 and abs(int(want["sum_east_m"][0, c]) + 111195) < 30
    brute, walked = dc.run_stage(ora.displacement_grid, case), walk_lists(case)
    for got in (brute, walked):
        for name in dp.STAGE_FIELDS:
            np.testing.assert_array_equal(got[name], want[name], err_msg=name)
    assert brute["n_visited"] == walked["n_visited"] > len(expect)


@pytest.mark.parametrize("kw", [dict(), dict(periodic=True, dlon=360.0 / 13, max_distance=9000.0), dict(basin=True), dict(cold=True),
                                dict(max_distance=20000.0), dict(max_distance=0.0)])
def test_first_entry_of_the_list_is_the_minimum_over_the_grid(kw):
    """the list walk (what the device does) against the brute force over all grid points, n_visited included"""
    import days_by_cases as dbc
    case = dc.stage_case(6, 13, 40, seed=3, dtype=np.float64, classes=dbc.every_step, **kw)
    want = dc.run_stage(ora.displacement_grid, case)
    dc.check_case(want, far=kw.get("max_distance") != 0.0, unreached=kw.get("max_distance") != 20000.0)
    dc.assert_same(walk_lists(case), want)


# ---- the public call ------------------------------------------------------------------------------------------------

def public_case(T=70, ny=5, nx=9, seed=1, **kw):
    g = tic.calendar_grid(T, ny, nx, seed=seed, **kw)
    C = int(g["keep"].sum())
    tab = coc.table(T, C, seed + 5)
    g["mhw"] = coc.dataset(tab, T, keep=g["keep"], sshape=(ny, nx))
    g["mhw"].coords = {"lat": g["lat"], "lon": g["lon"]}
    return g


def test_public_call_with_the_oracle_as_the_stage():
    g = public_case()
    seen = {}

    def stage(field, seas, rows, view, cell_index, table, classes, K, **kw):
        seen.update(field=field, seas=seas, rows=rows, table=table, kw=kw, cell_index=cell_index)
        return ora.displacement_grid(field, seas, rows, view, cell_index, table, classes, K, **kw)

    res = mhw_displacement(g["temp"], g["th"], g["se"], g["mhw"], classes="month", max_distance=1500.0, _compute=stage)
    assert isinstance(res, DisplacementDataset)
    np.testing.assert_array_equal(seen["field"], g["ts"])                  # the uncompacted grid, as stored
    np.testing.assert_array_equal(seen["seas"], g["seas"][:, g["keep"]])
    np.testing.assert_array_equal(seen["rows"], g["doy"] - 1)
    np.testing.assert_array_equal(seen["cell_index"], np.nonzero(g["keep"])[0])
    t = seen["table"]
    assert (t.ny, t.nx, t.dlon, t.periodic, t.max_m, t.radius) == (5, 9, 2.0, False, 1500000, 6371.0)
    np.testing.assert_array_equal(res.klass, [1, 2, 3])
    np.testing.assert_array_equal(res.n_steps, [31, 28, 11])
    # against the oracle run by hand on the same inputs, scattered on the grid
    month = np.array([1] * 31 + [2] * 28 + [3] * 11)
    want = ora.displacement_grid(g["ts"], g["seas"][:, g["keep"]], g["doy"] - 1, g["mhw"].compact_view(), np.nonzero(g["keep"])[0],
                                 t, month - 1, 3)
    dc.check_case(want, unreached=False)
    alive_r, alive_c = g["keep"].reshape(5, 9).any(axis=1), g["keep"].reshape(5, 9).any(axis=0)
    for name in dp.STAGE_FIELDS:
        full = np.zeros((3, 45), dtype=want[name].dtype)
        full[:, g["keep"]] = want[name]
        np.testing.assert_array_equal(getattr(res, name), full.reshape(3, 5, 9)[:, alive_r][:, :, alive_c], err_msg=name)
    np.testing.assert_array_equal(res.keep, g["keep"].reshape(5, 9)[alive_r][:, alive_c])
    assert res.attrs["n_visited"] == want["n_visited"] and res.attrs["n_sources"] == int(want["n_days"].sum())
    assert res.attrs["classes"] == "month" and res.attrs["max_distance_km"] == 1500.0 and res.attrs["periodic"] is None
    # periodic and basin reach the stage
    basin = np.arange(45).reshape(5, 9) % 2
    mhw_displacement(g["temp"], g["th"], g["se"], g["mhw"], periodic="lon", basin=basin, max_distance=300.0, _compute=stage)
    assert seen["table"].periodic and seen["table"].max_m == 300000
    np.testing.assert_array_equal(np.asarray(seen["kw"]["basin"]).reshape(-1), basin.reshape(-1))


def small_dataset():
    K, shape = 2, (2, 3)
    f = {n: np.zeros((K,) + shape, dt) for n, dt in dp._STAGE.items()}
    f["n_days"][0, 0, 0], f["n_found"][0, 0, 0] = 4, 2
    f["sum_m"][0, 0, 0], f["sum_north_m"][0, 0, 0], f["sum_east_m"][0, 0, 0], f["max_m"][0, 0, 0] = 3000, -1000, 2500, 2000
    f["n_days"][1, 1, 2] = 5                             # sources, none reached
    keep = np.ones(shape, dtype=bool)
    keep[1, 0] = False
    return DisplacementDataset([3, 9], [10, 20], f, keep, ("lat", "lon"), {"lat": [0.0, 1.0], "lon": [0.0, 1.0, 2.0]},
                               attrs={"n_visited": 7}), keep


def test_dataset_derived_fields():
    ds, _ = small_dataset()
    assert ds.displacement_mean_km[0, 0, 0] == 1.5 and ds.north_mean_km[0, 0, 0] == -0.5 and ds.east_mean_km[0, 0, 0] == 1.25
    assert ds.displacement_max_km[0, 0, 0] == 2.0 and ds.reached[0, 0, 0] == 0.5
    assert ds.reached[1, 1, 2] == 0.0 and np.isnan(ds.displacement_mean_km[1, 1, 2]) and np.isnan(ds.displacement_max_km[1, 1, 2])
    assert np.isnan(ds.reached[0, 1, 0]) and np.isnan(ds.north_mean_km[0, 1, 1]) and np.isnan(ds.east_mean_km[1, 0, 0])


def test_dataset_to_xarray():
    xr = pytest.importorskip("xarray")
    ds, keep = small_dataset()
    x = ds.to_xarray()
    assert isinstance(x, xr.Dataset) and x["sum_m"].dims == ("klass", "lat", "lon") and x.attrs["n_visited"] == 7
    np.testing.assert_array_equal(x["klass"], [3, 9])
    np.testing.assert_array_equal(x["keep"], keep)
    assert float(x["displacement_mean_km"][0, 0, 0]) == 1.5


def _refused(match, g=None, **kw):
    g = g or public_case()
    args = dict(temp=g["temp"], th=g["th"], se=g["se"], mhw=g["mhw"], _compute=ora.displacement_grid)
    args.update(kw)
    with pytest.raises(XmhwException, match=match):
        mhw_displacement(args.pop("temp"), args.pop("th"), args.pop("se"), args.pop("mhw"), **args)


def _renamed(g, names, coords=None):
    """temp / th / se of a public case with the spatial dims renamed (and coordinates replaced)"""
    out = {}
    for k, first in (("temp", "time"), ("th", "doy"), ("se", "doy")):
        s = g[k]
        c = {first: s.coords[first], names[0]: s.coords["lat"], names[1]: s.coords["lon"]}
        c.update(coords or {})
        out[k] = GridSeries(s.values, (first,) + tuple(names), c)
    return out


def test_refusals():
    g = public_case()
    _refused("expects the EventDataset", mhw=object())
    _refused("does not take maxPadLength: destination samples are read as stored", maxPadLength=3)
    _refused("max_distance", max_distance=-1.0)
    _refused("max_distance", max_distance=np.nan)
    _refused("radius", radius=0.0)
    _refused(r"below 2\*\*25", radius=20000.0)
    _refused("periodic should be None or the name of the longitude dim", periodic="lat")
    _refused("basin should hold one integer label per grid point", basin=np.zeros(7, dtype=np.int32))
    _refused("basin should hold one integer label per grid point", basin=np.zeros((5, 9)))
    _refused("classes should have one entry per time step", classes=np.zeros(3, dtype=np.int64))
    # the table against the device budget: the message names max_distance
    _refused("lower max_distance", max_batch_bytes=4096, max_distance=5000.0)
    # the detection does not belong to temp
    other = public_case(T=70, ny=5, nx=8)
    _refused("mhw does not belong to temp", mhw=other["mhw"])
    short = public_case(T=60)
    _refused("temp has 70 time steps, the detection 60", mhw=short["mhw"])
    moved = public_case(seed=2)
    _refused("the land mask of temp differs from mhw.keep", mhw=coc.dataset(coc.table(70, int(moved["keep"].sum()), 1), 70,
                                                                           keep=moved["keep"], sshape=(5, 9)))
    cold = public_case()
    cold["mhw"].attrs = {"xmhw_parameters": "MHW detected using: 5 days of minimum duration"}
    _refused("coldSpells=True differs from the detection's recorded parameters", g=cold, coldSpells=True)
    # a single-point series
    point = GridSeries(g["ts"][:, 0], ("time",), {"time": g["temp"].coords["time"]})
    _refused("needs a grid: a single-point series has no neighbours", temp=point)
    # packed int16 views
    packed = GridSeries(np.zeros((70, 5, 9), dtype=np.int16), ("time", "lat", "lon"), g["temp"].coords)
    packed.values = PackedArray(packed.values, dict(scale=0.01, offset=0.0, fill=None, out="float32"))      # as open_series() does
    _refused("does not read packed int16 views: pass decoded floats", temp=packed)


def test_grid_refusals():
    g = public_case()
    mhw = g["mhw"]

    def on(names, coords=None, **kw):
        r = _renamed(g, names, coords)
        size = {names[0]: 5, names[1]: 9}
        sd = tuple(sorted(names))
        keep = g["keep"].reshape(5, 9) if sd == tuple(names) else g["keep"].reshape(5, 9).T
        m = coc.dataset(coc.table(70, int(g["keep"].sum()), 6), 70, keep=keep.reshape(-1), sshape=tuple(size[d] for d in sd))
        m.sdims = sd
        return dict(temp=r["temp"], th=r["th"], se=r["se"], mhw=m, **kw)

    _refused("needs one latitude dim named one of", **on(("y", "lon")))
    _refused("needs one longitude dim named one of", **on(("lat", "x")))
    _refused("lat='nope' is not a spatial dim", lat="nope")
    _refused("should be the fast axis of the stacked layout", **on(("y", "x"), lat="y", lon="x"))
    _refused("longitude should be uniformly spaced", **on(("lat", "lon"), {"lon": np.array([0, 2, 4, 6, 8, 10, 12, 14, 16.1])}))
    _refused("latitude should be a 1-D array of finite degrees", **on(("lat", "lon"), {"lat": np.array([0, 1, 2, 3, 95.0])}))
    three = GridSeries(np.zeros((70, 2, 5, 9)), ("time", "depth", "lat", "lon"),
                       {"time": g["temp"].coords["time"], "depth": [0, 1], "lat": g["lat"], "lon": g["lon"]})
    _refused("needs two spatial dims", temp=three)
    # latitude / longitude under their long names, and given by name, are taken
    r = on(("latitude", "longitude"))
    res = mhw_displacement(r["temp"], r["th"], r["se"], r["mhw"], _compute=ora.displacement_grid)
    assert res.sdims == ("latitude", "longitude")
    r = on(("a", "b"), lat="a", lon="b")
    assert mhw_displacement(r.pop("temp"), r.pop("th"), r.pop("se"), r.pop("mhw"), _compute=ora.displacement_grid, **r).sdims == ("a", "b")
    assert mhw is g["mhw"]


def test_too_many_classes_and_stage_shape():
    g = public_case(T=1100, ny=2, nx=3, land=0.0)
    _refused("at most 1024 classes", g=g, classes=np.arange(1100))
    bad = lambda *a, **k: dict({n: np.zeros((1, 1), dt) for n, dt in dp._STAGE.items()}, n_visited=0)      # noqa: E731
    g = public_case()
    with pytest.raises(XmhwException, match="displacement stage returned n_days of shape"):
        mhw_displacement(g["temp"], g["th"], g["se"], g["mhw"], _compute=bad)


def test_stage_input_checks():
    case = dc.stage_case(3, 5, 9, land=0.0, land_row=False)
    args = [case[k] for k in ("field", "seas", "rows", "view", "cell_index", "table", "classes", "K", "basin")]

    def refused(match, **kw):
        a = list(args)
        for k, v in kw.items():
            a[("field", "seas", "rows", "view", "cell_index", "table", "classes", "K", "basin").index(k)] = v
        with pytest.raises(XmhwException, match=match):
            dp.check_stage_inputs(*a)

    refused("the series should be", field=case["field"][:, :-1])
    refused(r"seas should be \(D, 15\)", seas=case["seas"][:, :-1])
    refused("rows should hold the climatology row", rows=case["rows"] + 5)
    refused("class labels should be in", classes=case["classes"] + 1)
    refused("K should be >= 1", K=0)
    refused("at most 1024 classes", K=1025)
    refused("index_end outside the time axis", view=dict(case["view"], end=case["view"]["end"] + 9))
    refused("basin should hold one integer label", basin=np.zeros(15))
    dp.check_stage_inputs(*args)
    assert dp.time_blocks(10, 8, 24) == [(0, 3), (3, 3), (6, 3), (9, 1)]
    assert dp.time_blocks(10, 8, 0) == [(t, 1) for t in range(10)]
    assert dp.time_blocks(5, 8, 1 << 20) == [(0, 5)]
    assert dp.time_blocks(5, 8, 0, block_steps=4) == [(0, 4), (4, 1)]
