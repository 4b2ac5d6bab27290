"""The grid slab walk under coverage_grid(), class_days_grid() and track_intensity_grid(): five slabs of a 12 x 20 grid,
one of them all land, land in the first and in the last, climatologies compacted on the host or on the device (there on
the smaller grid threshold() hands over), with and without maxPadLength.  Every leg equals the dense stage on the
host-compacted inputs in one batch and the oracle, bit for bit; every refusal keeps its text and leaks no buffer.
The stages whose accumulators are sliced by column through series_stage.Accumulators -- heat_stress_grid(),
class_sums_grid(), regress_grid(), composite_grid() and lag_corr_grid() -- walk the same five slabs (k0 != 0, a skipped
slab, a ragged last slab, C < N), without padding, and meet the same two references.

The shape.  T = 203 (no multiple of 64: the last bit word is ragged), N = 240 float32 grid points, D = 37.  A slab cell
costs device._grid_batch() 203 * 4 * 3 + 203 * 4 (raw, decoded and compacted copy; the next slab's upload) plus the
stage's own extra, 6 * 37 * 8 + 203 // 4 + 64 for coverage and class days (5138 in all) and 6 * 37 * 8 + 64 for track
intensity (5088): a budget of 50 such cells gives the slabs [0, 50), [50, 100), [100, 150), [150, 200), [200, 240).
The column-sliced stages add 4 * Dr * 8 + 64 for a base of Dr rows (37, or the one land row of the class sums), the
composite T // 8 more for its anchor bitmap and the lag correlation 2 * 203 * 4 for the second field."""
import functools

import numpy as np
import numpy.testing as npt
import pytest

import composite_cases as cpc
import composite_oracle as cpo
import coverage_cases as cc
import coverage_oracle as co
import days_by_cases as dc
import days_by_oracle as dbo
import heat_stress_cases as hc
import heat_stress_oracle as ho
import index_regression_cases as irc
import index_regression_oracle as iro
import lag_correlation_oracle as lco
import pad_oracle as po
import track_intensity_cases as tc
import track_intensity_oracle as tio

pytestmark = pytest.mark.gpu

T, NY, NX, D, SLAB = 203, 12, 20, 37, 50
N = NY * NX
EXTRA = {"coverage": 6 * D * 8 + T // 4 + 64, "days_by": 6 * D * 8 + T // 4 + 64, "track_intensity": 6 * D * 8 + 64,
         "heat_stress": 4 * D * 8 + 64, "class_sums": 4 * 1 * 8 + 64, "regress": 4 * D * 8 + 64,
         "composite": 4 * D * 8 + T // 8 + 64, "lag_corr": 4 * D * 8 + 64 + 2 * T * 4}
BUDGET = {k: (T * 4 * 3 + T * 4 + v) * SLAB for k, v in EXTRA.items()}
TIME = np.datetime64("2001-01-01") + np.arange(T).astype("timedelta64[D]")
R = 3
LAND_TEXT = "All points of grid are either land or NaN"


def grid():
    """dict(ts (T, N) float32 with land and short NaN gaps, seas / thresh (D, N) with NaN on land, keep (N,), lines (N,):
    the points of the grid lines that are not all land, doy, doys)"""
    d = cc.synthetic(T, N, np.float32, seed=22, D=D, nan_frac=0.03)
    keep = np.ones(N, dtype=bool)
    keep[[3, 17, 18, 45]] = False                        # slab 0
    keep[50:100] = False                                 # slab 1, whole; it covers the grid lines 3 and 4
    keep[[205, 230, 239]] = False                        # slab 4, its last cell among them
    lines = np.repeat(keep.reshape(NY, NX).any(axis=1), NX)
    assert (~lines).sum() == 2 * NX and not lines[60:100].any()
    ts, seas, thresh = d["ts"].copy(), d["seas"].copy(), d["thresh"].copy()
    ts[:, ~keep] = np.nan
    seas[:, ~keep] = np.nan
    thresh[:, ~keep] = np.nan
    return dict(ts=ts, seas=seas, thresh=thresh, keep=keep, lines=lines, doy=d["doy"], doys=d["doys"])


@pytest.fixture(scope="module")
def gpu():
    from xmhw_amd._lib import require_gpu
    require_gpu()
    import xmhw_amd.device as dev
    g = grid()
    for name, extra in EXTRA.items():
        assert dev._grid_batch(g["ts"], BUDGET[name], per_cell_extra=extra) == SLAB, name
    return dev


@pytest.fixture(scope="module")
def pad3(gpu):
    from xmhw_amd.padding import make_pad
    pad = make_pad(np.timedelta64(3, "D"), TIME)
    yield pad
    pad.free()


@functools.lru_cache(maxsize=None)
def case(padded):
    """the grid, its host-compacted arrays and the series the oracles take (interpolated by the oracle when ``padded``)"""
    g = grid()
    keep = g["keep"]
    c = dict(g, ts_c=np.ascontiguousarray(g["ts"][:, keep]), seas_c=np.ascontiguousarray(g["seas"][:, keep]),
             thresh_c=np.ascontiguousarray(g["thresh"][:, keep]), C=int(keep.sum()))
    c["filled"] = po.interpolate_na(c["ts_c"], po.interp_index(TIME), 3 * 86400e9) if padded else c["ts_c"]
    assert c["filled"].dtype == np.float32 and (not padded or np.isnan(c["ts_c"]).sum() > np.isnan(c["filled"]).sum())
    c["wq"], c["reg"] = cc.weights_q(N), cc.scattered_regions(N, R)
    c["classes"], c["K"] = dc.runs_of_17(T)
    return c


def clims(c, stacked):
    """(seas, thresh, clim_stacked): compacted (D, C), or on the grid without its all-land lines (D, N' < N), NaN on land"""
    if stacked:
        se, th = c["seas"][:, c["lines"]], c["thresh"][:, c["lines"]]
        assert se.shape[1] == N - 2 * NX and np.isnan(se).all(axis=0).sum() == 17
        return np.ascontiguousarray(se), np.ascontiguousarray(th), True
    return c["seas_c"], c["thresh_c"], False


LEGS = [pytest.param(s, p, id=("stacked" if s else "compact") + ("-pad" if p else "")) for s in (False, True)
        for p in (False, True)]


# ---- coverage ----

@functools.lru_cache(maxsize=None)
def coverage_want(padded):
    c = case(padded)
    k = c["keep"]
    want = co.coverage_fast(c["filled"], c["seas_c"], c["thresh_c"], c["doy"], c["doys"], c["wq"][k], c["reg"][k], R)
    assert want[0][..., 4].sum() > 0, "a case without events proves nothing"
    return want


def coverage_call(c, se, th, stacked, pad=None, ts=None):
    from xmhw_amd.coverage import coverage_grid
    return coverage_grid(c["ts"] if ts is None else ts, False, se, th, c["doy"], c["doys"], c["wq"], c["reg"], R,
                         max_batch_bytes=BUDGET["coverage"], clim_stacked=stacked, pad=pad)


@pytest.mark.parametrize("stacked,padded", LEGS)
def test_coverage_grid_over_five_slabs(gpu, pad3, stacked, padded):
    from xmhw_amd.coverage import coverage_cells
    c, pad = case(padded), pad3 if padded else None
    cells, area, keep = coverage_call(c, *clims(c, stacked), pad=pad)
    npt.assert_array_equal(keep, c["keep"])
    k = c["keep"]
    dense = coverage_cells(c["ts_c"], c["seas_c"], c["thresh_c"], c["doy"], c["doys"], c["wq"][k], c["reg"][k], R, pad=pad)
    for got, one, want in zip((cells, area), dense, coverage_want(padded)):
        assert got.dtype == np.int64
        npt.assert_array_equal(got, one)
        npt.assert_array_equal(got, want)
    if padded:
        assert not np.array_equal(coverage_want(True)[0], coverage_want(False)[0])      # the interpolation matters


# ---- class days ----

@functools.lru_cache(maxsize=None)
def days_want(padded):
    c = case(padded)
    want = dbo.class_days_full(c["filled"], c["seas_c"], c["thresh_c"], c["doy"], c["doys"], c["classes"], c["K"])
    dc.check_case(want)
    assert want["n_range"] == 0
    return want


def days_call(c, se, th, stacked, pad=None, ts=None):
    from xmhw_amd.days_by import class_days_grid
    return class_days_grid(c["ts"] if ts is None else ts, False, se, th, c["doy"], c["doys"], c["classes"], c["K"],
                           max_batch_bytes=BUDGET["days_by"], clim_stacked=stacked, pad=pad)


@pytest.mark.parametrize("stacked,padded", LEGS)
def test_class_days_grid_over_five_slabs(gpu, pad3, stacked, padded):
    from xmhw_amd.days_by import class_days_cells
    c, pad = case(padded), pad3 if padded else None
    *got, keep = days_call(c, *clims(c, stacked), pad=pad)
    npt.assert_array_equal(keep, c["keep"])
    dense = class_days_cells(c["ts_c"], c["seas_c"], c["thresh_c"], c["doy"], c["doys"], c["classes"], c["K"], pad=pad)
    want = days_want(padded)
    for a, one, name in zip(got, dense, ("days", "isum_q", "intensity_max")):
        assert a.dtype == want[name].dtype
        npt.assert_array_equal(a, one, err_msg=name)
        npt.assert_array_equal(a, want[name], err_msg=name)


# ---- track intensity ----

@functools.lru_cache(maxsize=None)
def tracked(padded):
    """(rows, wi) of the detection of the (interpolated) series on the grid with its land: every object selected"""
    from xmhw_amd.detect import EventDataset
    from xmhw_amd.detect_front import detect_cells
    from xmhw_amd.track_intensity import intensity_bits
    c = case(padded)
    r = detect_cells(c["filled"], c["seas_c"], c["thresh_c"], c["doy"], c["doys"])
    coords = {"lat": np.linspace(-60, 60, NY), "lon": np.arange(NX) * 2.0, "time": TIME}
    mhw = EventDataset(np.asarray(r["table"], dtype=np.float64), np.asarray(r["offsets"], dtype=np.int64), TIME,
                       np.nonzero(c["keep"])[0], c["keep"], tc.SDIMS, (NY, NX), coords, {}, {}, {}, False)
    obj, tr, rows = tc.selection(mhw)
    assert obj.n_objects > 3 and rows.C == c["C"]
    rng = np.random.default_rng(5)
    return rows, rng.integers(0, (1 << intensity_bits(obj.weight_bits, c["C"])) + 1, c["C"]).astype(np.int64)


@functools.lru_cache(maxsize=None)
def intensity_want(padded):
    c = case(padded)
    rows, wi = tracked(padded)
    want = tio.stage_voxels(c["filled"], c["seas_c"], c["thresh_c"], c["doy"], c["doys"], rows, wi)
    assert want["n_valid"].sum() > 1000 and (want["cat_cells"].sum(axis=1) > 0).all() and want["n_range"] == 0
    return want


def intensity_call(c, padded, se, th, stacked, pad=None, ts=None, keep_want=None):
    from xmhw_amd.track_intensity import track_intensity_grid
    rows, wi = tracked(padded)
    return track_intensity_grid(c["ts"] if ts is None else ts, False, se, th, c["doy"], c["doys"], rows, wi,
                                c["keep"] if keep_want is None else keep_want, max_batch_bytes=BUDGET["track_intensity"],
                                clim_stacked=stacked, pad=pad)


@pytest.mark.parametrize("stacked,padded", LEGS)
def test_track_intensity_grid_over_five_slabs(gpu, pad3, stacked, padded):
    from xmhw_amd.track_intensity import track_intensity_cells
    c, pad = case(padded), pad3 if padded else None
    rows, wi = tracked(padded)
    got, keep = intensity_call(c, padded, *clims(c, stacked), pad=pad)
    npt.assert_array_equal(keep, c["keep"])
    assert got["n_range"] == 0 and got["n_bad"] == 0
    tio.same_integers(got, track_intensity_cells(c["ts_c"], c["seas_c"], c["thresh_c"], c["doy"], c["doys"], rows, wi, pad=pad))
    tio.same_integers(got, intensity_want(padded))


# ---- the stages with column-sliced accumulators ----

CLIMS = [pytest.param(False, id="compact"), pytest.param(True, id="stacked")]
WINDOW, H0, AT = 30, 0.5, np.array([0, 100, T - 1])
X0 = 15.0
J, BEFORE, AFTER, LAGS = 3, 2, 3, (-3, 5)


def slab_columns(keep):
    """the range of compact columns of every slab that is not all land"""
    k = np.concatenate(([0], np.cumsum(keep)))
    return [(int(k[lo]), int(k[min(lo + SLAB, N)])) for lo in range(0, N, SLAB) if keep[lo:lo + SLAB].any()]


def counted_in_every_slab(n, c):
    """a case that counts nothing in the columns of some slab cannot tell whether that slab's pointers were right"""
    cols = slab_columns(c["keep"])
    assert len(cols) == 4 and cols[0][0] == 0 and cols[-1][1] == c["C"] and cols[1][0] == cols[0][1] == 46
    for a, b in cols:
        assert (np.asarray(n)[..., a:b] != 0).any(), (a, b)


def same_as_both(got, dense, want, names):
    assert len(got) == len(dense) == len(want) == len(names)
    for a, one, w, name in zip(got, dense, want, names):
        assert a.dtype == one.dtype and a.shape == np.shape(w), name
        npt.assert_array_equal(a, one, err_msg=name)
        npt.assert_array_equal(a, w, err_msg=name)


def with_n_range_zero(oracle, *args):
    counters = {}
    out = oracle(*args, counters=counters)
    assert counters and not any(counters.values())
    return out


@functools.lru_cache(maxsize=None)
def stress_want():
    c = case(False)
    classes, K = hc.per_year(T)
    args = (c["doy"], c["doys"], classes, K, WINDOW, H0, hc.levels(2), AT)
    want = with_n_range_zero(ho.heat_stress_cells, c["ts_c"], c["seas_c"], *args)
    hc.check_case(dict(zip(("counts", "hsum_q", "peak_q", "peak_t", "snap_q"), want)))
    counted_in_every_slab(want[0][:, 1], c)                   # hot steps
    counted_in_every_slab(want[4], c)
    return args, want


@pytest.mark.parametrize("stacked", CLIMS)
def test_heat_stress_grid_over_five_slabs(gpu, stacked):
    from xmhw_amd.heat_stress import heat_stress_cells, heat_stress_grid
    c = case(False)
    args, want = stress_want()
    se, _, _ = clims(c, stacked)
    *got, keep = heat_stress_grid(c["ts"], False, se, *args, max_batch_bytes=BUDGET["heat_stress"], clim_stacked=stacked)
    npt.assert_array_equal(keep, c["keep"])
    same_as_both(got, heat_stress_cells(c["ts_c"], c["seas_c"], *args), want, ("counts", "hsum_q", "peak_q", "peak_t", "snap_q"))


@functools.lru_cache(maxsize=None)
def sums_want():
    c = case(False)
    want = with_n_range_zero(ho.class_sums_cells, c["ts_c"], c["classes"], c["K"], X0)
    counted_in_every_slab(want[0], c)
    counted_in_every_slab(want[1], c)
    return want


@pytest.mark.parametrize("stacked", CLIMS)
def test_class_sums_grid_over_five_slabs(gpu, stacked):
    from xmhw_amd.heat_stress import class_sums_cells, class_sums_grid
    c = case(False)
    land = np.where(c["keep"], 0.0, np.nan)[None]
    land = np.ascontiguousarray(land[:, c["lines"]]) if stacked else np.zeros((1, c["C"]))
    *got, keep = class_sums_grid(c["ts"], False, land, c["classes"], c["K"], X0, max_batch_bytes=BUDGET["class_sums"],
                                 clim_stacked=stacked)
    npt.assert_array_equal(keep, c["keep"])
    same_as_both(got, class_sums_cells(c["ts_c"], c["classes"], c["K"], X0), sums_want(), ("n_valid", "sum_q"))


@functools.lru_cache(maxsize=None)
def regress_want():
    c = case(False)
    classes, K = irc.runs(T)
    args = (c["doy"], c["doys"], classes, K, irc.predictors(T, J, 5))
    want = with_n_range_zero(iro.regress_cells, c["ts_c"], c["seas_c"], *args)
    irc.check_case(dict(zip(iro.FIELDS, want)))
    for name in ("n", "saz", "mz"):
        counted_in_every_slab(want[iro.FIELDS.index(name)], c)
    return args, want


@pytest.mark.parametrize("stacked", CLIMS)
def test_regress_grid_over_five_slabs(gpu, stacked):
    from xmhw_amd.index_regression import FIELDS, regress_cells, regress_grid
    c = case(False)
    args, want = regress_want()
    se, _, _ = clims(c, stacked)
    *got, keep = regress_grid(c["ts"], False, se, *args, max_batch_bytes=BUDGET["regress"], clim_stacked=stacked)
    npt.assert_array_equal(keep, c["keep"])
    assert got[5].shape == (args[3], J, c["C"])
    same_as_both(got, regress_cells(c["ts_c"], c["seas_c"], *args), want, FIELDS)


@functools.lru_cache(maxsize=None)
def composite_want():
    """(the anchor table of the ocean cells, the arguments after the cells, the oracle's arrays)"""
    c = case(False)
    A = cpc.anchor_columns(T, c["C"], BEFORE + AFTER + 1)
    for a, b in slab_columns(c["keep"]):
        assert A[:, a:b].any(), "an anchor in every slab"
    view = cpc.table_of(A)
    classes, K = cpc.every_step(T)
    args = (classes, K, BEFORE, AFTER, 0)
    want = with_n_range_zero(cpo.composite_cells, c["ts_c"], c["seas_c"], c["doy"], c["doys"], view, np.arange(c["C"]), *args)
    for a in want:
        counted_in_every_slab(a, c)
    return view, args, want


@pytest.mark.parametrize("stacked", CLIMS)
def test_composite_grid_over_five_slabs(gpu, stacked):
    from xmhw_amd.composite import FIELDS, composite_cells, composite_grid
    c = case(False)
    view, args, want = composite_want()
    se, _, _ = clims(c, stacked)
    of_point = np.zeros(N, dtype=np.int64)                    # the table cell of every grid point; land points are not read
    of_point[c["keep"]] = np.arange(c["C"])
    *got, keep = composite_grid(c["ts"], False, se, c["doy"], c["doys"], view, of_point, *args,
                                max_batch_bytes=BUDGET["composite"], clim_stacked=stacked)
    npt.assert_array_equal(keep, c["keep"])
    dense = composite_cells(c["ts_c"], c["seas_c"], c["doy"], c["doys"], view, np.arange(c["C"]), *args)
    same_as_both(got, dense, want, FIELDS)


@functools.lru_cache(maxsize=None)
def lag_want():
    """(y on the whole grid: no land of its own but NaN gaps and one all-NaN ocean cell of x, the arguments, the oracle)"""
    c = case(False)
    y = cc.synthetic(T, N, np.float32, seed=23, D=D, nan_frac=0.03)["ts"] + np.float32(0.4) * np.nan_to_num(c["ts"])
    y[:, 120] = np.nan
    assert c["keep"][120] and y.dtype == np.float32 and not np.isnan(y[:, ~c["keep"]]).all()
    classes = ((np.arange(T) // 17) % 2).astype(np.int32)
    args = (c["doy"], c["doys"], classes, 2, *LAGS)
    want = with_n_range_zero(lco.lag_corr_cells, c["ts_c"], y[:, c["keep"]], c["seas_c"], c["thresh_c"], *args)
    assert want[0].shape == (2, LAGS[1] - LAGS[0] + 1, c["C"])
    for a in want:
        counted_in_every_slab(a[:, :-LAGS[0]], c)             # the second pass: the negative lags
        counted_in_every_slab(a[:, -LAGS[0]:], c)
    assert not np.array_equal(want[1][:, 0], want[2][:, 0])   # sx and sy differ: the roles are told apart
    return y, args, want


@pytest.mark.parametrize("stacked", CLIMS)
def test_lag_corr_grid_over_five_slabs(gpu, stacked):
    from xmhw_amd.lag_correlation import FIELDS, lag_corr_cells, lag_corr_grid
    c = case(False)
    y, args, want = lag_want()
    se, th, _ = clims(c, stacked)
    *got, keep = lag_corr_grid(c["ts"], False, y, se, th, *args, max_batch_bytes=BUDGET["lag_corr"], clim_stacked=stacked)
    npt.assert_array_equal(keep, c["keep"])
    dense = lag_corr_cells(c["ts_c"], np.ascontiguousarray(y[:, c["keep"]]), c["seas_c"], c["thresh_c"], *args)
    same_as_both(got, dense, want, FIELDS)


# ---- the refusals ----

def refusals(c):
    """(id, text, kwargs of a *_call): climatologies with one ocean cell fewer and one more, an all-NaN grid, se and th with
    different ocean counts"""
    se, th = c["seas_c"], c["thresh_c"]
    more = lambda a: np.ascontiguousarray(np.concatenate([a, a[:, -1:]], axis=1))        # noqa: E731
    less = lambda a: np.ascontiguousarray(a[:, :-1])                                     # noqa: E731
    C = c["C"]
    return [("fewer", f"temp has more ocean cells than th and se \\({C - 1}\\)", dict(se=less(se), th=less(th))),
            ("more", f"temp has {C} ocean cells, th and se have {C + 1}", dict(se=more(se), th=more(th))),
            ("all_nan", LAND_TEXT, dict(se=se, th=th, ts=np.full((T, N), np.nan, dtype=np.float32))),
            ("se_th_differ", f"th and se do not have the same ocean cells: {C}, {C - 1}", dict(se=less(se), th=th))]


def refused_then_good(gpu, text, bad, good):
    from xmhw_amd import XmhwException
    before = gpu.device_cache_bytes()
    with pytest.raises(XmhwException, match=text):
        bad()
    good()
    assert gpu.device_cache_bytes() == before


@pytest.mark.parametrize("which", ["fewer", "more", "all_nan", "se_th_differ"])
def test_refusals_keep_their_text_and_leak_nothing(gpu, which):
    c = case(False)
    _, text, kw = next(r for r in refusals(c) if r[0] == which)

    def good_coverage():
        cells, area, _ = coverage_call(c, c["seas_c"], c["thresh_c"], False)
        npt.assert_array_equal(cells, coverage_want(False)[0])
        npt.assert_array_equal(area, coverage_want(False)[1])

    def good_days():
        days, isum, imax, _ = days_call(c, c["seas_c"], c["thresh_c"], False)
        npt.assert_array_equal(days, days_want(False)["days"])
        npt.assert_array_equal(isum, days_want(False)["isum_q"])

    def good_intensity():
        tio.same_integers(intensity_call(c, False, c["seas_c"], c["thresh_c"], False)[0], intensity_want(False))

    refused_then_good(gpu, text, lambda: coverage_call(c, kw["se"], kw["th"], False, ts=kw.get("ts")), good_coverage)
    refused_then_good(gpu, text, lambda: days_call(c, kw["se"], kw["th"], False, ts=kw.get("ts")), good_days)
    # (the detection of an all-NaN grid has no ocean cell: the mask comparison passes and the walk refuses the grid)
    keep_want = np.zeros(N, dtype=bool) if which == "all_nan" else None
    refused_then_good(gpu, text, lambda: intensity_call(c, False, kw["se"], kw["th"], False, ts=kw.get("ts"),
                                                        keep_want=keep_want), good_intensity)


def test_stacked_climatologies_that_are_all_land(gpu):
    c = case(False)
    se, th, _ = clims(c, True)
    for call in (coverage_call, days_call):
        refused_then_good(gpu, LAND_TEXT, lambda: call(c, np.full_like(se, np.nan), th, True),
                          lambda: npt.assert_array_equal(call(c, se, th, True)[-1], c["keep"]))


def test_track_intensity_refuses_a_mask_that_differs_in_the_last_slab(gpu):
    c = case(False)
    keep_want = c["keep"].copy()
    keep_want[238] = False                               # ocean in temp, land in the detection
    refused_then_good(gpu, "the land mask of temp differs from mhw.keep",
                      lambda: intensity_call(c, False, c["seas_c"], c["thresh_c"], False, keep_want=keep_want),
                      lambda: tio.same_integers(intensity_call(c, False, c["seas_c"], c["thresh_c"], False)[0],
                                                intensity_want(False)))
    keep_want = c["keep"].copy()
    keep_want[70] = True                                 # ... and in the slab that is all land
    refused_then_good(gpu, "the land mask of temp differs from mhw.keep",
                      lambda: intensity_call(c, False, c["seas_c"], c["thresh_c"], False, keep_want=keep_want),
                      lambda: None)
