"""The finish kernels on their own: xmhw_amd.device.clim_finish (the Feb-29 substitution and the circular running mean,
identify.py:137-181) on synthetic raw (D, C) climatologies written straight into device buffers -- no climatology kernel
runs -- against oracle_fast.finish_exact, the same positional semantics with every sum correctly rounded.

launch_finish (xmhw_amd/csrc/kernels_generic.hip) picks one of three kernels, and a fourth pass behind one of them:
  stream    clim_finish_stream<31, 31>   smooth, width 31, D >= 64 (one part of the doy axis, four above D = 732)
  redo      clim_finish(only = flags)    behind the stream kernel, on every column with an absent group (NaN row)
  tiled     clim_finish_tiled<16>        every other call with D <= 511; a column with absent groups on one thread
  untiled   clim_finish                  every other call with D > 511

* dyadic data (k/64: every sum exact in float64): every output of every variant bit-identical to the reference --
  a wrong window edge, wrap, present-row neighbour or Feb-29 operand shows as a wrong value, not as rounding;
* mixed-sign float data (a polar climatology crossing 0 degC, anomalies, Kelvin offsets): |gpu - exact| <= 16 eps M[d]
  (M: oracle_fast.finish_exact), the reference's inf / NaN classification exactly;
* cut independence, pitch canaries, the refusals of the C ABI."""
import functools

import numpy as np
import pytest

import oracle_fast as fast
import xmhw_amd.device as dev
from xmhw_amd.exception import XmhwException

EPS = np.finfo(np.float64).eps
TOL = 16           # eps * M


def _variant(D, width, smooth):
    """the kernel launch_finish (xmhw_amd/csrc/kernels_generic.hip) runs; "stream" is followed by the redo pass
    (clim_finish(only = flags)) on the columns that hold a NaN row"""
    if smooth and width == 31 and D >= 64:
        return "stream"
    if D * 16 * 8 + 64 <= 64 * 1024:
        return "tiled"
    return "untiled"


LABELS = {f"1..{D}": np.arange(1, D + 1) for D in (12, 52, 63, 64, 65, 366, 511, 512, 732, 733, 1460)}
LABELS["366 w/o 59"] = np.setdiff1d(np.arange(1, 367), [59])
LABELS["366 w/o 61"] = np.setdiff1d(np.arange(1, 367), [61])


@functools.lru_cache(maxsize=None)
def _plan(labels):
    """a plan on three repeats of the labels: D and the rows of labels 59/60/61 (-1: absent)"""
    return dev.Plan(np.tile(LABELS[labels], 3), 5)


def _rows(plan):
    return tuple(int(np.nonzero(plan.doys == k)[0][0]) if (plan.doys == k).any() else -1 for k in (59, 60, 61))


PATTERNS = ["no NaN", "row 0 absent", "row D-1 absent", "rows D-5 .. 3 absent (across the wrap)",
            "row 60 absent (no leap year)", "59 absent, 60 present", "61 absent, 60 present",
            "59 and 61 absent, 60 present", "one row present", "fewer present rows than width", "all rows NaN",
            "+inf in one row", "+inf and -inf two rows apart across the wrap (direct path)",
            "+inf, NaN, -inf (positional path)", "+inf at row 59", "row 15 absent (last row of the first stream window)",
            "5 % of rows absent"]


def _apply(col, p, rows, width, rng):
    """column pattern p of PATTERNS, in place (where labels 59/60/61 are absent, rows near D/2 stand in for them)"""
    D = col.shape[0]
    i59, i60, i61 = rows
    r60 = i60 if i60 >= 0 else D // 2
    r59 = i59 if i59 >= 0 else r60 - 1
    r61 = i61 if i61 >= 0 else min(r60 + 1, D - 1)
    if p == 1:
        col[0] = np.nan
    elif p == 2:
        col[D - 1] = np.nan
    elif p == 3:
        col[D - 5:] = np.nan
        col[:4] = np.nan
    elif p == 4:
        col[r60] = np.nan
    elif p == 5:
        col[r59] = np.nan
    elif p == 6:
        col[r61] = np.nan
    elif p == 7:
        col[[r59, r61]] = np.nan
    elif p == 8:
        keep = rng.integers(D)
        col[np.arange(D) != keep] = np.nan
    elif p == 9:
        k = min(max(width - 1, 1), D - 1)
        col[np.sort(rng.permutation(D)[k:])] = np.nan
    elif p == 10:
        col[:] = np.nan
    elif p == 11:
        col[rng.integers(D)] = np.inf
    elif p == 12:
        col[D - 1] = np.inf
        col[1] = -np.inf
    elif p == 13:
        r = D // 3
        col[r], col[r + 1], col[r + 2] = np.inf, np.nan, -np.inf
    elif p == 14:
        col[r59] = np.inf
    elif p == 15:
        col[min(15, D - 1)] = np.nan
    elif p == 16:
        col[rng.random(D) < 0.05] = np.nan


def _data(kind, rng, D, C):
    t = np.arange(D)[:, None]
    if kind == "dyadic":          # k/64, |k| < 2**19: sums of up to 1024 of them are exact
        return rng.integers(-(2 ** 19) + 1, 2 ** 19, size=(D, C)) / 64.0
    ph = rng.uniform(0, D, C)
    if kind == "arctic":          # a polar SST climatology in degC: -1.8 .. +3, crossing 0 twice a year
        return np.clip(0.6 + 2.4 * np.sin(2 * np.pi * (t - ph) / D) + 0.3 * rng.normal(size=(D, C)), -1.8, 3.0)
    if kind == "anomaly":         # anomalies: mean near 0
        return rng.normal(size=(D, C)) * rng.uniform(0.05, 2.0, C) + 0.05 * np.sin(2 * np.pi * (t - ph) / D)
    if kind == "kelvin":          # 271 .. 275 K
        return 273.0 + 1.8 * np.sin(2 * np.pi * (t - ph) / D) + 0.1 * rng.normal(size=(D, C))
    raise ValueError(kind)


def _columns(labels, C, width, kind, seed):
    """(th, se): (D, C) raw climatologies, column c in pattern (c + seed) % len(PATTERNS); seas takes another
    pattern than thresh in every odd column"""
    plan = _plan(labels)
    rng = np.random.default_rng(seed)
    rows = _rows(plan)
    th, se = _data(kind, rng, plan.D, C), _data(kind, rng, plan.D, C)
    for c in range(C):
        p = (c + seed) % len(PATTERNS)
        _apply(th[:, c], p, rows, width, rng)
        _apply(se[:, c], p if c % 2 == 0 else (p + 5) % len(PATTERNS), rows, width, rng)
    if kind == "dyadic":
        fast.dyadic_feb29(plan.doys, th)
        fast.dyadic_feb29(plan.doys, se)
    return th, se


CANARY = np.uint64(0xFFFFFFFFFFFFFFFF)


def _finish(labels, th, se, feb29_fix, smooth, width, ldo=None, junk=1e300):
    """clim_finish on (D, C) arrays laid out with pitch ldo (input pitch columns hold `junk`, output buffers start as
    0xFF bytes); returns the (D, C) outputs after checking that the output pitch columns kept their 0xFF bytes"""
    plan = _plan(labels)
    D, C = th.shape
    ldo = C if ldo is None else ldo
    bufs = []
    for a in (th, se):
        p = np.full((D, ldo), junk)
        p[:, :C] = a
        bufs.append(dev.DeviceBuffer.from_array(p))
    outs = [dev.DeviceBuffer.from_array(np.full((D, ldo), CANARY, np.uint64)) for _ in range(2)]
    dev.clim_finish(plan, bufs[0], bufs[1], C, feb29_fix, smooth, width, outs[0], outs[1], ldo=ldo)
    dev.hip().stream_sync(0)
    res = []
    for o in outs:
        a = o.to_array((D, ldo), np.uint64)
        assert (a[:, C:] == CANARY).all(), "a pitch column [C, ldo) was written"
        res.append(np.ascontiguousarray(a[:, :C]).view(np.float64))
    for b in bufs + outs:
        b.free()
    return res


def _reference(labels, a, feb29_fix, smooth, width, dyadic):
    doys = _plan(labels).doys
    out, M = np.empty_like(a), np.empty_like(a)
    for c in range(a.shape[1]):
        out[:, c], M[:, c] = fast.finish_exact(doys, a[:, c], feb29_fix, smooth, width, dyadic=dyadic)
    return out, M


def _widths(D):
    return [1, 5, 31, 33, 45 if D == 12 else D + 1 + D % 2]


def _cases():
    """(labels, width, smooth, feb29_fix, C): every label set x widths 1, 5, 31, 33 and one larger than D x smooth
    on / off x feb29 on / off at C = 257, and C = 1 and 17 at widths 5 and 31"""
    out = []
    for labels, lab in LABELS.items():
        has60 = (lab == 60).any()
        for feb29_fix in ((False, True) if has60 else (False,)):
            out.append((labels, 1, False, feb29_fix, 257))
            for width in _widths(lab.size):
                out.append((labels, width, True, feb29_fix, 257))
            for C in (1, 17):
                for width in (5, 31):
                    out.append((labels, width, True, feb29_fix, C))
    return out


CASES = _cases()


def _id(case):
    labels, width, smooth, feb29_fix, C = case
    return f"{labels}-w{width if smooth else '-'}-feb29{int(feb29_fix)}-C{C}"


def _reached(case):
    labels, width, smooth, _, C = case
    v = _variant(LABELS[labels].size, width, smooth)
    return {v, "redo"} if v == "stream" and C > 1 else {v}      # C > 1: columns with absent groups


def test_matrix_reaches_every_variant_at_its_edges():
    """every variant meets the D edges it can run at, and widths 1, 5, 31, 33 where it can run them"""
    edges = {12, 52, 63, 64, 65, 366, 511, 512, 732, 733, 1460}
    seen = {}
    for case in CASES:
        for v in _reached(case):
            s = seen.setdefault(v, {"D": set(), "width": set(), "C": set()})
            s["D"].add(LABELS[case[0]].size)
            s["width"].add(case[1] if case[2] else 0)
            s["C"].add(case[4])
    assert set(seen) == {"stream", "redo", "tiled", "untiled"}
    assert seen["stream"]["D"] == seen["redo"]["D"] == {d for d in edges if d >= 64} | {365}
    assert seen["tiled"]["D"] == {d for d in edges if d <= 511} | {365}
    assert seen["untiled"]["D"] == {d for d in edges if d > 511}
    assert {1, 5, 31, 33, 45, 0} <= seen["tiled"]["width"] and {1, 5, 33, 513, 0} <= seen["untiled"]["width"]
    assert any(_variant(LABELS[c[0]].size, c[1], c[2]) == "tiled" and c[1] == 31 and c[2] for c in CASES)
    assert seen["stream"]["C"] == {1, 17, 257} and {1, 17, 257} <= seen["tiled"]["C"] and {1, 17, 257} <= seen["untiled"]["C"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_dyadic_bit_identical(case):
    """every output bit-identical to the exact reference, NaN positions included"""
    labels, width, smooth, feb29_fix, C = case
    seed = CASES.index(case)
    th, se = _columns(labels, C, width, "dyadic", seed)
    got = _finish(labels, th, se, feb29_fix, smooth, width, ldo=C + 3)
    for name, a, g in (("thresh", th, got[0]), ("seas", se, got[1])):
        want, _ = _reference(labels, a, feb29_fix, smooth, width, dyadic=True)
        bad = ~((g == want) | (np.isnan(g) & np.isnan(want)))
        if bad.any():
            d, c = np.argwhere(bad)[0]
            p = (c + seed) % len(PATTERNS) if name == "thresh" or c % 2 == 0 else ((c + seed) % len(PATTERNS) + 5) % len(PATTERNS)
            raise AssertionError(f"{_variant(LABELS[labels].size, width, smooth)}: {name} differs at {bad.sum()} outputs, "
                                 f"first row {d} column {c} ({PATTERNS[p]}): {g[d, c]!r} != {want[d, c]!r}")


FLOAT_SHAPES = [("366", 31, True), ("1460", 31, True), ("733", 31, False), ("64", 31, True),
                ("366", 5, True), ("511", 33, True), ("63", 31, True), ("12", 45, False), ("366 w/o 59", 1, True),
                ("1460", 11, False), ("512", 33, True), ("733", 5, True), ("1460", 1, True)]
_worst = {}


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["arctic", "anomaly", "kelvin"])
@pytest.mark.parametrize("shape", FLOAT_SHAPES, ids=lambda s: f"{s[0]}-w{s[1]}-feb29{int(s[2])}")
def test_float_within_16_eps_M(shape, kind):
    """|gpu - exact| <= 16 eps M[d] on every finite output (M: the magnitude of the window sums a re-summed sliding sum
    goes through), the exact inf / NaN classification elsewhere"""
    D, width, feb29_fix = shape
    labels = D if D.startswith("366 ") else f"1..{D}"
    seed = 1000 + FLOAT_SHAPES.index(shape) * 3 + ["arctic", "anomaly", "kelvin"].index(kind)
    th, se = _columns(labels, 257, width, kind, seed)
    got = _finish(labels, th, se, feb29_fix, True, width)
    v = _variant(LABELS[labels].size, width, True)
    worst = 0.0
    for name, a, g in (("thresh", th, got[0]), ("seas", se, got[1])):
        want, M = _reference(labels, a, feb29_fix, True, width, dyadic=False)
        np.testing.assert_array_equal(np.isnan(g), np.isnan(want), err_msg=f"{v} {name}: NaN positions")
        inf = np.isinf(want)
        np.testing.assert_array_equal(g[inf], want[inf], err_msg=f"{v} {name}: infinities")
        fin = np.isfinite(want)
        assert np.isfinite(g[fin]).all()
        err = np.where(fin, np.abs(g - want) / (EPS * np.where(fin, M, 1.0)), 0.0)
        e = float(err.max(initial=0.0))
        # the worst of each variant, by the kernel that computed it (behind the stream kernel, the redo pass computes
        # every column of a cell with an absent group in thresh or seas)
        flagged = np.isnan(th).any(axis=0) | np.isnan(se).any(axis=0)
        parts = {v: slice(None)} if v != "stream" else {"stream": ~flagged, "redo": flagged}
        for var, sel in parts.items():
            _worst[var] = max(_worst.get(var, 0.0), float(err[:, sel].max(initial=0.0)))
        print(f"\nFINISH_ERR variant={v} labels={labels} width={width} feb29={int(feb29_fix)} kind={kind} {name} "
              f"max={e:.2f} eps*M; worst so far {dict((k, round(x, 2)) for k, x in sorted(_worst.items()))}")
        worst = max(worst, e)
    assert worst <= TOL, f"{v}: {worst:.1f} eps M > {TOL}"


CUT_SHAPES = [("1..366", 31), ("1..1460", 31), ("1..366", 5), ("1..63", 31), ("1..1460", 11), ("1..733", 33)]


@pytest.mark.gpu
@pytest.mark.parametrize("labels,width", CUT_SHAPES)
def test_cut_independence(labels, width):
    """cells [a, b) of a C = 1000, ldo = 1031 array finished through offset pointers: bit-identical to the same
    columns of the whole-array call, and so are the clean columns (no NaN in either array) finished on their own"""
    C, ldo = 1000, 1031
    th, se = _columns(labels, C, width, "arctic", 7)
    whole = _finish(labels, th, se, True, True, width, ldo=ldo)
    plan = _plan(labels)
    D = plan.D
    pitched = []
    for a in (th, se):
        p = np.full((D, ldo), -3.5)
        p[:, :C] = a
        pitched.append(dev.DeviceBuffer.from_array(p))
    outs = [dev.DeviceBuffer.from_array(np.full((D, ldo), CANARY, np.uint64)) for _ in range(2)]
    cuts = [(0, 1), (1, 17), (17, 255), (255, 513), (513, 999), (999, 1000)]
    for a, b in cuts:
        dev.clim_finish(plan, pitched[0].ptr + 8 * a, pitched[1].ptr + 8 * a, b - a, True, True, width,
                        outs[0].ptr + 8 * a, outs[1].ptr + 8 * a, ldo=ldo)
    dev.hip().stream_sync(0)
    for o, w in zip(outs, whole):
        got = o.to_array((D, ldo), np.uint64)
        assert (got[:, C:] == CANARY).all()
        np.testing.assert_array_equal(got[:, :C], w.view(np.uint64), err_msg=f"{_variant(D, width, True)}: cut at {cuts}")
    for b in pitched + outs:
        b.free()
    clean = ~(np.isnan(th).any(axis=0) | np.isnan(se).any(axis=0))
    assert 0 < clean.sum() < C
    alone = _finish(labels, th[:, clean], se[:, clean], True, True, width)
    for g, w in zip(alone, whole):
        np.testing.assert_array_equal(g.view(np.uint64), w[:, clean].view(np.uint64))


@pytest.mark.gpu
@pytest.mark.parametrize("labels,width", CUT_SHAPES)
def test_one_array_does_not_see_the_others_absent_groups(labels, width):
    """thresh and seas of a cell are finished independently: a clean seas column gives the same bits whether or not
    the thresh column of its cell has absent groups (the stream kernel flags the CELL, and its redo pass must then
    reproduce the stream kernel's arithmetic), and the other way round"""
    C = 257
    th, se = _columns(labels, C, width, "anomaly", 11)
    ref_th, ref_se = _columns(labels, C, width, "anomaly", 11)
    for a in (ref_th, ref_se):
        a[np.isnan(a)] = 0.25          # both arrays clean
        a[np.isinf(a)] = -0.5
    th_only = _finish(labels, th, ref_se, True, True, width)       # absent groups in thresh only
    se_only = _finish(labels, ref_th, se, True, True, width)       # in seas only
    both = _finish(labels, ref_th, ref_se, True, True, width)
    v = _variant(_plan(labels).D, width, True)
    np.testing.assert_array_equal(th_only[1].view(np.uint64), both[1].view(np.uint64), err_msg=f"{v}: seas")
    np.testing.assert_array_equal(se_only[0].view(np.uint64), both[0].view(np.uint64), err_msg=f"{v}: thresh")


@pytest.mark.gpu
def test_refusals_and_empty_call():
    plan = _plan("1..366")
    D, C = plan.D, 8
    a = dev.DeviceBuffer.from_array(np.zeros((D, C)))
    b = dev.DeviceBuffer.from_array(np.zeros((D, C)))
    o1 = dev.DeviceBuffer.from_array(np.full((D, C), CANARY, np.uint64))
    o2 = dev.DeviceBuffer.from_array(np.full((D, C), CANARY, np.uint64))
    for width in (0, -1, -31, 2, 30):
        with pytest.raises(XmhwException):
            dev.clim_finish(plan, a, b, C, True, True, width, o1, o2)
    with pytest.raises(XmhwException):
        dev.clim_finish(plan, a, b, C, True, True, 31, o1, o2, ldo=C - 1)
    with pytest.raises(XmhwException):
        dev.clim_finish(plan, a, b, C, True, True, 31, a, o2)
    with pytest.raises(XmhwException):
        dev.clim_finish(plan, a, b, C, True, True, 31, o1, b)
    dev.clim_finish(plan, a, b, 0, True, True, 31, o1, o2)
    dev.hip().stream_sync(0)
    for o in (o1, o2):
        assert (o.to_array((D, C), np.uint64) == CANARY).all()
