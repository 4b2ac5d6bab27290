"""Inputs for the float64 narrowing give-up (probe -> narrowing float32 ring kernel -> gated float64 kernel).
TEST INFRASTRUCTURE ONLY.  No GPU: tests/test_narrowing_cases.py checks this generator on the oracle,
tests/test_gpu_narrowing.py runs it through the kernels.

A float64 series of float32-representable samples (`series`) gets ONE sample float32 cannot hold (`hide`), on a row the
sparse probe does not look at (`probe_rows`), at the places where the three in-kernel checks could miss it
(`positions`, `cells`): the narrowing kernel has to find it in its own row loop."""
import numpy as np

from test_gpu_parity import _series, _daily

Y0 = 1901                          # first year of every record: leap years 1904, 1908, ...
OUTWARD = 1 + 0.123456789012345    # how far "top" moves the cell's extreme
KINDS = ("top", "ulp", "huge", "tiny", "above_max")
SPECIAL_CELLS = (1, 2, 3, 4, 5)    # series(): all-NaN, +inf run, +-0, float32 subnormals, +-FLT_MAX
FLT_MAX = 3.4028234663852886e38


def _route(w, years, narrow, gated):
    return dict(w=w, years=years, narrow=narrow, gated=gated, id=f"w{w}-{years}y-{narrow[0]}_{narrow[1]}_{narrow[2]}-{gated[0]}_{gated[1]}")


# one record per distinct (narrowing -> gated) pair of the default float64 dispatch (tests/golden/threshold_routes.npz,
# 0_routes: layout and kernel automatic, narrowing on, 8-byte samples), at its smallest record length:
# narrow = (family, layout, lanes) of launch 0, gated = (family, layout) of launch 1
ROUTES = (
    _route(5, 8, ("ring1", -1, 8), ("ring2", 12)),
    _route(5, 9, ("ring3", 22, 2), ("ring3", 20)),
    _route(5, 13, ("ring3", 22, 2), ("ring3", 21)),
    _route(5, 17, ("ring2", 10, 4), ("ring3", 21)),
    _route(5, 21, ("ring2", 8, 8), ("ring3", 20)),
    _route(5, 25, ("ring3", 21, 4), ("ring3", 20)),
    _route(5, 49, ("ring3", 20, 8), ("ring2", 12)),
    _route(5, 65, ("ring1", -1, 32), ("ring2", 12)),
    _route(5, 89, ("ring2", 12, 16), ("ring2", 12)),
    _route(5, 97, ("ring1", -1, 32), ("generic", -1)),
    _route(2, 9, ("ring1", -1, 8), ("generic", -1)),
    _route(7, 33, ("ring1", -1, 16), ("generic", -1)),
)


def calendar(route):
    """(time, doy) of a record: daily, Y0 .. Y0 + years - 1"""
    return _daily(Y0, Y0 + route["years"] - 1)


def ncells(route):
    """70 cells, 40 for the long records: the last wave and the last workgroup are ragged for every layout"""
    return 40 if route["years"] >= 65 else 70


def route_pair(r):
    """a Plan.route() as the ROUTES records state it: ((family, layout, lanes), (family, layout)); the flags of the
    two launches are asserted here (the first narrows, the second is gated)"""
    la = r["launches"]
    assert r["supported"] and len(la) == 2, r
    assert la[0]["narrows"] and not la[0]["gated"] and la[1]["gated"] and not la[1]["narrows"], r
    return (la[0]["family"], la[0]["layout"], la[0]["lanes"]), (la[1]["family"], la[1]["layout"])


def series(T, C, seed):
    """float64 samples that float32 holds exactly: the seasonal series of the parity tests with 2 % NaN, and (where C
    leaves room) the SPECIAL_CELLS: an all-NaN cell, a run of +inf, alternating +-0, float32 subnormals, +-FLT_MAX"""
    x = _series(T, C, seed, 0.02, dtype=np.float32).astype(np.float64)
    rng = np.random.default_rng(seed + 1000)
    if C > 1:
        x[:, 1] = np.nan
    if C > 2:
        x[100:140, 2] = np.inf
    if C > 3:
        x[:, 3] = np.where(np.arange(T) % 2 == 0, 0.0, -0.0)
    if C > 4:
        x[:, 4] = rng.integers(1, 2000, T).astype(np.uint32).view(np.float32).astype(np.float64)     # k * 2^-149
    if C > 5:
        x[:, 5] = np.where(rng.random(T) < 0.5, FLT_MAX, -FLT_MAX)
    assert representable(x).all()
    return x


def representable(x):
    """per sample: float32 holds it (NaN counts as held, as in the kernels)"""
    with np.errstate(over="ignore"):
        return (x.astype(np.float32).astype(np.float64) == x) | np.isnan(x)


def probe_rows(T):
    """the rows narrow_probe (kernels_ring.hip) reads of every cell"""
    return range(0, T, max(T // 32, 1))


def hidden_value(x, t, c, kind, cold):
    col = x[:, c]
    fin = col[np.isfinite(col)]
    if kind == "top":
        return float(fin.min() - OUTWARD if cold else fin.max() + OUTWARD)
    if kind == "ulp":
        base = col[t] if np.isfinite(col[t]) else np.float32(np.median(fin))
        assert np.float64(np.float32(base)) == base
        return float(np.nextafter(np.float64(base), np.inf))
    if kind == "huge":
        return -1e300 if cold else 1e300
    if kind == "tiny":
        return 2.0 ** -150
    if kind == "above_max":
        return 3.4028235677973366e38           # rounds to inf in float32
    raise ValueError(kind)


def checked_value(x, t, c, kind, cold=False):
    """hidden_value(), after the two conditions of hide(): a row the probe does not read, a double float32 cannot hold"""
    assert t not in probe_rows(x.shape[0]), t
    v = np.float64(hidden_value(x, t, c, kind, cold))
    assert np.isfinite(v) and not representable(np.array([v]))[0], (kind, v)
    return v


def hide(x, t, c, kind, cold=False):
    """a copy of x with x[t, c] replaced by a double float32 cannot hold, on a row the probe does not read"""
    out = x.copy()
    out[t, c] = checked_value(x, t, c, kind, cold)
    return out


def positions(doy, ntracks, nchunks=3):
    """[(t, label)]: the time steps where a hidden sample is placed; one that falls on a probe row moves to the
    neighbouring step and keeps its label.  Daily calendar that starts on Jan 1 (label 60 only in leap years)."""
    doy = np.asarray(doy)
    T = doy.shape[0]
    probe = set(probe_rows(T))
    starts = np.nonzero(doy == 1)[0]
    assert starts.shape[0] == ntracks and starts[0] == 0
    ends = np.append(starts[1:], T)
    feb29 = np.nonzero(doy == 60)[0]
    leap = np.searchsorted(starts, feb29, side="right") - 1           # the years that have one

    def day(year, label):
        return int(starts[year] + np.nonzero(doy[starts[year]:ends[year]] == label)[0][0])

    last_free = next(t for t in range(T - 1, -1, -1) if t not in probe)
    out = [(1, "first year, Jan 2"), (last_free, "last step off the probe rows"),
           (int(feb29[0]), "Feb 29, first leap year"), (int(feb29[-1]), "Feb 29, last leap year"),
           (int(ends[leap[0]] - 1), "Dec 31 of a leap year (366)"),
           (day(ntracks - 1, 61), "Mar 1 of the last year")]
    # the warm-up rows of chunk k = 1 of n and its first rows, in a middle year
    D, n, k = 366, nchunks if nchunks > 0 else 3, 1
    for off in (-6, -1, 0, 5):
        out.append((day(ntracks // 2, D * k // n + off), f"middle year, doy D*{k}/{n}{off:+d}"))
    moved = []
    for t, label in out:
        if t in probe:
            t = t + 1 if t + 1 < T and t + 1 not in probe else t - 1
        assert 0 <= t < T and t not in probe, (t, label)
        moved.append((t, label))
    return moved


def cells(C, lanes):
    """first cell, last cell, and the first cell of the (ragged) last wave's neighbour: C - 1 - 64 // lanes"""
    return tuple(dict.fromkeys(c for c in (0, C - 1, C - 1 - 64 // lanes) if 0 <= c < C))


def ordinary_cells(C):
    """cells of series() that hold the seasonal samples"""
    return [c for c in range(C) if c not in SPECIAL_CELLS]


def q_of(kind):
    """the quantile a kind is run with: 1.0 selects the hidden sample itself"""
    return 1.0 if kind in ("top", "huge") else 0.9


def cases(route, kinds_everywhere=("top", "ulp"), kinds_twice=("huge", "tiny", "above_max")):
    """[(t, label, cell, kind)] of a route: every position x cell x kinds_everywhere, kinds_twice at two positions each"""
    time, doy = calendar(route)
    C = ncells(route)
    pos = positions(doy, route["years"])
    cs = cells(C, route["narrow"][2])
    assert not set(cs) & set(SPECIAL_CELLS)
    out = [(t, label, c, kind) for t, label in pos for c in cs for kind in kinds_everywhere]
    for i, kind in enumerate(kinds_twice):
        for j, (t, label) in enumerate((pos[1 + i], pos[-1 - i])):
            out.append((t, label, cs[(i + j) % len(cs)], kind))
    return out


def hidden_columns(x, route_cases, cold):
    """(T, n) array: column i is the affected cell of case i with its sample hidden; the values hidden"""
    cols = np.empty((x.shape[0], len(route_cases)))
    vals = np.empty(len(route_cases))
    for i, (t, _, c, kind) in enumerate(route_cases):
        cols[:, i] = x[:, c]
        cols[t, i] = vals[i] = checked_value(x, t, c, kind, cold)     # (= hide(x, t, c, kind, cold)[:, c])
    return cols, vals


def affected_rows(doy, t, w):
    """rows (0-based, of the D doy rows in ascending label order) whose pool holds time step t"""
    doy = np.asarray(doy)
    labels = np.unique(doy)
    lo, hi = max(t - w, 0), min(t + w, doy.shape[0] - 1)
    return np.searchsorted(labels, np.unique(doy[lo:hi + 1]))
