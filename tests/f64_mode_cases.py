"""Cases for the 64-bit mode of the ring kernels (genuinely float64 input: selection on the high word of a 64-bit key,
ties settled on the low word), one pair of records per dispatchable instantiation.  TEST INFRASTRUCTURE ONLY.  No GPU:
tests/test_f64_mode_cases.py checks the cases and their inputs on the host, tests/f64_mode_child.py runs them through the
kernels, tests/test_gpu_f64_modes.py compares what it returns with the oracle.

The environment switches that move the float64 route are read once per process (route.cpp: route_defaults), so the cases
come in LEGS: the default environment runs in the test process, every other leg in a child process of its own.

Every instantiation a leg reaches, and no earlier leg reaches with the same padding, gets two records:
  least  whole years, the fewest tracks that dispatch to it (the last slot of a lane padded as much as can be);
         q = 0.9, heat waves, automatic chunks;
  most   the most tracks that dispatch to it, from 17 April of the first year to 3 October of the last (first and last
         track partial, the held Feb-29 step rotates both rings); q = 0.1, negate, three chunks.
The smallest record of a leg runs at q = 0.0, 0.5 and 1.0 as well, and one case per kernel family and leg runs as a slab
of a wider array (PITCH)."""
import numpy as np

import xmhw_oracle as ora

Y0 = 1901                       # first year of every record: leap years 1904, 1908, ... (1900 is none, 1901 + 95 = 1996)
W = 5                           # the only window the 64-bit mode is instantiated for
C = 37                          # cells: the last wave and the last workgroup are ragged at 4, 8 and 16 lanes per cell
EXTRA_Q = (0.0, 0.5, 1.0)
# a slab of a wider array: input rows C + 3 apart, the slab's first sample 5 doubles into the buffer (40 bytes: no
# 16-byte alignment); output rows C + 2 apart, pre-filled with 0xFF bytes
PITCH = dict(ld=C + 3, first=5, ldo=C + 2)

LEGS = (
    {},
    {"XMHW_RING3_F64": "0"},
    {"XMHW_RING3_F64_LANES": "8"},
    {"XMHW_RING3_F64": "0", "XMHW_RING2_F64_LDS": "0"},
)
# the leg's name in tools/record_routes.py (tests/golden/threshold_routes.npz); None: not recorded
RECORDED_AS = ("default", "XMHW_RING3_F64=0", "XMHW_RING3_F64_LANES=8", None)

# per leg: (expected instantiation = (family, layout, lanes, tracks per lane), least tracks or None, most tracks or None)
# -- None where an earlier leg runs the same instantiation at that track count (the same padding)
_REACH = (
    ((("ring2", 12, 16, 1), 1, 8), (("ring3", 20, 8, 2), 9, 12), (("ring3", 21, 4, 4), 13, 16), (("ring3", 21, 4, 5), 17, 20),
     (("ring3", 20, 8, 3), 21, 24), (("ring3", 20, 8, 4), 25, 32), (("ring3", 20, 8, 5), 33, 40), (("ring3", 20, 8, 6), 41, 48),
     (("ring2", 12, 16, 4), 49, 64), (("ring2", 12, 16, 5), 65, 80), (("ring2", 12, 16, 6), 81, 96)),
    ((("ring2", 8, 8, 2), 9, 16), (("ring2", 8, 8, 3), 17, 24), (("ring2", 8, 8, 4), 25, 32), (("ring2", 8, 8, 5), 33, 40),
     (("ring2", 8, 8, 6), 41, 48)),
    ((("ring3", 20, 8, 2), None, 16), (("ring3", 20, 8, 3), 17, None)),
    ((("ring2", 12, 16, 3), 33, 48),),
)
# (leg, tracks) of the cases that run pitched: one per kernel family and leg, on a "most" record where the leg has one
_PITCHED = {(0, 64), (0, 20), (1, 40), (2, 16), (3, 48)}


def _case(leg, no, tracks, kind, expect, q=None):
    least = kind == "least"
    c = dict(leg=leg, seed=1000 * leg + no, tracks=tracks, kind=kind, expect=expect, whole_years=least,
             q=(0.9 if least else 0.1) if q is None else q, negate=not least, nchunks=0 if least else 3,
             pitched=q is None and (leg, tracks) in _PITCHED)
    c["id"] = (f"leg{leg}-{expect[0]}_{expect[1]}_{expect[2]}_{expect[3]}-{tracks}tracks-{kind}-q{c['q']}"
               + ("-pitched" if c["pitched"] else ""))
    return c


def _leg_cases(leg):
    out = []
    for expect, least, most in _REACH[leg]:
        if least is not None:
            out.append(_case(leg, len(out), least, "least", expect))
        if most is not None:
            out.append(_case(leg, len(out), most, "most", expect))
    small = min(out, key=lambda c: c["tracks"])
    for q in EXTRA_Q:
        out.append(_case(leg, len(out), small["tracks"], small["kind"], small["expect"], q=q))
    return tuple(out)


CASES = tuple(_leg_cases(leg) for leg in range(len(LEGS)))


def calendar(case):
    """(time, doy) of a case's daily record"""
    y1 = Y0 + case["tracks"] - 1
    if case["whole_years"]:
        time = np.arange(f"{Y0}-01-01", f"{y1 + 1}-01-01", dtype="datetime64[D]")
    else:
        time = np.arange(f"{Y0}-04-17", f"{y1}-10-04", dtype="datetime64[D]")
    return time, ora.add_doy(time)


# ---- the samples ------------------------------------------------------------------------------------------------------

STEP = 0.5                      # distance of the levels
SPREAD = 2.0 ** -22             # a sample is its level times 1 + u * SPREAD, u in [0, 1): the high key word of the level
REPEAT = 2.0 ** -40             # the repeated double of a level: level * (1 + REPEAT) -- see clustered()
NEAR_FREEZING, ZEROS, ALL_NAN, INFS, HUGE, TINY = 3, 7, 11, 22, 29, 33
SPECIAL_CELLS = (NEAR_FREEZING, ZEROS, ALL_NAN, INFS, HUGE, TINY)
INF_RUN, MINUS_INF = (100, 140), (200, 250, 300)


def clustered(T, C, seed):
    """(T, C) float64 samples that defeat a selection on the high word of the key alone.

    A seasonal cycle around 10 plus noise, rounded to levels STEP apart; each sample is its level times 1 + u * SPREAD
    with u uniform in [0, 1): distinct doubles that share the high key word of their level (a level has at most 5
    mantissa bits, the factor moves it by less than 2^-21 of its leading bit).  15 % of the samples are exact repeats:
    the level's own double, which is the level times 1 + REPEAT and not the level itself -- a multiple of 0.5 is a
    float32, and no sample of a clustered cell may be one (a cell of float32s is the narrowing kernels' business,
    tests/narrowing_cases.py).  The upper half of the cells is negated (a negative double's key is the complement of its
    bits: its low words order the other way round).  Then the SPECIAL_CELLS, and 1 % NaN over everything."""
    assert T >= 365 and C > max(SPECIAL_CELLS)
    rng = np.random.default_rng(seed)
    t = np.arange(T)[:, None]
    base = 10.0 + rng.uniform(1.0, 2.0, C) * np.sin(2 * np.pi * (t - rng.uniform(0, 365, C)) / 365.25) \
        + 0.25 * rng.normal(size=(T, C))
    lev = np.round(base / STEP) * STEP
    x = lev * (1.0 + rng.random((T, C)) * SPREAD)
    rep = rng.random((T, C)) < 0.15
    x[rep] = lev[rep] * (1.0 + REPEAT)
    x[:, C // 2 + 1:] *= -1.0
    # sea ice: centred on -1.8, levels 2^-20 apart (neighbouring high words at that magnitude)
    k = np.round(rng.normal(size=T) * 2.0)
    x[:, NEAR_FREEZING] = (-1.8 + k * 2.0 ** -20) * (1.0 + rng.random(T) * SPREAD)
    # k * 1e-9, k = -2 .. 2: both signs, both zeros, many repeats
    k = rng.integers(-2, 3, T)
    x[:, ZEROS] = np.where(k == 0, np.where(rng.random(T) < 0.5, 0.0, -0.0), k * 1e-9)
    x[:, ALL_NAN] = np.nan
    x[INF_RUN[0]:INF_RUN[1], INFS] = np.inf
    x[list(MINUS_INF), INFS] = -np.inf
    x[:, HUGE] *= 1e300                                      # outside float32's range at both ends
    x[:, TINY] *= 1e-310                                     # (subnormal doubles)
    x[rng.random((T, C)) < 0.01] = np.nan
    return x


def clustered_cells(C):
    return [c for c in range(C) if c not in SPECIAL_CELLS]


def samples(case):
    """(doy, x) of a case"""
    time, doy = calendar(case)
    return doy, clustered(time.shape[0], C, case["seed"])


def representable(x):
    """per sample: float32 holds it"""
    with np.errstate(over="ignore", invalid="ignore"):
        return x.astype(np.float32).astype(np.float64) == x


def keys(x):
    """the 64-bit key of a double as the kernels order it: its bits, complemented if negative, sign bit set otherwise"""
    b = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    neg = (b >> np.uint64(63)).astype(bool)
    return np.where(neg, ~b, b | np.uint64(1 << 63))


def hazard_share(case, cells, x=None, doy=None):
    """the share of (doy, cell) rows, over `cells`, whose two bracketing order statistics share the high 32 bits of their
    key and are different doubles: a selection that ignored the low words could not tell them apart.

    The bracket is at position q (n - 1) of the sorted pool of the n samples that are no NaN (of the negated samples for
    negate=True): the order statistics floor(q (n - 1)) and the next.  Where that position is the last one (q = 1) the
    bracket is the last two: the maximum is selected rightly only if it is told from the runner-up.  A row with fewer
    than two samples counts as no hazard."""
    import oracle_fast as fast
    if x is None:
        doy, x = samples(case)
    xs = -x[:, cells] if case["negate"] else x[:, cells]
    doys, pools = fast.pool_index(doy, W)
    cols = np.arange(xs.shape[1])
    hits = 0
    for idx in pools:
        p = np.sort(xs[idx, :], axis=0)                      # NaN sorts last
        n = np.sum(~np.isnan(p), axis=0)
        ok = n >= 2
        nn = np.where(ok, n, 2)
        lo = np.minimum(np.floor((nn - 1) * case["q"]).astype(np.int64), nn - 2)
        a, b = p[lo, cols], p[lo + 1, cols]
        same_high = (keys(a) >> np.uint64(32)) == (keys(b) >> np.uint64(32))
        hits += int(np.sum(ok & same_high & (a != b)))
    return hits / (len(pools) * xs.shape[1])
