"""Generators of the synthetic mhw_coverage() cases shared by the host tests (which check on the CPU oracle that
every case contains events) and the GPU tests.  TEST INFRASTRUCTURE ONLY."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def golden_series():
    """The 108 reference series of mhw_features_cases.npz: (ts, seas, thresh, (minDuration, joinGaps, maxGap),
    golden table rows) per case; seas / thresh are already expanded along time."""
    g = np.load(os.path.join(GOLDEN, "mhw_features_cases.npz"))
    cols = list(g["columns"])
    offs, toffs = g["offsets"], g["table_offsets"]
    for i, (m, jg, gap) in enumerate(g["params"]):
        sl = slice(offs[i], offs[i + 1])
        yield (g["ts"][sl], g["seas"][sl], g["thresh"][sl], (int(m), bool(jg), int(gap)),
               g["table"][toffs[i]:toffs[i + 1]], cols)


def synthetic(T, C, dtype=np.float32, seed=0, D=37, nan_frac=0.0, cold=False):
    """A (T, C) series with a doy cycle of D labels, red noise around the seasonal cycle and thresholds low enough
    that every cell has events of all categories.  Returns dict(ts, seas, thresh, doy, doys)."""
    rng = np.random.default_rng(seed)
    doys = np.arange(1, D + 1)
    doy = doys[np.arange(T) % D]
    seas = 15.0 + 3.0 * np.sin(2 * np.pi * np.arange(D) / D)[:, None] + rng.normal(scale=0.2, size=(D, C))
    thresh = seas + rng.uniform(0.3, 0.8, size=(D, C))
    e = rng.normal(size=(T, C))
    x = np.empty((T, C))
    x[0] = e[0]
    for t in range(1, T):
        x[t] = 0.85 * x[t - 1] + e[t]
    ts = seas[np.arange(T) % D] + x
    if cold:                                   # cold spells: the climatologies are those of the negated series
        ts = -ts
    ts = ts.astype(dtype)
    if nan_frac:
        ts[rng.random((T, C)) < nan_frac] = np.nan
    return dict(ts=ts, seas=seas, thresh=thresh, doy=doy, doys=doys)


def scattered_regions(C, R, seed=1, excluded=0.1):
    """Region ids scattered per cell, every id in [0, R) present when C >= R, ~`excluded` of the cells -1."""
    rng = np.random.default_rng(seed)
    r = rng.integers(0, R, size=C).astype(np.int32)
    r[:min(C, R)] = np.arange(min(C, R)) if C >= R else r[:C]
    r[rng.random(C) < excluded] = -1
    if C >= R:                                 # the exclusion must not remove an id
        r[:R] = np.arange(R)
    return r


def wave_regions(C, R):
    """One region per 64 consecutive cells."""
    return ((np.arange(C) // 64) % R).astype(np.int32)


def weights_q(C, seed=2):
    """Quantised weights in [0, 2**31] with both ends present."""
    rng = np.random.default_rng(seed)
    wq = rng.integers(0, (1 << 31) + 1, size=C, dtype=np.int64)
    wq[rng.random(C) < 0.05] = 0
    wq[rng.random(C) < 0.05] = 1 << 31
    wq[0] = 1 << 31
    if C > 1:
        wq[-1] = 0
    return wq
