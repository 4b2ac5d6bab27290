"""The case generators and class patterns shared by the host and the GPU tests of index_regression().  TEST
INFRASTRUCTURE ONLY."""
import numpy as np

ZLIM = 1 << 23
EDGES = (64, 65)                # the forced block lengths whose edges the series and the labels straddle


def predictors(T, J, seed):
    """zq (T, J) int32: autocorrelated columns of a few units in fixed point, with the extreme values +-(2**23 - 1) and
    zeros sprinkled in"""
    rng = np.random.default_rng(seed)
    z = np.cumsum(rng.normal(0, 0.3, (T, J)), axis=0)
    z -= z.mean(axis=0)
    zq = np.clip(np.rint(z * 65536.0), -ZLIM + 1, ZLIM - 1).astype(np.int32)
    zq[rng.random((T, J)) < 0.02] = ZLIM - 1
    zq[rng.random((T, J)) < 0.02] = -ZLIM + 1
    zq[rng.random((T, J)) < 0.05] = 0
    return zq


def synthetic(T, C, dtype, seed, D=1, zq=None):
    """A (T, C) series around a (D, C) base with what the lag-1 pairs and the deficits have to get right: NaN at step
    0, on both sides of every multiple of the block lengths of EDGES (t0 - 1 and t0), in pairs and in runs, scattered
    NaN, a cell that is all NaN (cell 2) and one without a base (cell 3).  The anomalies follow the first predictor
    column a little, so that no sum is trivially small.  Returns ts, base, rows (T,), doy, doys."""
    rng = np.random.default_rng(seed)
    base = np.round(18.0 + 6.0 * rng.random((D, C)), 2)
    doys = np.arange(1, D + 1) if D > 1 else np.zeros(1, dtype=np.int64)
    rows = ((np.arange(T) + 37) % D).astype(np.int32)
    a = np.cumsum(rng.normal(0, 0.4, (T, C)), axis=0)
    a -= a.mean(axis=0)
    if zq is not None:
        a += 0.5 * (zq[:, :1] / 65536.0) * rng.random(C)
    ts = (base[rows] + np.clip(a, -100.0, 100.0)).astype(dtype)
    ts[0, rng.random(C) < 0.5] = np.nan
    for m in EDGES:
        for s in range(m, T, m):
            kind = rng.integers(0, 5, C)                     # nothing, t0 - 1, t0, the pair, a run across the edge
            ts[s - 1, (kind == 1) | (kind == 3)] = np.nan
            ts[s, (kind == 2) | (kind == 3)] = np.nan
            ts[max(0, s - 3):s + 3, kind == 4] = np.nan
    ts[rng.random((T, C)) < 0.02] = np.nan
    if C > 2:
        ts[:, 2] = np.nan
    if C > 3:
        base[:, 3] = np.nan
    return {"ts": ts, "base": base, "rows": rows, "doy": doys[rows], "doys": doys}


def one_class(T):
    return np.zeros(T, dtype=np.int32), 1


def runs(T):
    """classes in runs whose changes fall on and beside the block edges: ..., 63 | 64, 64 | 65, 127 | 128, ..."""
    t = np.arange(T)
    return (((t >= 63).astype(int) + (t >= 64) + (t >= 65) + (t >= 128) + (t >= 129) + t // 100) % 5).astype(np.int32), 5


def every_step(T):
    """Labels that change every step, some -1: the flush-per-step worst case (K = 7)."""
    return np.random.default_rng(11).integers(-1, 7, T).astype(np.int32), 7


def runs_of_minus_one(T):
    """two classes with runs of -1 that start and end on and beside the block edges"""
    t = np.arange(T)
    k = ((t // 13) % 2).astype(np.int32)
    for s in range(64, T, 64):
        k[s - 2:s] = -1                                      # ends at t0 - 1
    for s in range(65, T, 65):
        k[s:s + 3] = -1                                      # starts at t0
    k[(t // 29) % 4 == 3] = -1
    return k, 2


PATTERNS = (one_class, runs, every_step, runs_of_minus_one)


def check_case(want):
    """On the oracle's side: a case without lag-1 pairs, without deficits or without valid steps proves nothing."""
    assert want["n"].sum() > 0 and 0 < want["n1"].sum() < want["n"].sum()
    assert (want["mz"] != 0).any() and (want["mzz"] > 0).any() and (want["saz"] != 0).any() and (want["saa1"] != 0).any()
