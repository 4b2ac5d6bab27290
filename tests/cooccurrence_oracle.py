"""The CPU oracle of mhw_cooccurrence().  TEST INFRASTRUCTURE ONLY.  Dense boolean (T, C) arrays filled from the tables row
by row, the lag applied by slicing, the counts boolean sums per class: no bit words and no segment lists, nothing shared
with the device code.

The definition.  Two event tables A and B lie on the same time axis of T steps.  For column c and step t, A[t][c] = 1 iff
some table row of that cell has start <= t <= end (gap days of joined events included, as detect() stores them).  B is
defined the same way.  For a lag l (any int32) the pair (t, l) is *valid* iff 0 <= t + l < T.  Then:
    Bl[t] = B[t + l] on valid pairs and 0 otherwise.
    J[t]  = A[t] & Bl[t], with J[-1] = 0.
class_of_t[T] holds int32 labels in [-1, K); -1 counts nowhere.  A pair belongs to the class of t, which is A's step.  For
every class k, lag index i and column c, summed over the valid pairs with class_of_t[t] == k: both = A[t] & Bl[t],
a_only = A[t] & ~Bl[t], b_only = ~A[t] & Bl[t], onsets = J[t] & ~J[t-1] (the first steps of joint runs; the onset test
looks at t - 1 whatever the class of t - 1 is).  neither = n_pairs[k][i] - both - a_only - b_only, n_pairs = the number of
valid pairs of class k.  A lag with |l| >= T gives zeros everywhere."""
import numpy as np


def dense(start, end, offsets, cells, T):
    """bool (T, C): column j is set on start..end of every row offsets[cells[j]] .. offsets[cells[j] + 1]"""
    out = np.zeros((T, len(cells)), dtype=bool)
    for j, c in enumerate(cells):
        for r in range(int(offsets[c]), int(offsets[c + 1])):
            out[int(start[r]):int(end[r]) + 1, j] = True
    return out


def reduce_dense(A, B, classes, K, lags):
    """counts int32 (K, L, 4, C) from two bool (T, C) arrays"""
    T, C = A.shape
    classes = np.asarray(classes)
    out = np.zeros((K, len(lags), 4, C), dtype=np.int32)
    for i, lag in enumerate(int(v) for v in lags):
        lo, hi = max(0, -lag), min(T, T - lag)
        if lo >= hi:
            continue
        valid = np.zeros(T, dtype=bool)
        valid[lo:hi] = True
        Bl = np.zeros((T, C), dtype=bool)
        Bl[lo:hi] = B[lo + lag:hi + lag]
        J = A & Bl
        Jprev = np.zeros((T, C), dtype=bool)
        Jprev[1:] = J[:-1]
        chans = (J, A & ~Bl & valid[:, None], ~A & Bl, J & ~Jprev)
        for k in range(K):
            sel = (classes == k) & valid
            for ch, x in enumerate(chans):
                out[k, i, ch] = x[sel].sum(axis=0)
    return out


def cooccur_tables(view_a, view_b, cells_a, cells_b, T, classes, K, lags):
    """The stand-in for xmhw_amd.cooccurrence.cooccur_tables (same arguments)."""
    A = dense(view_a["start"], view_a["end"], view_a["offsets"], cells_a, T)
    B = dense(view_b["start"], view_b["end"], view_b["offsets"], cells_b, T)
    return reduce_dense(A, B, classes, K, lags)


def n_pairs(classes, K, lags):
    classes = np.asarray(classes)
    T = classes.shape[0]
    out = np.zeros((K, len(lags)), dtype=np.int64)
    for i, lag in enumerate(int(v) for v in lags):
        for t in range(T):
            if 0 <= t + lag < T and classes[t] >= 0:
                out[classes[t], i] += 1
    return out


def pack_bits(X):
    """bool (T, C) -> uint64 (W, C): bit t % 64 of word t // 64, zero above T"""
    T, C = X.shape
    W = (T + 63) // 64
    out = np.zeros((W, C), dtype=np.uint64)
    for t in range(T):
        out[t // 64] |= X[t].astype(np.uint64) << np.uint64(t % 64)
    return out


def ratios(both, a_only, b_only, neither, n):
    """The derived fields element by element, in plain Python floats; NaN where a denominator is 0"""
    import math
    both, a_only, b_only, neither = (np.asarray(v) for v in (both, a_only, b_only, neither))
    n = np.broadcast_to(np.asarray(n), both.shape)
    names = ("p_a", "p_b", "p_both", "lmf", "hit_rate", "false_alarm_rate", "false_alarm_ratio", "csi", "sedi")
    out = {k: np.full(both.shape, np.nan) for k in names}
    div = lambda x, y: x / y if y else math.nan                          # noqa: E731
    for idx in np.ndindex(both.shape):
        a, b, c, d, m = (int(v[idx]) for v in (both, a_only, b_only, neither, n))
        H, F = div(a, a + b), div(c, c + d)
        out["p_a"][idx], out["p_b"][idx], out["p_both"][idx] = div(a + b, m), div(a + c, m), div(a, m)
        out["lmf"][idx] = div(a * m, (a + b) * (a + c))
        out["hit_rate"][idx], out["false_alarm_rate"][idx] = H, F
        out["false_alarm_ratio"][idx], out["csi"][idx] = div(c, a + c), div(a, a + b + c)
        if 0 < H < 1 and 0 < F < 1:
            lf, lh, l1f, l1h = math.log(F), math.log(H), math.log(1 - F), math.log(1 - H)
            out["sedi"][idx] = (lf - lh - l1f + l1h) / (lf + lh + l1f + l1h)
    return out
