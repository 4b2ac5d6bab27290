"""CPU oracle of mhw_days_by()'s device stage.  TEST INFRASTRUCTURE ONLY.  Dumb and slow on purpose.

Cell by cell: coverage_oracle.cell_states() (pinned to oracle/) gives the five states of every step; the anomaly
a = x - seas[row(t)] is taken in numpy float64; then ONE Python loop over the in-event steps with plain comparisons,
Python integers (``int(np.rint(a * 65536))``: no overflow, no summation order to argue about) and math.fsum for the
unquantised mean.  class_days_cells() has the signature of xmhw_amd.days_by.class_days_cells.
"""
import math

import numpy as np

import coverage_oracle as co


def states_and_anomalies(ts, seas, thresh, doy, doys, minDuration=5, joinGaps=True, maxGap=2, coldSpells=False):
    """(st (T, C, 5) bool, a (T, C) float64): the part that does not depend on the classes; compute it once per case."""
    ts = np.asarray(ts)
    T, C = ts.shape
    rows = co.rows_of(doy, doys)
    st = np.zeros((T, C, 5), dtype=bool)
    for c in range(C):
        st[:, c] = co.cell_states(ts[:, c], seas[:, c], thresh[:, c], rows, minDuration, joinGaps, maxGap, coldSpells)
    x = ts.astype(np.float64)
    if coldSpells:
        x = -1.0 * x
    a = x - np.asarray(seas, dtype=np.float64)[rows]
    return st, a


def reduce_by_class(st, a, classes, K):
    """dict(days int32 (K, 6, C), isum_q int64 (K, C), intensity_max float64 (K, C), n_range int, mean_exact float64
    (K, C): math.fsum of the valid a / their number, NaN where there is none)."""
    T, C = a.shape
    days = [[[0] * C for _ in range(6)] for _ in range(K)]
    isum = [[0] * C for _ in range(K)]
    imax = [[math.nan] * C for _ in range(K)]
    vals = [[[] for _ in range(C)] for _ in range(K)]
    n_range = 0
    for c in range(C):
        for t in np.nonzero(st[:, c, 4])[0]:
            k = int(classes[t])
            if k < 0:
                continue
            assert k < K
            for j in range(4):
                if st[t, c, j]:
                    days[k][j][c] += 1
            days[k][4][c] += 1
            v = float(a[t, c])
            if v != v:
                continue
            if not abs(v) < 128.0:
                n_range += 1
                continue
            days[k][5][c] += 1
            isum[k][c] += int(np.rint(a[t, c] * 65536.0))
            v = v + 0.0                                          # -0.0 counts as 0.0
            if imax[k][c] != imax[k][c] or v > imax[k][c]:
                imax[k][c] = v
            vals[k][c].append(float(a[t, c]))
    mean = [[math.fsum(vals[k][c]) / len(vals[k][c]) if vals[k][c] else math.nan for c in range(C)] for k in range(K)]
    return dict(days=np.array(days, dtype=np.int32).reshape(K, 6, C), isum_q=np.array(isum, dtype=np.int64).reshape(K, C),
                intensity_max=np.array(imax, dtype=np.float64).reshape(K, C), n_range=n_range,
                mean_exact=np.array(mean, dtype=np.float64).reshape(K, C))


def class_days_full(ts, seas, thresh, doy, doys, classes, K, minDuration=5, joinGaps=True, maxGap=2, coldSpells=False):
    st, a = states_and_anomalies(ts, seas, thresh, doy, doys, minDuration, joinGaps, maxGap, coldSpells)
    return reduce_by_class(st, a, np.asarray(classes), int(K))


def class_days_cells(ts, seas, thresh, doy, doys, classes, K, minDuration=5, joinGaps=True, maxGap=2, coldSpells=False,
                     pad=None, counters=None):
    if pad is not None:
        raise NotImplementedError("the oracle takes an already interpolated series")
    r = class_days_full(ts, seas, thresh, doy, doys, classes, K, minDuration, joinGaps, maxGap, coldSpells)
    if counters is not None:
        counters["n_range"] = r["n_range"]
    return r["days"], r["isum_q"], r["intensity_max"]
