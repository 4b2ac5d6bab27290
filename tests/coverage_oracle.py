"""CPU oracle of mhw_coverage()'s device stage.  TEST INFRASTRUCTURE ONLY.  Dumb and slow on purpose.

The definition, cell by cell, with the functions of oracle/ that are pinned to the reference: detect_front()
decides which steps are in an event, intermediate_columns() gives their per-step category; then plain loops and
Python integers (no overflow, no summation order to argue about).  Same signature as xmhw_amd.coverage.coverage_cells.
"""
import numpy as np

import detect_oracle as det
import features_oracle as fo

STATES = ("duration_moderate", "duration_strong", "duration_severe", "duration_extreme")


def rows_of(doy, doys):
    doys = np.asarray(doys)
    order = np.argsort(doys, kind="stable")
    return order[np.searchsorted(doys, np.asarray(doy), sorter=order)]


def cell_states(x, seas_doy, thresh_doy, rows, minDuration=5, joinGaps=True, maxGap=2, coldSpells=False):
    """(T, 5) bool for one cell: moderate, strong, severe, extreme, event."""
    x = np.asarray(x, dtype=np.float64)
    _, _, _, events = det.detect_front(x, thresh_doy, rows, minDuration, joinGaps, maxGap, coldSpells)
    xs = -1.0 * x if coldSpells else x
    ic = fo.intermediate_columns(xs, np.asarray(seas_doy, dtype=np.float64)[rows],
                                 np.asarray(thresh_doy, dtype=np.float64)[rows], events)
    out = np.zeros((x.shape[0], 5), dtype=bool)
    for k, name in enumerate(STATES):
        out[:, k] = ic[name]
    out[:, 4] = ~np.isnan(events)
    return out


def coverage_cells(ts, seas, thresh, doy, doys, wq, region, R, minDuration=5, joinGaps=True, maxGap=2, coldSpells=False,
                   pad=None):
    if pad is not None:
        raise NotImplementedError("the oracle takes an already interpolated series")
    ts = np.asarray(ts)
    T, C = ts.shape
    rows = rows_of(doy, doys)
    cells = [[[0] * 5 for _ in range(R)] for _ in range(T)]
    area = [[[0] * 5 for _ in range(R)] for _ in range(T)]
    for c in range(C):
        r = int(region[c])
        if r < 0:
            continue
        w = int(wq[c])
        st = cell_states(ts[:, c], seas[:, c], thresh[:, c], rows, minDuration, joinGaps, maxGap, coldSpells)
        for t, k in zip(*np.nonzero(st)):
            cells[t][r][k] += 1
            area[t][r][k] += w
    return np.array(cells, dtype=np.int64).reshape(T, R, 5), np.array(area, dtype=np.int64).reshape(T, R, 5)


def coverage_fast(ts, seas, thresh, doy, doys, wq, region, R, minDuration=5, joinGaps=True, maxGap=2, coldSpells=False):
    """The same numbers with the per-cell states summed by numpy (np.add.at on int64): for the large cases,
    where Python-integer loops over every in-event day would take minutes.  Checked against coverage_cells()
    in the host tests."""
    ts = np.asarray(ts)
    T, C = ts.shape
    rows = rows_of(doy, doys)
    cells = np.zeros((T, R, 5), dtype=np.int64)
    area = np.zeros((T, R, 5), dtype=np.int64)
    for c in range(C):
        r = int(region[c])
        if r < 0:
            continue
        st = cell_states(ts[:, c], seas[:, c], thresh[:, c], rows, minDuration, joinGaps, maxGap, coldSpells)
        cells[:, r, :] += st
        area[:, r, :] += st.astype(np.int64) * np.int64(wq[c])
    return cells, area
