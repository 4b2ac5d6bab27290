"""The cases of the regrid() tests at the raw-table level: destination widths and heights, table kinds, periodic or not,
sample types and shares, with tables and data generated from seeds so that the oracle's result is computed once per
case.  No case is dropped: listed() asserts that it returns the full product.

    mx        1, 7, 130, 257, 1100: one lane, a partial wave, crossing a wave, crossing a workgroup, several tiles
    my        1, 3
    kinds     refine   many destinations share one source column (consecutive col_first equal), runs of 1 and 2
              coarsen  col_first strides 2 .. 8, runs of the stride or one more
              shift    2 x 2 footprints that overlap their neighbours by one
              random   monotone col_first in steps of 0 .. 3, run lengths drawn from RUNS (0 and 64 among them)
    periodic  the same tables on a source grid that ends where the last run starts, rotated by a random shift: runs
              cross the seam inside a tile; the random kind of a narrow destination holds a run of length nx
    rows      run lengths walk through RUNS from case to case and row to row
    weights   0 .. 4096 with 0 and 4096 frequent; the extent of a run is the sum of its weights plus 0 .. 5
    data      T = 23 steps, ld = ny * nx + 3 with NaN padding, 5 % scattered NaN and a land blob over whole footprints
The source grid is sized from the tables."""
import itertools
from collections import namedtuple

import numpy as np

WIDTHS = (1, 7, 130, 257, 1100)
HEIGHTS = (1, 3)
KINDS = ("refine", "coarsen", "shift", "random")
PERIODIC = (0, 1)
DTYPES = (np.float32, np.float64)
SHARES = (0, 32768, 65536, 12345)                                # a: the least covered share, in 65536ths
RUNS = (0, 1, 2, 3, 4, 5, 8, 17, 64)
T_STEPS = 23
MAX_WEIGHT = 4096
MAX_EXTENT = 1 << 18

Case = namedtuple("Case", "mx my kind periodic dtype a seed")


def listed():
    out = [Case(mx, my, kind, per, dtype, SHARES[k % len(SHARES)], 3000 + k)
           for k, (mx, my, kind, per, dtype) in enumerate(itertools.product(WIDTHS, HEIGHTS, KINDS, PERIODIC, DTYPES))]
    assert len(out) == len(WIDTHS) * len(HEIGHTS) * len(KINDS) * len(PERIODIC) * len(DTYPES)
    return out


def case_id(c):
    return f"{c.my}x{c.mx}-{c.kind}-{'periodic' if c.periodic else 'plane'}-{np.dtype(c.dtype).name}-a{c.a}"


def invariance_subset(cases=None):
    """one case per (mx, kind, periodic), heights and sample types alternating: every kind, both types, both periodic
    settings and every mx are among them"""
    cases = listed() if cases is None else cases
    out = []
    for g, (mx, kind, per) in enumerate(itertools.product(WIDTHS, KINDS, PERIODIC)):
        out.append(next(c for c in cases if (c.mx, c.kind, c.periodic) == (mx, kind, per) and
                        c.my == HEIGHTS[(g // 2) % 2] and c.dtype is DTYPES[(g // 3) % 2]))
    assert {c.dtype for c in out} == set(DTYPES) and {c.my for c in out} == set(HEIGHTS)
    return out


def weights_for(rng, count):
    """(weights int32 (sum count,), ptr, full): 0 .. 4096 with zeros and 4096 among them; full = sum + 0 .. 5"""
    ptr = np.concatenate([[0], np.cumsum(count)]).astype(np.int32)
    w = rng.integers(0, MAX_WEIGHT + 1, int(ptr[-1])).astype(np.int32)
    pick = rng.random(w.shape[0])
    w[pick < 0.1] = 0
    w[pick > 0.9] = MAX_WEIGHT
    sums = np.array([int(w[ptr[k]:ptr[k + 1]].sum()) for k in range(len(count))], dtype=np.int64)
    full = np.minimum(sums + rng.integers(0, 6, len(count)), MAX_EXTENT).astype(np.int32)
    return w, ptr, full


def column_runs(c, rng):
    """(first, count, nx) of the column table"""
    mx, I = c.mx, np.arange(c.mx)
    if c.kind == "refine":
        f = int(rng.integers(2, 5))
        first, count = I // f, np.where(I % f == f - 1, 2, 1)
    elif c.kind == "coarsen":
        s = int(rng.integers(2, 9))
        first, count = I * s, np.full(mx, s + int(rng.integers(0, 2)))
    elif c.kind == "shift":
        first, count = I.copy(), np.full(mx, 2)
    else:
        count = rng.choice(RUNS, mx, p=(0.05, 0.2, 0.2, 0.15, 0.15, 0.1, 0.1, 0.03, 0.02))
        count[int(rng.integers(0, mx))] = 64                     # the longest run is in every random case ...
        if mx >= 7:
            count[(int(np.argmax(count == 64)) + 3) % mx] = 0    # ... and an empty one where there is room
        first = np.cumsum(rng.integers(0, 4, mx))
    count = np.asarray(count, dtype=np.int64)
    first = np.asarray(first, dtype=np.int64)
    if not c.periodic:
        return first.astype(np.int32), count, int((first + count).max()) + 1
    # the grid ends where the last run starts (and holds the longest run): the last runs cross the seam; then rotate
    nx = max(int(first.max()) + 1, int(count.max()), 1)
    first = (first + int(rng.integers(0, nx))) % nx
    return first.astype(np.int32), count, nx


def row_runs(c, rng):
    k = c.seed
    count = np.array([RUNS[(k + 2 * J) % len(RUNS)] for J in range(c.my)], dtype=np.int64)
    first = np.concatenate([[0], np.cumsum(np.maximum(count // 2, 1))[:-1]]).astype(np.int64)
    if c.seed % 3 == 0:                                          # latitude descending: the rows in reverse order
        first, count = first[::-1].copy(), count[::-1].copy()
    return first.astype(np.int32), count, int((first + count).max()) + 1


def tables(c):
    """(ny, nx, rows, cols) with rows = (row_first, row_ptr, ay, wy) and cols likewise, int32"""
    rng = np.random.default_rng(c.seed)
    cf, cc, nx = column_runs(c, rng)
    rf, rc, ny = row_runs(c, rng)
    ax, cp, wx = weights_for(rng, cc)
    ay, rp, wy = weights_for(rng, rc)
    return ny, nx, (rf, rp, ay, wy), (cf, cp, ax, wx)


def make_data(c, T=T_STEPS, x0=0.0, nan_frac=0.05):
    """field (T, ld) with ld = ny * nx + 3 and NaN padding columns: samples around x0 inside the range, 5 % scattered
    NaN, a land blob (all rows of the source columns under two neighbouring destination cells, whole footprints)"""
    ny, nx, rows, cols = tables(c)
    rng = np.random.default_rng(c.seed + 77)
    x = (x0 + rng.normal(0.0, 8.0, (T, ny, nx))).astype(c.dtype)
    x[rng.random((T, ny, nx)) < nan_frac] = np.nan
    cf, cp = cols[0], cols[1]
    for I in range(c.mx // 3, min(c.mx // 3 + 2, c.mx)):
        land = (cf[I] + np.arange(cp[I + 1] - cp[I])) % nx
        x[:, :, land] = np.nan
    field = np.full((T, ny * nx + 3), np.nan, dtype=c.dtype)
    field[:, :ny * nx] = x.reshape(T, -1)
    return field
