"""The cases of the coarsen() tests: the grids, factors, coarse grids, windows and data the GPU tests run on, generated
from seeds so that the oracle's result is computed once per case.  No combination is dropped silently: the only ones that
are dropped are a factor larger than the grid under a floor coarse grid (no cell is left), and listed() asserts that they
are at most a quarter of the combinations listed (checked on the CPU as well: tests/test_host_coarsen.py)."""
from collections import namedtuple

import numpy as np

GRIDS = ((1, 1), (5, 7), (8, 130), (13, 257), (3, 4161))         # 4,161 / fx crosses a wave and a workgroup
FACTORS = ((1, 1), (2, 2), (3, 2), (2, 3), (4, 4), (5, 8), (8, 1), (1, 64))
BOUNDARIES = ("floor", "ceil")
DTYPES = (np.float32, np.float64)
WINDOWS = ("1", "2", "5", "31", "gaps")
SHARES = (0, 32768, 65536, 12345)                                # a: the least covered share, in 65536ths
T_STEPS = 70

Case = namedtuple("Case", "ny nx fy fx ncy ncx dtype window a seed")


def cells(n, f, boundary):
    return -(-n // f) if boundary == "ceil" else n // f


def listed():
    """every (grid, factors, boundary, dtype) of the lists above with a coarse grid that has cells; the window kind and
    the share cycle through theirs"""
    out, dropped, total = [], 0, 0
    for g, (ny, nx) in enumerate(GRIDS):
        for f, (fy, fx) in enumerate(FACTORS):
            for b, boundary in enumerate(BOUNDARIES):
                for d, dtype in enumerate(DTYPES):
                    total += 1
                    ncy, ncx = cells(ny, fy, boundary), cells(nx, fx, boundary)
                    if ncy == 0 or ncx == 0:
                        assert boundary == "floor" and (fy > ny or fx > nx)
                        dropped += 1
                        continue
                    k = len(out)
                    out.append(Case(ny, nx, fy, fx, ncy, ncx, dtype, WINDOWS[(g + f + b) % len(WINDOWS)],
                                    SHARES[(f + b + d) % len(SHARES)], 1000 + k))
    assert total == len(GRIDS) * len(FACTORS) * len(BOUNDARIES) * len(DTYPES)
    assert 4 * dropped <= total, (dropped, total)
    return out


def case_id(c):
    return f"{c.ny}x{c.nx}-f{c.fy}x{c.fx}-c{c.ncy}x{c.ncx}-{np.dtype(c.dtype).name}-w{c.window}-a{c.a}"


def windows(kind, T):
    """(S + 1,) int32 boundaries as the C entries take them: consecutive windows of 1, 2, 5 or 31 steps from step 0 (a
    partial last one is dropped), or unequal explicit windows that leave the first step and the last ones uncovered"""
    if kind == "gaps":
        return np.array([b for b in (1, 2, 9, 10, 15, 33, 38, 39, 64, 69) if b <= T], dtype=np.int32)
    n = int(kind)
    return np.arange(0, T - T % n + 1, n, dtype=np.int32)


def gap_pairs(T):
    """(S, 2) int32 [start, stop) pairs as the device stage takes them: unequal windows with uncovered steps BETWEEN them
    (every second window of the "gaps" table; the stage issues one C call per run of adjacent windows)"""
    w = windows("gaps", T)
    return np.array([(w[i], w[i + 1]) for i in range(0, len(w) - 1, 2)], dtype=np.int32)


def make_data(c, T=T_STEPS, x0=0.0, nan_frac=0.05):
    """(field (T, ld) with ld = ny * nx + 3 and NaN padding columns, wi int32 (ny * nx,)): samples around x0 inside the
    range, 5 % scattered NaN, a land blob (all NaN, among it whole blocks), weights up to 2^24 with zeros among them"""
    rng = np.random.default_rng(c.seed)
    N = c.ny * c.nx
    ld = N + 3
    x = (x0 + rng.normal(0.0, 8.0, (T, N))).astype(c.dtype)
    x[rng.random((T, N)) < nan_frac] = np.nan
    jj, ii = np.divmod(np.arange(N), c.nx)
    land = (jj < 2 * c.fy) & (ii >= c.fx) & (ii < 3 * c.fx) if N > 1 else np.zeros(N, dtype=bool)
    land |= rng.random(N) < 0.03
    x[:, land] = np.nan
    field = np.full((T, ld), np.nan, dtype=c.dtype)
    field[:, :N] = x
    wi = rng.integers(0, (1 << 24) + 1, N).astype(np.int32)
    wi[rng.random(N) < 0.1] = 0
    wi[rng.random(N) < 0.05] = 1 << 24
    return field, wi
