"""The case generators shared by the host and the GPU tests of spatial_correlation(): a spatially smooth field around its
base on an uncompacted ny x nx grid with the land that can go wrong made by construction, class patterns and offset lists.
TEST INFRASTRUCTURE ONLY."""
import numpy as np

LANDS = ("none", "island", "lines", "all")


def field(T, ny, nx, dtype, seed, Dr=1, land="none", scatter=0.05, spoil=True):
    """ts (T, ny * nx) around base (Dr, ny * nx): anomalies of a few units that are smooth in space (a sum of a field
    shared by neighbouring points and noise, so that products of neighbours do not cancel), exact zeros among them,
    ``scatter`` scattered NaN, and land as NaN in every step (the base is NaN there as well):
      island   the block of rows ny // 3 .. and columns nx // 3 .. (a third of each axis, one point at least)
      lines    the whole of row ny // 2 and the whole of column 0: a land column on the seam of a periodic grid
      all      every point
    With ``spoil`` and room for them: out-of-range and infinite samples at points (0, 0), (ny - 1, nx - 1) and the middle,
    a sample exactly 2**7 above its base (out of range) and one a unit of the fixed point inside.  With Dr > 1 row_of_t is
    not monotone.  Returns ts, base, rows, sea (ny * nx,) bool."""
    rng = np.random.default_rng(seed)
    N = ny * nx
    base = np.round(15.0 + 8.0 * rng.random((Dr, N)), 2)
    rows = ((np.arange(T) * 3 + 2) % Dr).astype(np.int32)
    common = rng.normal(0, 1.0, (T, ny + 2, nx + 2))
    smooth = sum(common[:, a:a + ny, b:b + nx] for a in range(3) for b in range(3)) / 3.0
    a = np.round(smooth + 0.5 * rng.normal(0, 1.0, (T, ny, nx)) + 0.4, 3).reshape(T, N)
    a[rng.random((T, N)) < 0.03] = 0.0
    ts = base[rows] + a
    ts[rng.random((T, N)) < scatter] = np.nan
    if spoil and N >= 3 and T >= 3:
        mid = (ny // 2) * nx + min(nx - 1, nx // 2 + 1)
        ts[0, 0], ts[T - 1, N - 1], ts[T // 2, mid] = 900.0, -np.inf, np.inf
        ts[1, N - 1] = base[rows[1], N - 1] - 700.0
        if N >= 5:
            base[:, 2], base[:, 3] = 20.0, 20.0
            ts[2, 2] = 148.0                                            # exactly 2**7 from the base: out of range
            ts[2, 3] = 20.0 + 128.0 - 2.0 ** -16                        # inside by one unit (float64 alone holds it)
    sea = np.ones((ny, nx), dtype=bool)
    if land == "island":
        sea[ny // 3:ny // 3 + max(ny // 3, 1), nx // 3:nx // 3 + max(nx // 3, 1)] = False
    elif land == "lines":
        sea[ny // 2, :] = False
        sea[:, 0] = False
    elif land == "all":
        sea[:] = False
    sea = sea.reshape(N)
    ts[:, ~sea] = np.nan
    base[:, ~sea] = np.nan
    return ts.astype(dtype), base, rows, sea


def one_class(T):
    return np.zeros(T, dtype=np.int32), 1


def every_step(T):
    """a label that changes every step, K = 3"""
    return (np.arange(T) % 3).astype(np.int32), 3


def with_minus_one(T):
    """two classes in runs of 5 steps with every third run unlabelled; the first and the last step are unlabelled too"""
    t = np.arange(T)
    k = ((t // 5) % 2).astype(np.int32)
    k[(t // 5) % 3 == 2] = -1
    k[[0, T - 1]] = -1
    if T > 2:
        k[1] = 1
    return k, 2


def sixty_four(T):
    """K = 64: the label is the step mod 64"""
    return (np.arange(T) % 64).astype(np.int32), 64


PATTERNS = (one_class, every_step, with_minus_one, sixty_four)


def offsets(D):
    """D offsets of both signs: (0, 0) first, the cap (+-32, +-32) and a duplicate as soon as D allows, near neighbours
    and single-axis offsets in between; D = 1, 8, 9, 17 and 64 cross the boundaries of the offset groups (one group of 8
    up to 8 offsets, groups of 16 beyond)"""
    pool = [(0, 0), (0, 1), (1, 0), (0, -1), (-1, 0), (1, 1), (-1, -1), (0, 1),                  # [7]: a duplicate of [1]
            (32, 32), (-32, -32), (32, -32), (-32, 32), (0, 32), (0, -32), (32, 0), (-32, 0), (2, -3)]
    rng = np.random.default_rng(64)
    while len(pool) < 64:
        pool.append((int(rng.integers(-9, 10)), int(rng.integers(-40, 41)) * 32 // 40))
    assert 1 <= D <= 64
    return np.array(pool[:D], dtype=np.int32)
