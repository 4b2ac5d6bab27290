"""Hand-drawn inputs shared by the host and the GPU tests of mhw_track_parts(), each with its expected counts, and the
larger synthetic grids of the GPU tests.  Every case is (ds, kwargs of mhw_objects, neighbours, expected) with
``expected`` = the n_parts series of object 0 (every case but the random ones holds one object)."""
import numpy as np

import objects_cases as oc


def grid(ny, nx, cells, T, keep=None):
    """cells: {(i, j): [(start, end), ...]}; every grid point is ocean unless ``keep`` says otherwise"""
    keep = np.ones((ny, nx), bool) if keep is None else np.asarray(keep, dtype=bool).reshape(ny, nx)
    per_cell = [cells.get((i, j), []) for i in range(ny) for j in range(nx) if keep[i, j]]
    return oc.dataset((ny, nx), keep, per_cell, T=T)


def ring():
    """a 3 x 3 ring around a hole, 4 days: one part of 8 cells"""
    cells = {(i, j): [(1, 4)] for i in (1, 2, 3) for j in (1, 2, 3) if (i, j) != (2, 2)}
    return grid(5, 5, cells, T=6)


def corner_squares():
    """two 2 x 2 squares that touch at a corner, 3 days: one object under connectivity 26; 2 parts under 4 neighbours,
    1 under 8"""
    cells = {(i, j): [(0, 2)] for i in (0, 1) for j in (0, 1)}
    cells.update({(i, j): [(0, 2)] for i in (2, 3) for j in (2, 3)})
    return grid(4, 5, cells, T=4)


def seam():
    """two cells at the two ends of a row of 6 for 6 days, the cells between them on the last 2: with the grid wrapping
    along lon the two are neighbours (1 part every day), without they are 2 parts on the first 4 days"""
    cells = {(1, 0): [(0, 5)], (1, 5): [(0, 5)]}
    cells.update({(1, j): [(4, 5)] for j in (1, 2, 3, 4)})
    return grid(3, 6, cells, T=7)


def broken_bar():
    """a bar of 5 cells for 9 days whose middle cell is missing on days 3..5: n_parts 1, 2, 1 and 3 days split"""
    cells = {(1, j): [(0, 8)] for j in (0, 1, 3, 4)}
    cells[(1, 2)] = [(0, 2), (6, 8)]
    return grid(3, 5, cells, T=10)


# (name, dataset, mhw_objects kwargs, neighbours, n_parts of object 0, cells_largest of object 0)
def hand_drawn():
    return [
        ("ring", ring(), dict(connectivity=6), None, [1] * 4, [8] * 4),
        ("ring-8", ring(), dict(connectivity=26), None, [1] * 4, [8] * 4),
        ("corner-4", corner_squares(), dict(connectivity=26), 4, [2] * 3, [4] * 3),
        ("corner-8", corner_squares(), dict(connectivity=26), None, [1] * 3, [8] * 3),
        ("seam-wrapped", seam(), dict(connectivity=6, periodic="lon"), None, [1] * 6, [2] * 4 + [6] * 2),
        ("seam-open", seam(), dict(connectivity=6), None, [2] * 4 + [1] * 2, [1] * 4 + [6] * 2),
        ("broken-bar", broken_bar(), dict(connectivity=6), None, [1, 1, 1, 2, 2, 2, 1, 1, 1], [5, 5, 5, 2, 2, 2, 5, 5, 5]),
    ]


def checkerboard(n=16, days=5):
    """the black squares of an n x n board, alive together for ``days`` days: n * n / 2 parts under 4 neighbours; one
    part under 8, where objects of connectivity 26 hold them all"""
    cells = {(i, j): [(2, 1 + days)] for i in range(n) for j in range(n) if (i + j) % 2 == 0}
    return grid(n, n, cells, T=days + 4)


def spiral(n=33, days=3):
    """a one-cell-wide square spiral on an n x n grid (a free line between the arms), alive for ``days`` days: one part
    reached through a chain of unions as long as the spiral.  Returns (ds, the number of its cells)."""
    on = np.zeros((n, n), dtype=bool)
    i, j, di, dj = 0, 0, 0, 1
    on[0, 0] = True
    while True:
        # walk while the cell two ahead is free (keeps a free line between the arms) and inside the grid
        moved = False
        while True:
            ii, jj = i + di, j + dj
            i2, j2 = ii + di, jj + dj
            if not (0 <= ii < n and 0 <= jj < n) or on[ii, jj]:
                break
            if 0 <= i2 < n and 0 <= j2 < n and on[i2, j2]:
                break
            i, j = ii, jj
            on[i, j] = True
            moved = True
        if not moved:
            break
        di, dj = dj, -di                                          # turn right
    cells = {(int(a), int(b)): [(1, days)] for a, b in zip(*np.nonzero(on))}
    return grid(n, n, cells, T=days + 2), int(on.sum())


def land_grid(seed=0, n=64, land=0.4, days=10, rows=None):
    """an n x n grid with a share ``land`` of land.  rows=None: every ocean cell in one event over the same ``days``
    days.  rows=(lo, hi): every ocean cell holds lo..hi rows of random length inside a window of 4 * days days, so the
    footprint changes from day to day."""
    rng = np.random.default_rng(seed)
    keep = rng.random((n, n)) >= land
    cells = {}
    for i, j in zip(*np.nonzero(keep)):
        if rows is None:
            cells[(int(i), int(j))] = [(3, 2 + days)]
        else:
            k = int(rng.integers(rows[0], rows[1] + 1))
            cuts = np.sort(rng.choice(np.arange(2 * days), 2 * k, replace=False)) * 2      # even positions: a free day between
            cells[(int(i), int(j))] = [(int(a), int(b) - 2) for a, b in zip(cuts[0::2], cuts[1::2])]
    return grid(n, n, cells, T=4 * days + 2, keep=keep)
