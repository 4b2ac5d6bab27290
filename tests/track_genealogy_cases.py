"""Hand-drawn inputs shared by the host and the GPU tests of mhw_track_genealogy(), each one object under connectivity 6
with every count and every edge written out by hand, and the larger grids of the GPU tests.

A case is (name, dataset, expected) with ``expected`` a dict of the six per-day lists of object 0, ``edges`` as
[(position of the later day, label before, label after), ...] in sorted order, and the per-object totals ``n_splits``,
``n_merges``, ``n_births``, ``n_ends``."""
import track_parts_cases as pc


def bridged_squares():
    """two 2 x 2 squares, three columns apart, for 6 days; the cell between their top rows is on on days 2 and 3 only.
    The squares never share a cell-day; they are one object through the bridge: a merge when it arrives, a split on the
    day before it leaves.  Labels: the left square and the whole 0, the right square 3 (a 3 x 5 grid)."""
    cells = {(i, j): [(0, 5)] for i in (0, 1) for j in (0, 1, 3, 4)}
    cells[(0, 2)] = [(2, 3)]
    return pc.grid(3, 5, cells, T=7)


def moving_patch():
    """a patch of two cells that moves one cell a day along the middle row of a 3 x 7 grid for 5 days: cells (1, t) and
    (1, t + 1) on day t.  Cell (1, t + 1) is on on both days, so every day overlaps the next: a chain.  The label of day
    t is 7 + t."""
    cells = {(1, j): [(max(0, j - 1), min(4, j))] for j in range(6)}
    return pc.grid(3, 7, cells, T=6)


def hand_drawn():
    bar = [(t, 5, 5) for t in (1, 2)] + [(3, 5, 5), (3, 5, 8), (4, 5, 5), (4, 8, 8), (5, 5, 5), (5, 8, 8), (6, 5, 5), (6, 8, 5),
                                         (7, 5, 5), (8, 5, 5)]
    squares = [(1, 0, 0), (1, 3, 3), (2, 0, 0), (2, 3, 0), (3, 0, 0), (4, 0, 0), (4, 0, 3), (5, 0, 0), (5, 3, 3)]
    return [
        # a bar of 5 cells in row 1 of a 3 x 5 grid for 9 days whose middle cell is off on days 3..5: the whole bar (label
        # 5) splits into a left (5) and a right half (8) after day 2, and the halves merge on day 6
        ("broken-bar", pc.broken_bar(), dict(
            n_parts=[1, 1, 1, 2, 2, 2, 1, 1, 1], n_links=[0, 1, 1, 2, 2, 2, 2, 1, 1], n_born=[1, 0, 0, 0, 0, 0, 0, 0, 0],
            n_merged=[0, 0, 0, 0, 0, 0, 1, 0, 0], n_ended=[0, 0, 0, 0, 0, 0, 0, 0, 1], n_split=[0, 0, 1, 0, 0, 0, 0, 0, 0],
            edges=bar, n_splits=1, n_merges=1, n_births=0, n_ends=0)),
        # a 3 x 3 ring around a hole in a 5 x 5 grid, days 1..4: one part (label 6), one link a day, nothing else
        ("ring", pc.ring(), dict(
            n_parts=[1] * 4, n_links=[0, 1, 1, 1], n_born=[1, 0, 0, 0], n_merged=[0] * 4, n_ended=[0, 0, 0, 1], n_split=[0] * 4,
            edges=[(t, 6, 6) for t in (2, 3, 4)], n_splits=0, n_merges=0, n_births=0, n_ends=0)),
        ("bridged-squares", bridged_squares(), dict(
            n_parts=[2, 2, 1, 1, 2, 2], n_links=[0, 2, 2, 1, 2, 2], n_born=[2, 0, 0, 0, 0, 0], n_merged=[0, 0, 1, 0, 0, 0],
            n_ended=[0, 0, 0, 0, 0, 2], n_split=[0, 0, 0, 1, 0, 0], edges=squares, n_splits=1, n_merges=1, n_births=0,
            n_ends=0)),
        ("moving-patch", moving_patch(), dict(
            n_parts=[1] * 5, n_links=[0, 1, 1, 1, 1], n_born=[1, 0, 0, 0, 0], n_merged=[0] * 5, n_ended=[0, 0, 0, 0, 1],
            n_split=[0] * 5, edges=[(t, 6 + t, 7 + t) for t in (1, 2, 3, 4)], n_splits=0, n_merges=0, n_births=0, n_ends=0)),
    ]


def check_hand_drawn(tg, want):
    """the TrackGenealogyDataset of a hand-drawn case (one object) against its expected dict"""
    assert tg.n_selected == 1
    for k in ("n_parts", "n_links", "n_born", "n_merged", "n_ended", "n_split"):
        assert getattr(tg, k).tolist() == want[k], k
    got = list(zip(tg.edge_pos.tolist(), tg.edge_from.tolist(), tg.edge_to.tolist()))
    assert got == want["edges"] and tg.edge_track.tolist() == [0] * len(got) and tg.edge_offsets.tolist() == [0, len(got)]
    for k in ("n_splits", "n_merges", "n_births", "n_ends"):
        assert getattr(tg, k).tolist() == [want[k]], k
    assert tg.n_nodes.tolist() == [sum(want["n_parts"])] and tg.n_edges.tolist() == [len(got)]


def full_grid(n=64, days=2):
    """every cell of an n x n grid in one row over the same ``days`` days: n * n pairs a day step, one distinct edge"""
    return pc.grid(n, n, {(i, j): [(1, days)] for i in range(n) for j in range(n)}, T=days + 2)
