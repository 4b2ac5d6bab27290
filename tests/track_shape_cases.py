"""Hand-drawn inputs shared by the host and the GPU tests of mhw_track_shape(), every expected number written out and
counted on the figure beside it.  In the figures ``o`` is a footprint cell, ``.`` ocean outside it, ``#`` land; rows
are dim 0 (lat), columns dim 1 (lon).  The grids and most of the shapes are those of track_parts_cases."""
import numpy as np

import track_parts_cases as pc

grid = pc.grid


def coast_ring():
    """the ring of track_parts_cases.ring() with its hole and the point above its top side made land

            j  0 1 2 3 4
        i = 0  . . # . .        the four faces into the hole (2, 2) and the top face of (1, 2) are coast: 5;
        i = 1  . o o o .        the outer faces of the ring are 12, one of them that coast face: 11 open
        i = 2  . o # o .
        i = 3  . o o o .
        i = 4  . . . . ."""
    keep = np.ones((5, 5), bool)
    keep[2, 2] = keep[0, 2] = False
    cells = {(i, j): [(1, 4)] for i in (1, 2, 3) for j in (1, 2, 3) if (i, j) != (2, 2)}
    return grid(5, 5, cells, T=6, keep=keep)


def folded():
    """a grid 3 x 1 that wraps along lon: the lon faces fold onto the cell itself and are counted nowhere

        i = 0  o        top: border; bottom: shared
        i = 1  o        top: shared; bottom: open
        i = 2  ."""
    return grid(3, 1, {(0, 0): [(0, 2)], (1, 0): [(0, 2)]}, T=4)


def wrap_of_two():
    """a grid 1 x 2 that wraps along lon: both lon faces of a cell lead to the other cell, and both are faces

        days 0..1   o .     top, bottom: border (2); left and right: both open towards (0, 1) (2)
        days 2..3   o o     top, bottom of both: border (4); the four lon faces: shared"""
    return grid(1, 2, {(0, 0): [(0, 3)], (0, 1): [(2, 3)]}, T=5)


def gap_beside_a_steady_cell():
    """one row of 5 cells; (0, 2) holds two rows of the object with a gap between them, (0, 1) and (0, 3) live through it

        days  0..1   . . o . .      border 2 (top, bottom)   open 2
        days  2..3   . o o o .      border 6                 open 2 (the two ends)
        days  4..7   . o . o .      border 4                 open 4 (both sides of both cells)
        days  8..9   . o o o .      border 6                 open 2
        days 10..11  . . o . .      border 2                 open 2
    the face between (0, 1) and (0, 2) is shared, open, then shared again"""
    return grid(1, 5, {(0, 2): [(0, 3), (8, 11)], (0, 1): [(2, 9)], (0, 3): [(2, 9)]}, T=14)


def _case(name, ds, kw, open_, coast, border, cells):
    return dict(name=name, ds=ds, kw=kw, edges_open=open_, edges_coast=coast, edges_border=border, cells_edge=cells)


def hand_drawn():
    """every case holds ONE object; the four lists are its series"""
    return [
        # 12 outer faces and the 4 faces into the hole, all open
        _case("ring", pc.ring(), dict(connectivity=6), [16] * 4, [0] * 4, [0] * 4, [8] * 4),
        # the square in the corner: 2 + 2 border (top, left), 2 + 2 open; the other: 2 border (bottom), 6 open
        _case("corner-squares", pc.corner_squares(), dict(connectivity=26), [10] * 3, [0] * 3, [6] * 3, [8] * 3),
        _case("coast-ring", coast_ring(), dict(connectivity=6), [11] * 4, [5] * 4, [0] * 4, [8] * 4),
        # two end cells of a row of 6 (4 days), then the whole row (2 days): top and bottom open throughout
        _case("seam-wrapped", pc.seam(), dict(connectivity=6, periodic="lon"), [6] * 4 + [12] * 2, [0] * 6, [0] * 6,
              [2] * 4 + [6] * 2),
        _case("seam-open", pc.seam(), dict(connectivity=6), [6] * 4 + [12] * 2, [0] * 6, [2] * 6, [2] * 4 + [6] * 2),
        _case("folded", folded(), dict(connectivity=6, periodic="lon"), [1] * 3, [0] * 3, [1] * 3, [2] * 3),
        _case("wrap-of-two", wrap_of_two(), dict(connectivity=6, periodic="lon"), [2, 2, 0, 0], [0] * 4, [2, 2, 4, 4], [1, 1, 2, 2]),
        # a bar of 5 (top and bottom 10, the two ends border); without its middle cell 8 + the two new ends = 10 again,
        # on 4 cells: the count of faces stays, their lengths need not (test_host_track_shape.py)
        _case("broken-bar", pc.broken_bar(), dict(connectivity=6), [10] * 9, [0] * 9, [2] * 9, [5, 5, 5, 4, 4, 4, 5, 5, 5]),
        _case("gap-beside-steady", gap_beside_a_steady_cell(), dict(connectivity=6), [2, 2, 2, 2, 4, 4, 4, 4, 2, 2, 2, 2],
              [0] * 12, [2, 2, 6, 6, 4, 4, 4, 4, 6, 6, 2, 2], [1, 1, 3, 3, 2, 2, 2, 2, 3, 3, 1, 1]),
    ]


def stage_arguments(ds, slot, time_start, durations, periodic_axis=None, lq=None):
    """the arguments of track_shape_device() for a hand-made partition of the rows of ``ds`` into objects: slot (n,), the
    selected object of every row or -1; time_start / durations (m,) of the selected objects"""
    from xmhw_amd.track_shape import face_table, length_bits
    view = ds.compact_view()
    C = view["C"]
    lq = np.full((C, 4), 1 << length_bits(C), dtype=np.int64) if lq is None else np.asarray(lq, dtype=np.int64)
    offsets = np.concatenate([[0], np.cumsum(durations)]).astype(np.int64)
    return (view["start"], view["end"], np.asarray(slot, dtype=np.int32), view["cell_of_row"].astype(np.int32), view["offsets"],
            face_table(view["cell_index"], ds.sshape, periodic_axis), lq, np.asarray(time_start, dtype=np.int32), offsets)


def two_objects_side_by_side():
    """two cells side by side on the same 3 days in DIFFERENT objects (mhw_objects() would join them: the partition is made
    by hand): the face between them is open for both

            j  0 1 2 3
        i = 0  . . . .
        i = 1  . a b .          a: 4 open faces, b: 4 open faces
        i = 2  . . . .
    Returns (ds, slot of every row with both selected, slot with only ``a`` selected)."""
    ds = grid(3, 4, {(1, 1): [(0, 2)], (1, 2): [(0, 2)]}, T=4)
    return ds, [0, 1], [0, -1]


def full_grid(n=64, days=2):
    """every cell of an n x n grid alive on the same days: one object whose only exposed faces are the edge of the grid"""
    return grid(n, n, {(i, j): [(1, days)] for i in range(n) for j in range(n)}, T=days + 2)
