"""mhw_track_shape(): what every object of mhw_objects() looks like on each of its days -- the length of its outline,
and how much of that outline is coast -- aligned entry for entry with the ragged (CSR) arrays of mhw_tracks(): entry
offsets[i] + (t - time_start[i]) belongs to object ids[i] on time position t.  With the area of mhw_tracks() the
perimeter gives compactness and deformation; the coast contact separates coastal heatwaves from open-ocean ones.  The
tracking tools of the field take both from regionprops on a dense labelled volume, or difference shifted label maps
day by day; here no map is built: every table row walks its own days against the rows of its four face neighbours
(csrc/kernels_shape.hip).

The definition.  Take a selected object o and a time position t in [time_start[o], time_end[o]].
  * Its footprint is that of track_parts.py: the ocean cells that hold a table row of o covering t (index_start..
    index_end inclusive, gap days of joined events included).
  * Every footprint cell has four faces, in the order of objects._DIAGONAL[:4]: dim 0 minus, dim 0 plus, dim 1 minus,
    dim 1 plus.  Adjacency is always by faces, whatever obj.connectivity is; the wrapping dim is obj.periodic.
  * Each face falls into exactly one class:
      shared   the cell across it is in the footprint of o on day t: nothing is counted;
      open     the cell across it is ocean (a cell of mhw.cell_index) and not in the footprint -- it may belong to
               another object or to none;
      coast    the grid point across it is land (not in mhw.cell_index);
      border   there is no grid point across it (the edge of a dim that does not wrap);
      folded   a wrapping dim of length 1: the cell across is the cell itself; this is no face, nothing is counted.
    A wrapping dim of length 2 has two real faces to the same other cell: both are classified, each with its own length.
Per entry, exact integers:
    edges_open, edges_coast, edges_border (int32)                       the number of faces of each class,
    perimeter_open_q, perimeter_coast_q, perimeter_border_q (int64)     the sum of the quantised lengths lq[c, k] of
                                                                        those faces,
    cells_edge (int32)      the footprint cells with at least one open, coast or border face.

Edge lengths, ``lengths=``:
    None        every face has length 1;
    "sphere"    km on a sphere of radius 6371.0088 km from the 1-D latitude and longitude coordinates of the two
                spatial dims in degrees (found as mhw_tracks() finds them).  The faces of a cell lie half way to the
                adjacent coordinate values; at the two ends of a dim the cell reaches half the adjacent spacing further;
                latitudes are clipped to [-90, 90].  A face across the latitude dim, at latitude phi, has the length
                R cos(phi) dlambda_j, dlambda_j the width of the cell in longitude; a face across the longitude dim
                has R dphi_i, dphi_i the height of the cell in latitude.  float64 on the host, sums and products in
                one fixed order; a face at a pole has length 0 exactly;
    an array of shape sshape + (4,), finite and >= 0 with at least one value > 0.
They are quantised as lq = rint(len / len.max() * 2**length_bits) (int64) with
    length_bits = min(31, 60 - bit_length(C)),
C = the ocean cells of the grid: a day holds at most 4 C faces of at most 2**length_bits each, and 4 C 2**length_bits <
2**63, so no sum can pass int64.  length_unit = len.max() / 2**length_bits turns the integers back.

Identities, against mhw_tracks() on the same ids:
    cells_edge <= n_cells;  cells_edge <= edges_exposed <= 4 cells_edge;  edges_exposed <= 4 n_cells;
    edges_exposed >= 4 on every entry of a grid without a wrapping dim, >= 2 with one (the outermost cells along a dim
    that does not wrap have a face that is not shared);
    with lengths=None, perimeter_*_q == edges_* << length_bits.

Derived on the host, per entry: edges_exposed (the sum of the three counts), perimeter_q (the sum of the three integer
perimeters), perimeter_open, perimeter_coast, perimeter_border and perimeter (``* length_unit``, float64), coast_fraction
= perimeter_coast_q / (perimeter_open_q + perimeter_coast_q), NaN where that is 0 / 0 (the border of the grid is neither
coast nor water); per selected object: perimeter_max and pos_perimeter_max (the first position that attains it),
days_coastal (the entries with edges_coast > 0).  compactness(shape, tracks) = 4 pi area / perimeter**2.

Host side here (validation, selection, face table, lengths, the derived fields); device side in csrc/kernels_shape.hip
behind track_shape_device().
"""
import numpy as np

from .exception import XmhwException
from .objects import _DIAGONAL
from .track_common import ChainDataset, Selection, device_stage, stage_inputs
from .tracks import EARTH_RADIUS_KM, TrackDataset, _latlon

CLASSES = ("open", "coast", "border")                                   # XMHW_SHAPE_* order
STAGE_FIELDS = ("edges_open", "edges_coast", "edges_border", "perimeter_open_q", "perimeter_coast_q", "perimeter_border_q",
                "cells_edge")
_DTYPES = dict(edges_open=np.int32, edges_coast=np.int32, edges_border=np.int32, perimeter_open_q=np.int64,
               perimeter_coast_q=np.int64, perimeter_border_q=np.int64, cells_edge=np.int32)
_INPUTS = dict(start=np.int32, end=np.int32, slot=np.int32, cell=np.int32, row_offsets=np.int64, faces=np.int32, lq=np.int64,
               time_start=np.int32, offsets=np.int64)
FACE_COAST, FACE_BORDER, FACE_FOLDED = -1, -2, -3                       # XMHW_SHAPE_FACE_* (include/xmhw_amd.h)
ENTRY_BYTES = 40


def face_table(cell_index, sshape, periodic_axis=None):
    """faces (C, 4) int32: what lies across the four faces (dim 0 minus, dim 0 plus, dim 1 minus, dim 1 plus) of every
    ocean cell: the compact number of the cell there, FACE_COAST (-1) for land, FACE_BORDER (-2) outside the grid,
    FACE_FOLDED (-3) along a wrapping dim of length 1.  objects.neighbour_table() folds the three into -1."""
    ny, nx = (int(v) for v in sshape)
    cell_index = np.asarray(cell_index, dtype=np.int64)
    C = cell_index.shape[0]
    number = np.full(ny * nx, FACE_COAST, dtype=np.int32)
    number[cell_index] = np.arange(C, dtype=np.int32)
    i, j = np.divmod(cell_index, nx)
    faces = np.empty((C, 4), dtype=np.int32)
    for k, (di, dj) in enumerate(_DIAGONAL[:4]):
        axis = 0 if di else 1
        if periodic_axis == axis and (ny, nx)[axis] == 1:
            faces[:, k] = FACE_FOLDED
            continue
        ii, jj = i + di, j + dj
        if periodic_axis == 0:
            ii %= ny
        if periodic_axis == 1:
            jj %= nx
        ok = (ii >= 0) & (ii < ny) & (jj >= 0) & (jj < nx)
        v = np.full(C, FACE_BORDER, dtype=np.int32)
        v[ok] = number[ii[ok] * nx + jj[ok]]
        faces[:, k] = v
    return faces


def length_bits(n_ocean):
    """length_bits of the module docstring"""
    return int(min(31, 60 - int(n_ocean).bit_length()))


def _cell_edges(x, clip=None):
    """(len(x) + 1,) float64: the faces of the cells centred on the 1-D coordinate ``x``: half way between adjacent values,
    half the adjacent spacing beyond the two ends"""
    mid = 0.5 * (x[:-1] + x[1:])
    e = np.concatenate([[x[0] - 0.5 * (x[1] - x[0])], mid, [x[-1] + 0.5 * (x[-1] - x[-2])]])
    return e if clip is None else np.clip(e, -clip, clip)


def sphere_lengths(coords, sdims, sshape):
    """(sshape + (4,)) float64, km: the lengths of the four faces of every grid cell on the sphere (module docstring)"""
    sdims = list(sdims)
    names = _latlon(coords, sdims)
    if names is None:
        raise XmhwException(f"lengths='sphere' needs latitude and longitude coordinates for the dims {tuple(sdims)}")
    lat = np.asarray(coords[names[0]], dtype=np.float64)
    lon = np.asarray(coords[names[1]], dtype=np.float64)
    a_lat, a_lon = sdims.index(names[0]), sdims.index(names[1])
    if lat.shape != (sshape[a_lat],) or lon.shape != (sshape[a_lon],):
        raise XmhwException("lengths='sphere': the latitude and longitude coordinates should be 1-D along their dims")
    if lat.shape[0] < 2 or lon.shape[0] < 2:
        raise XmhwException("lengths='sphere' takes the size of a cell from the spacing of the coordinates: both dims should "
                            "hold at least 2 values")
    if not (np.isfinite(lat).all() and np.isfinite(lon).all() and np.abs(lat).max() <= 90.0 + 1e-9):
        raise XmhwException("lengths='sphere': latitude should be within [-90, 90] degrees, and both coordinates finite")
    e_lat, e_lon = _cell_edges(lat, clip=90.0), _cell_edges(lon)
    cos_face = np.where(np.abs(e_lat) >= 90.0, 0.0, np.maximum(np.cos(np.deg2rad(e_lat)), 0.0))
    dlam = np.abs(np.deg2rad(e_lon[1:]) - np.deg2rad(e_lon[:-1]))
    dphi = np.abs(np.deg2rad(e_lat[1:]) - np.deg2rad(e_lat[:-1]))
    out = np.empty(tuple(sshape) + (4,), dtype=np.float64)
    shape_lat, shape_lon = [1, 1], [1, 1]
    shape_lat[a_lat], shape_lon[a_lon] = -1, -1
    across_lon = np.broadcast_to((EARTH_RADIUS_KM * dphi).reshape(shape_lat), sshape)
    out[..., 2 * a_lon] = out[..., 2 * a_lon + 1] = across_lon
    for side in (0, 1):                                               # the face towards the smaller, the larger index
        rc = (EARTH_RADIUS_KM * cos_face[side:side + lat.shape[0]]).reshape(shape_lat)
        out[..., 2 * a_lat + side] = rc * dlam.reshape(shape_lon)
    return out


def resolve_lengths(lengths, coords, sdims, sshape):
    """The float64 face lengths (sshape + (4,)) of ``lengths`` = None | "sphere" | array, validated"""
    sshape = tuple(int(v) for v in sshape)
    if lengths is None:
        return np.ones(sshape + (4,), dtype=np.float64)
    if isinstance(lengths, str):
        if lengths != "sphere":
            raise XmhwException(f"lengths should be None, 'sphere' or an array, got {lengths!r}")
        ln = sphere_lengths(coords, sdims, sshape)
    else:
        try:
            ln = np.asarray(lengths, dtype=np.float64)
        except (TypeError, ValueError):
            raise XmhwException(f"lengths should be None, 'sphere' or an array, got {type(lengths).__name__}") from None
        if ln.shape != sshape + (4,):
            raise XmhwException(f"lengths should have the shape {sshape + (4,)} (the grid, then the four faces), got {ln.shape}")
    if not np.isfinite(ln).all() or (ln < 0).any():
        raise XmhwException("lengths should be finite and >= 0")
    if not (ln > 0).any():
        raise XmhwException("lengths should hold at least one value > 0")
    return ln


def quantise_lengths(ln, bits):
    """(lq int64 of ln's shape, length_unit): lq = rint(ln / ln.max() * 2**bits)"""
    top = float(ln.max())
    return np.rint(ln / top * float(1 << bits)).astype(np.int64), top / float(1 << bits)


def lengths_label(lengths):
    return "none" if lengths is None else (lengths if isinstance(lengths, str) else "array")


def track_shape_device(start, end, slot, cell, row_offsets, faces, lq, time_start, offsets):
    """The device stage.  start / end (n,) int32 positions of every table row; slot (n,) int32, the position of the row's
    object in the selection or -1; cell (n,) int32, the row's compact cell; row_offsets (C + 1,) int64, the rows of every
    cell; faces (C, 4) int32 (face_table()); lq (C, 4) int64; time_start (m,) int32 and offsets (m + 1,) int64 of the
    selection.  Returns a dict of STAGE_FIELDS, (L,) each, L = offsets[-1]."""
    start, end, slot, cell, row_offsets, faces, lq, time_start, offsets = a = stage_inputs(
        _INPUTS, start, end, slot, cell, row_offsets, faces, lq, time_start, offsets)
    n, m, C = start.shape[0], time_start.shape[0], faces.shape[0]
    L = int(offsets[-1])
    if L == 0 or n == 0 or m == 0:
        return {k: np.zeros(L, dtype=_DTYPES[k]) for k in STAGE_FIELDS}
    if faces.shape != (C, 4) or lq.shape != (C, 4) or row_offsets.shape != (C + 1,):
        raise XmhwException("the face table, the face lengths and the row offsets do not fit the cells")
    with device_stage(a, (n, m, L, C), f"mhw_track_shape handles fewer than 2**31 rows, objects, series entries and cells, got "
                      f"{n}, {m}, {L}, {C}") as (h, s, d, launch):
        with launch:
            d_edges, d_perim, d_cells, d_bad = s.alloc(4 * 3 * L), s.alloc(8 * 3 * L), s.alloc(4 * L), s.alloc(4)
            h.object_shape(d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, n, d[4].ptr, C, d[5].ptr, 4, d[6].ptr, d[7].ptr, d[8].ptr, m, L,
                           d_edges.ptr, d_perim.ptr, d_cells.ptr, d_bad.ptr)
            h.stream_sync(0)
        edges, perim = d_edges.to_array((3, L), np.int32), d_perim.to_array((3, L), np.int64)
        out = {f"edges_{c}": np.ascontiguousarray(edges[k]) for k, c in enumerate(CLASSES)}
        out.update({f"perimeter_{c}_q": np.ascontiguousarray(perim[k]) for k, c in enumerate(CLASSES)})
        out["cells_edge"] = d_cells.to_array((L,), np.int32)
        bad = int(d_bad.to_array((1,), np.int32)[0])
    if bad:
        raise XmhwException(f"{bad} table rows do not lie within their object's days or cells, or hold a face that names no "
                            "cell: obj does not belong to mhw")
    return out


class TrackShapeDataset(ChainDataset):
    """What mhw_track_shape() returns, as plain arrays, aligned with the TrackDataset of the same ``ids``: m objects, L =
    offsets[-1] entries; entry offsets[i] + (t - time_start[i]) belongs to object ids[i] on time position t.

    ids, offsets, time_start, time_end, duration, pos    as in the TrackDataset;
    edges_open, edges_coast, edges_border (L,) int32     the faces of the object's footprint on that day towards ocean
                                    outside it, towards land, and on the edge of the grid;
    edges_exposed (L,) int32        their sum;
    perimeter_open_q, perimeter_coast_q, perimeter_border_q, perimeter_q (L,) int64     the sums of the quantised lengths
                                    of those faces, and the sum of the three;
    perimeter_open, perimeter_coast, perimeter_border, perimeter (L,) float64           ``* length_unit``;
    cells_edge (L,) int32           the footprint cells with at least one such face;
    coast_fraction (L,) float64     perimeter_coast_q / (perimeter_open_q + perimeter_coast_q); NaN where both are 0;
    perimeter_max (m,) float64      the largest perimeter of each object;
    pos_perimeter_max (m,) int32    the first time position that attains it;
    days_coastal (m,) int32         the object's days with edges_coast > 0;
    length_bits, length_unit, periodic."""

    _SERIES = ("pos",) + STAGE_FIELDS + ("edges_exposed", "perimeter_q", "perimeter_open", "perimeter_coast", "perimeter_border",
                                         "perimeter", "coast_fraction")
    _PER_OBJECT = ("ids", "time_start", "time_end", "duration", "perimeter_max", "pos_perimeter_max", "days_coastal")
    _ATTRS = ("periodic", "length_unit", "length_bits")

    def __init__(self, fields, time, sdims, sshape, periodic, length_bits, length_unit, attrs=None):
        super().__init__(fields, time, sdims, sshape, attrs)
        self.periodic, self.length_bits, self.length_unit = periodic, int(length_bits), float(length_unit)


def mhw_track_shape(mhw, obj, ids=None, lengths=None, _compute=None):
    """The daily outline of the objects of mhw_objects(): its length, and how much of it is coast.

    ``mhw``, ``obj`` and ``ids`` mean and validate what they do in mhw_tracks(); give the same ``ids`` and the result
    lines up with its TrackDataset entry for entry.  ``lengths``: None (every face 1), "sphere" (km from the latitude
    and longitude coordinates) or an array of shape sshape + (4,) (module docstring).  Adjacency is by faces whatever
    obj.connectivity is; the wrapping dim is ``obj.periodic``.

    Returns a TrackShapeDataset (module docstring: the definition and the identities; class docstring: the fields).
    Every number of the stage is an integer sum: exact, and the same from run to run.  ``_compute``: a stand-in for
    track_shape_device() (host tests)."""
    sel = Selection(mhw, obj, ids, "mhw_track_shape")
    axis = sel.periodic_axis()
    sshape = sel.sshape
    ln = resolve_lengths(lengths, mhw.coords, mhw.sdims, sshape)      # every refusal of lengths= before anything of size L
    sel.view()
    bits = length_bits(sel.C)
    lq, unit = quantise_lengths(ln, bits)
    sel.layout()
    L = sel.L
    if L == 0:
        got = sel.no_entries(_DTYPES)
    else:
        faces = face_table(sel.cell_index, sshape, axis)
        got = (_compute or track_shape_device)(sel.start, sel.end, sel.slot, sel.cell_of_row, sel.row_offsets, faces,
                                               lq.reshape(-1, 4)[sel.cell_index], sel.time_start, sel.offsets)
    try:
        f = sel.stage_arrays(got, _DTYPES, "track shape")
    except (KeyError, TypeError, ValueError):
        raise XmhwException(f"track shape stage should return the arrays {STAGE_FIELDS}") from None
    exposed = f["edges_open"].astype(np.int64) + f["edges_coast"] + f["edges_border"]
    # an object has no empty day, and the outermost cells of a footprint along a dim that does not wrap have a face that
    # is not shared: two such faces per dim that does not wrap
    least = 4 if axis is None else 2
    if L and (exposed.min() < least or f["cells_edge"].min() < 1):
        raise XmhwException(f"{int(((exposed < least) | (f['cells_edge'] < 1)).sum())} days of the selected objects hold no "
                            "cell: obj does not belong to mhw")
    f.update(sel.common_fields(), pos=sel.pos())
    f["edges_exposed"] = exposed.astype(np.int32)
    f["perimeter_q"] = f["perimeter_open_q"] + f["perimeter_coast_q"] + f["perimeter_border_q"]
    for c in CLASSES:
        f[f"perimeter_{c}"] = f[f"perimeter_{c}_q"] * unit
    f["perimeter"] = f["perimeter_q"] * unit
    wet = f["perimeter_open_q"] + f["perimeter_coast_q"]
    with np.errstate(divide="ignore", invalid="ignore"):
        f["coast_fraction"] = np.where(wet > 0, f["perimeter_coast_q"] / wet.astype(np.float64), np.nan)
    pmax, f["pos_perimeter_max"] = sel.first_max(f["perimeter_q"])
    f["perimeter_max"] = pmax * unit
    f["days_coastal"] = sel.count_days(f["edges_coast"] > 0)
    attrs = {"lengths": lengths_label(lengths)}
    return TrackShapeDataset(f, mhw.time, mhw.sdims, sshape, obj.periodic, bits, unit, attrs)


def compactness(shape, tracks):
    """(L,) float64: 4 pi area / perimeter**2 of every entry, from a TrackShapeDataset and the TrackDataset of the same
    ``ids``: 1 for a disc, pi / 4 for a square of grid cells, towards 0 for a ragged or stretched outline; NaN where the
    perimeter is 0.  The number means something when lengths and weights are in matching units: lengths="sphere" (km)
    with weights that are cell areas in km**2; lengths=None with weights=None gives the compactness in grid cells.
    Host arithmetic only."""
    if not isinstance(shape, TrackShapeDataset) or not isinstance(tracks, TrackDataset):
        raise XmhwException("compactness expects the TrackShapeDataset of mhw_track_shape() and the TrackDataset of mhw_tracks()")
    if not (np.array_equal(shape.ids, tracks.ids) and np.array_equal(shape.offsets, tracks.offsets)
            and np.array_equal(shape.time_start, tracks.time_start)):
        raise XmhwException("compactness needs the two datasets made with the same ids, from the same objects")
    p = np.asarray(shape.perimeter, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(p > 0, 4.0 * np.pi * np.asarray(tracks.area, dtype=np.float64) / (p * p), np.nan)
