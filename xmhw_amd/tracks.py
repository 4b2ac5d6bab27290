"""mhw_tracks(): how every object of mhw_objects() evolved -- its number of cells, its area and its centre on each
day from its first to its last, as ragged (CSR) arrays: object i of the selection owns the entries
offsets[i]..offsets[i + 1] - 1, one per time position from time_start[i] to time_end[i].  The tracking tools of the
field loop regionprops over a dense labelled (time, lat, lon) volume; here no volume and no voxel is visited: every
quantity is constant along a table row, so a row adds its vector on its first day and takes it away behind its last
(a difference array), and one prefix sum over the concatenated array gives every object's series
(csrc/kernels_tracks.hip).

The integers (the definition).  For a selected object o and a position t in [time_start[o], time_end[o]], over the
cells c that hold a row of o covering t (index_start..index_end inclusive: the voxels of objects.py):
    n_cells = the number of such cells,             area_q = sum wq[c],
    mx, my, mz = sum wm[c] * ux[c], ... uy[c], ... uz[c].
wq = rint(w / w.max() * 2**obj.weight_bits), the quantisation of mhw_objects(): with the same weights the series of
an object sums to its area_days_q, as n_cells sums to its cell_days.

Positions.  Mode "sphere", when ``mhw.coords`` holds the latitude and the longitude of the two spatial dims in
degrees: u[c] = rint(2**20 * (cos(lat) cos(lon), cos(lat) sin(lon), sin(lat))), a vector of the unit sphere in 20-bit
fixed point.  A sum of vectors has no date line: an object astride it has its centre on it, where a mean of
longitudes would say 0.  Mode "index" otherwise: u[c] = (i, j, 0), the indices along the two spatial dims, and
sum wm[c] rides in the third channel (``wsum``; ``mz`` is 0 by definition).  A mean index across a wrapping dim
means nothing, so an ObjectDataset made with ``periodic`` is refused in index mode.

The moment weights wm = rint(w / w.max() * 2**mb) are a second, coarser quantisation of the same weights, sized so
that no sum can pass int64 whatever the data.  A day of an object holds at most C cells (C = the ocean cells of the
grid), wm <= 2**mb and |u| <= 2**20, so |sum wm * u| <= C * 2**(mb + 20) < 2**(bit_length(C) + mb + 20).  With
    mb = min(obj.weight_bits, 61 - 20 - bit_length(C))
this is at most 2**61, below 2**62.  In index mode the indices are below 2**bit_length(max(ny, nx)), which takes the
place of the 20.  area_q is at most C * 2**weight_bits <= 2**62 / (days per cell), as in mhw_objects().  The device
adds and subtracts modulo 2**64 on the way; every value it delivers is one of these bounded sums, hence exact.

Host side here (validation, selection, weights and unit vectors, the float64 quantities derived from the
integers); device side in csrc/kernels_tracks.hip behind tracks_device().
"""
import numpy as np

from .exception import XmhwException
from .gridweights import LAT_NAMES, LON_NAMES, quantise_weights, resolve_weights, weights_label
from .track_common import ChainDataset, Selection, device_stage, stage_inputs

EARTH_RADIUS_KM = 6371.0088
UNIT_BITS = 20
_SQRT3 = 3.0 ** 0.5
_INPUTS = dict(start=np.int32, end=np.int32, slot=np.int32, cell=np.int32, vec=np.int64, time_start=np.int32, offsets=np.int64)
_STAGE = dict(n_cells=np.int32, sums=(np.int64, 4))


def tracks_device(start, end, slot, cell, vec, time_start, offsets):
    """The device stage.  start / end (n,) int32 positions of every table row; slot (n,) int32, the position of the
    row's object in the selection or -1; cell (n,) int32, the row's compact cell; vec (4, C) int64, the addends of
    every cell; time_start (m,) int32 and offsets (m + 1,) int64 of the selection.  Returns ``n_cells`` (L,) int32 and
    ``sums`` (4, L) int64, L = offsets[-1]."""
    start, end, slot, cell, vec, time_start, offsets = a = stage_inputs(_INPUTS, start, end, slot, cell, vec, time_start, offsets)
    n, m, C = start.shape[0], time_start.shape[0], vec.shape[1]
    L = int(offsets[-1])
    if L == 0 or n == 0 or m == 0:
        return dict(n_cells=np.zeros(L, dtype=np.int32), sums=np.zeros((4, L), dtype=np.int64))
    with device_stage(a, (n, m, L + 1), f"mhw_tracks handles fewer than 2**31 rows, objects and series entries, got {n}, {m}, "
                      f"{L + 1}") as (h, s, (d_start, d_end, d_slot, d_cell, d_vec, d_ts, d_off), launch):
        with launch:
            d_cnt, d_sums, d_bad = s.alloc(4 * (L + 1)), s.alloc(8 * 4 * (L + 1)), s.alloc(4)
            h.object_tracks(d_start.ptr, d_end.ptr, n, d_slot.ptr, d_cell.ptr, C, d_vec.ptr, C, d_ts.ptr, d_off.ptr, m, L,
                            d_cnt.ptr, d_sums.ptr, L + 1, d_bad.ptr)
            h.stream_sync(0)
        cnt = d_cnt.to_array((L + 1,), np.int32)
        sums = d_sums.to_array((4, L + 1), np.int64)
        bad = int(d_bad.to_array((1,), np.int32)[0])
    if bad:
        raise XmhwException(f"{bad} table rows do not lie within their object's days: obj does not belong to mhw")
    if cnt[L] != 0 or sums[:, L].any():
        raise XmhwException("the series do not return to zero behind the last object: obj does not belong to mhw")
    return dict(n_cells=np.ascontiguousarray(cnt[:L]), sums=np.ascontiguousarray(sums[:, :L]))


class TrackDataset(ChainDataset):
    """What mhw_tracks() returns, as plain arrays.  m objects selected, L = offsets[-1] = the sum of their durations;
    entry offsets[i] + (t - time_start[i]) of a series belongs to object ids[i] on time position t.

    ids (m,) int32                  the objects, in the order asked for (all of them in ascending order for ids=None);
    offsets (m + 1,) int64          where each object's series starts; offsets[-1] == L;
    time_start, time_end, duration  (m,) int32, copied from the ObjectDataset;
    pos (L,) int32                  the time position of every entry;
    n_cells (L,) int32              cells of the object on that day;
    area_q (L,) int64, area         the sum of their quantised weights, and ``area_q * weight_unit`` (float64);
    mx, my, mz (L,) int64           the first moments sum wm * u (module docstring); mz is 0 in index mode;
    wsum (L,) int64                 index mode: sum wm; None in sphere mode;
    lat, lon (L,) float64           sphere mode: the centre, atan2(mz, hypot(mx, my)) and atan2(my, mx) in degrees,
                                    the longitude within [lon0, lon0 + 360), lon0 = -180 if the grid's longitude
                                    coordinate goes below 0, else 0; NaN where the moment vector is zero (a day on which
                                    every cell of the object has a moment weight of 0, or the vectors cancel); None
                                    in index mode;
    ci, cj (L,) float64             index mode: the centre in index units along sdims[0], sdims[1] (mx / wsum,
                                    my / wsum; NaN where wsum is 0); None in sphere mode;
    area_max_q (m,) int64, area_max the largest area_q of each object, and in the units of the weights;
    pos_area_max (m,) int32         the first time position that attains it;
    path_km (m,) float64            sphere mode: the sum of the great-circle distances between consecutive defined
                                    centres (Earth radius 6371.0088 km); None in index mode;
    mode "sphere" | "index", weight_bits, weight_unit, moment_bits (mb), n_ocean (C)."""

    def __init__(self, fields, time, sdims, sshape, mode, weight_bits, weight_unit, moment_bits, n_ocean, attrs=None):
        super().__init__(fields, time, sdims, sshape, attrs)
        self.mode, self.weight_bits, self.weight_unit = mode, int(weight_bits), float(weight_unit)
        self.moment_bits, self.n_ocean = int(moment_bits), int(n_ocean)

    _SERIES = ("pos", "n_cells", "area_q", "area", "mx", "my", "mz", "wsum", "lat", "lon", "ci", "cj")
    _PER_OBJECT = ("ids", "time_start", "time_end", "duration", "area_max_q", "area_max", "pos_area_max", "path_km")
    _ATTRS = ("mode", "weight_unit", "weight_bits", "moment_bits")

    def quantisation_bound(self):
        """(L,) float64: how far the centre computed from the integers can lie from the centre computed from the
        unquantised float64 weights and exact unit vectors, for every entry.  Derived, not fitted.

        Sphere mode, degrees of arc.  Write s = 2**mb / w.max().  The stored numbers are wm[c] = s w[c] + d[c] with
        |d[c]| <= 1/2 and u[c] = 2**20 e[c] + r[c] with e[c] the exact unit vector and |r[c]| <= sqrt(3)/2 (1/2 per
        component).  Then M = sum wm u = s 2**20 sum w e + E, the exact moment scaled plus
            E = sum (2**20 d[c] e[c] + s w[c] r[c] + d[c] r[c]),
            |E| <= n (2**19 + sqrt(3)/4) + (sqrt(3)/2) s sum w[c],
        n = n_cells.  s w[c] is known to within its own quantisation, s w[c] <= (wq[c] + 1/2) / 2**(weight_bits - mb),
        so s sum w <= (area_q + n/2) / 2**(weight_bits - mb) =: W and |E| <= B = n (2**19 + sqrt(3)/4) + (sqrt(3)/2) W.
        Two vectors that differ by E are at most asin(|E| / |longer one|) apart, and the exact one is at least
        |M| - B long: the bound is asin(B / (|M| - B)), in degrees, where |M| > 2 B, and 180 (no statement; such a
        centre is the near-cancellation of vectors all over the globe) elsewhere.  NaN where the centre is.

        Index mode, index units (the larger of the two dims).  With the indices exact, (sum wm i) / (sum wm) -
        (sum w i) / (sum w) = sum d[c] (i[c] - mean) / wsum, at most (n / 2) (max(ny, nx) - 1) / wsum."""
        n = self.n_cells.astype(np.float64)
        if self.mode == "index":
            with np.errstate(divide="ignore", invalid="ignore"):
                return np.where(self.wsum > 0, 0.5 * n * (max(self.sshape) - 1) / self.wsum.astype(np.float64), np.nan)
        W = (self.area_q.astype(np.float64) + 0.5 * n) / 2.0 ** (self.weight_bits - self.moment_bits)
        B = n * (2.0 ** (UNIT_BITS - 1) + _SQRT3 / 4) + (_SQRT3 / 2) * W
        M = np.sqrt(self.mx.astype(np.float64) ** 2 + self.my.astype(np.float64) ** 2 + self.mz.astype(np.float64) ** 2)
        ok = M > 2 * B
        out = np.full(M.shape, 180.0)
        out[ok] = np.degrees(np.arcsin(B[ok] / (M[ok] - B[ok])))
        out[np.isnan(self.lat)] = np.nan
        return out


def _latlon(coords, sdims):
    """(name of the latitude dim, name of the longitude dim) when the two spatial dims are those and ``coords`` holds
    both, else None"""
    lat = [d for d in sdims if d.lower() in LAT_NAMES]
    lon = [d for d in sdims if d.lower() in LON_NAMES]
    if len(lat) == 1 and len(lon) == 1 and lat[0] != lon[0] and lat[0] in coords and lon[0] in coords:
        return lat[0], lon[0]
    return None


def unit_vectors(coords, sdims, sshape, names):
    """(3, N) int64 in stacked order: rint(2**20 * (cos lat cos lon, cos lat sin lon, sin lat))"""
    lat = np.deg2rad(np.asarray(coords[names[0]], dtype=np.float64))
    lon = np.deg2rad(np.asarray(coords[names[1]], dtype=np.float64))
    if lat.shape != (sshape[sdims.index(names[0])],) or lon.shape != (sshape[sdims.index(names[1])],):
        raise XmhwException("the latitude and longitude coordinates should be 1-D along their dims")
    if not (np.isfinite(lat).all() and np.isfinite(lon).all() and np.abs(lat).max() <= np.pi / 2 + 1e-12):
        raise XmhwException("latitude should be within [-90, 90] degrees, and both coordinates finite")
    shape = [1, 1]
    shape[sdims.index(names[0])] = -1
    la = np.broadcast_to(lat.reshape(shape), sshape).reshape(-1)
    shape = [1, 1]
    shape[sdims.index(names[1])] = -1
    lo = np.broadcast_to(lon.reshape(shape), sshape).reshape(-1)
    one = float(1 << UNIT_BITS)
    return np.rint(one * np.stack([np.cos(la) * np.cos(lo), np.cos(la) * np.sin(lo), np.sin(la)])).astype(np.int64)


def moment_bits(weight_bits, n_ocean, index_extent=None):
    """mb of the module docstring; ``index_extent`` = max(ny, nx) in index mode"""
    ubits = UNIT_BITS if index_extent is None else int(index_extent).bit_length()
    return int(min(int(weight_bits), 61 - ubits - int(n_ocean).bit_length()))


def mhw_tracks(mhw, obj, ids=None, weights=None, _compute=None):
    """The daily series of the objects of mhw_objects(): cells, area and centre on every day of every object.

    ``mhw``: the EventDataset of detect(); ``obj``: the ObjectDataset mhw_objects() returned for it.  ``ids``: None
    for every object, or a 1-D integer array of distinct object ids; the result keeps their order.  ``weights``:
    None, "coslat" or an array on the spatial grid, as for mhw_objects(); give the same ones and the area series of
    an object sums to its ``area_days_q``.  They are quantised with ``obj.weight_bits``.

    Returns a TrackDataset (module docstring: the definition; class docstring: the fields).  Every series is a sum
    of integers: exact, and the same from run to run.  ``_compute``: a stand-in for tracks_device() (host tests)."""
    sel = Selection(mhw, obj, ids, "mhw_tracks")
    sshape = sel.sshape
    N = int(np.prod(sshape, dtype=np.int64))
    sdims = list(mhw.sdims)
    w = resolve_weights(weights, mhw.coords, sdims, None, sdims, sshape)
    sel.view()
    C, cell_index = sel.C, sel.cell_index
    names = _latlon(mhw.coords, sdims)
    mode = "sphere" if names else "index"
    if mode == "index" and obj.periodic is not None:
        raise XmhwException(f"the centre of an object on a grid that wraps along {obj.periodic!r} needs latitude and "
                            f"longitude coordinates for the dims {mhw.sdims}: a mean index across a wrapping dim means nothing")
    bits = obj.weight_bits
    mb = moment_bits(bits, C, None if names else max(sshape))
    if mb < 1:
        raise XmhwException(f"a grid of {sshape} with {C} ocean cells leaves no bits for the moment weights")
    wq, unit = quantise_weights(w, bits)
    wm, _ = quantise_weights(w, mb)
    if names:
        u = unit_vectors(mhw.coords, sdims, sshape, names)
        vec = np.stack([wq, wm * u[0], wm * u[1], wm * u[2]])[:, cell_index]
    else:
        i, j = np.divmod(np.arange(N, dtype=np.int64), sshape[1])
        vec = np.stack([wq, wm * i, wm * j, wm])[:, cell_index]
    sel.layout()
    L, offsets = sel.L, sel.offsets
    if L == 0:
        got = sel.no_entries(_STAGE)
    else:
        got = (_compute or tracks_device)(sel.start, sel.end, sel.slot, sel.cell_of_row, vec, sel.time_start, offsets)
    got = sel.stage_arrays(got, _STAGE, "tracks")
    sums = got["sums"]
    f = dict(sel.common_fields(), n_cells=got["n_cells"], area_q=sums[0], mx=sums[1], my=sums[2], pos=sel.pos())
    f["area"] = f["area_q"] * unit
    f.update(lat=None, lon=None, ci=None, cj=None, wsum=None, path_km=None)
    if names:
        f["mz"] = sums[3]
        x, y, z = (f[k].astype(np.float64) for k in ("mx", "my", "mz"))
        zero = (f["mx"] == 0) & (f["my"] == 0) & (f["mz"] == 0)
        lon_coord = np.asarray(mhw.coords[names[1]], dtype=np.float64)
        lon0 = -180.0 if lon_coord.size and lon_coord.min() < 0 else 0.0
        lat = np.degrees(np.arctan2(z, np.hypot(x, y)))
        lon = np.degrees(np.arctan2(y, x))
        lon = np.where(lon < lon0, lon + 360.0, lon)
        lon = np.where(lon >= lon0 + 360.0, lon - 360.0, lon)
        f["lat"], f["lon"] = np.where(zero, np.nan, lat), np.where(zero, np.nan, lon)
        f["path_km"] = _path_km(x, y, z, ~zero, offsets)
    else:
        f["mz"], f["wsum"] = np.zeros(L, dtype=np.int64), sums[3]
        with np.errstate(divide="ignore", invalid="ignore"):
            ws = f["wsum"].astype(np.float64)
            f["ci"] = np.where(ws > 0, f["mx"] / ws, np.nan)
            f["cj"] = np.where(ws > 0, f["my"] / ws, np.nan)
    f["area_max_q"], f["pos_area_max"] = sel.first_max(f["area_q"])
    f["area_max"] = f["area_max_q"] * unit
    attrs = {"weights": weights_label(weights)}
    return TrackDataset(f, mhw.time, mhw.sdims, sshape, mode, bits, unit, mb, C, attrs)


def _path_km(x, y, z, defined, offsets):
    """per object: the great-circle length of the polyline through its defined centres, in km"""
    m = offsets.shape[0] - 1
    owner = np.repeat(np.arange(m, dtype=np.int64), np.diff(offsets))
    k = np.nonzero(defined)[0]
    a, b = k[:-1], k[1:]
    same = owner[a] == owner[b]
    a, b = a[same], b[same]
    norm = np.sqrt(x * x + y * y + z * z)
    with np.errstate(divide="ignore", invalid="ignore"):
        ex, ey, ez = x / norm, y / norm, z / norm
    cx = ey[a] * ez[b] - ez[a] * ey[b]
    cy = ez[a] * ex[b] - ex[a] * ez[b]
    cz = ex[a] * ey[b] - ey[a] * ex[b]
    ang = np.arctan2(np.sqrt(cx * cx + cy * cy + cz * cz), ex[a] * ex[b] + ey[a] * ey[b] + ez[a] * ez[b])
    return np.bincount(owner[a], weights=ang, minlength=m) * EARTH_RADIUS_KM
