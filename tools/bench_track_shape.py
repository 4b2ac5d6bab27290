#!/usr/bin/env python3
"""mhw_track_shape()'s device stage on the event tables of tools/bench_objects.py, beside mhw_track_parts()'s on the same
table and selection in the same run: one JSON line.

    python tools/bench_track_shape.py [--cells 518400,1036800] [--connectivity 6,26] [--years 40] [--reps 10] [--out FILE]

The tables, the objects and the two selections are those of tools/bench_track_parts.py: per cell count and
connectivity (6, 26; longitude wrapping) the objects come from mhw_objects()'s device stage on the *scattered* table
(the table-only detect() of a synthetic 40-year series: independent cells, small objects) and on the *giant* table
(the same rows per cell, every row in ONE object); selected are every object and the objects of at least --min-cells
cells.  Timed with HIP events around the one C ABI call xmhw_object_shape (four memsets + one launch), median of --reps
runs after a warm-up, everything on the device; faces of length 1.  Beside each time its byte floor -- the rows read
once (16 B), the face table and the lengths read once (48 B per cell), 40 B per entry written, at the copy rate of
DESIGN.md 5 -- and the time of xmhw_object_parts measured by tools/bench_track_parts.time_parts on the same arrays
(4 neighbours for connectivity 6, 8 for 26, as mhw_track_parts() takes them).  After the timed runs the result is
downloaded once: no row was left out, every entry has at least 2 exposed faces (the grid wraps along one dim), and no
day has more edge cells than mhw_objects() counted cells for the object."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

HBM = 6.29e12
ENTRY_BYTES, ROW_BYTES, CELL_BYTES = 40, 16, 48


def time_shape(h, dev, median_ms, start, end, slot, cell, row_offsets, faces, lq, t0, offsets, reps, max_bytes, n_cells_of_slot):
    n, m, C, L = start.shape[0], t0.shape[0], faces.shape[0], int(offsets[-1])
    out = {"rows": int(n), "rows_selected": int((slot >= 0).sum()), "objects_selected": int(m), "L": L}
    need = ENTRY_BYTES * L + ROW_BYTES * n + (8 + CELL_BYTES) * C + 12 * m
    if m == 0:
        out["skipped"] = "no object in the selection"
        return out
    if L >= 1 << 31:
        out["skipped"] = "2**31 entries and more: XMHW_ERR_UNSUPPORTED, select fewer objects"
        return out
    if need > max_bytes:
        out["skipped"] = f"{need / 2**30:.1f} GiB of device arrays, over the limit given"
        return out
    bufs = [dev.DeviceBuffer.from_array(np.ascontiguousarray(a)) for a in (start, end, slot, cell, row_offsets, faces, lq, t0, offsets)]
    try:
        d_edges, d_perim, d_cells, d_bad = (dev.DeviceBuffer(12 * L), dev.DeviceBuffer(24 * L), dev.DeviceBuffer(4 * L),
                                            dev.DeviceBuffer(4))
        bufs += [d_edges, d_perim, d_cells, d_bad]
        p = [b.ptr for b in bufs]
        ms, every = median_ms(h, lambda: h.object_shape(p[0], p[1], p[2], p[3], n, p[4], C, p[5], 4, p[6], p[7], p[8], m, L,
                                                        d_edges.ptr, d_perim.ptr, d_cells.ptr, d_bad.ptr), reps)
        edges, cells_edge = d_edges.to_array((3, L), np.int32), d_cells.to_array((L,), np.int32)
        exposed = edges.sum(axis=0, dtype=np.int64)
        assert int(d_bad.to_array((1,), np.int32)[0]) == 0 and exposed.min() >= 2 and cells_edge.min() >= 1
        assert (np.maximum.reduceat(cells_edge, offsets[:-1]) <= n_cells_of_slot).all()
        perim = d_perim.to_array((3, L), np.int64)
        assert (perim == edges.astype(np.int64) * int(lq.max())).all()
        days = np.where(slot >= 0, end.astype(np.int64) - start + 1, 0)
        floor = (ROW_BYTES * n + CELL_BYTES * C + ENTRY_BYTES * L) / HBM * 1e3
        out.update(object_shape_ms=round(ms, 3), object_shape_ms_all=every, floor_ms=round(floor, 4),
                   over_floor=round(ms / floor, 1), row_days=int(days.sum()), ns_per_row_day=round(ms * 1e6 / max(int(days.sum()), 1), 4),
                   longest_row_days=int(days.max()), edges_exposed=int(exposed.sum()), edges_open=int(edges[0].sum(dtype=np.int64)),
                   edges_border=int(edges[2].sum(dtype=np.int64)), cell_days_on_the_edge=int(cells_edge.sum(dtype=np.int64)),
                   checks_pass=True)
        return out
    finally:
        for b in bufs:
            b.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", default="518400,1036800")
    ap.add_argument("--connectivity", default="6,26")
    ap.add_argument("--years", type=int, default=40)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--min-cells", type=int, default=100)
    ap.add_argument("--max-gib", type=float, default=64.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import xmhw_amd.device as dev
    from bench_objects import detect_table, giant_table, grid_of, median_ms
    from bench_track_parts import time_parts
    from bench_tracks import selection
    from xmhw_amd._lib import hip, require_gpu
    from xmhw_amd.calendar import add_doy
    from xmhw_amd.coverage import quantise_weights
    from xmhw_amd.detect_front import _check_inputs
    from xmhw_amd.objects import neighbour_table, objects_device
    from xmhw_amd.track_shape import face_table, length_bits
    require_gpu()
    h = hip()
    t = np.arange("1982-01-01", f"{1982 + a.years}-01-01", dtype="datetime64[D]")
    doy = add_doy(t)
    T = t.shape[0]
    plan = dev.Plan(doy, 5)
    _, _, _, rows = _check_inputs(np.zeros((T, 1), np.float32), np.zeros((plan.D, 1)), np.zeros((plan.D, 1)), doy, np.unique(doy))
    res = {"bench": "mhw_track_shape", "T": int(T), "hbm_bytes_per_s": HBM, "reps": a.reps, "entry_bytes": ENTRY_BYTES,
           "min_cells": a.min_cells, "cases": []}
    for C in [int(c) for c in a.cells.split(",")]:
        grid = grid_of(C)
        start, end, imax, offsets = detect_table(h, dev, C, T, plan, rows)
        n = start.shape[0]
        w = np.repeat(np.cos(np.deg2rad(np.linspace(-89.875, 89.875, grid[0]))), grid[1])
        wq = quantise_weights(w, 31)[0]
        faces = face_table(np.arange(C), grid, 1)
        lq = np.full((C, 4), 1 << length_bits(C), dtype=np.int64)
        case = {"cells": C, "grid": list(grid), "periodic": "lon", "length_bits": length_bits(C)}
        per_cell = max(1, int(round(n / C)))
        gs, ge, gi, go = giant_table(C, grid, per_cell)
        for conn in [int(c) for c in a.connectivity.split(",")]:
            nbr = neighbour_table(np.arange(C), grid, conn, 1)
            gap = 0 if conn == 6 else 1
            entry = {"parts_neighbours": int(nbr.shape[1])}
            for name, (s, e, im, off) in (("scattered", (start, end, imax, offsets)), ("giant", (gs, ge, gi, go))):
                per = objects_device(s, e, im, off, nbr, gap, wq)
                roots = np.nonzero(per["root"] == np.arange(s.shape[0], dtype=np.int32))[0]
                lut = np.empty(s.shape[0], dtype=np.int32)
                lut[roots] = np.arange(roots.shape[0], dtype=np.int32)
                object_of_row = lut[per["root"]]
                cell = np.repeat(np.arange(C, dtype=np.int32), np.diff(off))
                entry[name] = {"objects": int(roots.shape[0]), "largest_object_cells": int(per["n_cells"].max())}
                for sel, keep in (("all", np.ones(roots.shape[0], bool)), ("large", per["n_cells"] >= a.min_cells)):
                    position, t0, offs, ids = selection(per, keep)
                    slot = position[object_of_row]
                    got = time_shape(h, dev, median_ms, s, e, slot, cell, off, faces, lq, t0, offs, a.reps, a.max_gib * 2**30,
                                     per["n_cells"][ids])
                    parts = time_parts(h, dev, median_ms, s, e, slot, cell, off, nbr, wq, t0, offs, a.reps, a.max_gib * 2**30,
                                       per["n_cells"][ids])
                    got["object_parts"] = {k: parts[k] for k in ("voxels", "object_parts_ms", "object_parts_ms_all", "skipped")
                                           if k in parts}
                    if "object_shape_ms" in got and "object_parts_ms" in parts:
                        got["shape_over_parts"] = round(got["object_shape_ms"] / parts["object_parts_ms"], 3)
                    entry[name][sel] = got
                del per, object_of_row
            case[f"connectivity_{conn}"] = entry
        res["cases"].append(case)
        print(case, file=sys.stderr, flush=True)
    plan.destroy()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
