#!/usr/bin/env python3
"""mhw_track_genealogy()'s device stage on the event tables of tools/bench_objects.py: one JSON line.

    python tools/bench_track_genealogy.py [--cells 518400,1036800] [--years 40] [--reps 10] [--out FILE]

The tables, the objects and the two selections are those of tools/bench_track_parts.py: per cell count and
connectivity (6, 26; longitude wrapping) the *scattered* table (the table-only detect() of a synthetic 40-year series:
independent cells, small objects) and the *giant* table (the same rows per cell, every row in ONE object: every
footprint one large part, every lane of a day step on one key of the hash set), every object and the objects of at
least --min-cells cells, parts under 4 neighbours for connectivity 6 and 8 for 26.  Timed with HIP events around the
one C ABI call xmhw_object_genealogy (memsets + init + link + flatten + pairs + collect + count), median of --reps
runs after a warm-up, everything on the device.  Beside each time its byte floor: the rows read once (16 B), 12 B per
voxel and 8 B per slot of the hash set written and read, 24 B per entry and 8 B per edge written, at the copy rate of
DESIGN.md 5.  A selection whose voxels reach 2**31, or whose arrays do not fit --max-gib of device memory, is reported
as such and not run.  After the timed runs the result is downloaded once: no row was left out, the set did not
overflow, every entry holds at least one part, the links of all entries number the edges, and the first day of every
object has no link."""
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
VOXEL_BYTES, SLOT_BYTES, ENTRY_BYTES, EDGE_BYTES, ROW_BYTES = 12, 8, 24, 8, 16


def time_genealogy(h, dev, median_ms, start, end, slot, cell, row_offsets, nbr, t0, offsets, reps, max_bytes):
    from xmhw_amd.track_genealogy import edge_capacity, table_slots
    n, m, C, L = start.shape[0], t0.shape[0], row_offsets.shape[0] - 1, int(offsets[-1])
    days = np.where(slot >= 0, end.astype(np.int64) - start + 1, 0)
    vox_off = np.concatenate([[0], np.cumsum(days)]).astype(np.int64)
    V = int(vox_off[-1])
    cap = edge_capacity(start, end, slot, cell)
    slots = table_slots(cap)
    out = {"rows": int(n), "rows_selected": int((slot >= 0).sum()), "objects_selected": int(m), "L": L, "voxels": V,
           "edge_capacity": int(cap), "table_slots": int(slots)}
    need = VOXEL_BYTES * V + SLOT_BYTES * slots + ENTRY_BYTES * L + EDGE_BYTES * cap + 24 * n + (8 + 4 * nbr.shape[1]) * C + 12 * m
    if m == 0:
        out["skipped"] = "no object in the selection"
        return out
    if max(V, L) >= 1 << 31:
        out["skipped"] = "2**31 voxels or entries and more: XMHW_ERR_UNSUPPORTED, select fewer objects"
        return out
    if need > max_bytes:
        out["skipped"] = f"{need / 2**30:.1f} GiB of device arrays, over the limit given"
        return out
    bufs = [dev.DeviceBuffer.from_array(np.ascontiguousarray(a)) for a in (start, end, slot, cell, row_offsets, nbr, vox_off, t0, offsets)]
    try:
        d_counts, d_edges = dev.DeviceBuffer(4 * 6 * L), dev.DeviceBuffer(8 * max(cap, 1))
        d_ne, d_bad, d_over = dev.DeviceBuffer(8), dev.DeviceBuffer(4), dev.DeviceBuffer(4)
        bufs += [d_counts, d_edges, d_ne, d_bad, d_over]
        p = [b.ptr for b in bufs]
        ms, every = median_ms(h, lambda: h.object_genealogy(p[0], p[1], p[2], p[3], n, p[4], C, p[5], nbr.shape[1], p[6], V, p[7], p[8],
                                                            m, L, d_counts.ptr, d_edges.ptr, cap, d_ne.ptr, d_bad.ptr, d_over.ptr), reps)
        counts = d_counts.to_array((6, L), np.int32)
        E = int(d_ne.to_array((1,), np.int64)[0])
        assert int(d_bad.to_array((1,), np.int32)[0]) == 0 and int(d_over.to_array((1,), np.int32)[0]) == 0
        assert counts[0].min() >= 1 and int(counts[1].sum(dtype=np.int64)) == E <= cap and (counts[1][offsets[:-1]] == 0).all()
        floor = (ROW_BYTES * n + 2 * VOXEL_BYTES * V + 2 * SLOT_BYTES * slots + ENTRY_BYTES * L + EDGE_BYTES * E) / HBM * 1e3
        out.update(object_genealogy_ms=round(ms, 3), object_genealogy_ms_all=every, floor_ms=round(floor, 4),
                   over_floor=round(ms / floor, 1), ns_per_voxel=round(ms * 1e6 / max(V, 1), 3), edges=E,
                   keys_per_edge=round(cap / max(E, 1), 2), n_parts_max=int(counts[0].max()),
                   parts_merged=int(counts[3].sum(dtype=np.int64)), parts_split=int(counts[5].sum(dtype=np.int64)), checks_pass=True)
        return out
    finally:
        for b in bufs:
            b.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", default="518400,1036800")
    ap.add_argument("--years", type=int, default=40)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--min-cells", type=int, default=100)
    ap.add_argument("--max-gib", type=float, default=64.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import xmhw_amd.device as dev
    from bench_objects import detect_table, giant_table, grid_of, median_ms
    from bench_tracks import selection
    from xmhw_amd._lib import hip, require_gpu
    from xmhw_amd.calendar import add_doy
    from xmhw_amd.coverage import quantise_weights
    from xmhw_amd.detect_front import _check_inputs
    from xmhw_amd.objects import neighbour_table, objects_device
    require_gpu()
    h = hip()
    t = np.arange("1982-01-01", f"{1982 + a.years}-01-01", dtype="datetime64[D]")
    doy = add_doy(t)
    T = t.shape[0]
    plan = dev.Plan(doy, 5)
    _, _, _, rows = _check_inputs(np.zeros((T, 1), np.float32), np.zeros((plan.D, 1)), np.zeros((plan.D, 1)), doy, np.unique(doy))
    res = {"bench": "mhw_track_genealogy", "T": int(T), "hbm_bytes_per_s": HBM, "reps": a.reps,
           "voxel_bytes": int(h.GENEALOGY_VOXEL_BYTES), "slot_bytes": int(h.GENEALOGY_SLOT_BYTES), "min_cells": a.min_cells, "cases": []}
    for C in [int(c) for c in a.cells.split(",")]:
        grid = grid_of(C)
        start, end, imax, offsets = detect_table(h, dev, C, T, plan, rows)
        n = start.shape[0]
        w = np.repeat(np.cos(np.deg2rad(np.linspace(-89.875, 89.875, grid[0]))), grid[1])
        wq = quantise_weights(w, 31)[0]
        case = {"cells": C, "grid": list(grid), "periodic": "lon"}
        per_cell = max(1, int(round(n / C)))
        gs, ge, gi, go = giant_table(C, grid, per_cell)
        for conn in (6, 26):
            nbr = neighbour_table(np.arange(C), grid, conn, 1)
            gap = 0 if conn == 6 else 1
            entry = {"neighbours": int(nbr.shape[1])}
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
                    entry[name][sel] = time_genealogy(h, dev, median_ms, s, e, position[object_of_row], cell, off, nbr, t0, offs,
                                                      a.reps, a.max_gib * 2**30)
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
