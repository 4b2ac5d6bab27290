#!/usr/bin/env python3
"""mhw_track_parts()'s device stage on the event tables of tools/bench_objects.py: one JSON line.

    python tools/bench_track_parts.py [--cells 518400,1036800] [--years 40] [--reps 10] [--out FILE]

Per cell count and connectivity (6, 26; longitude wrapping) the objects come from mhw_objects()'s device stage on
the *scattered* table (the table-only detect() of a synthetic 40-year series: independent cells, small objects) and
on the *giant* table (the same rows per cell, every row in ONE object).  Timed with HIP events around the one C ABI
call xmhw_object_parts (memset + init + link + flatten + reduce + count), median of --reps runs after a warm-up,
everything on the device, for two selections: every object (ids=None) and the objects of at least --min-cells cells;
the parts use 4 neighbours for connectivity 6 and 8 for 26, as mhw_track_parts() does by default.  Beside each time
its byte floor: the rows read once (16 B), 16 B per voxel written and read, 16 B per entry written, at the copy rate
of DESIGN.md 5.  A selection whose voxels reach 2**31, or whose arrays do not fit --max-gib of device memory, is
reported as such and not run.  After the timed runs the result is downloaded once: no row was left out, every entry
holds at least one part, and no largest part is larger than mhw_objects()'s cell count of its object."""
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
VOXEL_BYTES, ENTRY_BYTES, ROW_BYTES = 16, 16, 16


def time_parts(h, dev, median_ms, start, end, slot, cell, row_offsets, nbr, wq, t0, offsets, reps, max_bytes, n_cells_of_slot):
    n, m, C, L = start.shape[0], t0.shape[0], wq.shape[0], int(offsets[-1])
    days = np.where(slot >= 0, end.astype(np.int64) - start + 1, 0)
    vox_off = np.concatenate([[0], np.cumsum(days)]).astype(np.int64)
    V = int(vox_off[-1])
    out = {"rows": int(n), "rows_selected": int((slot >= 0).sum()), "objects_selected": int(m), "L": L, "voxels": V}
    need = VOXEL_BYTES * V + ENTRY_BYTES * L + 24 * n + (8 + 8 + 4 * nbr.shape[1]) * C + 12 * m
    if m == 0:
        out["skipped"] = "no object in the selection"
        return out
    if max(V, L) >= 1 << 31:
        out["skipped"] = "2**31 voxels or entries and more: XMHW_ERR_UNSUPPORTED, select fewer objects"
        return out
    if need > max_bytes:
        out["skipped"] = f"{need / 2**30:.1f} GiB of device arrays, over the limit given"
        return out
    bufs = [dev.DeviceBuffer.from_array(np.ascontiguousarray(a)) for a in (start, end, slot, cell, row_offsets, nbr, wq, vox_off, t0,
                                                                           offsets)]
    try:
        d_np, d_cl, d_al, d_bad = dev.DeviceBuffer(4 * L), dev.DeviceBuffer(4 * L), dev.DeviceBuffer(8 * L), dev.DeviceBuffer(4)
        bufs += [d_np, d_cl, d_al, d_bad]
        p = [b.ptr for b in bufs]
        ms, every = median_ms(h, lambda: h.object_parts(p[0], p[1], p[2], p[3], n, p[4], C, p[5], nbr.shape[1], p[6], p[7], V, p[8],
                                                        p[9], m, L, d_np.ptr, d_cl.ptr, d_al.ptr, d_bad.ptr), reps)
        n_parts, largest = d_np.to_array((L,), np.int32), d_cl.to_array((L,), np.int32)
        assert int(d_bad.to_array((1,), np.int32)[0]) == 0 and n_parts.min() >= 1
        assert (np.maximum.reduceat(largest, offsets[:-1]) <= n_cells_of_slot).all()
        floor = (ROW_BYTES * n + 2 * VOXEL_BYTES * V + ENTRY_BYTES * L) / HBM * 1e3
        out.update(object_parts_ms=round(ms, 3), object_parts_ms_all=every, floor_ms=round(floor, 4),
                   over_floor=round(ms / floor, 1), ns_per_voxel=round(ms * 1e6 / max(V, 1), 3),
                   n_parts_max=int(n_parts.max()), entries_split=int((n_parts > 1).sum()), checks_pass=True)
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
    res = {"bench": "mhw_track_parts", "T": int(T), "hbm_bytes_per_s": HBM, "reps": a.reps, "voxel_bytes": int(h.PARTS_VOXEL_BYTES),
           "min_cells": a.min_cells, "cases": []}
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
                    entry[name][sel] = time_parts(h, dev, median_ms, s, e, position[object_of_row], cell, off, nbr, wq, t0, offs,
                                                  a.reps, a.max_gib * 2**30, per["n_cells"][ids])
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
