#!/usr/bin/env python3
"""mhw_tracks()'s device stage on the event tables of tools/bench_objects.py: one JSON line.

    python tools/bench_tracks.py [--cells 518400,1036800] [--years 40] [--reps 10] [--route-cells 4096] [--out FILE]

Per cell count and connectivity (6, 26; longitude wrapping) the objects come from mhw_objects()'s device stage on
the *scattered* table (the table-only detect() of a synthetic 40-year series: independent cells, small objects) and
on the *giant* table (the same rows per cell, every row in ONE object).  Timed with HIP events around the one C ABI
call xmhw_object_tracks (memsets + scatter + the scan's launches), median of --reps runs after a warm-up, everything
on the device, for two selections: every object (ids=None) and the objects of at least 100 cells.  Beside each time
its byte floor: the rows read once (16 B), the five difference arrays (36 B per entry) written once, read twice and
the series written once, at the 6.29 TB/s copy rate of DESIGN.md 5.  A selection whose L + 1 reaches 2**31, or whose
arrays do not fit --max-gib of device memory, is reported as such and not run.  After the timed runs the result is
downloaded once and its cell-days are checked against mhw_objects()'s.

The CPU route -- numpy add.at over the expanded voxels (tests/tracks_oracle.stage_voxels) -- is timed on the rows of
the first --route-cells cells of the first scattered table and SCALED per cell."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

HBM = 6.29e12
ENTRY_BYTES = 4 + 4 * 8


def selection(per, keep):
    """slot of every object (-1: not selected), time_start and offsets of the selected ones"""
    ids = np.nonzero(keep)[0]
    position = np.full(per["time_start"].shape[0], -1, dtype=np.int32)
    position[ids] = np.arange(ids.shape[0], dtype=np.int32)
    dur = per["time_end"][ids].astype(np.int64) - per["time_start"][ids] + 1
    return position, np.ascontiguousarray(per["time_start"][ids]), np.concatenate([[0], np.cumsum(dur)]).astype(np.int64), ids


def time_tracks(h, dev, median_ms, start, end, slot, cell, vec, t0, offsets, reps, max_bytes, cell_days):
    n, m, C, L = start.shape[0], t0.shape[0], vec.shape[1], int(offsets[-1])
    out = {"rows": int(n), "rows_selected": int((slot >= 0).sum()), "objects_selected": int(m), "L": L}
    need = ENTRY_BYTES * (L + 1) + 16 * n + 32 * C + 12 * m
    if m == 0:
        out["skipped"] = "no object in the selection"
        return out
    if L + 1 >= 1 << 31:
        out["skipped"] = "L + 1 >= 2**31: XMHW_ERR_UNSUPPORTED, select fewer objects"
        return out
    if need > max_bytes:
        out["skipped"] = f"{need / 2**30:.1f} GiB of device arrays, over the limit given"
        return out
    bufs = [dev.DeviceBuffer.from_array(np.ascontiguousarray(a)) for a in (start, end, slot, cell, vec, t0, offsets)]
    try:
        d_cnt, d_sums, d_bad = dev.DeviceBuffer(4 * (L + 1)), dev.DeviceBuffer(32 * (L + 1)), dev.DeviceBuffer(4)
        bufs += [d_cnt, d_sums, d_bad]
        ptr = [b.ptr for b in bufs]
        ms, every = median_ms(h, lambda: h.object_tracks(ptr[0], ptr[1], n, ptr[2], ptr[3], C, ptr[4], C, ptr[5], ptr[6], m, L,
                                                         d_cnt.ptr, d_sums.ptr, L + 1, d_bad.ptr), reps)
        cnt = d_cnt.to_array((L + 1,), np.int32)
        assert cnt[L] == 0 and int(d_bad.to_array((1,), np.int32)[0]) == 0
        assert int(cnt.sum(dtype=np.int64)) == int(cell_days)
        floor = (16 * n + 4 * ENTRY_BYTES * (L + 1)) / HBM * 1e3
        out.update(object_tracks_ms=round(ms, 3), object_tracks_ms_all=every, floor_ms=round(floor, 4),
                   over_floor=round(ms / floor, 1), ns_per_selected_row=round(ms * 1e6 / max(out["rows_selected"], 1), 3),
                   ns_per_entry=round(ms * 1e6 / L, 3), cell_days_match=True)
        return out
    finally:
        for b in bufs:
            b.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", default="518400,1036800")
    ap.add_argument("--years", type=int, default=40)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--route-cells", type=int, default=4096)
    ap.add_argument("--min-cells", type=int, default=100)
    ap.add_argument("--max-gib", type=float, default=64.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import tracks_oracle as to
    import xmhw_amd.device as dev
    from bench_objects import detect_table, giant_table, grid_of, median_ms
    from xmhw_amd._lib import hip, require_gpu
    from xmhw_amd.calendar import add_doy
    from xmhw_amd.coverage import quantise_weights
    from xmhw_amd.detect_front import _check_inputs
    from xmhw_amd.objects import neighbour_table, objects_device
    from xmhw_amd.tracks import moment_bits, unit_vectors
    require_gpu()
    h = hip()
    t = np.arange("1982-01-01", f"{1982 + a.years}-01-01", dtype="datetime64[D]")
    doy = add_doy(t)
    T = t.shape[0]
    plan = dev.Plan(doy, 5)
    _, _, _, rows = _check_inputs(np.zeros((T, 1), np.float32), np.zeros((plan.D, 1)), np.zeros((plan.D, 1)), doy, np.unique(doy))
    res = {"bench": "mhw_tracks", "T": int(T), "hbm_bytes_per_s": HBM, "reps": a.reps, "tile": int(h.TRACKS_TILE),
           "min_cells": a.min_cells, "cases": []}
    first = None
    for C in [int(c) for c in a.cells.split(",")]:
        grid = grid_of(C)
        start, end, imax, offsets = detect_table(h, dev, C, T, plan, rows)
        if first is None:
            first = (start, end, offsets)
        n = start.shape[0]
        coords = {"lat": np.linspace(-89.875, 89.875, grid[0]), "lon": np.arange(grid[1]) * 360.0 / grid[1]}
        w = np.repeat(np.cos(np.deg2rad(coords["lat"])), grid[1])
        mb = moment_bits(31, C)
        wq, wm = quantise_weights(w, 31)[0], quantise_weights(w, mb)[0]
        u = unit_vectors(coords, ["lat", "lon"], grid, ("lat", "lon"))
        vec = np.stack([wq, wm * u[0], wm * u[1], wm * u[2]])
        case = {"cells": C, "grid": list(grid), "periodic": "lon", "moment_bits": mb}
        per_cell = max(1, int(round(n / C)))
        gs, ge, gi, go = giant_table(C, grid, per_cell)
        for conn in (6, 26):
            nbr = neighbour_table(np.arange(C), grid, conn, 1)
            gap = 0 if conn == 6 else 1
            entry = {}
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
                    entry[name][sel] = time_tracks(h, dev, median_ms, s, e, position[object_of_row], cell, vec, t0, offs, a.reps,
                                                   a.max_gib * 2**30, per["cell_days"][ids].sum())
                del per, object_of_row
            sc, gt = entry["scattered"]["all"], entry["giant"]["all"]
            if "object_tracks_ms" in sc and "object_tracks_ms" in gt:
                entry["giant_over_scattered_per_row"] = round(gt["ns_per_selected_row"] / sc["ns_per_selected_row"], 2)
            case[f"connectivity_{conn}"] = entry
        res["cases"].append(case)
        print(case, file=sys.stderr, flush=True)

    # the CPU route on the rows of a few cells, every cell its own object's worth of days, scaled per cell
    start, end, offsets = first
    nc = a.route_cells
    nr = int(offsets[nc])
    s, e = start[:nr], end[:nr]
    cell = np.repeat(np.arange(nc, dtype=np.int32), np.diff(offsets[:nc + 1]))
    slot = np.arange(nr, dtype=np.int32)                             # one object per row: L = the voxels of these rows
    offs = np.concatenate([[0], np.cumsum(e.astype(np.int64) - s + 1)])
    vec = np.ones((4, nc), dtype=np.int64)
    t0 = time.perf_counter()
    got = to.stage_voxels(s, e, slot, cell, vec, s, offs)
    t_cpu = time.perf_counter() - t0
    assert got["n_cells"].min() == 1 == got["n_cells"].max()
    res["cpu_route"] = {"how": "numpy add.at over the expanded voxels (tests/tracks_oracle.stage_voxels)", "cells": nc, "rows": nr,
                        "voxels": int(offs[-1]), "seconds": round(t_cpu, 3)}
    for c in res["cases"]:
        scaled = t_cpu * c["cells"] / nc
        c["cpu_route_scaled_s"] = round(scaled, 1)
        sc = c["connectivity_6"]["scattered"]["all"]
        if "object_tracks_ms" in sc:
            c["cpu_route_scaled_over_device_stage"] = round(scaled * 1e3 / sc["object_tracks_ms"], 0)
    plan.destroy()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
