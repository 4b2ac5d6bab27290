#!/usr/bin/env python3
"""mhw_track_intensity()'s device stage on the event tables of tools/bench_objects.py with their series: one JSON line.

    python tools/bench_track_intensity.py [--cells 518400,1036800] [--years 40] [--reps 10] [--route-cells 4096] [--out FILE]

Per cell count the synthetic 40-year float32 series stays on the device with its raw climatology; the *scattered* table
is the table-only detect() of that series grouped by mhw_objects()'s device stage (connectivity 6, longitude wrapping:
independent cells, small objects), the *giant* table holds the same number of rows per cell, every row in ONE object.
Every object is selected.  Timed with HIP events around the C ABI calls xmhw_track_intensity_init / _accumulate_f32 /
_finish, one slab, median of --reps runs after a warm-up, with the runs of equal entries combined in the wave and
without.  Beside each time its byte floor at the 6.29 TB/s copy rate of DESIGN.md 5: the series read once (4 B per
sample), the seas / thresh rows of the in-event steps (16 B per voxel), the row arrays (12 B per row, 16 B per cell) and
the accumulators (44 B per entry, written by the init and read and written once more).  After the timed runs n_valid is
downloaded once and its sum is checked against the voxels of the selected rows (the synthetic series holds no NaN).

The CPU route -- numpy add.at / maximum.at over the expanded voxels -- is timed on the first --route-cells cells of the
first scattered table, every row its own object, and SCALED per cell."""
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
ENTRY_BYTES = 4 + 8 + 8 + 8 + 16


def series_and_table(h, dev, C, T, plan, rows, keep):
    """the synthetic series and its raw climatology on the device (appended to ``keep``), and (start, end, imax, offsets)
    of the table-only detect() device stage on them"""
    D = plan.D
    W = (T + 63) // 64
    d_ts, d_th, d_se = dev.DeviceBuffer(4 * T * C), dev.DeviceBuffer(8 * D * C), dev.DeviceBuffer(8 * D * C)
    keep += [d_ts, d_th, d_se]
    h.synth_sst(d_ts.ptr, 4, T, C, C, 0, 7, 0.0)
    dev.clim_raw(plan, d_ts, 4, C, 0.9, False, d_th, d_se)
    bufs = []
    try:
        d_bits, d_n, d_off = dev.DeviceBuffer(8 * W * C), dev.DeviceBuffer(4 * C), dev.DeviceBuffer(8 * (C + 1))
        bufs += [d_bits, d_n, d_off]
        h.exceed_bits(d_ts.ptr, 4, T, C, C, d_th.ptr, C, D, rows, 0, d_bits.ptr, C)
        h.events_from_bits(d_bits.ptr, T, C, C, 5, 1, 2, 0, d_n.ptr, 0)
        h.offsets_from_counts(d_n.ptr, C, d_off.ptr)
        h.stream_sync(0)
        offsets = d_off.to_array((C + 1,), np.int64)
        n = int(offsets[-1])
        ncol = h.EVENT_COLUMNS
        d_tab = dev.DeviceBuffer(8 * max(n, 1) * ncol)
        bufs.append(d_tab)
        h.events_from_bits(d_bits.ptr, T, C, C, 5, 1, 2, d_off.ptr, 0, d_tab.ptr)
        h.event_stats_sparse(d_ts.ptr, 4, T, C, C, d_se.ptr, d_th.ptr, C, rows, 0, n, d_tab.ptr)
        h.stream_sync(0)
        start, end, imax = np.empty(n, np.int32), np.empty(n, np.int32), np.empty(n, np.float64)
        step = 1 << 20
        chunk = np.empty((step, ncol), dtype=np.float64)
        for r0 in range(0, n, step):
            m = min(step, n - r0)
            h.memcpy_d2h(chunk[:m], d_tab.ptr + 8 * ncol * r0)
            start[r0:r0 + m], end[r0:r0 + m], imax[r0:r0 + m] = chunk[:m, 1], chunk[:m, 2], chunk[:m, 6]
        return d_ts, d_th, d_se, start, end, imax, offsets
    finally:
        for b in bufs:
            b.free()


def time_stage(h, dev, median_ms, d_ts, d_th, d_se, T, C, D, rows, start, end, slot, offsets_rows, wi, t0, offs, reps, max_bytes):
    n, m, L = start.shape[0], t0.shape[0], int(offs[-1])
    voxels = int((end.astype(np.int64) - start + 1)[slot >= 0].sum())
    out = {"rows": int(n), "objects": int(m), "L": L, "voxels": voxels}
    if L >= 1 << 31 or ENTRY_BYTES * L + 12 * n > max_bytes:
        out["skipped"] = f"L = {L}: 2**31 entries and more, or {ENTRY_BYTES * L / 2**30:.1f} GiB of accumulators over the limit given"
        return out
    bufs = [dev.DeviceBuffer.from_array(np.ascontiguousarray(a)) for a in (start, end, slot, offsets_rows, wi, t0, offs)]
    try:
        acc = [dev.DeviceBuffer(k * L) for k in (4, 8, 8, 8, 16)] + [dev.DeviceBuffer(16)]
        bufs += acc
        p = [b.ptr for b in bufs]
        o = (acc[0].ptr, acc[1].ptr, acc[2].ptr, acc[3].ptr, acc[4].ptr, L, acc[5].ptr, acc[5].ptr + 8)
        floor = (4 * T * C + 16 * voxels + 12 * n + 16 * C + 3 * ENTRY_BYTES * L) / HBM * 1e3
        out["floor_ms"] = round(floor, 3)
        out["floor_series_only_ms"] = round(4 * T * C / HBM * 1e3, 3)
        ms, every = median_ms(h, lambda: h.track_intensity_init(L, *o), reps)
        out.update(init_ms=round(ms, 3))
        for combine in (1, 0):
            h.set_track_intensity_combine(combine)
            try:
                h.track_intensity_init(L, *o)
                # a timed run ADDS into the accumulators: values pile up over the runs, the work per run is the same
                ms, every = median_ms(h, lambda: h.track_intensity_accumulate(
                    d_ts.ptr, 4, T, C, C, d_se.ptr, d_th.ptr, C, D, rows, 0, p[0], p[1], p[2], n, p[3], p[4], p[5], p[6], m, L, *o),
                    reps)
            finally:
                h.set_track_intensity_combine(1)
            key = "accumulate_ms" if combine else "accumulate_uncombined_ms"
            out.update({key: round(ms, 3), key + "_all": every})
            if combine:
                out.update(over_floor=round(ms / floor, 2), series_GBps=round(4 * T * C / ms / 1e6, 1),
                           ns_per_voxel=round(ms * 1e6 / max(voxels, 1), 4))
        h.track_intensity_init(L, *o)
        h.track_intensity_accumulate(d_ts.ptr, 4, T, C, C, d_se.ptr, d_th.ptr, C, D, rows, 0, p[0], p[1], p[2], n, p[3], p[4],
                                     p[5], p[6], m, L, *o)
        ms, every = median_ms(h, lambda: h.track_intensity_finish(L, acc[3].ptr), reps)
        out.update(finish_ms=round(ms, 3))
        h.stream_sync(0)
        count = acc[5].to_array((2,), np.int64)
        assert count[0] == 0 and count[1] == 0, count
        assert int(acc[0].to_array((L,), np.int32).sum(dtype=np.int64)) == voxels
        out["n_valid_matches_voxels"] = True
        return out
    finally:
        for b in bufs:
            b.free()


def numpy_route(ts, seas, thresh, row_of_t, start, end, cell, wi):
    """every row its own object: the expanded voxels reduced with add.at / maximum.at"""
    d = end.astype(np.int64) - start + 1
    offs = np.concatenate([[0], np.cumsum(d)])
    r = np.repeat(np.arange(start.shape[0]), d)
    day = np.arange(int(offs[-1]), dtype=np.int64) - np.repeat(offs[:-1], d) + start[r]
    c = cell[r]
    entry = offs[r] + (day - start[r])                             # offsets[slot] + (t - time_start[slot])
    k = row_of_t[day]
    x = ts[day, c].astype(np.float64)
    se, th = seas[k, c], thresh[k, c]
    a = x - se
    L = int(offs[-1])
    n_valid, wsum, isum = np.zeros(L, np.int32), np.zeros(L, np.int64), np.zeros(L, np.int64)
    imax = np.full(L, -np.inf)
    ok = ~np.isnan(a)
    np.add.at(n_valid, entry[ok], 1)
    np.add.at(wsum, entry[ok], wi[c[ok]])
    np.add.at(isum, entry[ok], wi[c[ok]] * np.rint(a[ok] * 65536.0).astype(np.int64))
    np.maximum.at(imax, entry[ok], a[ok])
    with np.errstate(divide="ignore", invalid="ignore"):
        cats = np.floor(1.0 + (x - th) / (th - se))
    cat = np.zeros((4, L), np.int32)
    for i, m in enumerate((cats == 1, cats == 2, cats == 3, cats >= 4)):
        np.add.at(cat[i], entry[m & ok], 1)
    return L, int(n_valid.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", default="518400,1036800")
    ap.add_argument("--years", type=int, default=40)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--route-cells", type=int, default=4096)
    ap.add_argument("--max-gib", type=float, default=96.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import xmhw_amd.device as dev
    from bench_objects import giant_table, grid_of, median_ms
    from xmhw_amd._lib import hip, require_gpu
    from xmhw_amd.calendar import add_doy
    from xmhw_amd.coverage import quantise_weights
    from xmhw_amd.detect_front import _check_inputs
    from xmhw_amd.objects import neighbour_table, objects_device
    from xmhw_amd.track_intensity import intensity_bits
    require_gpu()
    h = hip()
    t = np.arange("1982-01-01", f"{1982 + a.years}-01-01", dtype="datetime64[D]")
    doy = add_doy(t)
    T = t.shape[0]
    plan = dev.Plan(doy, 5)
    D = plan.D
    _, _, _, rows = _check_inputs(np.zeros((T, 1), np.float32), np.zeros((D, 1)), np.zeros((D, 1)), doy, np.unique(doy))
    res = {"bench": "mhw_track_intensity", "T": int(T), "dtype": "float32", "hbm_bytes_per_s": HBM, "reps": a.reps,
           "chunk": int(h.TRACK_INTENSITY_CHUNK), "cases": []}
    first = None
    for C in [int(c) for c in a.cells.split(",")]:
        grid = grid_of(C)
        keep = []
        try:
            d_ts, d_th, d_se, start, end, imax, offsets = series_and_table(h, dev, C, T, plan, rows, keep)
            n = start.shape[0]
            w = np.repeat(np.cos(np.deg2rad(np.linspace(-89.875, 89.875, grid[0]))), grid[1])
            ib = intensity_bits(31, C)
            wi = quantise_weights(w, ib)[0]
            if first is None:
                first = (start[:int(offsets[a.route_cells])].copy(), end[:int(offsets[a.route_cells])].copy(),
                         offsets[:a.route_cells + 1].copy(), wi[:a.route_cells].copy())
            case = {"cells": C, "grid": list(grid), "intensity_weight_bits": ib}
            per = objects_device(start, end, imax, offsets, neighbour_table(np.arange(C), grid, 6, 1), 0, quantise_weights(w, 31)[0])
            roots = np.nonzero(per["root"] == np.arange(n, dtype=np.int32))[0]
            lut = np.empty(n, dtype=np.int32)
            lut[roots] = np.arange(roots.shape[0], dtype=np.int32)
            dur = per["time_end"].astype(np.int64) - per["time_start"] + 1
            case["scattered"] = time_stage(h, dev, median_ms, d_ts, d_th, d_se, T, C, D, rows, start, end, lut[per["root"]], offsets,
                                           wi, per["time_start"], np.concatenate([[0], np.cumsum(dur)]).astype(np.int64), a.reps,
                                           a.max_gib * 2**30)
            case["scattered"]["largest_object_cells"] = int(per["n_cells"].max())
            del per, lut
            gs, ge, _, go = giant_table(C, grid, max(1, int(round(n / C))))
            case["giant"] = time_stage(h, dev, median_ms, d_ts, d_th, d_se, T, C, D, rows, gs, ge, np.zeros(gs.shape[0], np.int32), go,
                                       wi, np.array([gs.min()], np.int32), np.array([0, int(ge.max()) - int(gs.min()) + 1], np.int64),
                                       a.reps, a.max_gib * 2**30)
            for k in ("scattered", "giant"):
                c = case[k]
                if "accumulate_ms" in c:
                    c["combining_speedup"] = round(c["accumulate_uncombined_ms"] / c["accumulate_ms"], 2)
        finally:
            for b in keep:
                b.free()
        res["cases"].append(case)
        print(case, file=sys.stderr, flush=True)

    # the numpy route on the first cells of the first table, scaled per cell
    nc = a.route_cells
    s, e, off, wi = first
    bufs = []
    try:
        d_ts, d_th, d_se = dev.DeviceBuffer(4 * T * nc), dev.DeviceBuffer(8 * D * nc), dev.DeviceBuffer(8 * D * nc)
        bufs += [d_ts, d_th, d_se]
        h.synth_sst(d_ts.ptr, 4, T, nc, nc, 0, 7, 0.0)
        dev.clim_raw(plan, d_ts, 4, nc, 0.9, False, d_th, d_se)
        h.stream_sync(0)
        ts, th, se = d_ts.to_array((T, nc), np.float32), d_th.to_array((D, nc), np.float64), d_se.to_array((D, nc), np.float64)
    finally:
        for b in bufs:
            b.free()
    cell = np.repeat(np.arange(nc, dtype=np.int64), np.diff(off))
    t0 = time.perf_counter()
    L, nv = numpy_route(ts, se, th, rows.astype(np.int64), s, e, cell, wi)
    t_cpu = time.perf_counter() - t0
    assert nv == L
    res["cpu_route"] = {"how": "numpy add.at / maximum.at over the expanded voxels, every row its own object", "cells": nc,
                        "rows": int(s.shape[0]), "voxels": L, "seconds": round(t_cpu, 3)}
    for c in res["cases"]:
        scaled = t_cpu * c["cells"] / nc
        c["cpu_route_scaled_s"] = round(scaled, 1)
        if "accumulate_ms" in c["scattered"]:
            c["cpu_route_scaled_over_device_stage"] = round(scaled * 1e3 / c["scattered"]["accumulate_ms"], 0)
    plan.destroy()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
