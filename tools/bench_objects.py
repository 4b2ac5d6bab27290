#!/usr/bin/env python3
"""mhw_objects()'s device stage on the event table of a synthetic 40-year daily series: one JSON line.

    python tools/bench_objects.py [--cells 518400,1036800] [--years 40] [--reps 10] [--route-cells 4096] [--out FILE]

Per cell count (laid row-major on a 540 x 960 / 720 x 1440 grid, longitude wrapping, every point ocean) the event
table comes from the table-only detect() device stage on the series of tools/bench_coverage.py (device generator,
raw 90th-percentile climatology of the threshold kernel); only its index_start, index_end and intensity_max columns
are kept.  Timed with HIP events around the two C ABI calls (xmhw_event_objects: init + link + flatten;
xmhw_object_reduce: memsets + reduce + peak + finish; each call initialises its own buffers), median of --reps runs
after a warm-up, everything on the device, for connectivity 6 and 26.  Each is set against its byte floor (inputs
once + outputs once at 6.3 TB/s, the copy rate of the project's other tables), and the whole mhw_objects() call
(uploads, the host's slot numbering between the two stages, downloads, renumbering) is timed by the wall clock.

The synthetic cells are independent, so the objects are small: the *scattered* case.  The *giant* case has the
same number of cells and rows per cell laid out so that every row is in ONE object (neighbouring cells' runs are
staggered by half a period); its times per row are compared with the scattered ones -- this is where a reduction
that funnels every row into one address would collapse.

The CPU route this replaces -- scipy.ndimage.label on the rasterised (T, ny, nx) volume (the oracle's flood fill
where scipy does not import) -- is timed on the first --route-cells cells as a 64-wide grid and SCALED per cell;
the partition it finds is compared with the device's on those cells."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM = 6.3e12
GRIDS = {518400: (540, 960), 1036800: (720, 1440)}


def median_ms(h, fn, reps):
    e0, e1 = h.event_create(), h.event_create()
    out = []
    for _ in range(reps + 1):
        h.event_record(e0, 0)
        fn()
        h.event_record(e1, 0)
        h.stream_sync(0)
        out.append(h.event_elapsed_ms(e0, e1))
    h.event_destroy(e0)
    h.event_destroy(e1)
    return float(np.median(out[1:])), [round(v, 3) for v in out[1:]]


def grid_of(C):
    if C in GRIDS:
        return GRIDS[C]
    ny = int(np.sqrt(C))
    while C % ny:
        ny -= 1
    return ny, C // ny


def detect_table(h, dev, C, T, plan, rows):
    """(start, end, imax, offsets) of the table-only detect() device stage on the synthetic series"""
    D = plan.D
    W = (T + 63) // 64
    bufs = []
    try:
        d_ts = dev.DeviceBuffer(4 * T * C); bufs.append(d_ts)
        h.synth_sst(d_ts.ptr, 4, T, C, C, 0, 7, 0.0)
        d_th, d_se = dev.DeviceBuffer(8 * D * C), dev.DeviceBuffer(8 * D * C)
        bufs += [d_th, d_se]
        dev.clim_raw(plan, d_ts, 4, C, 0.9, False, d_th, d_se)
        d_bits = dev.DeviceBuffer(8 * W * C); bufs.append(d_bits)
        h.exceed_bits(d_ts.ptr, 4, T, C, C, d_th.ptr, C, D, rows, 0, d_bits.ptr, C)
        d_n, d_off = dev.DeviceBuffer(4 * C), dev.DeviceBuffer(8 * (C + 1))
        bufs += [d_n, d_off]
        h.events_from_bits(d_bits.ptr, T, C, C, 5, 1, 2, 0, d_n.ptr, 0)
        h.offsets_from_counts(d_n.ptr, C, d_off.ptr)
        h.stream_sync(0)
        offsets = d_off.to_array((C + 1,), np.int64)
        n = int(offsets[-1])
        ncol = h.EVENT_COLUMNS
        d_tab = dev.DeviceBuffer(8 * max(n, 1) * ncol); bufs.append(d_tab)
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
        return start, end, imax, offsets
    finally:
        for b in bufs:
            b.free()


def giant_table(C, grid, per_cell):
    """C x per_cell rows, every one in a single object: runs of 8 days every 10, shifted by 5 on odd i + j"""
    ny, nx = grid
    par = (np.add.outer(np.arange(ny), np.arange(nx)) % 2).reshape(-1)
    k = np.arange(per_cell)
    start = (10 * k[None, :] + 5 * par[:, None]).astype(np.int32).reshape(-1)
    end = start + 7
    rng = np.random.default_rng(5)
    imax = rng.normal(size=start.shape[0]).astype(np.float32).astype(np.float64)
    return start, end, imax, np.arange(C + 1, dtype=np.int64) * per_cell


def time_stages(h, dev, args, reps):
    start, end, imax, offsets, nbr, gap, wq = args
    n, C = start.shape[0], offsets.shape[0] - 1
    bufs = [dev.DeviceBuffer.from_array(np.ascontiguousarray(a)) for a in (start, end, imax, offsets, nbr, wq)]
    d_start, d_end, d_imax, d_off, d_nbr, d_wq = bufs
    try:
        d_cell, d_root = dev.DeviceBuffer(4 * n), dev.DeviceBuffer(4 * n)
        bufs += [d_cell, d_root]
        link_ms, link_all = median_ms(h, lambda: h.event_objects(d_start.ptr, d_end.ptr, n, d_off.ptr, C, d_nbr.ptr,
                                                                 nbr.shape[1], gap, d_cell.ptr, d_root.ptr), reps)
        root = d_root.to_array((n,), np.int32)
        roots = np.nonzero(root == np.arange(n, dtype=np.int32))[0]
        m = roots.shape[0]
        lut = np.empty(n, dtype=np.int32)
        lut[roots] = np.arange(m, dtype=np.int32)
        d_slot = dev.DeviceBuffer.from_array(lut[root]); bufs.append(d_slot)
        sizes = (4, 4, 4, 4, 8, 8, 8, 4)
        outs = [dev.DeviceBuffer(s * m) for s in sizes]
        bufs += outs
        red_ms, red_all = median_ms(h, lambda: h.object_reduce(d_start.ptr, d_end.ptr, d_imax.ptr, n, d_cell.ptr, d_off.ptr,
                                                               d_wq.ptr, d_slot.ptr, m, *[o.ptr for o in outs]), reps)
        n_events = outs[0].to_array((m,), np.int32)
        assert int(n_events.sum()) == n
        link_floor = (8 * n + 8 * (C + 1) + 4 * nbr.size + 8 * n) / HBM * 1e3
        red_floor = (16 * n + 8 * n + 16 * C + sum(sizes) * m) / HBM * 1e3
        return {"rows": n, "objects": int(m), "largest_object_rows": int(n_events.max()),
                "event_objects_ms": round(link_ms, 3), "event_objects_ms_all": link_all,
                "object_reduce_ms": round(red_ms, 3), "object_reduce_ms_all": red_all,
                "event_objects_floor_ms": round(link_floor, 4), "object_reduce_floor_ms": round(red_floor, 4),
                "event_objects_over_floor": round(link_ms / link_floor, 1),
                "object_reduce_over_floor": round(red_ms / red_floor, 1),
                "ns_per_row": round((link_ms + red_ms) * 1e6 / n, 3),
                "reduce_ns_per_row": round(red_ms * 1e6 / n, 3)}, root
    finally:
        for b in bufs:
            b.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", default="518400,1036800")
    ap.add_argument("--years", type=int, default=40)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--route-cells", type=int, default=4096)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import objects_oracle as oo
    import xmhw_amd.device as dev
    from xmhw_amd import mhw_objects
    from xmhw_amd._lib import hip, require_gpu
    from xmhw_amd.calendar import add_doy
    from xmhw_amd.detect import EventDataset
    from xmhw_amd.detect_front import _check_inputs
    from xmhw_amd.objects import neighbour_table
    require_gpu()
    h = hip()
    t = np.arange("1982-01-01", f"{1982 + a.years}-01-01", dtype="datetime64[D]")
    doy = add_doy(t)
    T = t.shape[0]
    plan = dev.Plan(doy, 5)
    doys = np.unique(doy)
    _, _, _, rows = _check_inputs(np.zeros((T, 1), np.float32), np.zeros((plan.D, 1)), np.zeros((plan.D, 1)), doy, doys)
    res = {"bench": "mhw_objects", "T": int(T), "hbm_bytes_per_s": HBM, "reps": a.reps, "cases": []}
    first = None
    for C in [int(c) for c in a.cells.split(",")]:
        grid = grid_of(C)
        start, end, imax, offsets = detect_table(h, dev, C, T, plan, rows)
        if first is None:
            first = (start, end, imax, offsets)
        n = start.shape[0]
        wq = np.random.default_rng(3).integers(0, (1 << 31) + 1, C, dtype=np.int64) >> 8
        case = {"cells": C, "grid": list(grid), "periodic": "lon"}
        for conn in (6, 26):
            nbr = neighbour_table(np.arange(C), grid, conn, 1)
            gap = 0 if conn == 6 else 1
            sc, _ = time_stages(h, dev, (start, end, imax, offsets, nbr, gap, wq), a.reps)
            per_cell = max(1, int(round(n / C)))
            gs, ge, gi, go = giant_table(C, grid, per_cell)
            gt, groot = time_stages(h, dev, (gs, ge, gi, go, nbr, gap, wq), a.reps)
            assert gt["objects"] == 1 and not groot.any()
            case[f"connectivity_{conn}"] = {
                "scattered": sc, "giant": gt,
                "giant_over_scattered_per_row": round(gt["ns_per_row"] / sc["ns_per_row"], 2),
                "giant_over_scattered_reduce_per_row": round(gt["reduce_ns_per_row"] / sc["reduce_ns_per_row"], 2)}
        # the whole call, from a host EventDataset (a narrow table: the columns mhw_objects() reads)
        tab = np.zeros((n, 5))
        tab[:, 1], tab[:, 2], tab[:, 3], tab[:, 4] = start, end, imax, start
        ds = EventDataset(tab, offsets, t, np.arange(C), np.ones(C, bool), ("lat", "lon"), grid,
                          {"lat": np.linspace(-89.875, 89.875, grid[0]), "lon": np.arange(grid[1]) * 360.0 / grid[1]},
                          {}, {}, {}, False)
        ds.columns = ["event", "index_start", "index_end", "intensity_max", "time_peak"]
        mhw_objects(ds, periodic="lon", weights="coslat")
        t0 = time.perf_counter()
        ob = mhw_objects(ds, periodic="lon", weights="coslat")
        case["mhw_objects_call_s"] = round(time.perf_counter() - t0, 3)
        case["mhw_objects_call_objects"] = ob.n_objects
        res["cases"].append(case)
        print(case, file=sys.stderr, flush=True)
        del tab, ds, ob

    # the CPU route on a sub-grid, scaled per cell
    start, end, imax, offsets = first
    nc = a.route_cells
    sub = (nc // 64, 64)
    nr = int(offsets[nc])
    s, e = start[:nr], end[:nr]
    flat = np.repeat(np.arange(nc), np.diff(offsets[:nc + 1]))
    t0 = time.perf_counter()
    vol = np.zeros((T,) + sub, dtype=bool)
    inc = np.zeros((T + 1, nc), dtype=np.int8)
    np.add.at(inc, (s, flat), 1)
    np.add.at(inc, (e + 1, flat), -1)
    vol[:] = (np.cumsum(inc[:T], axis=0, dtype=np.int32) > 0).reshape((T,) + sub)
    t_raster = time.perf_counter() - t0
    t0 = time.perf_counter()
    try:
        import scipy.ndimage as ndi
        lab, _ = ndi.label(vol, structure=ndi.generate_binary_structure(3, 1))
        rows_lab = lab[s, flat // 64, flat % 64]
        want = oo.roots_from_labels(rows_lab)
        how = "scipy.ndimage.label"
    except ImportError:
        want, _ = oo.voxel_roots(s, e, flat, sub, T, 6, None)
        how = "objects_oracle.voxel_roots"
    t_label = time.perf_counter() - t0
    nbr = neighbour_table(np.arange(nc), sub, 6, None)
    _, got = time_stages(h, dev, (s, e, imax[:nr], offsets[:nc + 1], nbr, 0, np.ones(nc, np.int64)), 1)
    assert np.array_equal(got, want)
    res["cpu_route"] = {"how": how, "cells": nc, "rows": nr, "rasterise_s": round(t_raster, 3), "label_s": round(t_label, 3),
                        "same_partition_as_device": True}
    for c in res["cases"]:
        scaled = t_label * c["cells"] / nc
        c["cpu_label_scaled_s"] = round(scaled, 1)
        stage = c["connectivity_6"]["scattered"]
        c["cpu_label_scaled_over_device_stages"] = round(scaled * 1e3 / (stage["event_objects_ms"] + stage["object_reduce_ms"]), 0)
        c["cpu_label_scaled_over_call"] = round(scaled / c["mhw_objects_call_s"], 1)
    plan.destroy()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
