#!/usr/bin/env python3
"""mhw_displacement()'s device stage on a resident global quarter-degree grid: one JSON line.

    python tools/bench_displacement.py [--ny 720 --nx 1440] [--years 40] [--reps 3] [--probe-steps 366]
                                       [--max-call-s 20] [--route-cells 4096] [--out FILE]

The field is made on the host, block of steps by block of steps, and uploaded into one resident float32 (T, ny * nx)
buffer: a zonal base state that cools towards the poles, a seasonal cycle, a smooth anomaly (48 plane waves of 15 to 360
degrees of wavelength with AR(1) amplitudes, 30 days of memory, 0.8 K of standard deviation) and 0.15 K of white noise;
30 % of the points are land (NaN) in continent-sized patches.  seas is the base state plus the cycle, thresh lies
1.2816 standard deviations of the smooth anomaly above it (its 90th percentile), and the event table comes from the
device's own detect() stage on that series (xmhw_exceed_bits, xmhw_events_from_bits, xmhw_event_stats_sparse): warm
patches of weeks, as a detection gives them.  Every grid point is a cell of the table (land has no rows), so C = ny * nx
here.

Per max_distance (500, 1000, 2000 km, periodic) and class pattern ("all", calendar months) xmhw_displacement_accumulate
is timed with HIP events around the C ABI call, everything already on the device: first on a block of --probe-steps
steps in the middle of the axis, then -- if that projects to less than --max-call-s seconds -- on all T steps in one
call (median of --reps after a warm-up call; otherwise the JSON says that the full call was not timed and carries the
projection).  One more run takes the southern half of the grid (518,400 cells).  Reported with each: n_visited per source,
the share of unreached sources, and the ratio to the byte floor (one read of the series block and of its bitmap words,
one write of the accumulators, at 6.3 TB/s, the measured copy rate).  Alongside, in the same run: the numpy brute-force
route (per source the first qualifying entry of its row's list, vectorised per row and day) on the event-richest square of
--route-cells cells and 64 steps at 500 km, scaled linearly in cell-steps; those cells double as the spot check: both routes must give
identical integers."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM = 6.3e12
SIGMA, NOISE, MODES, MEMORY = 0.8, 0.15, 48, 30.0


class Field:
    """the synthetic SST of the module docstring, one block of steps at a time"""

    def __init__(self, ny, nx, time, seed=23):
        from xmhw_amd.calendar import add_doy
        rng = np.random.default_rng(seed)
        self.ny, self.nx, self.N, self.T = ny, nx, ny * nx, time.shape[0]
        self.lat = (np.arange(ny) + 0.5) * (180.0 / ny) - 90.0
        self.dlon = 360.0 / nx
        self.lon = (np.arange(nx) + 0.5) * self.dlon
        phi, lam = np.deg2rad(self.lat)[:, None], np.deg2rad(self.lon)[None, :]
        self.doy = add_doy(time)
        self.doys = np.unique(self.doy)
        self.base = (2.0 + 26.0 * np.cos(phi) ** 2 + 0.0 * lam).reshape(-1)
        self.amp = (4.0 * np.sin(phi) + 0.0 * lam).reshape(-1)
        kx, ky = rng.integers(1, 25, MODES), rng.integers(0, 13, MODES)
        ph = rng.uniform(0, 2 * np.pi, MODES)
        self.modes = np.stack([np.cos(a * lam + 2.0 * b * phi + c).reshape(-1) for a, b, c in zip(kx, ky, ph)])
        self.modes = (self.modes * (SIGMA / np.sqrt(MODES / 2.0))).astype(np.float32)
        rho = np.exp(-1.0 / MEMORY)
        c = np.empty((self.T, MODES))
        c[0] = rng.standard_normal(MODES)
        shocks = rng.standard_normal((self.T, MODES)) * np.sqrt(1.0 - rho * rho)
        for t in range(1, self.T):
            c[t] = rho * c[t - 1] + shocks[t]
        self.coef = c.astype(np.float32)
        lk, lp = rng.integers(1, 5, 6), rng.uniform(0, 2 * np.pi, (6, 2))
        cont = sum(np.cos(k * lam + p[0]) * np.cos(k * phi + p[1]) for k, p in zip(lk, lp)).reshape(-1)
        self.land = cont > np.quantile(cont, 0.7)
        self.pool = (NOISE * rng.standard_normal((16, self.N))).astype(np.float32)
        self.shift = rng.integers(0, self.N, self.T)

    def cycle(self, doy):
        return np.sin(2.0 * np.pi * (np.asarray(doy, dtype=np.float64) - 80.0) / 366.0)

    def seas(self):
        """(D, N) float64: the climatology row of every doy label, NaN on land"""
        se = self.base[None, :] + self.cycle(self.doys)[:, None] * self.amp[None, :]
        se[:, self.land] = np.nan
        return se

    def block(self, t0, nt):
        x = self.coef[t0:t0 + nt] @ self.modes
        x += np.outer(self.cycle(self.doy[t0:t0 + nt]).astype(np.float32), self.amp.astype(np.float32))
        x += self.base.astype(np.float32)[None, :]
        for k in range(nt):
            x[k] += np.roll(self.pool[(t0 + k) % 16], int(self.shift[t0 + k]))
        x[:, self.land] = np.nan
        return x


def median_ms(h, fn, reps, warm=1):
    e0, e1 = h.event_create(), h.event_create()
    out = []
    for _ in range(reps + warm):
        h.event_record(e0, 0)
        fn()
        h.event_record(e1, 0)
        h.stream_sync(0)
        out.append(h.event_elapsed_ms(e0, e1))
    h.event_destroy(e0)
    h.event_destroy(e1)
    return float(np.median(out[warm:])), [round(v, 3) for v in out[warm:]]


def numpy_route(field, seas, rows, view, table, T):
    """the first qualifying entry of the row's list for every source of a small non-periodic, all-ocean-cells grid, one
    class: (n_days, n_found, sum_m) per cell"""
    ny, nx = table.ny, table.nx
    N = ny * nx
    ev = np.zeros((T, N), dtype=bool)
    cell = np.repeat(np.arange(N), np.diff(view["offsets"]))
    for c, s, e in zip(cell, view["start"], view["end"]):
        ev[s:e + 1, c] = True
    n_days, n_found, sum_m = np.zeros(N, np.int32), np.zeros(N, np.int32), np.zeros(N, np.int64)
    x = field.astype(np.float64).reshape(T, ny, nx)
    pad = np.full((T, ny, 3 * nx), np.nan)
    pad[:, :, nx:2 * nx] = x                                    # columns outside the grid never qualify
    for j in range(ny):
        dj, di, dist, _, _ = table.row(j)
        jj = j + dj.astype(np.int64)
        for t in range(T):
            src = np.nonzero(ev[t, j * nx:(j + 1) * nx])[0]
            if not src.size:
                continue
            g = seas[rows[t], j * nx + src]
            cand = pad[t][jj[None, :], nx + src[:, None] + di[None, :].astype(np.int64)]          # (S, E)
            with np.errstate(invalid="ignore"):
                q = cand <= g[:, None]
            first = q.argmax(axis=1)
            hit = q[np.arange(src.size), first]
            n_days[j * nx + src] += 1
            n_found[j * nx + src[hit]] += 1
            sum_m[j * nx + src[hit]] += dist[first[hit]]
    return n_days, n_found, sum_m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ny", type=int, default=720)
    ap.add_argument("--nx", type=int, default=1440)
    ap.add_argument("--years", type=int, default=40)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--probe-steps", type=int, default=366)
    ap.add_argument("--max-call-s", type=float, default=20.0)
    ap.add_argument("--route-cells", type=int, default=4096)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import xmhw_amd.device as dev
    from xmhw_amd._lib import hip, require_gpu
    from xmhw_amd.days_by import class_labels
    from xmhw_amd.detect import EVENT_COLUMNS
    from xmhw_amd.detect_front import _check_inputs
    from xmhw_amd.displacement import _Accumulators, displacement_grid, displacement_offsets
    require_gpu()
    h = hip()
    ny, nx = a.ny, a.nx
    N = ny * nx
    time_axis = np.arange("1982-01-01", f"{1982 + a.years}-01-01", dtype="datetime64[D]")
    T = time_axis.shape[0]
    W = (T + 63) // 64
    t_host = time.perf_counter()
    f = Field(ny, nx, time_axis)
    seas = f.seas()
    thresh = seas + 1.2816 * SIGMA
    D = seas.shape[0]
    _, _, _, rows = _check_inputs(np.zeros((T, 1), np.float32), seas[:, :1], thresh[:, :1], f.doy, f.doys)
    res = {"bench": "mhw_displacement", "ny": ny, "nx": nx, "cells": N, "T": int(T), "land_share": round(float(f.land.mean()), 3),
           "hbm_bytes_per_s": HBM, "reps": a.reps, "probe_steps": a.probe_steps, "periodic": True, "cases": []}

    def dump():
        if a.out:
            with open(a.out, "w") as fo:
                fo.write(json.dumps(res) + "\n")

    # the resident series, block by block
    d_ts = dev.DeviceBuffer(4 * T * N)
    step = max(1, (1 << 31) // (4 * N))
    for t0 in range(0, T, step):
        nt = min(step, T - t0)
        h.memcpy_h2d(d_ts.ptr + 4 * N * t0, f.block(t0, nt))
    res["field_on_device_s"] = round(time.perf_counter() - t_host, 1)
    print("field resident", res["field_on_device_s"], "s", file=sys.stderr, flush=True)

    # the event table of the device's detect() stage; every grid point is a cell
    with dev.DeviceScope() as s:
        d_th, d_se = s.upload(thresh), dev.DeviceBuffer.from_array(seas)
        d_bits, d_n, d_off = s.alloc(8 * W * N), s.alloc(4 * N), s.alloc(8 * (N + 1))
        h.exceed_bits(d_ts.ptr, 4, T, N, N, d_th.ptr, N, D, rows, 0, d_bits.ptr, N)
        h.events_from_bits(d_bits.ptr, T, N, N, 5, 1, 2, 0, d_n.ptr, 0)
        h.offsets_from_counts(d_n.ptr, N, d_off.ptr)
        h.stream_sync(0)
        offsets = d_off.to_array((N + 1,), np.int64)
        n = int(offsets[-1])
        ncol = h.EVENT_COLUMNS
        d_tab = s.alloc(8 * max(n, 1) * ncol)
        h.events_from_bits(d_bits.ptr, T, N, N, 5, 1, 2, d_off.ptr, 0, d_tab.ptr)
        h.event_stats_sparse(d_ts.ptr, 4, T, N, N, d_se.ptr, d_th.ptr, N, rows, 0, n, d_tab.ptr)
        h.stream_sync(0)
        start, end = np.empty(max(n, 1), np.int32), np.empty(max(n, 1), np.int32)
        chunk_rows = 1 << 20
        chunk = np.empty((chunk_rows, ncol), dtype=np.float64)
        i0, i1 = EVENT_COLUMNS.index("index_start"), EVENT_COLUMNS.index("index_end")
        for r0 in range(0, n, chunk_rows):
            m = min(chunk_rows, n - r0)
            h.memcpy_d2h(chunk[:m], d_tab.ptr + 8 * ncol * r0)
            start[r0:r0 + m], end[r0:r0 + m] = chunk[:m, i0], chunk[:m, i1]
    view = dict(n=n, C=N, offsets=offsets, start=start[:n], end=end[:n], cell_index=np.arange(N, dtype=np.int64))
    event_days = int((view["end"].astype(np.int64) - view["start"] + 1).sum())
    res.update(events=n, event_cell_days=event_days, event_share_of_ocean_cell_days=round(event_days / (T * (~f.land).sum()), 4))
    print("events", n, "cell-days", event_days, file=sys.stderr, flush=True)

    patterns = [("all", np.zeros(T, np.int32), 1), ("months", (class_labels("month", time_axis) - 1).astype(np.int32), 12)]
    cell_of_point = np.arange(N, dtype=np.int32)
    p0 = max(0, (T - a.probe_steps) // 2)
    pn = min(a.probe_steps, T)

    def run(table, classes, K, t0, nt, reps):
        """time one accumulate call over the steps [t0, t0 + nt); the counters of one call"""
        rows_j = table.ny
        acc = _Accumulators(view, cell_of_point, table, classes, K, None, False, T, rows)
        try:
            call = lambda: acc.add_block(d_ts.ptr + 4 * N * t0, 4, N, t0, nt, d_se.ptr, N, D)                     # noqa: E731
            ms, every = median_ms(h, call, reps, warm=1 if reps > 1 else 0)
            h.displacement_init(acc.K, acc.C, *acc._out())
            call()
            out = acc.result()
        finally:
            acc.free()
        src, found = int(out["n_days"].sum()), int(out["n_found"].sum())
        cells = rows_j * nx
        floor_ms = (4 * nt * cells + 8 * ((nt + 63) // 64 + 1) * cells + 36 * K * cells) / HBM * 1e3
        return {"steps": int(nt), "ms": round(ms, 3), "ms_all": every, "sources": src,
                "n_visited_per_source": round(out["n_visited"] / max(src, 1), 2),
                "unreached_share": round(1.0 - found / max(src, 1), 4),
                "mean_displacement_km": round(float(out["sum_m"].sum()) / max(found, 1) / 1000.0, 1),
                "byte_floor_ms": round(floor_ms, 4), "over_floor": round(ms / floor_ms, 1)}

    tables = {}
    for maxd in (500.0, 1000.0, 2000.0):
        t0_ = time.perf_counter()
        tables[maxd] = displacement_offsets(f.lat, nx, f.dlon, maxd, True)
        print("table", maxd, tables[maxd].n_entries, "entries", round(time.perf_counter() - t0_, 1), "s", file=sys.stderr, flush=True)
    for maxd, table in tables.items():
        for name, classes, K in patterns:
            case = {"max_distance_km": maxd, "classes": name, "K": K, "cells": N, "list_entries": table.n_entries,
                    "table_bytes": table.nbytes, "probe": run(table, classes, K, p0, pn, 1)}
            projected = case["probe"]["ms"] * T / pn / 1e3
            case["projected_full_call_s"] = round(projected, 2)
            if projected <= a.max_call_s:
                case["full"] = run(table, classes, K, 0, T, a.reps)
            else:
                case["full"] = None
                case["note"] = f"the call over all {T} steps was not timed: projected above {a.max_call_s} s"
            res["cases"].append(case)
            print(case, file=sys.stderr, flush=True)
            dump()                                      # what is measured so far survives a later failure

    # 518,400 cells: the southern half of the grid (rows 0 .. ny / 2 - 1 are the first half of every step's row)
    hy = ny // 2
    hc = hy * nx
    cut = np.searchsorted(np.repeat(np.arange(N), np.diff(offsets)), hc)
    half_view = dict(n=int(cut), C=hc, offsets=offsets[:hc + 1], start=view["start"][:cut], end=view["end"][:cut],
                     cell_index=np.arange(hc, dtype=np.int64))
    d_se_half = dev.DeviceBuffer.from_array(np.ascontiguousarray(seas[:, :hc]))
    table = displacement_offsets(f.lat[:hy], nx, f.dlon, 1000.0, True)
    acc = _Accumulators(half_view, cell_of_point[:hc], table, patterns[0][1], 1, None, False, T, rows)
    try:
        call = lambda: acc.add_block(d_ts.ptr + 4 * N * p0, 4, N, p0, pn, d_se_half.ptr, hc, D)               # noqa: E731
        ms, every = median_ms(h, call, 1, warm=0)
        h.displacement_init(1, hc, *acc._out())
        call()
        out = acc.result()
    finally:
        acc.free()
        d_se_half.free()
    src = int(out["n_days"].sum())
    res["half_grid"] = {"cells": hc, "max_distance_km": 1000.0, "classes": "all", "steps": int(pn), "ms": round(ms, 3),
                        "sources": src, "n_visited_per_source": round(out["n_visited"] / max(src, 1), 2),
                        "unreached_share": round(1.0 - int(out["n_found"].sum()) / max(src, 1), 4)}
    print(res["half_grid"], file=sys.stderr, flush=True)
    dump()
    d_se.free()

    # the numpy route on a square cut from the grid, 64 steps, 500 km, no wrap: the square (corners on a lattice of 8
    # points) with the most event cell-days in those steps, a land point counting as 64 days less
    side = int(round(np.sqrt(a.route_cells)))
    ts0, tn = p0, min(64, T - p0)
    days = np.clip(np.minimum(view["end"], ts0 + tn - 1).astype(np.int64) - np.maximum(view["start"], ts0) + 1, 0, None)
    per_cell = np.bincount(np.repeat(np.arange(N), np.diff(offsets)), weights=days, minlength=N).reshape(ny, nx)
    per_cell[f.land.reshape(ny, nx)] = -64.0
    box = np.zeros((ny + 1, nx + 1))
    box[1:, 1:] = per_cell.cumsum(axis=0).cumsum(axis=1)
    sums = (box[side:, side:] - box[:-side, side:] - box[side:, :-side] + box[:-side, :-side])[::8, ::8]
    j0, i0_ = (int(v) * 8 for v in np.unravel_index(int(sums.argmax()), sums.shape))
    sub = np.empty((tn, side * side), dtype=np.float32)
    whole = np.empty((1, N), dtype=np.float32)
    for k in range(tn):
        h.memcpy_d2h(whole, d_ts.ptr + 4 * N * (ts0 + k))
        sub[k] = whole.reshape(ny, nx)[j0:j0 + side, i0_:i0_ + side].reshape(-1)
    pts = (np.arange(j0, j0 + side)[:, None] * nx + np.arange(i0_, i0_ + side)[None, :]).reshape(-1)
    sub_rows, sub_start, sub_end, sub_off = rows[ts0:ts0 + tn], [], [], [0]
    for p in pts:
        for r in range(int(offsets[p]), int(offsets[p + 1])):
            s_, e_ = max(int(view["start"][r]), ts0), min(int(view["end"][r]), ts0 + tn - 1)
            if s_ <= e_:
                sub_start.append(s_ - ts0)
                sub_end.append(e_ - ts0)
        sub_off.append(len(sub_start))
    sub_view = dict(n=len(sub_start), C=side * side, offsets=np.asarray(sub_off, np.int64), start=np.asarray(sub_start, np.int32),
                    end=np.asarray(sub_end, np.int32), cell_index=np.arange(side * side, dtype=np.int64))
    sub_table = displacement_offsets(f.lat[j0:j0 + side], side, f.dlon, 500.0, False)
    sub_seas = np.ascontiguousarray(seas[:, pts])
    t0_ = time.perf_counter()
    want = numpy_route(sub, sub_seas, sub_rows, sub_view, sub_table, tn)
    t_numpy = time.perf_counter() - t0_
    t0_ = time.perf_counter()
    got = displacement_grid(sub, sub_seas, sub_rows, sub_view, sub_view["cell_index"], sub_table, np.zeros(tn, np.int32), 1)
    t_stage = time.perf_counter() - t0_
    same = all(np.array_equal(got[k][0], w) for k, w in zip(("n_days", "n_found", "sum_m"), want))
    assert want[0].sum() > 0, "the numpy route saw no source"
    assert same, "the numpy route and the device stage differ"
    scale = (N * T) / (side * side * tn)
    res["numpy_route"] = {"cells": side * side, "corner": [j0, i0_], "land_cells": int(f.land[pts].sum()), "steps": tn, "max_distance_km": 500.0, "periodic": False,
                          "sources": int(want[0].sum()), "numpy_s": round(t_numpy, 3), "displacement_grid_wall_s": round(t_stage, 3),
                          "identical_integers": True, "scaled_to_full_grid_s": round(t_numpy * scale, 0)}
    d_ts.free()
    print(json.dumps(res))
    dump()


if __name__ == "__main__":
    main()
