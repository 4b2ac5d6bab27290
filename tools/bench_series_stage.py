#!/usr/bin/env python3
"""Wall time of the public series stages -- mhw_coverage(), mhw_days_by(), mhw_track_intensity(), heat_stress(),
index_regression(), mhw_composite(), lag_correlation() -- on a grid that goes through the device in several slabs: one
JSON line.  What it is for: the host time per slab of the grid walker
(xmhw_amd/series_stage.py), which no kernel timing shows.

    python tools/bench_series_stage.py [--grid 160x320] [--tile 1] [--years 10] [--slabs 10] [--reps 3] [--package DIR]
                                       [--once [--only STAGE]]

A synthetic float32 (time, lat, lon) series with 20 % land, AR(1) anomalies around a 366-row climatology; detect(),
mhw_objects() and mhw_tracks() run once, untimed, for the track-intensity call.  ``--tile K`` repeats the grid K times
along the longitude (a larger series at the cost of a copy, not of K times the random numbers).  ``max_batch_bytes`` is set so that
device._grid_batch() cuts the grid into --slabs slabs for the first three stages (the number it gives is reported; a stage
with fewer bytes a cell takes a slab or two fewer, lag_correlation() with its second field a few more).  heat_stress()
and index_regression() (one index, lags 0, 30, 60) take ``se`` as their base, mhw_composite() the detection's events
(30 steps either side), lag_correlation() the series against its own negation with lags -5 .. 10.  Each stage: one warm-up call,
then the median of --reps calls, time.perf_counter() around the public function.  ``--package DIR`` imports xmhw_amd
from DIR instead of this checkout (an A/B of two checkouts with the same compiled library); ``--once`` makes one call
of each stage (``--only``: of that stage) and times nothing, for a kernel trace."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAGES = ("mhw_coverage", "mhw_days_by", "mhw_track_intensity", "heat_stress", "index_regression", "mhw_composite",
          "lag_correlation")


def grid_case(ny, nx, years, tile=1, seed=0):
    from xmhw_amd import GridSeries
    from xmhw_amd.calendar import add_doy
    rng = np.random.default_rng(seed)
    time64 = np.arange("2001-01-01", f"{2001 + years}-01-01", dtype="datetime64[D]")
    T, N = time64.shape[0], ny * nx
    row = add_doy(time64) - 1
    seas = (15.0 + 3.0 * np.sin(2 * np.pi * np.arange(366) / 366.0)[:, None] + rng.normal(scale=0.2, size=(366, N)))
    thresh = seas + rng.uniform(0.3, 0.8, size=(366, N))
    ts = np.empty((T, N), dtype=np.float32)
    x = rng.standard_normal(N)
    for t in range(T):
        x = 0.85 * x + rng.standard_normal(N)
        ts[t] = seas[row[t]] + x
    land = rng.random(N) < 0.2
    land[0] = False
    ts[:, land] = np.nan
    seas[:, land] = np.nan
    thresh[:, land] = np.nan
    ts, thresh, seas = (np.tile(a.reshape(-1, ny, nx), (1, 1, tile)) for a in (ts, thresh, seas))
    lat, lon = np.linspace(-60, 60, ny), np.arange(nx * tile) * (360.0 / (nx * tile))
    doys = np.arange(1, 367)
    temp = GridSeries(ts, ("time", "lat", "lon"), {"time": time64, "lat": lat, "lon": lon})
    th = GridSeries(thresh, ("doy", "lat", "lon"), {"doy": doys, "lat": lat, "lon": lon})
    se = GridSeries(seas, ("doy", "lat", "lon"), {"doy": doys, "lat": lat, "lon": lon})
    return temp, th, se


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", default="160x320")
    ap.add_argument("--tile", type=int, default=1)
    ap.add_argument("--years", type=int, default=10)
    ap.add_argument("--slabs", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--package", default=ROOT)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--only", default=None, choices=STAGES)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.package))
    import xmhw_amd
    from xmhw_amd._lib import require_gpu
    from xmhw_amd.device import _grid_batch
    require_gpu()
    ny, nx = (int(v) for v in a.grid.split("x"))
    temp, th, se = grid_case(ny, nx, a.years, a.tile)
    nx *= a.tile
    T, N = temp.values.shape[0], ny * nx
    stacked = temp.values.reshape(T, N)
    extra = 6 * 366 * 8 + T // 4 + 64                    # the largest per-cell extra of the three stages
    per_cell = T * 4 * 4 + extra
    budget = per_cell * -(-N // a.slabs)
    slabs = -(-N // _grid_batch(stacked, budget, per_cell_extra=extra))
    res = {"bench": "series_stage", "package": os.path.dirname(os.path.abspath(xmhw_amd.__file__)), "grid": [ny, nx], "T": T,
           "dtype": "float32", "max_batch_bytes": budget, "slabs": slabs, "reps": a.reps, "seconds": {}}
    if a.only in (None, "mhw_track_intensity", "mhw_composite"):
        mhw = xmhw_amd.detect(temp, th, se)
        res.update(ocean_cells=int(mhw.n_cells), events=int(mhw.n_events))
    if a.only in (None, "mhw_track_intensity"):
        obj = xmhw_amd.mhw_objects(mhw)
        tr = xmhw_amd.mhw_tracks(mhw, obj)
        res.update(objects=int(obj.n_objects))
    index = {"index": np.cumsum(np.random.default_rng(1).normal(0, 0.1, T))}
    other = xmhw_amd.GridSeries(-temp.values, temp.dims, temp.coords) if a.only in (None, "lag_correlation") else None
    calls = {"mhw_coverage": lambda: xmhw_amd.mhw_coverage(temp, th, se, weights="coslat", max_batch_bytes=budget),
             "mhw_days_by": lambda: xmhw_amd.mhw_days_by(temp, th, se, classes="month", max_batch_bytes=budget),
             "mhw_track_intensity": lambda: xmhw_amd.mhw_track_intensity(temp, th, se, mhw, obj, tr, max_batch_bytes=budget),
             "heat_stress": lambda: xmhw_amd.heat_stress(temp, se, max_batch_bytes=budget),
             "index_regression": lambda: xmhw_amd.index_regression(temp, se, index, lags=(0, 30, 60), max_batch_bytes=budget),
             "mhw_composite": lambda: xmhw_amd.mhw_composite(temp, se, mhw, max_batch_bytes=budget),
             "lag_correlation": lambda: xmhw_amd.lag_correlation(temp, other, se, None, lags=(-5, 10),
                                                                 max_batch_bytes=budget)}
    for name, call in calls.items():
        if a.only not in (None, name):
            continue
        call()
        if a.once:
            continue
        every = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            call()
            every.append(time.perf_counter() - t0)
        res["seconds"][name] = {"median": statistics.median(every), "all": every}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
