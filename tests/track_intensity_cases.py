"""Inputs shared by the host and the GPU tests of mhw_track_intensity().  TEST INFRASTRUCTURE ONLY.

* calendar_grid(): a small (time, lat, lon) GridSeries with land, 366-row climatologies labelled by the calendar doy
  and seeded red noise around them (coverage_cases.synthetic), as the public function takes it;
* event_dataset(): an EventDataset on a (ny, nx) grid from a compact table, for the stage tests;
* selection(): mhw -> (obj, tr, rows) with a given device stage each."""
import numpy as np

import coverage_cases as cc
from xmhw_amd import GridSeries
from xmhw_amd import calendar as cal
from xmhw_amd.detect import EventDataset

SDIMS = ("lat", "lon")


def calendar_grid(T, ny, nx, seed=0, dtype=np.float32, land=0.2, nan_frac=0.0, cold=False):
    """dict(temp, th, se: GridSeries; keep (ny * nx,) bool; w: float64 weights (ny, nx); lat, lon)"""
    rng = np.random.default_rng(seed + 1000)
    N = ny * nx
    d = cc.synthetic(T, N, np.float64, seed=seed, D=366, cold=cold)
    time = np.datetime64("2001-01-01") + np.arange(T)
    row = cal.add_doy(time) - 1
    sign = -1.0 if cold else 1.0
    anom = sign * d["ts"] - d["seas"][np.arange(T) % 366]
    ts = (sign * (d["seas"][row] + anom)).astype(dtype)
    if nan_frac:
        ts[rng.random((T, N)) < nan_frac] = np.nan
    keep = rng.random(N) >= land
    keep[0] = True
    ts[:, ~keep] = np.nan
    seas, thresh = d["seas"].copy(), d["thresh"].copy()
    seas[:, ~keep] = np.nan
    thresh[:, ~keep] = np.nan
    lat, lon = np.linspace(-60, 60, ny), np.arange(nx) * 2.0
    temp = GridSeries(ts.reshape(T, ny, nx), ("time", "lat", "lon"), {"time": time, "lat": lat, "lon": lon})
    doys = np.arange(1, 367)
    th = GridSeries(thresh.reshape(366, ny, nx), ("doy", "lat", "lon"), {"doy": doys, "lat": lat, "lon": lon})
    se = GridSeries(seas.reshape(366, ny, nx), ("doy", "lat", "lon"), {"doy": doys, "lat": lat, "lon": lon})
    return dict(temp=temp, th=th, se=se, keep=keep, w=rng.uniform(0.0, 3.0, (ny, nx)), lat=lat, lon=lon, T=T,
                ts=ts, seas=seas, thresh=thresh, doy=row + 1, doys=doys)


def event_dataset(table, offsets, T, ny, nx):
    """the EventDataset of a compact table on a (ny, nx) grid without land"""
    C = ny * nx
    assert offsets.shape[0] == C + 1
    time = np.datetime64("2001-01-01") + np.arange(T)
    coords = {"lat": np.linspace(-60, 60, ny), "lon": np.arange(nx) * 2.0, "time": time}
    return EventDataset(np.asarray(table, dtype=np.float64), np.asarray(offsets, dtype=np.int64), time, np.arange(C),
                        np.ones(C, dtype=bool), SDIMS, (ny, nx), coords, {}, {}, {}, False)


def selection(mhw, ids=None, weights=None, objects_stage=None, tracks_stage=None):
    from xmhw_amd import mhw_objects, mhw_tracks
    from xmhw_amd.track_intensity import selection_rows
    obj = mhw_objects(mhw, weights=weights, _compute=objects_stage)
    tr = mhw_tracks(mhw, obj, ids=ids, weights=weights, _compute=tracks_stage)
    return obj, tr, selection_rows(mhw, obj, tr)
