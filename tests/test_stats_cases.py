"""The exact block-statistics reference (tests/stats_exact_oracle.py) against the reference's own outputs and the
pairwise-sum oracle, and the conditions the synthetic cases of tests/stats_cases.py must meet -- asserted here, on
the CPU, for the very seeds and shapes tests/test_gpu_stats.py runs on the device."""
import os

import numpy as np
import numpy.testing as npt
import pandas as pd
import pytest

import stats_cases as sc
import stats_exact_oracle as xo
import stats_oracle as so
from xmhw_amd.detect_front import EVENT_COLUMNS
from xmhw_amd.stats import _bin_of_t

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def test_bin_of_t_is_cut_right_false():
    """bin b covers the years [edges[b], edges[b + 1]); everything else is -1: by definition and by searchsorted"""
    years = np.arange(1995, 2015).repeat(3)
    for edges in (np.array([2000, 2001, 2002, 2003]), np.array([2000, 2002, 2004, 2006]), np.array([2005, 2006]),
                  np.array([1990, 2030]), np.array([2020, 2021])):
        want = np.full(years.shape, -1)
        for b in range(len(edges) - 1):
            want[(years >= edges[b]) & (years < edges[b + 1])] = b
        got = _bin_of_t(years, edges)
        assert got.dtype == np.int32
        npt.assert_array_equal(got, want)
        s = np.searchsorted(edges, years, side="right") - 1
        npt.assert_array_equal(got, np.where((s >= 0) & (s < len(edges) - 1), s, -1))


def test_source_columns_are_the_aggregation_dictionary():
    assert sorted(sc.SOURCE_COLUMNS) == xo.EVENT_SOURCE_COLUMNS
    assert [EVENT_COLUMNS.index(c) for c in sc.MTIMES] == [3, 5, 4] == list(sc.TIME_COLUMNS)


def test_exact_oracle_reproduces_the_reference_outputs():
    """tests/golden/block_stats_cases.npz (outputs of the reference's pandas aggregation) within the bounds of a
    float64 sum in any order"""
    g = np.load(os.path.join(GOLD, "mhw_features_cases.npz"))
    b = np.load(os.path.join(GOLD, "block_stats_cases.npz"))
    seen = 0
    for i, (case, blockLength, mt, nb, y0) in enumerate(b["event_meta"]):
        T = int(g["offsets"][case + 1] - g["offsets"][case])
        tab = g["table"][g["table_offsets"][case]:g["table_offsets"][case + 1]]
        years = pd.date_range("2001-01-01", periods=T).year.to_numpy()
        edges = so.block_bins(int(years[0]), int(years[-1]), int(blockLength))
        ref = xo.event_stats(tab, np.array([0, tab.shape[0]]), _bin_of_t(years, edges), int(nb), (3, 5)[mt])
        want = b["event_stats"][b["event_offsets"][i]:b["event_offsets"][i + 1]]
        xo.assert_event_stats(want.T[:, :, None], ref, f"golden event block {i}")
        seen += nb
    assert seen == b["event_stats"].shape[0] > 900
    k = 0
    for case in range(len(g["offsets"]) - 1):
        sl = slice(g["offsets"][case], g["offsets"][case + 1])
        ts, se, th = g["ts"][sl], g["seas"][sl], g["thresh"][sl]
        years = pd.date_range("2001-01-01", periods=ts.shape[0]).year.to_numpy()
        cats = np.floor(1 + (ts - th) / (th - se))
        for blockLength in (1, 2):
            edges = so.block_bins(int(years[0]), int(years[-1]), blockLength)
            ref = xo.time_stats(ts[:, None], cats[:, None], _bin_of_t(years, edges), len(edges) - 1)
            want = b["time_stats"][b["time_offsets"][k]:b["time_offsets"][k + 1]]
            xo.assert_time_stats(want.T[:, :, None], ref, f"golden time block {k}")
            k += 1
    assert k == len(b["time_offsets"]) - 1


def test_exact_oracle_agrees_with_the_pairwise_oracle_on_positive_data():
    """on all-positive data a relative tolerance means something: stats_oracle.agg_mhw / agg_time to 1e-12"""
    rng = np.random.default_rng(11)
    T, C = 800, 7
    years = 2001 + np.arange(T) // 200
    edges = np.array([2001, 2003, 2005])
    bins = _bin_of_t(years, edges)
    n_ev = rng.integers(0, 30, size=C)
    offsets = np.concatenate([[0], np.cumsum(n_ev)])
    table = rng.uniform(0.5, 9.0, size=(offsets[-1], 31))
    for c in range(C):
        table[offsets[c]:offsets[c + 1], 3] = np.sort(rng.choice(T, size=n_ev[c], replace=False))
    ts = rng.uniform(1.0, 30.0, size=(T, C))
    cats = rng.integers(0, 6, size=(T, C)).astype(np.float64)
    ev, tm = xo.event_stats(table, offsets, bins, 2, 3), xo.time_stats(ts, cats, bins, 2)
    for c in range(C):
        tab = table[offsets[c]:offsets[c + 1]]
        want = so.agg_mhw(tab, EVENT_COLUMNS, years[tab[:, 3].astype(int)], edges)
        npt.assert_allclose(ev["val"][:, :, c].T, want, rtol=1e-12, atol=0, equal_nan=True)
        npt.assert_allclose(tm["val"][:, :, c].T, so.agg_time(ts[:, c], cats[:, c], years, edges), rtol=1e-12, atol=0)
    assert np.isnan(ev["val"]).sum() == 0 or (n_ev == 0).any()


def test_exact_oracle_empty_and_single_groups():
    """an empty and an all-NaN group: NaN / 0.0; one value: itself, n = 1, so bit-equality is asked"""
    nan = np.nan
    assert xo.agg([], "count") == (0.0, 0, 0.0) and xo.agg([nan, nan], "sum") == (0.0, 0, 0.0)
    for how in ("mean", "max", "min"):
        v, n, S = xo.agg([nan], how)
        assert np.isnan(v) and n == 0 and S == 0.0
        assert xo.agg([nan, -2.5, nan], how) == (-2.5, 1, 2.5)
    assert xo.agg([1e16, 1.0, -1e16], "sum") == (1.0, 3, 2e16 + 1.0)
    assert xo.agg([-3.0, -1.0, nan], "max")[0] == -1.0 and xo.agg([3.0, 1.0, nan], "min")[0] == 1.0
    # events that are in no group: NaT, before the axis, behind it, in a step outside every bin
    table = np.zeros((5, 31))
    table[:, 3] = [nan, -1.0, 8.0, 0.0, 5.0]
    bins = np.array([-1, 0, 0, 0, 1, 1, 1, 2], dtype=np.int32)          # (bin 2 lies outside nbins = 2)
    npt.assert_array_equal(xo.event_bins(table, bins, 2, 3), [-1, -1, -1, -1, 1])


def _classes(inp, mtime):
    """How often each special class of input occurs in a case, counted with numpy alone (no oracle: the bins of the
    events are worked out here); ``groups`` counts the (cell, bin) pairs of the bins that hold a step."""
    table, offsets, ts = inp["table"], inp["offsets"], np.asarray(inp["ts"], dtype=np.float64)
    bins = _bin_of_t(inp["years"], inp["edges"])
    nb, C, T = len(inp["edges"]) - 1, len(offsets) - 1, ts.shape[0]
    cell = np.repeat(np.arange(C), np.diff(offsets))
    pos = table[:, sc.COL[mtime]]
    b = np.full(pos.shape, -1, dtype=np.int64)
    on_axis = (pos >= 0) & (pos < T)                       # (NaT compares False)
    b[on_axis] = bins[pos[on_axis].astype(np.int64)]       # _bin_of_t gives -1 outside the edges, never >= nb
    g = b >= 0

    def per_group(mask):
        n = np.zeros((nb, C), dtype=np.int64)
        np.add.at(n, (b[g & mask], cell[g & mask]), 1)
        return n
    n_events = per_group(np.ones(b.shape, dtype=bool))
    has_events = np.diff(offsets) > 0
    imax = table[:, sc.COL["intensity_max"]]
    top = np.full((nb, C), -np.inf)
    sel = g & ~np.isnan(imax)
    np.maximum.at(top, (b[sel], cell[sel]), imax[sel])
    finite = np.stack([(~np.isnan(ts[bins == k])).sum(axis=0) for k in range(nb)])
    steps = np.array([(bins == k).sum() for k in range(nb)])[:, None]
    top_ts = np.stack([np.where(np.isnan(ts[bins == k]), -np.inf, ts[bins == k]).max(axis=0, initial=-np.inf) for k in range(nb)])
    low_ts = np.stack([np.where(np.isnan(ts[bins == k]), np.inf, ts[bins == k]).min(axis=0, initial=np.inf) for k in range(nb)])
    return dict(groups=int((steps > 0).sum()) * C, groups_with_event=int((n_events > 0).sum()), ts_groups_finite=int((finite > 0).sum()),
                empty_cell=int((~has_events).sum()),
                skipped_bin=int(((n_events == 0) & has_events[None, :]).sum()),
                single_event_bin=int((n_events == 1).sum()),
                all_nan_column=int(((per_group(~np.isnan(table[:, sc.COL["rate_onset"]])) == 0)
                                    & (per_group(~np.isnan(table[:, sc.COL["duration"]])) > 0)).sum()),
                all_negative_max=int(((top < 0) & np.isfinite(top)).sum()),
                nat_event=int(np.isnan(pos).sum()), out_of_axis_event=int(((pos < 0) | (pos >= T)).sum()),
                all_nan_ts_group=int(((finite == 0) & (steps > 0)).sum()),
                negative_ts_max=int(((top_ts < 0) & np.isfinite(top_ts)).sum()),
                positive_ts_min=int(((low_ts > 0) & np.isfinite(low_ts)).sum()))


SPECIAL = ["empty_cell", "skipped_bin", "single_event_bin", "all_nan_column", "all_negative_max", "nat_event",
           "out_of_axis_event", "all_nan_ts_group", "negative_ts_max", "positive_ts_min"]


def _device_cases():
    """(label, inputs maker, mtime, C) of every case the GPU tests run, once each"""
    seen, out = set(), []
    for C, T, bl, mtime, dtype, _ in sc.whole_call_cases() + [(c, t, b, m, d, True) for c, t, b, m, d in sc.STRIDE_CASES]:
        if (C, T, bl, mtime) not in seen:
            seen.add((C, T, bl, mtime))
            out.append(pytest.param("whole", (C, T, bl, dtype), mtime, id=f"C{C}-T{T}-bl{bl}-{mtime}"))
    for C, T, mtime, dtype, _ in sc.NARROW_CASES:
        out.append(pytest.param("narrow", (C, T, dtype), mtime, id=f"narrow-C{C}-T{T}-{mtime}"))
    for C, T, dtype in sc.WIDE_CASES:
        out.append(pytest.param("wide", (C, T, dtype), "time_end", id=f"wide-C{C}-T{T}"))
    return out


@pytest.mark.parametrize("which,args,mtime", _device_cases())
def test_generated_cases_hold_every_class(which, args, mtime):
    inp = dict(whole=sc.whole_call_inputs, narrow=sc.narrow_inputs, wide=sc.wide_inputs)[which](*args)
    C, T = len(inp["offsets"]) - 1, inp["ts"].shape[0]
    table, offsets = inp["table"], inp["offsets"]
    assert table.shape == (offsets[-1], 31) and offsets[0] == 0 and inp["ts"].shape == inp["cats"].shape == (T, C)
    assert np.diff(offsets).max(initial=0) <= 40 and (C == 1 or (offsets[1] == 0 and offsets[C] == offsets[C - 1]))
    start, peak, end = (table[:, c] for c in sc.TIME_COLUMNS)
    ok = ~np.isnan(start)
    npt.assert_array_equal(np.isnan(peak) | np.isnan(end), ~ok)
    assert (start[ok] <= peak[ok]).all() and (peak[ok] <= end[ok]).all() and (start[ok] == np.floor(start[ok])).all()
    for c in range(C):                                   # disjoint and in time order (NaT events aside)
        s, e = start[offsets[c]:offsets[c + 1]], end[offsets[c]:offsets[c + 1]]
        s, e = s[~np.isnan(s)], e[~np.isnan(e)]
        assert (s[1:] > e[:-1]).all()
    assert set(np.unique(inp["cats"][~np.isnan(inp["cats"])])) == {-1, 0, 1, 2, 3, 4, 5} and np.isnan(inp["cats"]).any()
    n = _classes(inp, mtime)
    if C == 1:                                  # one cell keeps its events: several groups, more than one event in one
        assert n["groups_with_event"] >= 2 and n["groups_with_event"] > n["single_event_bin"], n
    if C >= 63:
        assert 2 * n["groups_with_event"] >= n["groups"], n
        assert 2 * n["ts_groups_finite"] >= n["groups"], n
    if C >= 255:
        assert all(n[k] >= 5 for k in SPECIAL), n


def test_class_counts_agree_with_the_exact_oracle():
    """the counts above, re-derived from the n the exact oracle returns: the two cannot drift apart"""
    C, T, bl, mtime, dtype = sc.STRIDE_CASES[0]
    inp = sc.whole_call_inputs(C, T, bl, dtype)
    bins = _bin_of_t(inp["years"], inp["edges"])
    nb = len(inp["edges"]) - 1
    ev = xo.event_stats(inp["table"], inp["offsets"], bins, nb, sc.COL[mtime])
    tm = xo.time_stats(inp["ts"], None, bins, nb)
    n = _classes(inp, mtime)
    names = so.MHW_STATS
    onset, dur, top = (ev[k][names.index(s)] for k, s in (("n", "rate_onset"), ("n", "duration"), ("val", "intensity_max_max")))
    assert n["all_nan_column"] == int(((onset == 0) & (dur > 0)).sum())
    assert n["all_negative_max"] == int((top < 0).sum())
    assert n["all_nan_ts_group"] == int((tm["n"] == 0).sum()) and n["ts_groups_finite"] == int((tm["n"] > 0).sum())
    assert n["negative_ts_max"] == int((tm["val"][1] < 0).sum()) and n["positive_ts_min"] == int((tm["val"][2] > 0).sum())
