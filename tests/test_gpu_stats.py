"""block_average() on the device (csrc/kernels_stats.hip) against outputs of the reference's own
agg_mhw / agg_ts / agg_cats (tests/golden/block_stats_cases.npz: made by RUNNING xmhw/stats.py) and,
on a gridded detect() result, against the oracle-driven host path; then both kernels on multi-cell grids
against exact sums (tests/stats_exact_oracle.py) of synthetic cases that hold every class of input the kernels
branch on (tests/stats_cases.py, conditions asserted in tests/test_stats_cases.py): more than one workgroup and
partial waves, every length of the time axis mod the 8 rows block_time loads at a time with a bin edge in the
last group, bins narrower than the axis, NaT and out-of-axis events, empty cells and tables, skipped and
single-event bins, all-negative maxima, all-NaN columns, leading dimensions wider than the grid, and the
refusals of the C ABI."""
import functools
import os

import numpy as np
import numpy.testing as npt
import pandas as pd
import pytest

import stats_cases as sc
import stats_exact_oracle as xo
import stats_oracle as so

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def gpu():
    from xmhw_amd._lib import require_gpu
    require_gpu()
    from xmhw_amd import stats
    return stats


def test_kernels_against_reference_outputs(gpu):
    g = np.load(os.path.join(GOLD, "mhw_features_cases.npz"))
    b = np.load(os.path.join(GOLD, "block_stats_cases.npz"))
    meta = b["event_meta"]
    k_time = 0
    seen = 0
    for case in range(len(g["offsets"]) - 1):
        sl = slice(g["offsets"][case], g["offsets"][case + 1])
        ts, se, th = g["ts"][sl], g["seas"][sl], g["thresh"][sl]
        T = ts.shape[0]
        tab = g["table"][g["table_offsets"][case]:g["table_offsets"][case + 1]]
        years = pd.date_range("2001-01-01", periods=T).year.to_numpy()
        cats = np.floor(1 + (ts - th) / (th - se))
        offsets = np.array([0, tab.shape[0]], dtype=np.int64)
        for blockLength in (1, 2):
            edges = so.block_bins(int(years[0]), int(years[-1]), blockLength)
            for mt, name in ((0, "time_start"), (1, "time_peak")):
                i = int(np.nonzero((meta[:, 0] == case) & (meta[:, 1] == blockLength) & (meta[:, 2] == mt))[0][0])
                want = b["event_stats"][b["event_offsets"][i]:b["event_offsets"][i + 1]]
                res = gpu.block_stats_device(tab, offsets, years, edges, name, ts[:, None], cats[:, None])
                got = np.stack([res[k][:, 0] for k in so.MHW_STATS], axis=1)
                npt.assert_allclose(got, want, rtol=1e-12, atol=0, equal_nan=True)
                seen += want.shape[0]
            wt = b["time_stats"][b["time_offsets"][k_time]:b["time_offsets"][k_time + 1]]
            k_time += 1
            gt = np.stack([res[k][:, 0] for k in so.TIME_STATS], axis=1)
            npt.assert_allclose(gt, wt, rtol=1e-12, atol=0, equal_nan=True)
            npt.assert_array_equal(res["total_days"][:, 0], wt[:, 3:].sum(axis=1))
    assert seen == b["event_stats"].shape[0]


def test_gridded_block_average_equals_oracle_path(gpu):
    """threshold() -> detect(intermediate) -> block_average() on the OISST fixture grid, float32 series"""
    import xmhw_amd
    from xmhw_amd import GridSeries, climatology_series
    from test_host_stats import oracle_compute
    g = np.load(os.path.join(GOLD, "oisst_2003_2004.npz"))
    time = np.datetime64("2003-01-01") + g["time"].astype("timedelta64[D]")
    temp = GridSeries(g["sst"], ("time", "lat", "lon"), {"time": time, "lat": g["lat"], "lon": g["lon"]},
                      time_encoding={"calendar": "proleptic_gregorian"})
    clim = xmhw_amd.threshold(temp, pctile=80)
    mhw, inter = xmhw_amd.detect(temp, climatology_series(clim, "thresh"), climatology_series(clim, "seas"),
                                 intermediate=True)
    assert mhw.n_events > 20
    for kwargs in (dict(period=[2003, 2004]), dict(dstime=temp, blockLength=2), dict(dstime=inter, mtime="time_peak")):
        got = gpu.block_average(mhw, **kwargs)
        want = gpu.block_average(mhw, _compute=oracle_compute, **kwargs)
        assert got.dims == want.dims == ("years", "lat", "lon") and set(got.data_vars) == set(want.data_vars)
        for k in want.data_vars:
            npt.assert_allclose(got[k], want[k], rtol=1e-12, atol=0, equal_nan=True, err_msg=k)
        npt.assert_array_equal(got.coords["years"], want.coords["years"])
    assert "total_days" in got.data_vars and np.nansum(got["ecount"]) == mhw.n_events


# ---- multi-cell grids against exact sums ---------------------------------------------------------------------
# A NaN whose payload no kernel writes.  Read back as float64 it would pass for a NaN default that was written, so
# an output is always read back as uint64 and searched for these bits before it is viewed as float64 (_payload_and_pads)
SENTINEL = np.uint64(0x7FF8DEADBEEF1234)


@pytest.fixture(scope="module")
def dev():
    from xmhw_amd._lib import require_gpu
    require_gpu()
    import xmhw_amd.device as d
    return d


def _inputs(which, C, T, bl, dtype):
    if which == "whole":
        return sc.whole_call_inputs(C, T, bl, dtype)
    return sc.narrow_inputs(C, T, dtype) if which == "narrow" else sc.wide_inputs(C, T, dtype)


@functools.lru_cache(maxsize=8)
def _reference(kind, which, C, T, bl, dtype, mtime=None):
    """exact statistics of a case (kind "events": binned by the column ``mtime``; "time": all 7 time statistics),
    computed once and shared by the tests that follow each other on the same case: read-only"""
    from xmhw_amd.stats import _bin_of_t
    inp = _inputs(which, C, T, bl, dtype)
    bins = _bin_of_t(inp["years"], inp["edges"])
    nb = len(inp["edges"]) - 1
    if kind == "events":
        return xo.event_stats(inp["table"], inp["offsets"], bins, nb, sc.COL[mtime])
    return xo.time_stats(inp["ts"], inp["cats"], bins, nb)


def _time_reference(ref, with_cats):
    return ref if with_cats else dict(val=ref["val"][:3], n=ref["n"], S=ref["S"])


def _check_whole_call(res, inp, ev_ref, t_ref, with_cats, what):
    nb, C = len(inp["edges"]) - 1, len(inp["offsets"]) - 1
    tnames = so.TIME_STATS[:7 if with_cats else 3]
    assert list(res) == so.MHW_STATS + tnames + (["total_days"] if with_cats else [])
    assert all(v.shape == (nb, C) and v.dtype == np.float64 for v in res.values())
    xo.assert_event_stats(np.stack([res[k] for k in so.MHW_STATS]), ev_ref, what)
    xo.assert_time_stats(np.stack([res[k] for k in tnames]), _time_reference(t_ref, with_cats), what)
    if with_cats:
        npt.assert_array_equal(res["total_days"], t_ref["val"][3:].sum(axis=0))


@pytest.mark.parametrize("case", sc.whole_call_cases(), ids=sc.case_id)
def test_whole_call_against_exact_sums(gpu, case):
    """block_stats_device(): the 15 event statistics, the 3 or 7 time statistics and total_days"""
    C, T, bl, mtime, dtype, with_cats = case
    inp = sc.whole_call_inputs(C, T, bl, dtype)
    res = gpu.block_stats_device(inp["table"], inp["offsets"], inp["years"], inp["edges"], mtime, inp["ts"],
                                 inp["cats"] if with_cats else None)
    _check_whole_call(res, inp, _reference("events", "whole", C, T, bl, dtype, mtime),
                      _reference("time", "whole", C, T, bl, dtype), with_cats, sc.case_id(case))


@pytest.mark.parametrize("C,T,mtime,dtype,with_cats", sc.NARROW_CASES)
def test_period_narrower_than_the_axis(gpu, C, T, mtime, dtype, with_cats):
    """one bin, the middle year: the steps and the events before and behind it belong to no bin, in both kernels"""
    inp = sc.narrow_inputs(C, T, dtype)
    res = gpu.block_stats_device(inp["table"], inp["offsets"], inp["years"], inp["edges"], mtime, inp["ts"],
                                 inp["cats"] if with_cats else None)
    ev_ref = _reference("events", "narrow", C, T, None, dtype, mtime)
    assert 0 < ev_ref["val"][0].sum() < 0.6 * inp["table"].shape[0]        # most events are outside the bin
    _check_whole_call(res, inp, ev_ref, _reference("time", "narrow", C, T, None, dtype), with_cats, "narrow")


class _Buffers:
    """device buffers of one test, freed on the way out"""

    def __init__(self, dev):
        self.dev, self.owned = dev, []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for b in self.owned:
            b.free()
        return False

    def upload(self, a):
        self.owned.append(self.dev.DeviceBuffer.from_array(a))
        return self.owned[-1]


def _padded(a, ld, poison):
    out = np.full((a.shape[0], ld), poison, dtype=a.dtype)
    out[:, :a.shape[1]] = a
    return out


def _payload_and_pads(raw, C):
    """(nstat, nbins, ldo) uint64 as read back -> the float64 payload columns: every pad column must still hold the
    sentinel and no payload entry may (a default is WRITTEN, NaN included: compared as bits, not as float64)"""
    npt.assert_array_equal(raw[:, :, C:], SENTINEL, err_msg="pad columns of the output were written")
    left = raw[:, :, :C] == SENTINEL
    assert not left.any(), f"{int(left.sum())} of {left.size} payload entries were never written; (stat, bin, cell) " \
                           f"of the first: {tuple(int(i[0]) for i in np.nonzero(left))}"
    return np.ascontiguousarray(raw[:, :, :C]).view(np.float64)


@pytest.mark.parametrize("C,T,bl,mtime,dtype", sc.STRIDE_CASES)
def test_leading_dimensions_wider_than_the_grid(dev, C, T, bl, mtime, dtype):
    """ld = C + 3, ldcat = C + 5, ldo = C + 7 through the bindings: the pad columns of ts hold 1e30 and those of
    cats 1.0 (a wrong stride moves a sum and a day count), the output is pre-filled with a sentinel: the payload
    matches the exact reference, every pad column of every plane keeps the sentinel.  The pads are written here:
    a DeviceBuffer may be recycled memory."""
    from xmhw_amd.stats import _bin_of_t
    h = dev.hip()
    inp = sc.whole_call_inputs(C, T, bl, dtype)
    nb = len(inp["edges"]) - 1
    ld, ldcat, ldo = C + 3, C + 5, C + 7
    with _Buffers(dev) as s:
        d_bin = s.upload(_bin_of_t(inp["years"], inp["edges"]))
        d_tab, d_off = s.upload(inp["table"]), s.upload(inp["offsets"])
        d_ev = s.upload(np.full((len(so.MHW_STATS), nb, ldo), SENTINEL))
        h.block_events(d_tab.ptr, d_off.ptr, C, d_bin.ptr, T, nb, sc.COL[mtime], d_ev.ptr, ldo)
        d_ts, d_cat = s.upload(_padded(inp["ts"], ld, 1e30)), s.upload(_padded(inp["cats"], ldcat, 1.0))
        d_t7 = s.upload(np.full((7, nb, ldo), SENTINEL))
        h.block_time(d_ts.ptr, np.dtype(dtype).itemsize, T, C, ld, d_cat.ptr, ldcat, d_bin.ptr, nb, d_t7.ptr, ldo)
        d_t3 = s.upload(np.full((3, nb, ldo), SENTINEL))
        h.block_time(d_ts.ptr, np.dtype(dtype).itemsize, T, C, ld, 0, ldcat, d_bin.ptr, nb, d_t3.ptr, ldo)
        h.stream_sync(0)
        ev = d_ev.to_array((len(so.MHW_STATS), nb, ldo), np.uint64)
        t7, t3 = d_t7.to_array((7, nb, ldo), np.uint64), d_t3.to_array((3, nb, ldo), np.uint64)
    t_ref = _reference("time", "whole", C, T, bl, dtype)
    xo.assert_event_stats(_payload_and_pads(ev, C), _reference("events", "whole", C, T, bl, dtype, mtime), "strided")
    xo.assert_time_stats(_payload_and_pads(t7, C), t_ref, "strided, cats")
    xo.assert_time_stats(_payload_and_pads(t3, C), _time_reference(t_ref, False), "strided, no cats")


@pytest.mark.parametrize("C,T,dtype", sc.WIDE_CASES)
def test_bins_without_a_step_hold_written_defaults(dev, C, T, dtype):
    """edges from the year before the axis to two years behind it, through the bindings on outputs pre-filled with
    the sentinel: no step and no event ever reaches the first bin and the last two, so what they hold -- day counts
    0.0, ts statistics NaN, event counts and sums 0.0, the rest NaN -- is the defaults, and they must be written"""
    from xmhw_amd.stats import _bin_of_t
    h = dev.hip()
    inp = sc.wide_inputs(C, T, dtype)
    bins = _bin_of_t(inp["years"], inp["edges"])
    nb = len(inp["edges"]) - 1
    assert nb == len(np.unique(inp["years"])) + 3 and sorted(set(range(nb)) - set(bins.tolist())) == [0, nb - 2, nb - 1]
    with _Buffers(dev) as s:
        d_bin, d_tab, d_off = s.upload(bins), s.upload(inp["table"]), s.upload(inp["offsets"])
        d_ts, d_cat = s.upload(inp["ts"]), s.upload(inp["cats"])
        d_ev, d_t7, d_t3 = (s.upload(np.full((n, nb, C), SENTINEL)) for n in (len(so.MHW_STATS), 7, 3))
        h.block_events(d_tab.ptr, d_off.ptr, C, d_bin.ptr, T, nb, sc.COL["time_end"], d_ev.ptr, C)
        h.block_time(d_ts.ptr, np.dtype(dtype).itemsize, T, C, C, d_cat.ptr, C, d_bin.ptr, nb, d_t7.ptr, C)
        h.block_time(d_ts.ptr, np.dtype(dtype).itemsize, T, C, C, 0, C, d_bin.ptr, nb, d_t3.ptr, C)
        h.stream_sync(0)
        ev = _payload_and_pads(d_ev.to_array((len(so.MHW_STATS), nb, C), np.uint64), C)
        t7 = _payload_and_pads(d_t7.to_array((7, nb, C), np.uint64), C)
        t3 = _payload_and_pads(d_t3.to_array((3, nb, C), np.uint64), C)
    t_ref = _reference("time", "wide", C, T, None, dtype)
    for b in (0, nb - 2, nb - 1):
        assert np.isnan(t_ref["val"][:3, b]).all() and (t_ref["val"][3:, b] == 0.0).all()
    xo.assert_event_stats(ev, _reference("events", "wide", C, T, None, dtype, "time_end"), "wide")
    xo.assert_time_stats(t7, t_ref, "wide, cats")
    xo.assert_time_stats(t3, _time_reference(t_ref, False), "wide, no cats")


def test_table_without_events(gpu, dev):
    """257 cells, no event: counts and sums 0.0, everything else NaN -- through block_stats_device() and, on an
    output pre-filled with a sentinel (the defaults must be WRITTEN: no entry keeps the sentinel's bits), through
    the bindings"""
    C, T = 257, 1096
    years = sc.years_of_axis(T)
    edges = gpu.block_bins([years[0], years[-1]], 1)
    nb = len(edges) - 1
    want = np.full((len(so.MHW_STATS), nb, C), np.nan)
    for j, (_, _, how) in enumerate(so.MHW_AGG):
        if how in ("count", "sum"):
            want[j] = 0.0
    assert np.isnan(want).sum() == 13 * nb * C
    res = gpu.block_stats_device(np.zeros((0, 31)), np.zeros(C + 1, dtype=np.int64), years, edges)
    assert list(res) == so.MHW_STATS
    npt.assert_array_equal(np.stack([res[k] for k in so.MHW_STATS]), want)
    h = dev.hip()
    with _Buffers(dev) as s:
        d_bin = s.upload(gpu._bin_of_t(years, edges))
        d_tab, d_off = s.upload(np.zeros((1, 31))), s.upload(np.zeros(C + 1, dtype=np.int64))
        d_out = s.upload(np.full((len(so.MHW_STATS), nb, C), SENTINEL))
        h.block_events(d_tab.ptr, d_off.ptr, C, d_bin.ptr, T, nb, sc.COL["time_start"], d_out.ptr, C)
        h.stream_sync(0)
        npt.assert_array_equal(_payload_and_pads(d_out.to_array((len(so.MHW_STATS), nb, C), np.uint64), C), want)


@pytest.mark.parametrize("with_ts,with_cats", [(False, False), (True, False), (True, True)])
def test_no_cells_gives_the_keys_of_a_call_with_cells(gpu, with_ts, with_cats):
    """C = 0: nothing is launched; the same keys as the call with cells, every array (nbins, 0)"""
    T = 1096
    years = sc.years_of_axis(T)
    edges = gpu.block_bins([years[0], years[-1]], 2)
    nb = len(edges) - 1

    def call(C):
        return gpu.block_stats_device(np.zeros((0, 31)), np.zeros(C + 1, dtype=np.int64), years, edges, "time_peak",
                                      np.ones((T, C), dtype=np.float32) if with_ts else None,
                                      np.ones((T, C)) if with_cats else None)
    empty, one = call(0), call(1)
    assert list(empty) == list(one) and len(one) == 15 + 3 * with_ts + 5 * with_cats
    assert all(v.shape == (nb, 0) and v.dtype == np.float64 for v in empty.values())
    assert all(v.shape == (nb, 1) for v in one.values())


# C = 5 cells, T = 16 steps, 2 bins, one event per cell; every refusal changes ONE argument of a valid call
_ABI = dict(C=5, T=16, nbins=2, col=3, ld=5, ldcat=5, ldo=5)


@pytest.mark.parametrize("kernel,change", [("events", dict(ldo=4)), ("events", dict(nbins=0)), ("events", dict(T=0)),
                                           ("events", dict(col=-1)), ("events", dict(col=31)),
                                           ("time", dict(ldo=4)), ("time", dict(ld=4)), ("time", dict(ldcat=4)),
                                           ("time", dict(nbins=0)), ("time", dict(T=0)), ("time", dict(itemsize=2))],
                         ids=lambda v: v if isinstance(v, str) else "-".join(f"{k}{x}" for k, x in v.items()))
def test_abi_refusals_launch_nothing(dev, kernel, change):
    """the invalid-argument error of the bindings; the output keeps its sentinel.  The valid call runs first, on a
    second output, so the refusal is the changed argument's."""
    h = dev.hip()
    a = dict(_ABI, itemsize=4)
    C, T, nb = a["C"], a["T"], a["nbins"]
    table = np.zeros((C, 31))
    table[:, 3] = np.arange(C)
    with _Buffers(dev) as s:
        d_bin = s.upload((np.arange(T) // 8).astype(np.int32))
        d_tab, d_off = s.upload(table), s.upload(np.arange(C + 1, dtype=np.int64))
        d_ts, d_cat = s.upload(np.ones((T, C), dtype=np.float32)), s.upload(np.ones((T, C)))
        d_ok, d_out = s.upload(np.full((15, nb, C), SENTINEL)), s.upload(np.full((15, nb, C), SENTINEL))

        def call(a, out):
            if kernel == "events":
                h.block_events(d_tab.ptr, d_off.ptr, a["C"], d_bin.ptr, a["T"], a["nbins"], a["col"], out.ptr, a["ldo"])
            else:
                h.block_time(d_ts.ptr, a["itemsize"], a["T"], a["C"], a["ld"], d_cat.ptr, a["ldcat"], d_bin.ptr, a["nbins"],
                             out.ptr, a["ldo"])
        call(a, d_ok)
        h.stream_sync(0)
        nstat = 15 if kernel == "events" else 7
        assert not (d_ok.to_array((15, nb, C), np.uint64)[:nstat] == SENTINEL).any()
        with pytest.raises(h.InvalidArgument):
            call(dict(a, **change), d_out)
        h.stream_sync(0)
        npt.assert_array_equal(d_out.to_array((15, nb, C), np.uint64), SENTINEL)
