"""mhw_cooccurrence(): per cell, per CLASS of time steps and per LAG, the joint event days of TWO detections -- compound
extremes (a marine heatwave together with a low-chlorophyll, low-oxygen or high-acidity extreme, an atmospheric heatwave
that leads an oceanic one: joint frequency and likelihood multiplication factor, Le Grix et al. 2021; Zscheischler &
Seneviratne 2017) and verification (observed against forecast events, Jacox et al. 2022: the 2x2 contingency table per
cell and lead, hit rate, false-alarm rate and ratio, CSI, SEDI).  Every other stage after detect() takes one detection;
this one takes two event tables and never builds a dense (T, cells) array on the host: each table is rasterised into the
one-bit-per-sample bitmap of exceed_bits on the device and the two bitmaps are reduced by popcounts
(csrc/kernels_cooccur.hip).

The definition.  Two event tables A and B lie on the same time axis of T steps.  For column c and step t, A[t][c] = 1 iff
some table row of that cell has start <= t <= end (gap days of joined events included, as detect() stores them).  B is
defined the same way.  For a lag l (any int32) the pair (t, l) is *valid* iff 0 <= t + l < T.  Then:
    Bl[t] = B[t + l] on valid pairs and 0 otherwise.
    J[t]  = A[t] & Bl[t], with J[-1] = 0.
``class_of_t[T]`` holds int32 labels in [-1, K); -1 counts nowhere.  A pair belongs to the class of t, which is A's step.
For every class k, lag index i and column c, summed over the valid pairs with class_of_t[t] == k:
    counts[k, i, 0, c]  both     A[t] & Bl[t]
    counts[k, i, 1, c]  a_only   A[t] & ~Bl[t]
    counts[k, i, 2, c]  b_only   ~A[t] & Bl[t]
    counts[k, i, 3, c]  onsets   J[t] & ~J[t-1]: the first steps of joint runs
The onset test looks at t - 1 whatever the class of t - 1 is.  ``neither`` is not computed on the device: it is
n_pairs[k, i] - both - a_only - b_only, where n_pairs (the number of valid pairs of class k) is computed on the host from
the labels and the lag.  All counts are int32 and <= T < 2**31.  A lag with |l| >= T gives zeros everywhere.  Everything
is an integer sum, so the result does not depend on the time blocks, the lag groups, the slabs or the schedule.

Host side here (validation, class labels, the cells common to both datasets, slabs, land, derived ratios); device side
behind cooccur_tables().
"""
import numpy as np

from ._lib import hip
from .device import DeviceScope, as_xmhw_errors, device_budget_bytes
from .exception import XmhwException
from .series_stage import (CellFrame, check_class_ids, check_view, class_labels, dense_ids,     # noqa: F401
                           same_axis)                         # (check_view: imported from here too)

MAX_CLASSES = 1024              # XMHW_COOCCUR_MAX_CLASSES (include/xmhw_amd.h)
MAX_LAGS = 64                   # XMHW_COOCCUR_MAX_LAGS
CHANNELS = 4                    # XMHW_COOCCUR_CHANNELS
CHANNEL_NAMES = ("both", "a_only", "b_only", "onsets")
RATIOS = ("p_a", "p_b", "p_both", "lmf", "hit_rate", "false_alarm_rate", "false_alarm_ratio", "csi", "sedi")


def _check_lags(lags):
    arr = np.asarray(lags)
    if arr.ndim == 0:
        arr = arr.reshape(1)
    if arr.ndim != 1 or (arr.size and arr.dtype.kind not in "iu"):
        raise XmhwException(f"lags should be a sequence of integers, got {lags!r}")
    if not 1 <= arr.shape[0] <= MAX_LAGS:
        raise XmhwException(f"mhw_cooccurrence takes 1 to {MAX_LAGS} lags, got {arr.shape[0]}")
    arr = arr.astype(np.int64)
    if arr.min() < -(1 << 31) or arr.max() >= (1 << 31):
        raise XmhwException("lags should fit int32")
    if np.unique(arr).shape[0] != arr.shape[0]:
        raise XmhwException("lags should be distinct")
    return np.ascontiguousarray(arr, dtype=np.int32)


def n_valid_pairs(kid, K, lags):
    """n_pairs (K, L) int64: the valid pairs (t, lag) of every class -- 0 <= t + lag < T, class of t."""
    kid = np.asarray(kid)
    T = kid.shape[0]
    out = np.zeros((K, len(lags)), dtype=np.int64)
    for i, lag in enumerate(int(v) for v in lags):
        lo, hi = max(0, -lag), min(T, T - lag)
        if lo < hi:
            part = kid[lo:hi]
            out[:, i] = np.bincount(part[part >= 0], minlength=K)
    return out


def cooccur_tables(view_a, view_b, cells_a, cells_b, T, classes, K, lags, max_batch_bytes=None):
    """The device stage: ``view_a`` / ``view_b`` are EventDataset.compact_view() dicts, ``cells_a`` / ``cells_b`` the (C,)
    ascending positions of the C common cells in each table, ``classes`` (T,) int labels in [-1, K), ``lags`` (L,) ints.
    Returns counts int32 (K, L, 4, C): both, a_only, b_only, onsets.  Slabs of cells go through the device below
    max_batch_bytes: each uploads the contiguous row range of each table that covers its cells (offsets rebased), is
    rasterised into two bitmaps and ADDS into the accumulator, which lives across the slabs and is read back once."""
    T = int(T)
    classes, K = check_class_ids(T, classes, K, MAX_CLASSES, "mhw_cooccurrence")
    lags = _check_lags(lags)
    L = lags.shape[0]
    cells_a, cells_b = check_view(view_a, cells_a, T, "a"), check_view(view_b, cells_b, T, "b")
    C = cells_a.shape[0]
    if cells_b.shape[0] != C:
        raise XmhwException(f"a and b have {C} and {cells_b.shape[0]} common cells")
    if C == 0 or T == 0:
        return np.zeros((K, L, CHANNELS, C), dtype=np.int32)
    for cells in (cells_a, cells_b):
        if (np.diff(cells) <= 0).any():
            raise XmhwException("cell positions should be ascending")
    if max_batch_bytes is None:
        max_batch_bytes = device_budget_bytes()
    h = hip()
    W = (T + 63) // 64
    rows_per_cell = (view_a["n"] + view_b["n"]) / max(C, 1)
    per_cell = 16 * W + int(8 * rows_per_cell) + 32
    batch = int(max(1, min(C, (max_batch_bytes - 4 * CHANNELS * K * L * C) // per_cell)))
    with DeviceScope() as acc:
        d_counts = acc.alloc(4 * CHANNELS * K * L * C)
        with as_xmhw_errors(also="Unsupported"):
            h.cooccur_init(K, L, C, d_counts.ptr, C)
        for c0 in range(0, C, batch):
            c1 = min(C, c0 + batch)
            n = c1 - c0
            with DeviceScope() as s:
                bits = []
                for view, cells in ((view_a, cells_a[c0:c1]), (view_b, cells_b[c0:c1])):
                    first, last = int(cells[0]), int(cells[-1])
                    off = view["offsets"][first:last + 2]
                    r0, r1 = int(off[0]), int(off[-1])
                    d_start = s.upload(view["start"][r0:r1] if r1 > r0 else np.zeros(1, np.int32))
                    d_end = s.upload(view["end"][r0:r1] if r1 > r0 else np.zeros(1, np.int32))
                    d_off, d_cell = s.upload(off - r0), s.upload(cells - first)
                    d_bits = s.alloc(8 * W * n)
                    with as_xmhw_errors(also="Unsupported"):
                        h.event_table_bits(d_start.ptr, d_end.ptr, d_off.ptr, d_cell.ptr, n, T, d_bits.ptr, n)
                    bits.append(d_bits)
                with as_xmhw_errors(also="Unsupported"):
                    h.cooccur_accumulate(bits[0].ptr, n, bits[1].ptr, n, T, n, classes, K, lags, d_counts.ptr + 4 * c0, C)
                h.stream_sync(0)                        # the slab's buffers are freed on the way out
        h.stream_sync(0)
        return d_counts.to_array((K, L, CHANNELS, C), np.int32)


def _ratio(num, den):
    """num / den in float64, NaN where the denominator is 0"""
    num, den = np.asarray(num, dtype=np.float64), np.asarray(den, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        out = num / den
    out = np.where(den == 0, np.nan, out)
    return out


def derived_ratios(both, a_only, b_only, neither, n_pairs):
    """The float64 fields of a CooccurrenceDataset from its integers (n_pairs broadcast against the counts): a dict over
    RATIOS, NaN where a denominator is 0."""
    both, a_only, b_only, neither = (np.asarray(v, dtype=np.int64) for v in (both, a_only, b_only, neither))
    n = np.broadcast_to(np.asarray(n_pairs, dtype=np.int64), both.shape)
    na, nb = both + a_only, both + b_only
    H, F = _ratio(both, na), _ratio(b_only, b_only + neither)
    with np.errstate(divide="ignore", invalid="ignore"):
        lf, lh, l1f, l1h = np.log(F), np.log(H), np.log(1.0 - F), np.log(1.0 - H)
        sedi = (lf - lh - l1f + l1h) / (lf + lh + l1f + l1h)
    edge = ~((H > 0) & (H < 1) & (F > 0) & (F < 1))               # NaN when H or F is 0, 1 or undefined
    sedi = np.where(edge, np.nan, sedi)
    return {"p_a": _ratio(na, n), "p_b": _ratio(nb, n), "p_both": _ratio(both, n),
            "lmf": _ratio(both.astype(np.float64) * n.astype(np.float64), na.astype(np.float64) * nb.astype(np.float64)),
            "hit_rate": H, "false_alarm_rate": F, "false_alarm_ratio": _ratio(b_only, nb),
            "csi": _ratio(both, both + a_only + b_only), "sedi": sedi}


class CooccurrenceDataset:
    """What mhw_cooccurrence() returns, as plain arrays over (klass, lag, *spatial dims).

    klass (K,) the class labels (sorted non-negative labels found), lag (L,) the lags in the given order, n_pairs (K, L)
    the valid pairs of each class and lag;
    int32 both, a_only, b_only, neither, onsets (K, L, ...) and the boolean ``keep`` (...) mask of the cells that are
    ocean in BOTH datasets;
    float64, NaN where a denominator is 0 and on land: p_a = (both + a_only) / n_pairs, p_b = (both + b_only) / n_pairs,
    p_both = both / n_pairs, lmf = both * n_pairs / ((both + a_only)(both + b_only)), hit_rate H = both / (both + a_only),
    false_alarm_rate F = b_only / (b_only + neither), false_alarm_ratio = b_only / (both + b_only),
    csi = both / (both + a_only + b_only), sedi = (ln F - ln H - ln(1-F) + ln(1-H)) / (ln F + ln H + ln(1-F) + ln(1-H)),
    NaN when H or F is 0 or 1.
    Land: grid lines without a common ocean cell are dropped, as in ClassDaysDataset; float fields are NaN on the remaining
    land cells, integer fields are 0 there."""

    def __init__(self, klass, lag, n_pairs, both, a_only, b_only, onsets, keep, sdims, coords, attrs=None):
        self.klass, self.lag, self.n_pairs = np.asarray(klass), np.asarray(lag), np.asarray(n_pairs, dtype=np.int64)
        self.keep, self.sdims, self.coords, self.attrs = keep, tuple(sdims), dict(coords), dict(attrs or {})
        self.both, self.a_only, self.b_only, self.onsets = both, a_only, b_only, onsets
        n = self.n_pairs.reshape(self.n_pairs.shape + (1,) * (both.ndim - 2))
        ocean = np.broadcast_to(keep, both.shape)
        neither = n - both.astype(np.int64) - a_only - b_only
        self.neither = np.where(ocean, neither, 0).astype(np.int32)
        for name, v in derived_ratios(both, a_only, b_only, self.neither, n).items():
            v[~ocean] = np.nan
            setattr(self, name, v)

    def to_xarray(self):
        import xarray as xr
        cell = ("klass", "lag") + self.sdims
        fields = ("both", "a_only", "b_only", "neither", "onsets") + RATIOS
        data = {f: (cell, getattr(self, f)) for f in fields}
        data["n_pairs"] = (("klass", "lag"), self.n_pairs)
        data["keep"] = (self.sdims, self.keep)
        return xr.Dataset(data, coords=dict({"klass": self.klass, "lag": self.lag}, **{d: self.coords[d] for d in self.sdims if d in self.coords}),
                          attrs=self.attrs)


def mhw_cooccurrence(a, b, classes="all", lags=(0,), max_batch_bytes=None, _compute=None):
    """Per cell, class of time steps and lag: the steps on which the events of ``a`` and of ``b`` coincide.

    ``a`` and ``b`` are the EventDatasets of two detect() calls on the same grid and time axis (``b is a`` is allowed);
    their land masks may differ: the cells of the result are those that are ocean in BOTH, every other cell is land.
    ``classes``: as in mhw_days_by() -- an integer array with one label per time step, or "all", "month" (1..12), "season"
    (DJF, MAM, JJA, SON = 0..3) or "year" from a datetime64 time axis; negative labels count nowhere, the classes of the
    result are the sorted non-negative labels found (at most MAX_CLASSES).  ``lags``: 1 to MAX_LAGS distinct integers, kept
    in the given order; a positive lag pairs A at t with B at t + lag (A leads).  In verification terms A is the
    observation and B the forecast: hit_rate = both / (both + a_only).

    Returns a CooccurrenceDataset.  ``_compute``: a stand-in for cooccur_tables() (host tests)."""
    from .detect import EventDataset
    if not isinstance(a, EventDataset) or not isinstance(b, EventDataset):
        raise XmhwException("mhw_cooccurrence expects the two EventDatasets returned by xmhw_amd.detect()")
    if bool(a.point) != bool(b.point):
        raise XmhwException("mhw_cooccurrence cannot pair a single-point series with a grid")
    if tuple(a.sdims) != tuple(b.sdims) or tuple(a.sshape) != tuple(b.sshape):
        raise XmhwException(f"a and b are not on the same grid: {a.sdims} {a.sshape} and {b.sdims} {b.sshape}")
    time = np.asarray(a.time)
    T = time.shape[0]
    if np.asarray(b.time).shape[0] != T:
        raise XmhwException(f"a and b have {T} and {np.asarray(b.time).shape[0]} time steps")
    if not same_axis(time, b.time):
        raise XmhwException("a and b do not have the same time axis")
    found, kid, K = dense_ids(class_labels(classes, time), MAX_CLASSES, "mhw_cooccurrence", "classes")
    lags = _check_lags(lags)
    L = lags.shape[0]
    view_a = a.compact_view()
    view_b = view_a if b is a else b.compact_view()
    if a.point:
        cells_a = cells_b = np.zeros(1, dtype=np.int64)
        common = np.zeros(1, dtype=np.int64)
    else:
        ia, ib = view_a["cell_index"], view_b["cell_index"]
        for idx in (ia, ib):
            if idx.size and (np.diff(idx) <= 0).any():
                raise XmhwException("cell_index should be ascending")
        common = np.intersect1d(ia, ib)
        if common.size == 0:
            raise XmhwException("a and b have no ocean cell in common")
        cells_a, cells_b = np.searchsorted(ia, common).astype(np.int64), np.searchsorted(ib, common).astype(np.int64)
    C = int(common.shape[0])
    stage = _compute or cooccur_tables
    extra = {"max_batch_bytes": max_batch_bytes} if (_compute is None and max_batch_bytes is not None) else {}
    counts = np.asarray(stage(view_a, view_b, cells_a, cells_b, T, kid, K, lags, **extra))
    if counts.shape != (K, L, CHANNELS, C):
        raise XmhwException(f"co-occurrence stage returned {counts.shape}, expected {(K, L, CHANNELS, C)}")
    counts = counts.astype(np.int32)
    n_pairs = n_valid_pairs(kid, K, lags)
    klass = found if found.shape[0] else np.zeros(1, dtype=np.int64)
    attrs = {"classes": classes if isinstance(classes, str) else "array",
             "xmhw_parameters_a": a.attrs.get("xmhw_parameters", ""), "xmhw_parameters_b": b.attrs.get("xmhw_parameters", "")}
    keep = np.zeros(1 if a.point else int(np.prod(tuple(a.sshape))), dtype=bool)
    keep[common] = True
    f = CellFrame(keep, common, a.point, a.sdims, a.sshape, a.coords)
    return CooccurrenceDataset(klass, lags, n_pairs, *(f.place(counts[:, :, j], 0, np.int32) for j in range(CHANNELS)), f.keep,
                               f.sdims, f.coords, attrs)
