"""Generators of the random event tables shared by the host and the GPU tests of mhw_cooccurrence().  TEST
INFRASTRUCTURE ONLY.  A table is a dict like EventDataset.compact_view(): n, C, offsets, start, end (and cell_index)."""
import numpy as np


def _intervals(rng, T, mean_len, mean_gap):
    """disjoint, time-ordered (start, end) pairs inside [0, T)"""
    out = []
    t = int(rng.integers(0, mean_gap + 1))
    while t < T:
        e = min(T - 1, t + int(rng.geometric(1.0 / mean_len)) - 1)
        out.append((t, e))
        t = e + 2 + int(rng.geometric(1.0 / mean_gap))                   # at least one step between two rows
    return out


def _special(kind, T):
    if kind == "empty":
        return []
    if kind == "whole":
        return [(0, T - 1)]
    if kind == "ends":                                                    # rows touching step 0 and step T - 1
        return [(0, 0)] if T == 1 else ([(0, 0), (T - 1, T - 1)] if T < 4 else [(0, 1), (T - 2, T - 1)])
    if kind == "edges":                                                   # rows spanning word edges, one-step rows
        rows = [(s, e) for s, e in ((5, 5), (62, 65), (67, 67), (120, 130), (191, 192)) if e < T]
        return rows
    raise ValueError(kind)


SPECIALS = ("empty", "whole", "ends", "edges")


def table(T, C, seed, mean_len=6, mean_gap=9):
    """A random table over C cells: cell j < 4 (where C allows) is SPECIALS[j], every 7th cell has no rows, the others
    random disjoint intervals (one-step rows included: geometric lengths)."""
    rng = np.random.default_rng(seed)
    rows, offsets = [], [0]
    for j in range(C):
        if j < len(SPECIALS) and C > len(SPECIALS):
            r = _special(SPECIALS[j], T)
        elif C == 1:
            r = _intervals(rng, T, mean_len, mean_gap) or [(0, T - 1)]
        elif j % 7 == 6:
            r = []
        else:
            r = _intervals(rng, T, mean_len, mean_gap)
        rows += r
        offsets.append(len(rows))
    arr = np.asarray(rows, dtype=np.int32).reshape(-1, 2)
    return dict(n=len(rows), C=C, offsets=np.asarray(offsets, dtype=np.int64), start=np.ascontiguousarray(arr[:, 0]),
                end=np.ascontiguousarray(arr[:, 1]), cell_index=np.arange(C, dtype=np.int64))


def correlated(a, T, seed, shift=2, drop=0.3):
    """A table correlated with ``a``: its rows moved by up to ``shift`` steps and clipped, some dropped (still disjoint
    and time-ordered: a moved row never reaches its neighbour's old place by more than the gap allows, overlaps are
    merged away)."""
    rng = np.random.default_rng(seed)
    rows, offsets = [], [0]
    for c in range(a["C"]):
        last = -2
        for r in range(int(a["offsets"][c]), int(a["offsets"][c + 1])):
            if rng.random() < drop:
                continue
            d = int(rng.integers(-shift, shift + 1))
            s, e = max(0, int(a["start"][r]) + d), min(T - 1, int(a["end"][r]) + d)
            s = max(s, last + 2)
            if s > e:
                continue
            rows.append((s, e))
            last = e
        offsets.append(len(rows))
    arr = np.asarray(rows, dtype=np.int32).reshape(-1, 2)
    return dict(n=len(rows), C=a["C"], offsets=np.asarray(offsets, dtype=np.int64), start=np.ascontiguousarray(arr[:, 0]),
                end=np.ascontiguousarray(arr[:, 1]), cell_index=np.arange(a["C"], dtype=np.int64))


def runs_with_gaps(T):
    """Five classes in runs of 11 steps with runs of -1 between them (a run of -1 also crosses the first word edge)."""
    k = ((np.arange(T) // 11) % 6).astype(np.int32) - 1
    k[60:70] = -1
    return k, 5


def dataset(tab, T, keep=None, sshape=None, point=False):
    """An EventDataset around a table (index_start / index_end are the only columns filled)."""
    from xmhw_amd import EventDataset
    cols = EventDataset.columns
    t = np.zeros((tab["n"], len(cols)))
    t[:, cols.index("index_start")] = tab["start"]
    t[:, cols.index("index_end")] = tab["end"]
    time = np.datetime64("2001-01-01") + np.arange(T).astype("timedelta64[D]")
    if point:
        return EventDataset(t, tab["offsets"], time, np.array([0]), np.array([True]), (), (), {}, {}, {}, {}, True)
    keep = np.ones(tab["C"], dtype=bool) if keep is None else np.asarray(keep, dtype=bool)
    sshape = (keep.size // 4, 4) if sshape is None else tuple(sshape)
    coords = {"lat": np.arange(sshape[0]) * 10.0, "lon": np.arange(sshape[1]) + 1.0}
    return EventDataset(t, tab["offsets"], time, np.nonzero(keep)[0], keep, ("lat", "lon"), sshape, coords, {}, {}, {}, False)
