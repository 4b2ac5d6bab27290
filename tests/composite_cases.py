"""The case generators shared by the host and the GPU tests of mhw_composite(): series, bases, anchor columns made by
construction, class patterns.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

WINDOWS = ((0, 0), (0, 5), (5, 0), (30, 30), (31, 32), (32, 32), (63, 64), (127, 0), (0, 127))
KINDS = ("ends", "word_edges", "one_apart", "window_apart", "all_ones", "empty", "sparse", "dense")


def series(T, C, dtype, seed, Dr=1):
    """A (T, C) series around a (Dr, C) base: anomalies of a few units with zeros (q = 0 adds to n alone), scattered NaN,
    a cell that is all NaN (cell 2), one without a base (cell 3), and, with Dr > 1, a row_of_t that is not monotone.
    Returns ts, base, rows, doy, doys."""
    rng = np.random.default_rng(seed)
    base = np.round(18.0 + 6.0 * rng.random((Dr, C)), 2)
    doys = np.arange(1, Dr + 1) if Dr > 1 else np.zeros(1, dtype=np.int64)
    rows = ((np.arange(T) * 3 + 2) % Dr).astype(np.int32)
    a = np.round(rng.normal(0, 2.0, (T, C)), 3)
    a[rng.random((T, C)) < 0.05] = 0.0
    ts = (base[rows] + a).astype(dtype)
    ts[rng.random((T, C)) < 0.04] = np.nan
    if C > 2:
        ts[:, 2] = np.nan
    if C > 3:
        base[:, 3] = np.nan
    return {"ts": ts, "base": base, "rows": rows, "doy": doys[rows], "doys": doys}


def anchor_columns(T, C, D, seed=3):
    """anchors (T, C) bool: column j is of kind KINDS[j % 8] --
    ends          anchors at steps 0 and T - 1: the windows leave the record on both sides
    word_edges    anchors at 63, 64, 127, 128 (those below T)
    one_apart     two anchors 1 step apart (where the pair moves with the column), windows overlap in D - 1 offsets
    window_apart  two anchors D - 1 apart: the windows share one step
    all_ones      every step is an anchor: every window bit is set, the mask must hold
    empty         no anchor
    sparse, dense random, about T / 40 anchors and every second step"""
    rng = np.random.default_rng(seed)
    A = np.zeros((T, C), dtype=bool)
    for j in range(C):
        kind = KINDS[j % len(KINDS)]
        p = (7 * j) % T
        if kind == "ends":
            A[[0, T - 1], j] = True
        elif kind == "word_edges":
            A[[t for t in (63, 64, 127, 128) if t < T], j] = True
        elif kind == "one_apart":
            A[[p, min(p + 1, T - 1)], j] = True
        elif kind == "window_apart":
            A[[p, min(p + D - 1, T - 1)], j] = True
        elif kind == "all_ones":
            A[:, j] = True
        elif kind == "sparse":
            A[:, j] = rng.random(T) < 1.0 / 40.0
        elif kind == "dense":
            A[:, j] = rng.random(T) < 0.5
    return A


def bitmap(anchors):
    """the layout of xmhw_event_table_bits: uint64 (W, C), bit t & 63 of word t >> 6; the bits at t >= T are zero"""
    T, C = anchors.shape
    W = (T + 63) // 64
    padded = np.zeros((W * 64, C), dtype=np.uint64)
    padded[:T] = anchors
    weights = (np.uint64(1) << np.arange(64, dtype=np.uint64))[None, :, None]
    return (padded.reshape(W, 64, C) * weights).sum(axis=1, dtype=np.uint64)


def table_of(anchors):
    """the anchor table of (T, C) anchors: start == end, the rows of a cell in time order, offsets (C + 1,)"""
    T, C = anchors.shape
    c, t = np.nonzero(anchors.T)
    offsets = np.concatenate(([0], np.cumsum(np.bincount(c, minlength=C)))).astype(np.int64)
    return dict(n=int(t.shape[0]), C=C, offsets=offsets, start=t.astype(np.int32), end=t.astype(np.int32))


def one_class(T):
    return np.zeros(T, dtype=np.int32), 1


def every_step(T):
    """labels that change every step, K = 3"""
    return (np.arange(T) % 3).astype(np.int32), 3


def stretches_of_minus_one(T):
    """two classes with stretches of -1, among them steps 0, 63 and 64 and the last step when T allows"""
    t = np.arange(T)
    k = ((t // 11) % 2).astype(np.int32)
    k[(t // 17) % 3 == 2] = -1
    k[[v for v in (0, 63, 64, T - 1) if v < T]] = -1
    if T > 3:
        k[1] = 1                                             # one labelled step at the least
    return k, 2


def anchor_class_apart(T):
    """class 1 on the isolated steps 5, 45, 85, ... (they become the only anchors of the case), class 0 on every other
    step: with before, after < 40 the class of an anchor differs from the class of every other sample of its window"""
    k = np.zeros(T, dtype=np.int32)
    k[5::40] = 1
    return k, 2


PATTERNS = (one_class, every_step, stretches_of_minus_one)
