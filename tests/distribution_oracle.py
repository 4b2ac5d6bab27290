"""The oracle of anomaly_distribution(): the definition (include/xmhw_amd.h, "anomaly_distribution()";
xmhw_amd/distribution.py, module docstring) by brute force, in Python integers throughout: the bins by integer floor
division, the power sums as sums of q**3 over Python integers, the ranks from the sorted q of every class and cell.  The
fixed point of csrc/stage_reduce.h is the one lag_correlation_oracle.fixed() restates.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

from lag_correlation_oracle import fixed

NO_SAMPLE = -(1 << 31)
SUMS = ("n", "s1", "s2", "s3", "s4", "kmin", "kmax")
RANKS = ("qbin", "qbelow", "qcount")
FIELDS = SUMS + RANKS + ("n_at_least",)
MASK64 = (1 << 64) - 1


def anomalies(ts, base, rows, shift):
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.asarray(ts).astype(np.float64) - np.asarray(base, dtype=np.float64)[rows]) * 2.0 ** -int(shift)


def rows_of(q, lo_q, width_q, B):
    """the histogram row of every q: 0 UNDER, 1 + b, B + 1 OVER"""
    b = (np.asarray(q, dtype=np.int64) - lo_q) // width_q                  # (numpy's // is the floor, like Python's)
    return np.where(b < 0, 0, np.where(b >= B, B + 1, 1 + b))


def words(S):
    """Python integers (an object array) as (low word, high word) int64 along a new axis 1: 128-bit two's complement"""
    S = np.asarray(S, dtype=object)
    out = np.zeros((S.shape[0], 2) + S.shape[1:], dtype=np.int64)
    for i in np.ndindex(*S.shape):
        v = int(S[i]) & ((1 << 128) - 1)
        lo, hi = v & MASK64, v >> 64
        out[(i[0], 0) + i[1:]] = lo - (1 << 64) if lo >> 63 else lo
        out[(i[0], 1) + i[1:]] = hi - (1 << 64) if hi >> 63 else hi
    return out


def rank(p_q, n):
    return max(1, -((-int(p_q) * int(n)) >> 32))


def distribution_sums(ts, base, rows, shift, classes, K, lo_q, width_q, B, p_q=(), edges=()):
    """ts (T, C) float, base (Dr, C) float64 with rows (T,), classes (T,) in [-1, K).  Returns a dict: hist (K, B + 2, C)
    int32, n int32, s1 and s2 int64, s3 and s4 (K, 2, C) int64 words with S3 and S4 the Python integers, kmin and kmax
    float64 (NaN: none), qbin, qbelow, qcount (K, P, C) and n_at_least (K, L, C) int32, n_range int."""
    ts = np.asarray(ts)
    T, C = ts.shape
    classes = np.asarray(classes)
    q, valid, outside = fixed(ts, base, rows, shift)
    d = anomalies(ts, base, rows, shift)
    row = rows_of(q, lo_q, width_q, B)
    P, L = len(p_q), len(edges)
    out = {"hist": np.zeros((K, B + 2, C), np.int32), "n": np.zeros((K, C), np.int32), "s1": np.zeros((K, C), np.int64),
           "s2": np.zeros((K, C), np.int64), "S3": np.zeros((K, C), object), "S4": np.zeros((K, C), object),
           "kmin": np.full((K, C), np.nan), "kmax": np.full((K, C), np.nan),
           "qbin": np.full((K, P, C), NO_SAMPLE, np.int32), "qbelow": np.zeros((K, P, C), np.int32),
           "qcount": np.zeros((K, P, C), np.int32), "n_at_least": np.zeros((K, L, C), np.int32),
           "sorted": []}
    qo = q.astype(object)
    cols = np.broadcast_to(np.arange(C), (T, C))
    big = 1 << 40
    for k in range(K):
        m = valid & (classes == k)[:, None]
        n = m.sum(axis=0)
        out["n"][k] = n
        out["s1"][k], out["s2"][k] = np.where(m, q, 0).sum(axis=0), np.where(m, q * q, 0).sum(axis=0)
        out["S3"][k], out["S4"][k] = np.where(m, qo ** 3, 0).sum(axis=0), np.where(m, qo ** 4, 0).sum(axis=0)
        some = n > 0
        with np.errstate(invalid="ignore"):
            out["kmin"][k] = np.where(some, np.where(m, d, np.inf).min(axis=0, initial=np.inf) + 0.0, np.nan)
            out["kmax"][k] = np.where(some, np.where(m, d, -np.inf).max(axis=0, initial=-np.inf) + 0.0, np.nan)
        np.add.at(out["hist"][k], (row[m], cols[m]), 1)
        srt = np.sort(np.where(m, q, big), axis=0)                         # the valid q of every cell in order, then `big`
        out["sorted"].append(srt)
        rr = np.where(np.arange(T)[:, None] < n, rows_of(srt, lo_q, width_q, B), B + 5)
        for j, p in enumerate(p_q):
            r = np.array([rank(p, v) for v in n])                           # Python integers
            at = rr[np.minimum(r - 1, T - 1), np.arange(C)]                 # the row of the r-th smallest
            out["qbin"][k, j] = np.where(some, at - 1, NO_SAMPLE)
            out["qbelow"][k, j] = np.where(some, (rr < at).sum(axis=0), 0)
            out["qcount"][k, j] = np.where(some, (rr == at).sum(axis=0), 0)
        for l, e in enumerate(edges):
            out["n_at_least"][k, l] = ((rr >= 1 + e) & (rr <= B + 1)).sum(axis=0)
    out["s3"], out["s4"] = words(out["S3"]), words(out["S4"])
    out["n_range"] = int((outside & (classes >= 0)[:, None]).sum())
    assert (row[valid] >= 0).all()
    return out


def distribution_cells(ts, base, doy, doys, classes, K, lo_q, width_q, B, p_q, edges, shift=0, return_histogram=False,
                       counters=None, **_):
    """the stand-in of the device stage (host tests: _compute=)"""
    rows = np.searchsorted(np.asarray(doys), np.asarray(doy))
    r = distribution_sums(np.asarray(ts), base, rows, shift, classes, K, lo_q, width_q, B, [int(p) for p in p_q],
                          [int(e) for e in edges])
    if counters is not None:
        counters["n_range"] = r["n_range"]
    return tuple(r[k] for k in FIELDS) + ((r["hist"],) if return_histogram else ())
