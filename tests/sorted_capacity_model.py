"""A host model (numpy, no GPU) of the one thing the sorted-list kernel's description says can fail: the capacity of a
row-list (xmhw_amd/csrc/kernels_sorted.hip, steps 4 / 4b / 4c and pool_order_stats).  TEST INFRASTRUCTURE ONLY.

The kernel keeps, of the samples all tracks push at one step (a row-list), the K largest keys; the pool of an output
row is the union of its R = 11 last row-lists and the two order statistics numpy's linear quantile needs are read off a
TOP SET of Cs keys.  A list that holds more valid keys than K can hide keys of the top set; the kernel flags such a
cell-row and the whole wave recomputes it from the samples (pool_order_stats, starting from the select's own answer).

For every output row of a plan and every cell this module restates, from the samples and the kernel's OWN step table
(hip().plan_sorted_table, decoded as tests/test_sorted_plan.py decodes it):

  lists        the row's 11 row-lists (time indices), their union checked against oracle_fast.pool_index by the caller;
  keys         the kernel's 32-bit keys: (sign | 0x80000000) ^ bits of the float32 sample, of the NEGATED sample when
               negate != mirror (mirror: q < 0.5, served for q <= 0.15); NaN is no key (0);
  n, lo, Cs    valid keys of the pool, floor((n - 1) q), and the size of the top set: n - 1 - lo, mirrored lo + 1;
  truth        the keys of order statistics lo and min(lo + 1, n - 1) of the full pool;
  select_only  the same two ranks taken over the K largest keys of each list only: what the kernel would write if it
               skipped the recomputation (0 = no such key);
  flagged      the kernel's own rule applied to select_only: some list holds more than K valid keys and its K-th
               largest key lies strictly above the select's key outside the top set;
  proven       some list holds more than K valid keys and its K-th largest key lies strictly above the TRUE key
               outside the top set.  The stored keys are a subset of the pool, so the select's boundary is not above
               the true one: all K stored keys of that list sit inside the select's top set (P[j] == K, or
               pv[j] == EXT on the two-tier bodies) and the last of them above its boundary -- the kernel must flag
               the row.  proven implies flagged; it is a lower bound on the kernel's flag counter;
  distance     the distinct pool keys pool_order_stats has to step over from its guess (the select's key outside the
               top set) to the answer, and the direction: `up` = the guess is below the answer (next_above), `down` =
               above it (next_below).  More than 32: the stepping loop gives up and the bit-by-bit search runs;
  guess_none   the stored keys number Cs or fewer: the select has no key outside the top set, the guess is 0;
  tie          the two true keys are equal (pool_order_stats: vhi = v, the key at its rank is duplicated past it);
  dup_below    the key at pool_order_stats' rank also sits below that rank (cl < lo: `cl <= lo && lo < cl + ev` is
               entered with a count, not at a run's first key).

Everything is vectorised over cells; a 48-year record x 96 cells takes a few seconds.
"""
import functools

import numpy as np

R = 11
W = 5
FAR = 32          # pool_order_stats steps at most this often before it searches bit by bit


def keys_of(x32, kneg):
    """the kernel's keys (key_fast<NEG>): uint32, order of the (negated) samples, -0.0 below +0.0; NaN -> 0"""
    x32 = np.ascontiguousarray(x32, dtype=np.float32)
    b = x32.view(np.uint32)
    if kneg:
        b = b ^ np.uint32(0x80000000)
    k = np.where((b >> np.uint32(31)) != 0, ~b, b | np.uint32(0x80000000)).astype(np.uint32)
    k[np.isnan(x32)] = 0
    return k


def key_values(k, flip):
    """float64 value of a key (key_f32), negated for `flip` (the mirrored epilogue); key 0 -> NaN"""
    k = np.asarray(k, dtype=np.uint32)
    b = np.where((k >> np.uint32(31)) != 0, k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32)
    v = b.view(np.float32).astype(np.float64)
    v = np.where(k == 0, np.nan, v)
    return -v if flip else v


def numpy_lerp(a, b, g):
    """numpy's _lerp (method="linear"), as oracle_fast.raw_clim restates it"""
    with np.errstate(invalid="ignore"):
        d = b - a
        return np.where(g >= 0.5, b - d * (1 - g), a + d * g)


@functools.lru_cache(maxsize=None)
def _plan_lists(doy_bytes, T, pieces):
    from xmhw_amd.device import Plan
    import xmhw_amd.device as dev
    doy = np.frombuffer(doy_bytes, dtype=np.int64)
    plan = Plan(doy, W)
    try:
        K, lds, _ = dev.hip().plan_sorted_info(plan.handle, 64)
        chunks, table, _ = dev.hip().plan_sorted_table(plan.handle, pieces)
        D, ntracks = plan.D, plan.ntracks
    finally:
        plan.destroy()
    chunks = np.asarray(chunks).astype(np.int64)
    code = np.asarray(table).astype(np.int64) >> 1
    idx = np.full((D, R, code.shape[1]), -1, dtype=np.int64)
    served = np.zeros(D, dtype=np.int64)
    for ws, b, e, r0 in chunks:
        assert ws == b - (R - 1)
        for s in range(b, e):
            rows = code[r0 + (s - ws) - (R - 1): r0 + (s - ws) + 1]
            assert rows.shape[0] == R and not np.any(rows == 0), "a held step inside a chunk"
            idx[s] = np.where(rows >= 2, rows - 2, -1)
            served[s] += 1
    assert np.all(served == 1) and idx.max() < T
    idx.setflags(write=False)
    return dict(D=D, K=int(K), lds=int(lds), ntracks=int(ntracks), idx=idx, chunks=chunks)


def plan_lists(doy, pieces=1):
    """the kernel's own partition of every output row's pool into 11 row-lists: dict with D, K (keys a cell keeps of a
    list), lds (bytes per wave), ntracks, idx[D, 11, NTP] (time index of the sample a track pushes into the list, -1:
    nothing) and chunks[(warm_start, begin, end, trow0)] for a row axis cut into `pieces`"""
    doy = np.ascontiguousarray(doy, dtype=np.int64)
    return _plan_lists(doy.tobytes(), doy.shape[0], int(pieces))


def kl_of(K, lds):
    """ranks of a list kept in LDS: the allocation is 11 x KL x 128 bytes rounded up to 1,280"""
    return next(kl for kl in (K, K - 2, K - 4) if (R * kl * 128 + 1279) // 1280 * 1280 == lds)


class Model:
    """the arrays of the module docstring, each [D, C] (keys: uint32, 0 = none)"""


def model(x32, doy, q, negate):
    """x32: the float32 series (T, C) the kernel keys (decoded, for packed input); returns a Model over all cells"""
    pl = plan_lists(doy)
    D, K, idx = pl["D"], pl["K"], pl["idx"]
    x32 = np.asarray(x32, dtype=np.float32)
    T, C = x32.shape
    mirror = q < 0.5
    kneg = bool(negate) != mirror
    keys = np.concatenate([keys_of(x32, kneg), np.zeros((1, C), np.uint32)], axis=0)
    kk = keys[np.where(idx < 0, T, idx)]                         # [D, R, NTP, C]
    kk = np.sort(kk, axis=2)[:, :, ::-1]                         # every list descending, no-keys last
    nv = (kk != 0).sum(axis=2)                                   # [D, R, C]
    ntp = kk.shape[2]
    stored = kk[:, :, :K]
    kth = stored[:, :, K - 1]                                    # a list's K-th largest key (0: fewer than K)
    over = nv > K
    pool = np.sort(kk.reshape(D, R * ntp, C), axis=1)[:, ::-1]   # descending
    spool = np.sort(stored.reshape(D, R * K, C), axis=1)[:, ::-1]
    n = (pool != 0).sum(axis=1)
    nn = np.maximum(n, 1)
    vi = (nn - 1) * q
    lo = np.floor(vi).astype(np.int64)
    g = vi - lo
    need2 = lo + 1 <= nn - 1
    Cs = np.where(mirror, lo + 1, nn - 1 - lo)
    zero = np.zeros((D, 1, C), np.uint32)

    def at(a, i):                                                # a[i] along axis 1, 0 outside
        a = np.concatenate([zero, a, zero], axis=1)
        i = np.clip(i + 1, 0, a.shape[1] - 1)
        return np.take_along_axis(a, i[:, None, :], axis=1)[:, 0]

    m = Model()
    m.D, m.C, m.K, m.KL, m.ntracks = D, C, K, kl_of(K, pl["lds"]), pl["ntracks"]
    m.n, m.lo, m.g, m.Cs, m.need2 = n, lo, g, Cs, need2
    m.nv, m.over = nv, over
    m.t_out, m.t_in = at(pool, Cs), at(pool, Cs - 1)             # largest key outside the top set, smallest inside
    m.s_out, m.s_in = at(spool, Cs), at(spool, Cs - 1)

    def two(out, ins):                                           # (a[lo], a[lo + 1]) as keys
        if mirror:
            return ins, np.where(need2, out, ins)
        return out, np.where(need2, ins, out)

    m.truth = two(m.t_out, m.t_in)
    m.select_only = two(m.s_out, m.s_in)
    valid = n > 0

    def thresh(pair):
        a, b = key_values(pair[0], mirror), key_values(pair[1], mirror)
        return np.where(valid, numpy_lerp(a, b, g), np.nan)

    m.thresh_truth, m.thresh_select = thresh(m.truth), thresh(m.select_only)
    with np.errstate(invalid="ignore"):
        m.skip_wrong = valid & ~((m.thresh_truth == m.thresh_select) | (np.isnan(m.thresh_truth) & np.isnan(m.thresh_select)))
    m.select_is_truth = (m.truth[0] == m.select_only[0]) & (m.truth[1] == m.select_only[1])
    m.proving = over & (kth > m.t_out[:, None, :])               # [D, R, C]: the lists that prove the row
    m.proven = valid & m.proving.any(axis=1)
    m.flagged = valid & (over & (kth > m.s_out[:, None, :])).any(axis=1)
    m.overfull = over.any(axis=1)
    m.guess_none = valid & (np.minimum(nv, K).sum(axis=1) <= Cs)
    # distinct pool keys in (guess, answer] (up) or [answer, guess) (down): the steps from the guess
    first = np.concatenate([np.ones((D, 1, C), bool), pool[:, 1:] != pool[:, :-1]], axis=1) & (pool != 0)
    up = (first & (pool > m.s_out[:, None, :]) & (pool <= m.t_out[:, None, :])).sum(axis=1)
    down = (first & (pool >= m.t_out[:, None, :]) & (pool < m.s_out[:, None, :])).sum(axis=1)
    m.steps_up, m.steps_down = up, down
    m.distance = np.where(m.s_out <= m.t_out, up, -down)
    # pool_order_stats' own rank: ascending index lo of the keys, mirrored n - 2 - lo (0 without a[lo + 1]); descending:
    rank_d = np.where(mirror, np.where(need2, lo + 1, nn - 1), nn - 1 - lo)
    v = at(pool, rank_d)
    m.tie = valid & need2 & (at(pool, rank_d - 1) == v)          # the next key up is the same: vhi = v
    m.dup_below = valid & (rank_d + 1 <= nn - 1) & (at(pool, rank_d + 1) == v)
    return m


def classes(m):
    """rows of the proven set by what pool_order_stats has to do for them: a dict of counts"""
    p = m.proven
    d = m.distance
    return {
        "proven": int(p.sum()),
        "flagged": int(m.flagged.sum()),
        "d0": int((p & (d == 0)).sum()),
        "up_1_32": int((p & (d >= 1) & (d <= FAR)).sum()),
        "down_1_32": int((p & (d <= -1) & (d >= -FAR)).sum()),
        "far": int((p & (np.abs(d) > FAR)).sum()),
        "guess_none": int((p & m.guess_none).sum()),
        "tie": int((p & m.tie).sum()),
        "no_tie": int((p & ~m.tie).sum()),
        "dup_below": int((p & m.dup_below).sum()),
        "skip_wrong": int((p & m.skip_wrong).sum()),
    }
