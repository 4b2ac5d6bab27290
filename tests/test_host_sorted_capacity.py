"""The capacity-miss cases of the sorted-list kernel (tests/sorted_capacity_cases.py), checked on the CPU against the host
model of the kernel's flag rule (tests/sorted_capacity_model.py).  No GPU: the plan queries run without a device.

For every case:
- the model's pools -- the union of the 11 row-lists the kernel's own step table gives every output row -- are the oracle's
  pools (oracle_fast.pool_index: window_roll from `doy` alone), and the model's true thresh is the oracle's, bit for bit:
  the model does not inherit a table error;
- the model invariant (the kernel's design claim): a row the kernel's rule does not flag has select_only == truth -- in
  particular every row that is not proven and has no list with more than K valid keys; proven rows are flagged rows;
- the coverage the case names (`need`), from the model alone, and at least 20 proven rows whose thresh would be wrong
  without the recomputation; `control` cases have no proven and no flagged row.

Over all cases (test_union_coverage): proven rows on every (K, KL) of kSorted -- records of 10, 12, 16, 17, 24, 31, 36,
39, 40, 43, 48 tracks --, on all four (negate, mirror) and at q = 0.85, 0.9, 0.15, 0.1.

What the model shows UNREACHABLE, with its counts (asserted below, so that a change of the kernel's rule or of K shows):
- stepping DOWN from the guess (next_below, its `v == 0` break): 0 rows in every case.  The stored keys are a subset of
  the pool, so the select's key outside the top set is never above the true one: pool_order_stats only ever steps up
  (next_above), and the answer exists, so the `all ones` break is not reached either.  Distance classes are therefore
  0, 1..32 up, more than 32 (up).
- a select without a guess (`guess == 0`, the stored keys number Cs or fewer) on a proven row: 0 rows in every case,
  NaN shares of 60 % and 80 % at q = 0.85 / 0.15 on the 10- and 12-track records included.  A list stores min(nv, K) keys
  and K >= 0.375 x tracks for every record, Cs <= 0.15 (n - 1) + 1: the stored keys outnumber Cs for every pool that has a
  list of more than K keys.  (Rows with n == 1, mirrored, have Cs = 1 stored key and no guess; they are never flagged.)
- more than 32 steps on the records of 10, 12, 16 and 17 tracks: 0 rows; the largest distance the model finds there is
  8, 18, 16 and 7 (amplitudes up to 1000; q = 0.85, 0.15, 0.9, 0.1).  The keys to step over are hidden keys -- at most
  tracks - K of a list -- that lie between the select's boundary and the true one; a finding of the model, not a proof:
  a sweep of amplitudes 10..3000 at q = 0.9, 0.85, 0.15 found at most 8, 18, 24 and 14 there.  Every record from 24
  tracks on reaches it (asserted).
- proven rows at q = 0.97, 0.03, 0.999, 1.0: 0 rows.  A proving list has its K stored keys inside the top set, and there
  Cs < K for every record (q = 0.97: Cs = 16 of K = 18 at 48 tracks, 6 of 8 at 16; q = 1.0: Cs = 0; q = 0.999 on 48
  tracks: Cs = 1, lo + 1 == n - 1).
"""
import functools

import numpy as np
import pytest

import oracle_fast as fast
import sorted_capacity_cases as scc
import sorted_capacity_model as scm

NAMES = list(scc.CASES)
MIN = 20


def _runs(col):
    """lengths of the runs of True in a 1-D bool array"""
    d = np.diff(np.concatenate([[0], col.astype(np.int8), [0]]))
    return np.nonzero(d == -1)[0] - np.nonzero(d == 1)[0]


@functools.lru_cache(maxsize=None)
def summary(name):
    c, doy, _, x32 = scc.load(name)
    m = scc.modelled(name)
    pl = scm.plan_lists(doy)
    idx, K = pl["idx"], pl["K"]
    s = dict(scm.classes(m))
    s.update(K=(m.K, m.KL), ntracks=m.ntracks, max_distance=int(m.distance[m.proven].max()) if m.proven.any() else 0,
             min_distance=int(m.distance.min()))
    # -- pools and truth against the oracle
    doys, pools = fast.pool_index(doy, scm.W)
    assert m.D == len(doys)
    for r in range(m.D):
        got = idx[r][idx[r] >= 0]
        np.testing.assert_array_equal(np.sort(got), np.sort(pools[r]), err_msg=f"{name}: pool of row {r}")
    xs = x32.astype(np.float64)
    _, th, _ = fast.raw_clim(-xs if c["negate"] else xs, doy, c["q"], scm.W)
    np.testing.assert_array_equal(m.thresh_truth, th, err_msg=f"{name}: the model's truth is not the oracle's thresh")
    # -- invariants
    s["unflagged_wrong"] = int((~m.flagged & ~m.select_is_truth).sum())
    s["stated_invariant_wrong"] = int((~m.proven & ~m.overfull & ~m.select_is_truth).sum())
    s["proven_not_flagged"] = int((m.proven & ~m.flagged).sum())
    s["proving_without_hidden_keys"] = int((m.proving & (m.nv <= K)).sum())
    s["guess_none_flagged"] = int((m.guess_none & m.flagged).sum())
    # -- coverage items
    p, f = m.proven, m.flagged
    C = m.C
    nanshare = np.isnan(x32).mean(axis=0)
    nchange = np.zeros_like(p)
    nchange[1:] = m.n[1:] != m.n[:-1]
    s["nan30"] = int((p & nchange)[:, (nanshare > 0.25) & (nanshare < 0.35)].sum())
    # a list with exactly K valid keys beside a proving one with K + 1
    s["exact_k"] = int((((m.nv == K).any(axis=1)) & ((m.proving & (m.nv == K + 1)).any(axis=1))).sum())
    s["cell0"], s["last_cell"] = int(p[:, 0].sum()), int(p[:, C - 1].sum())
    s["ragged"] = int(p[:, 32 * (C // 32):].sum()) if C % 32 else 0
    waves = [slice(a, min(a + 32, C)) for a in range(0, C, 32)]
    s["one_in_calm_wave"] = int(any(int(p[:, w].any(axis=0).sum()) == 1 and int(f[:, w].any(axis=0).sum()) == 1 for w in waves))
    s["whole_wave"] = int(sum(int(p[:, w].all(axis=1).sum()) for w in waves if w.stop - w.start == 32))
    both = p[:, :-1] & p[:, 1:]
    both[:, 31::32] = False                                     # (cells 31 | 32: not the same wave)
    calm_wave = np.array([not p[:, w].all(axis=1).any() for w in waves])
    s["adjacent"] = int(sum(both[:, w.start:w.stop - 1].sum() for w, ok in zip(waves, calm_wave) if ok))
    s["long_run"] = int(max((_runs(p[:, k]).max(initial=0) for k in range(C)), default=0))
    nxt = np.zeros_like(p)
    nxt[:-1] = ~f[1:] & (m.n[1:] > 0)
    prv = np.zeros_like(p)
    prv[1:] = ~f[:-1] & (m.n[:-1] > 0)
    inner = np.ones(m.D, bool)
    for _, b, e, _ in pl["chunks"]:                             # (the neighbours must be rows of the same chunk)
        inner[[b, e - 1]] = False
    s["unproven_after_proven"] = int((p & nxt)[inner].sum())
    s["isolated"] = int((p & nxt & prv)[inner].sum())
    s["chunk_edges"] = scc.forced_nchunks(name) or 0
    # rows of doy 55..66 of a calendar with leap days; the Feb-29 row itself pools the leap years only (the other tracks'
    # entries carry codes below 2): fewer than K keys a list, never proven
    feb29 = [r for r in range(m.D) if (idx[r] >= 0).sum() < scm.R * m.ntracks // 2]
    s["leap_rows"] = len([r for r in range(54, 66) if p[r].any()]) if feb29 == [59] and not f[59].any() else 0
    s["tiny_pools"] = int(min(((m.n == 1) & ~f).sum(), ((m.n == 2) & ~f).sum()))
    cr = list(c["crossing"])
    s["crossing"] = int(p[:, cr].sum()) if cr and all((x32[:, k] > 0).any() and (x32[:, k] < 0).any() for k in cr) else 0
    one_sign = [k for k in range(C) if k not in cr]
    s["one_signed"] = bool(np.all((np.nan_to_num(x32[:, one_sign], nan=1.0) > 0).all(axis=0)
                                  | (np.nan_to_num(x32[:, one_sign], nan=-1.0) < 0).all(axis=0)))
    pushes = (idx >= 0).sum(axis=2)                             # [D, R]
    s["fill_in_proving"] = int((m.proving & (m.nv < pushes[:, :, None])).sum())
    return s


@pytest.mark.parametrize("name", NAMES)
def test_case_reaches_its_coverage(name):
    c = scc.CASES[name]
    s = summary(name)
    print(name, s)
    assert s["K"] == c["K"], "the record runs on another instantiation than the case was written for"
    # the invariant and the unreachable classes
    assert s["unflagged_wrong"] == 0 and s["stated_invariant_wrong"] == 0
    assert s["proven_not_flagged"] == 0 and s["proving_without_hidden_keys"] == 0
    assert s["min_distance"] >= 0 and s["down_1_32"] == 0, "the select's boundary above the true one"
    assert s["guess_none"] == 0 and s["guess_none_flagged"] == 0
    assert s["one_signed"] or c["packed"]
    if c["control"]:
        assert s["proven"] == 0 and s["flagged"] == 0
        return
    assert s["skip_wrong"] >= scc.MIN_WRONG
    for item in c["need"]:
        floor = {"d0": MIN, "up_1_32": MIN, "far": MIN, "tie": MIN, "no_tie": MIN, "dup_below": MIN, "nan30": MIN, "crossing": MIN,
                 "long_run": 30, "chunk_edges": 2, "leap_rows": 5, "unproven_after_proven": 5, "isolated": 5}.get(item, 1)
        assert s[item] >= floor, (item, s[item], floor)


def test_union_coverage():
    real = {n: summary(n) for n in NAMES if not scc.CASES[n]["control"]}
    proven_on = lambda key: {key(scc.CASES[n], s) for n, s in real.items() if s["proven"] >= MIN}     # noqa: E731
    assert proven_on(lambda c, s: s["K"]) == {(6, 6), (8, 8), (10, 10), (12, 12), (14, 14), (16, 14), (18, 16)}
    assert proven_on(lambda c, s: s["ntracks"]) == {10, 12, 16, 17, 24, 31, 36, 39, 40, 43, 48}
    assert proven_on(lambda c, s: (c["negate"], c["q"] < 0.5)) == {(False, False), (False, True), (True, False), (True, True)}
    assert proven_on(lambda c, s: c["q"]) == {0.85, 0.9, 0.15, 0.1}
    qs = {(c["negate"], c["q"]) for c in scc.CASES.values()}
    assert {(n, q) for n in (False, True) for q in (0.97, 0.03)} <= qs and {(False, 1.0), (False, 0.999)} <= qs
    assert {c["C"] for n, c in scc.CASES.items() if "ragged" in c["need"]} == {33, 77}
    # more than 32 steps: not on the short records (the docstring's figures), on every longer one
    short = {s["ntracks"]: (s["far"], s["max_distance"]) for s in real.values() if s["ntracks"] <= 17}
    assert short == {10: (0, 8), 12: (0, 18), 16: (0, 16), 17: (0, 7)}, short
    assert all(s["far"] >= MIN for s in real.values() if s["ntracks"] >= 24)
    assert {scc.CASES[n]["packed"] for n in real} >= {"f32_pos", "f64_pos"}
