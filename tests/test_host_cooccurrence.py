"""mhw_cooccurrence() without a GPU: the host layer (validation, the cells common to both datasets, n_pairs, derived
fields, land) with the oracle (tests/cooccurrence_oracle.py) as the device stage."""
import numpy as np
import numpy.testing as npt
import pytest

import cooccurrence_cases as cx
import cooccurrence_oracle as co
import xmhw_amd
from xmhw_amd import CooccurrenceDataset, XmhwException, mhw_cooccurrence
from xmhw_amd.cooccurrence import MAX_CLASSES, MAX_LAGS, RATIOS, check_view, derived_ratios, n_valid_pairs

T = 203


def run(a, b, **kw):
    return mhw_cooccurrence(a, b, _compute=co.cooccur_tables, **kw)


@pytest.fixture(scope="module")
def pair():
    ta = cx.table(T, 24, seed=1)
    return ta, cx.correlated(ta, T, seed=2)


def test_exported():
    assert "mhw_cooccurrence" in xmhw_amd.__all__ and "CooccurrenceDataset" in xmhw_amd.__all__


def test_cases_contain_what_they_promise(pair):
    ta, tb = pair
    assert ta["start"].min() == 0 and ta["end"].max() == T - 1                      # rows touching both ends
    assert ((ta["start"] <= 63) & (ta["end"] >= 64)).any()                           # a row across a word edge
    assert (ta["start"] == ta["end"]).any() and (np.diff(ta["offsets"]) == 0).any()  # one-step rows, cells without rows
    whole = (ta["start"] == 0) & (ta["end"] == T - 1)
    assert whole.sum() == 1 and np.diff(ta["offsets"])[1] == 1                       # one cell, a single row over the record
    for t in (ta, tb, cx.table(T, 24, seed=3)):
        for c in range(t["C"]):
            s, e = t["start"][t["offsets"][c]:t["offsets"][c + 1]], t["end"][t["offsets"][c]:t["offsets"][c + 1]]
            assert (s <= e).all() and (s[1:] > e[:-1]).all()                         # disjoint and time-ordered
    A = co.dense(ta["start"], ta["end"], ta["offsets"], range(24), T)
    B = co.dense(tb["start"], tb["end"], tb["offsets"], range(24), T)
    Bi = co.dense(*(cx.table(T, 24, seed=3)[k] for k in ("start", "end", "offsets")), range(24), T)
    overlap = lambda X, Y: (X & Y).sum() / max(1, min(X.sum(), Y.sum()))             # noqa: E731
    assert overlap(A[:, 4:], B[:, 4:]) > 0.6 > overlap(A[:, 4:], Bi[:, 4:]) > 0      # correlated against independent seeds


def test_validation_errors(pair):
    ta, tb = pair
    a, b = cx.dataset(ta, T), cx.dataset(tb, T)
    point = cx.dataset(cx.table(T, 1, seed=5), T, point=True)
    for bad in ((a, "b"), (None, b), (a, ta)):
        with pytest.raises(XmhwException, match="EventDatasets"):
            run(*bad)
    with pytest.raises(XmhwException, match="single-point"):
        run(a, point)
    with pytest.raises(XmhwException, match="single-point"):
        run(point, a)
    with pytest.raises(XmhwException, match="same grid"):
        run(a, cx.dataset(tb, T, sshape=(4, 6)))
    renamed = cx.dataset(tb, T)
    renamed.sdims = ("y", "x")
    with pytest.raises(XmhwException, match="same grid"):
        run(a, renamed)
    with pytest.raises(XmhwException, match="time steps"):
        run(a, cx.dataset(cx.table(T + 1, 24, seed=2), T + 1))
    moved = cx.dataset(tb, T)
    moved.time = moved.time + np.timedelta64(1, "D")
    with pytest.raises(XmhwException, match="same time axis"):
        run(a, moved)
    # classes: as in mhw_days_by
    for bad in ("week", np.zeros(T), np.zeros(T - 1, dtype=int), np.zeros((T, 1), dtype=int)):
        with pytest.raises(XmhwException):
            run(a, b, classes=bad)
    long_t = MAX_CLASSES + 1
    la = cx.dataset(cx.table(long_t, 4, seed=1), long_t)
    with pytest.raises(XmhwException, match=f"at most {MAX_CLASSES} classes"):
        run(la, la, classes=np.arange(long_t))
    plain = cx.dataset(ta, T)
    plain.time = np.arange(T)
    with pytest.raises(XmhwException, match="integer array"):
        run(plain, plain, classes="month")
    # lags
    for bad, what in (((), "1 to 64"), (tuple(range(MAX_LAGS + 1)), "1 to 64"), ((0, 1, 0), "distinct"), ((0.5,), "integers"),
                      (((0, 1),), "integers"), ((1 << 31,), "int32"), ("lead", "integers")):
        with pytest.raises(XmhwException, match=what):
            run(a, b, lags=bad)
    # the table itself
    late = cx.dataset(dict(tb, end=np.where(tb["end"] == tb["end"].max(), T, tb["end"]).astype(np.int32)), T)
    with pytest.raises(XmhwException, match="index_end outside the time axis"):
        mhw_cooccurrence(a, late, _compute=lambda va, vb, ca, cb, T, *r: (check_view(vb, cb, T, "b"), co.cooccur_tables)[1](
            va, vb, ca, cb, T, *r))
    swapped = dict(ta, start=ta["start"].copy(), end=ta["end"].copy())
    r0 = int(ta["offsets"][5])
    assert ta["offsets"][6] - r0 >= 2
    for k in ("start", "end"):
        swapped[k][[r0, r0 + 1]] = swapped[k][[r0 + 1, r0]]
    with pytest.raises(XmhwException, match="not in time order"):
        check_view(swapped, np.arange(24), T, "a")
    with pytest.raises(XmhwException, match="outside the table"):
        check_view(ta, np.array([24]), T, "a")
    check_view(ta, np.arange(24), T, "a")
    with pytest.raises(XmhwException, match="stage returned"):
        mhw_cooccurrence(a, b, _compute=lambda *r: np.zeros((1, 1, 4, 23), np.int32))


def test_cell_intersection_under_two_land_masks():
    """a 6 x 4 grid; a has land at cells 1, 9 and the whole line 4, b at cells 2, 9 and the whole line 5: line 4 is alive
    in b only, line 5 in a only, both disappear."""
    keep_a, keep_b = np.ones(24, dtype=bool), np.ones(24, dtype=bool)
    keep_a[[1, 9]] = False
    keep_a[16:20] = False
    keep_b[[2, 9]] = False
    keep_b[20:24] = False
    ta, tb = cx.table(T, int(keep_a.sum()), seed=11), cx.table(T, int(keep_b.sum()), seed=12)
    a, b = cx.dataset(ta, T, keep_a, (6, 4)), cx.dataset(tb, T, keep_b, (6, 4))
    cls, K = cx.runs_with_gaps(T)
    ds = run(a, b, classes=cls, lags=(0, 3))
    common = keep_a & keep_b
    assert common.sum() == 13
    assert isinstance(ds, CooccurrenceDataset) and ds.both.shape == (5, 2, 4, 4) and ds.both.dtype == np.int32
    npt.assert_array_equal(ds.keep, common.reshape(6, 4)[:4])
    npt.assert_array_equal(ds.coords["lat"], [0.0, 10.0, 20.0, 30.0])
    npt.assert_array_equal(ds.klass, np.arange(5))
    npt.assert_array_equal(ds.lag, [0, 3])
    # against the dense arrays placed on the grid by hand
    A, B = np.zeros((T, 24), dtype=bool), np.zeros((T, 24), dtype=bool)
    A[:, keep_a] = co.dense(ta["start"], ta["end"], ta["offsets"], range(ta["C"]), T)
    B[:, keep_b] = co.dense(tb["start"], tb["end"], tb["offsets"], range(tb["C"]), T)
    want = co.reduce_dense(A[:, common], B[:, common], cls, K, (0, 3))
    kg = ds.keep
    for j, name in enumerate(("both", "a_only", "b_only", "onsets")):
        npt.assert_array_equal(getattr(ds, name)[..., kg], want[:, :, j], err_msg=name)
        assert (getattr(ds, name)[..., ~kg] == 0).all()
    assert want[:, :, 0].sum() > 0 and want[:, :, 1].sum() > 0 and want[:, :, 3].sum() > 0
    n = co.n_pairs(cls, K, (0, 3))
    npt.assert_array_equal(ds.n_pairs, n)
    npt.assert_array_equal(ds.neither[..., kg], n[:, :, None] - want[:, :, :3].sum(axis=2))
    assert (ds.neither[..., ~kg] == 0).all() and (ds.neither >= 0).all()
    for f in RATIOS:
        assert np.isnan(getattr(ds, f)[..., ~kg]).all(), f
    assert not np.isnan(ds.p_both[..., kg]).any()
    want_r = co.ratios(*(getattr(ds, f)[..., kg] for f in ("both", "a_only", "b_only", "neither")), n[:, :, None])
    for f in RATIOS:
        npt.assert_allclose(getattr(ds, f)[..., kg], want_r[f], rtol=1e-14, atol=0, err_msg=f)
    # a cell that is ocean in one dataset only is land
    none = np.zeros(24, dtype=bool)
    none[0] = True
    other = np.zeros(24, dtype=bool)
    other[1] = True
    with pytest.raises(XmhwException, match="no ocean cell in common"):
        run(cx.dataset(cx.table(T, 1, seed=1), T, none, (6, 4)), cx.dataset(cx.table(T, 1, seed=1), T, other, (6, 4)))


def test_n_pairs_under_classes_with_gaps():
    cls = np.array([0, 1, -1, 1, 0, -1, -1, 2, 2, 0], dtype=np.int32)
    Tn = cls.shape[0]
    lags = (0, 1, -1, Tn - 1, -(Tn - 1), Tn, -Tn)
    got = n_valid_pairs(cls, 3, lags)
    npt.assert_array_equal(got, co.n_pairs(cls, 3, lags))
    npt.assert_array_equal(got[:, 0], [3, 2, 2])
    npt.assert_array_equal(got[:, 1], [2, 2, 2])                 # t = T - 1 (class 0) has no partner
    npt.assert_array_equal(got[:, 2], [2, 2, 2])                 # t = 0 (class 0) has no partner
    npt.assert_array_equal(got[:, 3], [1, 0, 0])                 # only t = 0
    npt.assert_array_equal(got[:, 4], [1, 0, 0])                 # only t = T - 1
    npt.assert_array_equal(got[:, 5:], 0)
    one = cx.dataset(cx.table(Tn, 1, seed=4), Tn, point=True)
    ds = run(one, one, classes=cls, lags=lags)
    npt.assert_array_equal(ds.n_pairs, got)
    assert (ds.both[:, 5:] == 0).all() and (ds.neither[:, 5:] == 0).all() and np.isnan(ds.p_a[:, 5:]).all()


def test_derived_fields_against_hand_worked_tables():
    #            a hits  b misses  c false alarms  d correct negatives
    both, a_only, b_only, neither = (np.array(v) for v in ([30, 0, 5, 0, 10], [10, 4, 0, 0, 0], [20, 6, 0, 0, 0], [40, 10, 15, 20, 0]))
    n = both + a_only + b_only + neither
    r = derived_ratios(both, a_only, b_only, neither, n)
    nan = np.nan
    npt.assert_allclose(r["p_a"], [0.4, 0.2, 0.25, 0.0, 1.0])
    npt.assert_allclose(r["p_b"], [0.5, 0.3, 0.25, 0.0, 1.0])
    npt.assert_allclose(r["p_both"], [0.3, 0.0, 0.25, 0.0, 1.0])
    npt.assert_allclose(r["lmf"], [30 * 100 / (40 * 50), 0.0, 5 * 20 / 25, nan, 1.0])
    npt.assert_allclose(r["hit_rate"], [0.75, 0.0, 1.0, nan, 1.0])
    npt.assert_allclose(r["false_alarm_rate"], [20 / 60, 6 / 16, 0.0, 0.0, nan])
    npt.assert_allclose(r["false_alarm_ratio"], [0.4, 1.0, 0.0, nan, 0.0])
    npt.assert_allclose(r["csi"], [0.5, 0.0, 1.0, nan, 1.0])
    H, F = 0.75, 1 / 3
    sedi = (np.log(F) - np.log(H) - np.log(1 - F) + np.log(1 - H)) / (np.log(F) + np.log(H) + np.log(1 - F) + np.log(1 - H))
    npt.assert_allclose(r["sedi"], [sedi, nan, nan, nan, nan], rtol=1e-15)
    assert 0 < sedi < 1
    zero = derived_ratios(*(np.zeros(1, int),) * 4, np.zeros(1, int))
    assert all(np.isnan(zero[f]).all() for f in RATIOS)


def test_a_dataset_against_itself(pair):
    ta, _ = pair
    a = cx.dataset(ta, T)
    ds = run(a, a, classes="all", lags=(0,))
    assert (ds.a_only == 0).all() and (ds.b_only == 0).all()
    rows = np.diff(ta["offsets"])
    npt.assert_array_equal(ds.onsets[0, 0].reshape(-1), rows)             # disjoint rows with a step between them
    npt.assert_array_equal(ds.both[0, 0].reshape(-1), [(ta["end"][o0:o1] - ta["start"][o0:o1] + 1).sum()
                                                       for o0, o1 in zip(ta["offsets"][:-1], ta["offsets"][1:])])
    has = rows > 0
    npt.assert_array_equal(ds.csi[0, 0].reshape(-1)[has], 1.0)
    assert np.isnan(ds.csi[0, 0].reshape(-1)[~has]).all() and (~has).any()
    npt.assert_array_equal(ds.n_pairs, [[T]])


def test_b_is_a_shifted_by_three_steps(pair):
    ta, _ = pair
    stays = ta["start"] + 3 <= T - 1                                       # a row pushed off the record entirely is gone
    cell_of_row = np.repeat(np.arange(24), np.diff(ta["offsets"]))
    offsets = np.concatenate([[0], np.cumsum(np.bincount(cell_of_row[stays], minlength=24))])
    tb = dict(ta, n=int(stays.sum()), offsets=offsets, start=(ta["start"][stays] + 3).astype(np.int32),
              end=np.minimum(ta["end"][stays] + 3, T - 1).astype(np.int32))
    assert (ta["end"] + 3 > T - 1).any()
    a, b = cx.dataset(ta, T), cx.dataset(tb, T)
    ds = run(a, b, lags=(3, 0))
    # at lag 3 the valid pairs are t < T - 3: every A step there meets its own copy; the A steps at t >= T - 3 are no pairs
    assert (ds.a_only[0, 0] == 0).all() and (ds.b_only[0, 0] == 0).all()
    A = co.dense(ta["start"], ta["end"], ta["offsets"], range(24), T)
    npt.assert_array_equal(ds.both[0, 0].reshape(-1), A[:T - 3].sum(axis=0))
    cut = A[T - 3:].sum(axis=0)
    assert cut.sum() > 0
    npt.assert_array_equal(A.sum(axis=0) - ds.both[0, 0].reshape(-1), cut)     # the rows cut at the end of the record
    assert ds.a_only[0, 1].sum() > 0 and ds.b_only[0, 1].sum() > 0
    npt.assert_array_equal(ds.n_pairs, [[T - 3, T]])


def test_point_input():
    ta = cx.table(T, 1, seed=21)
    tb = cx.correlated(ta, T, seed=22)
    a, b = cx.dataset(ta, T, point=True), cx.dataset(tb, T, point=True)
    ds = run(a, b, classes="season", lags=(-2, 0, 2))
    assert ds.both.shape == (3, 3) and ds.sdims == () and ds.keep.shape == () and ds.csi.shape == (3, 3)
    npt.assert_array_equal(ds.klass, [0, 1, 2])                           # 203 days from 1 January: DJF, MAM, JJA
    kid = xmhw_amd.days_by.class_labels("season", a.time)
    want = co.cooccur_tables(ta, tb, [0], [0], T, kid, 3, (-2, 0, 2))
    npt.assert_array_equal(ds.both, want[:, :, 0, 0])
    npt.assert_array_equal(ds.onsets, want[:, :, 3, 0])
    assert want[:, :, 0].sum() > 0
    # classes_from_events() works unchanged: the classes are the phases of b
    lab = xmhw_amd.classes_from_events(T, b)
    by_phase = run(a, a, classes=lab)
    npt.assert_array_equal(by_phase.klass, [0, 1])
    assert by_phase.both[1, 0] == ds.both[:, 1].sum()


def test_to_xarray_dims(pair):
    pytest.importorskip("xarray")
    ta, tb = pair
    ds = run(cx.dataset(ta, T), cx.dataset(tb, T), classes="month", lags=(0, 5))
    x = ds.to_xarray()
    assert x["both"].dims == ("klass", "lag", "lat", "lon") and x["sedi"].dims == ("klass", "lag", "lat", "lon")
    assert x["n_pairs"].dims == ("klass", "lag") and x["keep"].dims == ("lat", "lon")
    npt.assert_array_equal(x["lag"].values, [0, 5])
    npt.assert_array_equal(x["klass"].values, np.arange(1, 8))            # 203 days from 1 January
    npt.assert_array_equal(x["lmf"].values, ds.lmf)
