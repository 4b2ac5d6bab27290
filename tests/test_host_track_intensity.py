"""Host side of mhw_track_intensity() (xmhw_amd/track_intensity.py) with the device stage replaced by the voxel-by-voxel
oracle (tests/track_intensity_oracle.stage_voxels): the refusals, the alignment with the TrackDataset and the order of
``ids``, quantisation_bound() against the math.fsum ratio of the unquantised weights and anomalies, and the derived
per-object fields."""
import numpy as np
import numpy.testing as npt
import pytest

import objects_oracle as oo
import track_intensity_cases as tc
import track_intensity_oracle as tio
import tracks_oracle as to
from detect_standin import oracle_detect_cells
from xmhw_amd import (GridSeries, TrackIntensityDataset, XmhwException, mhw_objects, mhw_track_intensity, mhw_tracks)
from xmhw_amd.detect import _detect
from xmhw_amd.track_intensity import INTENSITY_BITS, intensity_bits


def detected(g, **kw):
    return _detect(g["temp"], g["th"], g["se"], oracle_detect_cells, **kw)


def chain(g, weights=None, ids=None, **kw):
    mhw = detected(g, **kw)
    obj = mhw_objects(mhw, weights=weights, _compute=oo.objects_graph)
    tr = mhw_tracks(mhw, obj, ids=ids, weights=weights, _compute=to.stage_voxels)
    return mhw, obj, tr


def intensity(g, mhw, obj, tr, weights=None, stage=tio.stage_voxels, **kw):
    return mhw_track_intensity(g["temp"], g["th"], g["se"], mhw, obj, tr, weights=weights, _compute=stage, **kw)


@pytest.fixture(scope="module")
def case():
    g = tc.calendar_grid(420, 5, 7, seed=3, nan_frac=0.03)
    return (g,) + chain(g)


def test_refusals(case):
    g, mhw, obj, tr = case
    for bad in (dict(mhw=obj), dict(obj=tr), dict(tr=obj)):
        a = dict(mhw=mhw, obj=obj, tr=tr)
        a.update(bad)
        with pytest.raises(XmhwException, match="expects"):
            mhw_track_intensity(g["temp"], g["th"], g["se"], a["mhw"], a["obj"], a["tr"], _compute=tio.stage_voxels)
    with pytest.raises(XmhwException, match="weights"):
        intensity(g, mhw, obj, tr, weights="coslat")               # tr was made with uniform weights
    with pytest.raises(XmhwException, match="coldSpells"):
        intensity(g, mhw, obj, tr, coldSpells=True)
    ts = g["temp"].values.copy()
    ts[:, 0, 0] = np.nan                                           # one more land cell than the detection saw
    other = GridSeries(ts, g["temp"].dims, g["temp"].coords)
    th, se = (GridSeries(np.where(np.isnan(ts[:1]), np.nan, a.values), a.dims, a.coords) for a in (g["th"], g["se"]))
    with pytest.raises(XmhwException, match="land mask"):
        mhw_track_intensity(other, th, se, mhw, obj, tr, _compute=tio.stage_voxels)
    point = GridSeries(g["temp"].values[:, 0, 0], ("time",), {"time": g["temp"].coords["time"]})
    with pytest.raises(XmhwException, match="single-point"):
        mhw_track_intensity(point, g["th"], g["se"], mhw, obj, tr, _compute=tio.stage_voxels)
    with pytest.raises(XmhwException, match="dimension not present"):
        intensity(g, mhw, obj, tr, tdim="t")


def test_too_many_entries_and_no_weight_bits(case):
    g, mhw, obj, tr = case
    import copy
    big = copy.copy(tr)
    big.offsets = tr.offsets.copy()
    big.offsets[-1] = 1 << 31
    with pytest.raises(XmhwException):
        intensity(g, mhw, obj, big)
    assert intensity_bits(31, 35) == 31 and intensity_bits(31, 1_036_800) == 61 - 16 - 7 - 20 and intensity_bits(3, 50) == 3
    small = copy.copy(obj)
    small.weight_bits = 0
    with pytest.raises(XmhwException, match="no bits"):
        intensity(g, mhw, small, tr)


def test_anomaly_out_of_range_raises(case):
    g, mhw, obj, tr = case
    start = mhw.table[0, mhw.columns.index("index_start")]
    c = int(mhw.cell_index[0])
    ts = g["temp"].values.copy()
    ts.reshape(ts.shape[0], -1)[int(start), c] += 200.0
    with pytest.raises(XmhwException, match="anomaly"):
        mhw_track_intensity(GridSeries(ts, g["temp"].dims, g["temp"].coords), g["th"], g["se"], mhw, obj, tr,
                            _compute=tio.stage_voxels)


def test_alignment_ids_order_and_derived_fields(case):
    g, mhw, obj, tr = case
    full = intensity(g, mhw, obj, tr)
    assert isinstance(full, TrackIntensityDataset) and full.n_selected == obj.n_objects > 3
    for k in ("ids", "offsets", "time_start", "pos"):
        assert getattr(full, k) is getattr(tr, k)
    assert full.n_valid.dtype == np.int32 and full.cat_cells.dtype == np.int32 and full.cat_cells.shape == (4, tr.offsets[-1])
    assert (full.n_valid <= tr.n_cells).all() and (full.cat_cells.sum(axis=0) <= full.n_valid).all()
    assert (full.n_valid < tr.n_cells).any()                       # the NaN samples are voxels without a value
    ids = np.arange(obj.n_objects)[::-1][::2]
    sub_tr = mhw_tracks(mhw, obj, ids=ids, _compute=to.stage_voxels)
    sub = intensity(g, mhw, obj, sub_tr)
    npt.assert_array_equal(sub.ids, ids)
    for i, o in enumerate(ids):                                    # the subset holds the slices of the full result
        a, b = sub.series(i), full.series(int(o))
        assert set(a) == {"pos", "n_valid", "wsum_i", "isum_q", "intensity_mean", "intensity_max", "cat_cells", "time"}
        for k in a:
            npt.assert_array_equal(a[k], b[k], err_msg=k)
        # the derived per-object fields, restated with Python floats
        mean = [int(q) / (int(w) * 2.0 ** INTENSITY_BITS) for q, w in zip(a["isum_q"], a["wsum_i"]) if w]
        assert sub.intensity_cumulative[i] == pytest.approx(sum(mean), rel=1e-13)
        mx = [v for v in a["intensity_max"] if v == v]
        if mx:
            assert sub.intensity_peak[i] == max(mx)
            assert sub.pos_peak[i] == a["pos"][list(a["intensity_max"]).index(max(mx))]
        else:
            assert np.isnan(sub.intensity_peak[i]) and sub.pos_peak[i] == -1
    with pytest.raises(XmhwException):
        full.series(full.n_selected)
    # unit weights: the mean of the day is the plain mean of rint(a * 2**16) / 2**16
    npt.assert_array_equal(full.wsum_i, full.n_valid.astype(np.int64) << full.intensity_weight_bits)


def test_to_xarray(case):
    pytest.importorskip("xarray")
    g, mhw, obj, tr = case
    ds = intensity(g, mhw, obj, tr).to_xarray()
    assert ds["cat_cells"].shape == (4, int(tr.offsets[-1])) and ds["object_id"].shape == (obj.n_objects,)


@pytest.mark.parametrize("weights", ["coslat", "random"])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_quantisation_bound_against_fsum(seed, weights):
    g = tc.calendar_grid(400, 4, 6, seed=seed, nan_frac=0.02)
    w = "coslat" if weights == "coslat" else g["w"]
    mhw, obj, tr = chain(g, weights=w)
    wf = to.grid_weights(mhw, w)[mhw.cell_index]                   # the float64 weights of the compact cells
    box = {}

    def stage(*a, **k):
        box["r"] = tio.stage_voxels(*a, w=wf, **k)
        return box["r"]

    got = intensity(g, mhw, obj, tr, weights=w, stage=stage)
    want, bound = box["r"]["mean_unquantised"], got.quantisation_bound()
    ok = got.wsum_i > 0
    assert ok.sum() > 20 and np.isnan(bound[~ok]).all() and not np.isnan(want[ok]).any()
    assert (np.abs(got.intensity_mean - want)[ok] <= bound[ok]).all()
    assert bound[ok].max() < 1e-3                                  # the bound says something


def test_cold_spells(case):
    g = tc.calendar_grid(400, 4, 5, seed=7, cold=True)
    mhw, obj, tr = chain(g, coldSpells=True)
    got = intensity(g, mhw, obj, tr, coldSpells=True)
    assert mhw.n_events > 5 and (got.intensity_peak > 0).all()        # the device's sign, before the flip
    with pytest.raises(XmhwException, match="coldSpells"):
        intensity(g, mhw, obj, tr)
