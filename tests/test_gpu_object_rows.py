"""The one fit rule of the object chain (csrc/object_rows.h, fit_row) across the four stages that walk the table rows:
mhw_tracks(), mhw_track_parts(), mhw_track_genealogy() and mhw_track_shape().  One selected row of a small table is
broken in one clause of the rule at a time; every stage must count exactly that row in n_bad (a slot outside the
selection is no selected row: nothing is counted), deliver what its own oracle delivers for the table with that row
unselected, and its public device function must refuse.  Every input array stays valid memory throughout: a row that is
not fit is rejected before anything is read through it or written for it."""
import numpy as np
import numpy.testing as npt
import pytest

import object_chain_raw as ocr
import objects_cases as oc

pytestmark = pytest.mark.gpu

STAGES = ("tracks", "parts", "genealogy", "shape")
START, END, SLOT, CELL = 0, 1, 2, 3                                 # the first four arguments of every stage
VOX_OFF = dict(parts=7, genealogy=6)                               # vox_off among the arguments of the two voxel stages
CHANGES = ("starts-early", "ends-late", "cell-C", "cell-minus-1", "slot-m")
CASES = [(s, c) for s in STAGES for c in CHANGES] + [(s, "voxels-short") for s in VOX_OFF]


@pytest.fixture(scope="module")
def case():
    """per stage: its module, its device function, its captured arguments on random_grid(3) (every object selected) and its
    oracle; the unbroken table comes out as the oracle has it, nothing counted"""
    from xmhw_amd._lib import require_gpu
    require_gpu()
    import xmhw_amd
    from xmhw_amd import track_genealogy, track_parts, track_shape, tracks
    ds = oc.random_grid(3, T=40)
    obj = xmhw_amd.mhw_objects(ds)
    modules = dict(tracks=(tracks, tracks.tracks_device), parts=(track_parts, track_parts.track_parts_device),
                   genealogy=(track_genealogy, track_genealogy.track_genealogy_device),
                   shape=(track_shape, track_shape.track_shape_device))
    out = {}
    for stage in STAGES:
        kw = dict(lengths="sphere") if stage == "shape" else {}
        args, oracle = ocr.captured_arguments(stage, ds, obj, **kw), ocr.oracle_for(stage, ds, obj)
        assert (args[SLOT] >= 0).all()
        good, bad = ocr.RAW[stage](args)
        assert bad == 0
        same(good, oracle(*args), f"{stage} unbroken")
        out[stage] = modules[stage] + (args, oracle)
    return out


def same(got, want, what):
    assert set(want) <= set(got)
    for k in want:
        npt.assert_array_equal(got[k], want[k], err_msg=f"{what} {k}")


def broken_table(stage, args, change):
    """(the arguments with one selected row broken in ``change``, that row)"""
    cell = args[CELL]
    row = int(np.argmax(args[END] - args[START]))                  # the longest row
    broken = [a.copy() for a in args]
    if change == "starts-early":
        broken[START][row] -= 10_000
    elif change == "ends-late":                                    # the last row of its cell (the rows of a cell follow
        row = int(np.nonzero(cell == cell[row])[0][-1])            # each other): the ends stay in order
        broken[END][row] += 10_000
    elif change == "cell-C":                                       # C: the columns of vec, the cells of row_offsets
        broken[CELL][row] = args[4].shape[1] if stage == "tracks" else args[4].shape[0] - 1
    elif change == "cell-minus-1":
        broken[CELL][row] = -1
    elif change == "slot-m":
        broken[SLOT][row] = args[-2].shape[0]                      # time_start (m,) is the last argument but one
    else:                                                          # its voxel numbers are one short of its days; the
        broken[VOX_OFF[stage]][row + 1:] -= 1                      # rows behind it keep theirs, one lower, and V follows
    return broken, row


@pytest.mark.parametrize("stage, change", CASES)
def test_one_clause_broken(case, stage, change):
    module, device, args, oracle = case[stage]
    broken, row = broken_table(stage, args, change)
    got, bad = ocr.RAW[stage](broken)
    assert bad == (0 if change == "slot-m" else 1)
    without = [a.copy() for a in args]
    without[SLOT][row] = -1
    same(got, oracle(*without), change)
    if bad:
        with pytest.raises(module.XmhwException, match="do not lie within"):
            device(*broken)
