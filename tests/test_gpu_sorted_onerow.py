"""One-row chunks of the sorted-list kernel (Feb 29 of a daily record) settled DIRECTLY (kernels_sorted.hip: direct_row):
the pool read once, its 24 largest keys sorted, the sums in the order of the row-list walk.  The walk is still there
behind XMHW_SORTED_ONEROW=0 (process-wide, read once), so every case (tests/sorted_onerow_cases.py) runs in two fresh child
processes: thresh AND seas must be bit-identical on every row (a NaN equal to a NaN), and each equals the generic kernel on the Feb-29 row by
the rule of tests/test_gpu_sorted.py (thresh bit for bit; seas, a sum in another order, to 1e-12)."""
import os
import subprocess
import sys

import numpy as np
import numpy.testing as npt
import pytest

import sorted_onerow_cases as soc

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SORTED = 40


def _child(tmp, switch):
    out = tmp / f"gpu_{switch}.npz"
    env = dict(os.environ)
    env["XMHW_SORTED_ONEROW"] = switch
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "sorted_onerow_cases.py"), ROOT, "gpu", str(out)],
                       capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    with np.load(out) as d:
        return {k: d[k] for k in d.files}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    from xmhw_amd._lib import require_gpu
    require_gpu()
    tmp = tmp_path_factory.mktemp("onerow_gpu")
    return _child(tmp, "1"), _child(tmp, "0")


CASES = soc.cases()


def _assert_same_bits(a, b, what):
    """bit for bit, signed zeros and infinities included; a NaN equals a NaN -- its sign and payload are those of
    whichever operand the adder forwarded, and the compiler is free to commute a float addition (a pool that holds
    +inf and -inf has a NaN mean on both paths, of either sign)"""
    assert a.shape == b.shape and a.dtype == np.float64 and b.dtype == np.float64
    na, nb = np.isnan(a), np.isnan(b)
    npt.assert_array_equal(na, nb, err_msg=what)
    npt.assert_array_equal(np.where(na, 0, a.view(np.uint64)), np.where(nb, 0, b.view(np.uint64)), err_msg=what)


def _id(no):
    r, C, q, negate = CASES[no]
    return f"{soc.RECORDS[r][0]}-C{C}-q{q}-{'cold' if negate else 'warm'}"


def test_the_cases_cover_what_they_are_meant_to():
    assert {c[0] for c in CASES} == set(range(len(soc.RECORDS)))
    assert {c[1] for c in CASES} == set(soc.CELLS)
    assert {(c[2], c[3]) for c in CASES} >= {(q, neg) for q in soc.QS for neg in (False, True)}


@pytest.mark.parametrize("no", range(len(CASES)), ids=_id)
def test_direct_equals_the_walk_bit_for_bit_and_the_generic_kernel(runs, no):
    on, off = runs
    # the direct path ran in the first child and not in the second
    assert int(on[f"layout_{no}"]) == SORTED and int(off[f"layout_{no}"]) == SORTED
    assert int(on[f"direct_{no}"]) > 0
    assert int(off[f"direct_{no}"]) == 0
    row = int(on[f"row_{no}"])
    for name in ("th", "se"):
        _assert_same_bits(on[f"auto_{name}_{no}"], off[f"auto_{name}_{no}"], name)
    for run in (on, off):
        npt.assert_array_equal(run[f"auto_th_{no}"][row], run[f"generic_th_{no}"][row])
        npt.assert_allclose(run[f"auto_se_{no}"][row], run[f"generic_se_{no}"][row], rtol=1e-12, atol=1e-300, equal_nan=True)
    # (the generic kernel does not know the switch)
    _assert_same_bits(on[f"generic_th_{no}"], off[f"generic_th_{no}"], "generic")
