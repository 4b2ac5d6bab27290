"""The sorted-list kernel's capacity-miss path (kernels_sorted.hip: the flag of steps 4 / 4c, the recomputation of step 4b,
pool_order_stats) on rows PROVEN to miss.  The cases (tests/sorted_capacity_cases.py) and what each must reach are checked
on the CPU by tests/test_host_sorted_capacity.py against the host model of the flag rule
(tests/sorted_capacity_model.py): proven rows on every (K, KL) of kSorted, guesses 0, 1..32 and more than 32 distinct keys
from the answer (the bit-by-bit search), ties, NaN shares, every wave composition, chunk edges, packed codes of both byte
orders -- and in every case at least 20 proven rows whose thresh would be WRONG if the kernel wrote its select's answer.

For every case, over all rows and cells (proven or not):
- thresh of layout="sorted" is bit for bit the float64 oracle's (oracle_fast.raw_clim) and kernel="generic"'s;
- seas, one-signed cells: rtol 1e-12 against both (at most 11 x 48 = 528 exactly representable addends of one sign: any
  summation order errs by at most (n - 1) 2^-53, about 6e-14, relative); sign-crossing cells: against math.fsum / n within
  n 2^-53 max|x| + 2^-53 |want| (the worst ratio to that bound is printed);
- nchunks = 1 and a forced count that puts proven rows at a chunk's first and last output row: identical bits;
- the proven cells computed alone (C = 1), and the grid with its columns reversed (every cell in another lane pair and
  wave): identical bits;
- ld > C and ldo > C with the base pointers 13 cells into wider arrays: identical bits, the output bytes outside the C
  columns untouched (0xFF), the input columns outside them +Inf (int16: 32767) -- a key read across the pitch would surface;
- packed: thresh bit-equal to the float32 path on the host-decoded series (mode 1), to the oracle on the float64-decoded
  series (mode 2; tests/test_gpu_packed_oracle.py's _check), big-endian codes identical to little-endian ones;
- STATS builds only (hip().debug_stats_available()): the kernel's flag counter >= the model's proven rows (the model's
  rule is sufficient, not necessary).  The normal build says nothing about the counter.

Figures of the first MI355X run, all 20 cases passing in 4.6 s (the model's, printed by every case before it asserts:
proven rows / by distance 0, 1..32, > 32 / ties / rows where skipping the recomputation would be wrong; no case has a
row that steps down):
    t10_q85                   1573 /  203   1370      0 /    0 /  1370
    t12_q15                   1661 /  412   1249      0 /    0 /  1249
    t16_q90_cold              1255 /  123   1132      0 /    0 /  1132
    t17_q10_cold              1195 /   45   1150      0 /    0 /  1150
    t24_q85                   1767 /  104    994    669 /    0 /  1663
    t31_q15                   1846 /  154    674   1018 /    1 /  1682
    t36_noleap_q15_cold       1398 /   54    338   1006 /    3 /  1344
    t39_sep_mar_q10           1481 /   52    672    757 /    0 /  1429
    t40_waves_q90            12289 /   86   1657  10546 /    4 / 12203
    t40_ties_q90              1690 /  222   1134    334 /  829 /  1479
    t43_q85_cold              1325 /   20    644    661 /    1 /  1305
    t48_crossing_q90          1142 /   28    542    572 /    0 /  1114
    packed40_mode1_q90       11434 /  333  10276    825 / 1897 / 11146
    packed40_mode2_q15_cold  12845 /  267   5807   6771 / 2654 / 12622
    the six controls (q = 1.0, 0.999, 0.97, 0.03)   0 proven, 0 flagged by the kernel's rule
t48_crossing_q90, the sign-crossing cells 5 and 95: worst |seas - fsum / n| / bound = 0 and 0 (528 float32 values of one
binade or two: every partial sum is exact in float64, whatever the order).
A counter-twin build (make STATS=1) of the same sources, same machine: the kernel's flag counter EQUALS the model's proven
rows in every case (1573, 1661, 1255, 1195, 1767, 1846, 1398, 1481, 12289, 1325, 1142; 0 in the six controls) but
t40_ties_q90: 1816 flagged by the kernel, 1762 by its LDS-rank rule in the model, 1690 proven (on the two-tier bodies a
saturated list with hidden keys is flagged without the comparison with the boundary).

What the file catches, tried once on scratch copies of the kernel (value-only changes): the select's answer written for
flagged rows, and the stepping loop capped at 4 steps without the bit-by-bit search, each fail the 14 cases that have
proven rows (the first with exactly the model's count of wrong rows where proven == flagged: 1370, 1249, 1132, ...);
4b without its byte swap fails the two packed cases (big-endian against little-endian).  The controls pass all three.
"""
import math

import numpy as np
import numpy.testing as npt
import pytest

import oracle_fast as fast
import sorted_capacity_cases as scc
import sorted_capacity_model as scm

pytestmark = pytest.mark.gpu

SORTED = 40
LEAD = 13            # cells the base pointers are shifted into the wider arrays


@pytest.fixture(scope="module")
def dev():
    from xmhw_amd._lib import require_gpu
    require_gpu()
    import xmhw_amd.device as d
    return d


def _recipe(c):
    import test_gpu_packed_oracle as tpo
    return tpo.RECIPES[c["packed"]] if c["packed"] else None


def _run(dev, c, data, doy, nchunks=0, kernel="auto", layout="sorted", pitched=False, big_endian=False, q=None):
    """one clim_raw / clim_raw_packed launch on `data` (T, C): float32 samples or int16 codes.  `pitched`: the data sit in
    columns [LEAD, LEAD + C) of wider arrays whose other input columns hold +Inf (32767) and whose outputs are prefilled
    with 0xFF bytes.  Returns thresh, seas (D, C), the debug counters and the layout in use."""
    h = dev.hip()
    T, C = data.shape
    packed = data.dtype == np.int16
    lead, ld, ldo = (LEAD, LEAD + C + 6, LEAD + C + 3) if pitched else (0, C, C)
    stored = np.full((T, ld), 32767 if packed else np.inf, dtype=data.dtype)
    stored[:, lead:lead + C] = data
    if big_endian:
        stored = np.ascontiguousarray(stored.astype(">i2")).view(np.int16)
    plan = dev.Plan(doy, 5, kernel=kernel, nchunks=nchunks, layout=layout)
    bufs = []
    try:
        use = plan.layout_in_use()
        D = plan.D
        d_in = dev.DeviceBuffer.from_array(stored); bufs.append(d_in)
        blank = np.full((D, ldo), 0xFF, dtype=np.uint8).repeat(8, axis=1)
        th = dev.DeviceBuffer.from_array(blank); bufs.append(th)
        se = dev.DeviceBuffer.from_array(blank); bufs.append(se)
        isz = stored.dtype.itemsize
        args = (plan, d_in.ptr + isz * lead)
        out = (th.ptr + 8 * lead, se.ptr + 8 * lead)
        h.plan_debug_stats(plan.handle, 1, False)
        if packed:
            scale, offset, fill, decoded, _ = _recipe(c)
            dev.clim_raw_packed(*args, C, c["q"] if q is None else q, c["negate"], *out, scale_factor=scale, add_offset=offset,
                                fill=fill, decoded=decoded, big_endian=big_endian, ld=ld, ldo=ldo)
        else:
            dev.clim_raw(*args, 4, C, c["q"] if q is None else q, c["negate"], *out, ld=ld, ldo=ldo)
        h.stream_sync(0)
        st = h.plan_debug_stats(plan.handle, 1, True)
        res = []
        for b in (th, se):
            raw = b.to_array((D, ldo * 8), np.uint8).reshape(D, ldo, 8)
            outside = np.ones(ldo, bool)
            outside[lead:lead + C] = False
            assert (raw[:, outside] == 0xFF).all(), "the kernel wrote outside its C columns"
            res.append(np.ascontiguousarray(raw[:, lead:lead + C]).view(np.float64)[:, :, 0])
        return res[0], res[1], st, use
    finally:
        for b in bufs:
            b.free()
        plan.destroy()


def _same(a, b, msg):
    npt.assert_array_equal(a[0], b[0], err_msg=f"thresh: {msg}")
    npt.assert_array_equal(a[1], b[1], err_msg=f"seas: {msg}")


def _fsum_seas(x64, doy, cell, negate):
    """(want, bound) per row for one cell: math.fsum of the pool / n and n 2^-53 max|x| + 2^-53 |want|"""
    _, pools = fast.pool_index(doy, 5)
    want = np.full(len(pools), np.nan)
    bound = np.zeros(len(pools))
    col = -x64[:, cell] if negate else x64[:, cell]
    for r, idx in enumerate(pools):
        v = col[idx]
        v = v[~np.isnan(v)]
        if v.size:
            want[r] = math.fsum(v.tolist()) / v.size
            bound[r] = v.size * 2.0 ** -53 * np.abs(v).max() + 2.0 ** -53 * abs(want[r])
    return want, bound


@pytest.mark.parametrize("name", list(scc.CASES))
def test_capacity_misses_are_recomputed_exactly(dev, name):
    import test_gpu_packed_oracle as tpo
    c, doy, data, x32 = scc.load(name)
    m = scc.modelled(name)
    fig = scm.classes(m)
    print(f"\n{name}: K={m.K}/{m.KL} tracks={m.ntracks} proven {fig['proven']} / distance 0: {fig['d0']}  1..32: {fig['up_1_32']}"
          f"  >32: {fig['far']}  down: {fig['down_1_32']} / ties {fig['tie']} / skipping wrong {fig['skip_wrong']}"
          f" / flagged by the kernel's rule {fig['flagged']}")
    assert (fig["proven"] == 0) if c["control"] else (fig["skip_wrong"] >= scc.MIN_WRONG)
    packed = c["packed"] is not None
    C = c["C"]

    got = _run(dev, c, data, doy)
    assert got[3] == SORTED
    # ---- thresh: the oracle and the generic kernel, bit for bit; seas
    if packed:
        recipe = _recipe(c)
        tpo._check(dev, data, doy, c["q"], c["negate"], recipe, got[0], got[1], name)
        big = _run(dev, c, data, doy, big_endian=True)
        _same(big, got, "big-endian codes against little-endian ones")
        if recipe[4] == 1:
            f32 = _run(dev, c, x32, doy)                        # the float32 path on the host-decoded series
            gen = _run(dev, c, x32, doy, kernel="generic", layout=None)
            npt.assert_array_equal(got[0], f32[0], err_msg="thresh: codes in place against the decoded series")
            npt.assert_array_equal(got[0], gen[0], err_msg="thresh: codes in place against the generic kernel")
    else:
        x64 = x32.astype(np.float64)
        _, oth, ose = fast.raw_clim(-x64 if c["negate"] else x64, doy, c["q"], 5)
        gen = _run(dev, c, data, doy, kernel="generic", layout=None)
        npt.assert_array_equal(got[0], oth, err_msg="thresh against the oracle")
        npt.assert_array_equal(got[0], gen[0], err_msg="thresh against the generic kernel")
        npt.assert_array_equal(got[0], m.thresh_truth, err_msg="thresh against the model's truth")
        one = np.array([k not in c["crossing"] for k in range(C)])
        npt.assert_allclose(got[1][:, one], ose[:, one], rtol=1e-12, atol=0, equal_nan=True, err_msg="seas against the oracle")
        npt.assert_allclose(got[1][:, one], gen[1][:, one], rtol=1e-12, atol=0, equal_nan=True, err_msg="seas against generic")
        for k in c["crossing"]:
            want, bound = _fsum_seas(x64, doy, k, c["negate"])
            npt.assert_array_equal(np.isnan(got[1][:, k]), np.isnan(want))
            ok = ~np.isnan(want)
            ratio = np.abs(got[1][ok, k] - want[ok]) / bound[ok]
            print(f"{name}: sign-crossing cell {k}: worst |seas - fsum / n| / bound = {ratio.max():.2g}")
            assert ratio.max() <= 1.0
    # ---- chunk cuts
    forced = scc.forced_nchunks(name) or 5
    for nch in (1, forced):
        _same(_run(dev, c, data, doy, nchunks=nch), got, f"nchunks = {nch}")
    # ---- cell splits
    alone = list(c["alone"]) or [int(k) for k in np.argsort(-m.proven.sum(axis=0), kind="stable")[:2]]
    for k in alone:
        part = _run(dev, c, np.ascontiguousarray(data[:, k:k + 1]), doy)
        _same(part, (got[0][:, k:k + 1], got[1][:, k:k + 1]), f"cell {k} alone")
    rev = _run(dev, c, np.ascontiguousarray(data[:, ::-1]), doy)
    _same((rev[0][:, ::-1], rev[1][:, ::-1]), got, "columns reversed")
    # ---- pitch
    _same(_run(dev, c, data, doy, pitched=True), got, "ld > C, ldo > C, base pointers 13 cells in")
    # ---- counters (STATS builds)
    if dev.hip().debug_stats_available() and not packed:
        print(f"{name}: kernel flag counter {int(got[2][2])}, model proven {fig['proven']}, model flagged {fig['flagged']}")
        assert got[2][0] > 0, "the sorted kernel did not run"
        assert int(got[2][2]) >= fig["proven"]
