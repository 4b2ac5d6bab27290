"""Cases that drive the sorted-list kernel's capacity-miss path (kernels_sorted.hip, steps 4 / 4b / 4c, pool_order_stats)
on rows PROVEN to miss by tests/sorted_capacity_model.py.  TEST INFRASTRUCTURE ONLY.

Every case is small (33..96 cells, at most 48 daily years): `base + amp * seasonal + noise` with base > amp, so that all
samples of a cell have one sign (the seas tolerance of the GPU test rests on it); cells listed under `crossing` cross 0.
A case names the coverage it must reach (`need`); tests/test_host_sorted_capacity.py asserts it from the model alone, on
the CPU, so that tests/test_gpu_sorted_capacity.py cannot pass vacuously.  `control` cases must have NO proven row (q = 1.0,
0.999, 0.97, 0.03: the top set is smaller than K, no list can have its K stored keys inside it).
"""
import functools

import numpy as np

import xmhw_oracle as ora
import sorted_capacity_model as scm

MIN_WRONG = 20          # proven rows of a case whose thresh would be wrong without the recomputation


def daily(start, stop):
    return ora.add_doy(np.arange(start, stop, dtype="datetime64[D]"))


def years(n, y0=1975):
    """n full daily years with leap days: n tracks"""
    return daily(f"{y0}-01-01", f"{y0 + n}-01-01")


def noleap(n):
    """a 365-day calendar (no doy 60): one chunk, every row regular"""
    d = np.arange(n * 365) % 365 + 1
    return np.where(d >= 60, d + 1, d).astype(np.int64)


def seasonal(T, seed, amp, phase=40.0, base=None, sigma=1.0, quant=None, nan=None, period=365.25):
    """float32 (T, C): base + amp sin(2 pi (t - phase) / period) + N(0, sigma); base defaults to 1.5 amp + 8 (one sign);
    per-cell arrays or scalars; quant: rounded to multiples of it (0: not); nan: share of samples set to NaN"""
    amp = np.atleast_1d(np.asarray(amp, dtype=np.float64))
    C = amp.shape[0]
    full = lambda v, d: np.broadcast_to(np.asarray(d if v is None else v, dtype=np.float64), (C,))     # noqa: E731
    phase, sigma, quant, nan = full(phase, 40.0), full(sigma, 1.0), full(quant, 0.0), full(nan, 0.0)
    base = 1.5 * amp + 8.0 if base is None else full(base, 0.0)
    rng = np.random.default_rng(seed)
    t = np.arange(T)[:, None]
    x = base + amp * np.sin(2 * np.pi * (t - phase) / period) + sigma * rng.normal(size=(T, C))
    qz = quant > 0
    x[:, qz] = np.round(x[:, qz] / quant[qz]) * quant[qz]
    x = x.astype(np.float32)
    x[rng.random((T, C)) < nan] = np.nan
    return x


def exact_k_lists(x, doy, cell, row):
    """NaN out samples of `cell` so that, in the pool of plan row `row`, the list of the window's last day keeps exactly
    K + 1 valid samples and the one before it exactly K (the others stay full)"""
    pl = scm.plan_lists(doy)
    idx, K = pl["idx"][row], pl["K"]
    last = np.argsort(idx.max(axis=1))          # the lists by the day they hold
    for j, keep in ((last[-1], K + 1), (last[-2], K)):
        t = idx[j][idx[j] >= 0]
        assert t.shape[0] > K + 1
        x[t[keep:], cell] = np.nan
    return x


CASES = {}


def case(name, **kw):
    def deco(fn):
        CASES[name] = dict(name=name, build=fn, control=False, crossing=(), packed=None, need=(), alone=())
        CASES[name].update(kw)
        return fn
    return deco


CALM = 0.5      # amplitude of a calm cell: no list ever holds K of the top set


# ---- the records: every (K, KL) of kSorted, both three-wave builds (10, 12, 16 tracks) and two-wave builds ------------

@case("t10_q85", doy=lambda: years(10), C=33, q=0.85, negate=False, K=(6, 6),
      need=("d0", "up_1_32", "nan30", "exact_k", "last_cell", "cell0", "ragged"))
def _t10(doy):
    amp = np.full(33, CALM)
    nan = np.zeros(33)
    amp[[0, 3, 5, 7, 9, 11, 13, 32]] = [30, 10, 300, 300, 1000, 1000, 1000, 100]
    nan[[5, 9, 11, 13]] = [0.3, 0.3, 0.6, 0.8]          # (0.6, 0.8: the attempts at a select without a guess)
    x = seasonal(doy.shape[0], 1010, amp, nan=nan)
    return exact_k_lists(x, doy, 7, 45)


@case("t12_q15", doy=lambda: years(12), C=40, q=0.15, negate=False, K=(6, 6), need=("d0", "up_1_32", "nan30"))
def _t12(doy):
    amp = np.full(40, CALM)
    nan = np.zeros(40)
    amp[[1, 2, 8, 33, 39]] = [30, 100, 1000, 300, 60]
    nan[[8, 33]] = [0.3, 0.8]
    return seasonal(doy.shape[0], 1012, amp, phase=np.linspace(0, 300, 40), nan=nan)


@case("t16_q90_cold", doy=lambda: years(16), C=45, q=0.9, negate=True, K=(8, 8), need=("d0", "up_1_32", "nan30"))
def _t16(doy):
    amp = np.full(45, CALM)
    nan = np.zeros(45)
    amp[[0, 17, 18, 40, 44]] = [100, 30, 30, 1000, 300]
    nan[[40]] = 0.3
    return seasonal(doy.shape[0], 1016, amp, phase=np.linspace(0, 200, 45), nan=nan)


@case("t17_q10_cold", doy=lambda: years(17), C=50, q=0.1, negate=True, K=(10, 10), need=("d0", "up_1_32"))
def _t17(doy):
    amp = np.full(50, CALM)
    amp[[4, 5, 31, 49]] = [60, 300, 100, 1000]
    return seasonal(doy.shape[0], 1017, amp)


@case("t24_q85", doy=lambda: years(24), C=40, q=0.85, negate=False, K=(10, 10), need=("d0", "up_1_32", "far", "nan30"))
def _t24(doy):
    amp = np.full(40, CALM)
    nan = np.zeros(40)
    amp[[0, 6, 7, 21, 39]] = [30, 100, 1000, 300, 60]
    nan[[21]] = 0.3
    return seasonal(doy.shape[0], 1024, amp, nan=nan)


@case("t31_q15", doy=lambda: years(31), C=64, q=0.15, negate=False, K=(12, 12), need=("d0", "up_1_32", "far"))
def _t31(doy):
    amp = np.full(64, CALM)
    amp[[2, 30, 31, 32, 63]] = [30, 100, 1000, 300, 30]
    return seasonal(doy.shape[0], 1031, amp, phase=np.linspace(0, 100, 64))


@case("t36_noleap_q15_cold", doy=lambda: noleap(36), C=40, q=0.15, negate=True, K=(14, 14), need=("d0", "up_1_32", "far"))
def _t36(doy):
    amp = np.full(40, CALM)
    amp[[0, 9, 10, 38]] = [30, 100, 1000, 300]
    return seasonal(doy.shape[0], 1036, amp, period=365.0)


@case("t39_sep_mar_q10", doy=lambda: daily("1983-09-01", "2021-03-15"), C=48, q=0.1, negate=False, K=(16, 14),
      need=("d0", "up_1_32", "far", "nan30"))
def _t39(doy):
    amp = np.full(48, CALM)
    nan = np.zeros(48)
    amp[[0, 1, 20, 33, 47]] = [30, 100, 1000, 300, 100]
    nan[[47]] = 0.3
    return seasonal(doy.shape[0], 1039, amp, phase=np.linspace(0, 340, 48), nan=nan)


@case("t40_waves_q90", doy=lambda: years(40, 1982), C=77, q=0.9, negate=False, K=(16, 14), alone=(0, 33, 70, 76),
      need=("d0", "up_1_32", "far", "one_in_calm_wave", "whole_wave", "adjacent", "ragged", "cell0", "last_cell", "long_run",
            "unproven_after_proven", "isolated", "chunk_edges", "leap_rows"))
def _t40(doy):
    # wave 0: cell 0 steep among 31 calm cells; wave 1: all 32 cells steep, in phase; wave 2 (13 cells): two steep cells in
    # adjacent lane pairs and the last cell of the grid
    amp = np.full(77, CALM)
    amp[0] = 100
    amp[32:64] = 300
    amp[[70, 71, 76]] = [30, 30, 1000]
    return seasonal(doy.shape[0], 1040, amp)


@case("t40_ties_q90", doy=lambda: years(40, 1982), C=40, q=0.9, negate=False, K=(16, 14),
      need=("d0", "up_1_32", "far", "tie", "no_tie", "dup_below", "exact_k", "tiny_pools"))
def _ties(doy):
    amp = np.full(40, CALM)
    quant = np.zeros(40)
    amp[[0, 1, 2, 3, 4, 20, 36]] = [30, 100, 30, 100, 300, 100, 30]
    quant[[0, 1]] = 0.01
    quant[[2, 3, 4, 36]] = 0.5
    x = seasonal(doy.shape[0], 1041, amp, quant=quant)
    x = exact_k_lists(x, doy, 20, 45)
    one = x[5000, 10], x[7000:7002, 11].copy()
    x[:, 10:12] = np.nan                      # pools of n == 1 and of n == 2 (and n == 0 elsewhere)
    x[5000, 10] = one[0]
    x[7000:7002, 11] = one[1]
    return x


@case("t43_q85_cold", doy=lambda: years(43), C=40, q=0.85, negate=True, K=(18, 16), need=("d0", "up_1_32", "far", "nan30"))
def _t43(doy):
    amp = np.full(40, CALM)
    nan = np.zeros(40)
    amp[[0, 14, 15, 39]] = [30, 100, 1000, 300]
    nan[[39]] = 0.3
    return seasonal(doy.shape[0], 1043, amp, nan=nan)


@case("t48_crossing_q90", doy=lambda: years(48, 1970), C=96, q=0.9, negate=False, K=(18, 16), crossing=(5, 95),
      alone=(5,), need=("d0", "up_1_32", "far", "crossing"))
def _t48(doy):
    amp = np.full(96, CALM)
    amp[[5, 40, 64, 95]] = [100, 30, 300, 30]
    base = 1.5 * amp + 8.0
    base[[5, 95]] = 0.0                        # the marked cells cross zero
    return seasonal(doy.shape[0], 1048, amp, base=base)


# ---- controls: the top set is smaller than K -- no row can be proven, the recomputation must not be needed -------------

def _control_data(doy):
    amp = np.full(40, CALM)
    amp[[0, 1, 2, 38, 39]] = [30, 100, 300, 1000, 60]
    return seasonal(doy.shape[0], 2000 + doy.shape[0] % 97, amp, quant=[0.5] + [0.0] * 39)


for _name, _doy, _q, _neg, _K in (("t40_q100", lambda: years(40, 1982), 1.0, False, (16, 14)),
                                  ("t48_q999", lambda: years(48, 1970), 0.999, False, (18, 16)),
                                  ("t40_q97", lambda: years(40, 1982), 0.97, False, (16, 14)),
                                  ("t16_q97_cold", lambda: years(16), 0.97, True, (8, 8)),
                                  ("t40_q03", lambda: years(40, 1982), 0.03, False, (16, 14)),
                                  ("t24_q03_cold", lambda: years(24), 0.03, True, (10, 10))):
    case(_name, doy=_doy, C=40, q=_q, negate=_neg, K=_K)(_control_data)
    CASES[_name]["control"] = True


# ---- int16 codes read in place: 40 tracks, modes 1 and 2, both byte orders ----------------------------------------------

def _codes(doy):
    import test_gpu_packed_oracle as tpo
    return tpo._gen(doy.shape[0], 40, 3040, center=(-500, 500), amp=(3000, 10000), noise=100.0, fillfrac=0.03)


case("packed40_mode1_q90", doy=lambda: years(40, 1982), C=40, q=0.9, negate=False, K=(16, 14),
     need=("d0", "up_1_32", "far", "fill_in_proving"))(_codes)
CASES["packed40_mode1_q90"]["packed"] = "f32_pos"
case("packed40_mode2_q15_cold", doy=lambda: years(40, 1982), C=40, q=0.15, negate=True, K=(16, 14),
     need=("up_1_32", "far", "fill_in_proving"))(_codes)
CASES["packed40_mode2_q15_cold"]["packed"] = "f64_pos"


@functools.lru_cache(maxsize=2)
def load(name):
    """(case, doy, data, x32): data = the float32 series, or the int16 codes of a packed case; x32 = what the kernel keys
    (the series; mode 1: the float32-decoded codes; mode 2: the codes themselves, fill -> NaN).  Read-only."""
    c = CASES[name]
    doy = np.asarray(c["doy"](), dtype=np.int64)
    data = c["build"](doy)
    assert data.shape == (doy.shape[0], c["C"])
    if c["packed"]:
        import test_gpu_packed_oracle as tpo
        from ingest_oracle import decode_cf
        scale, offset, fill, decoded, mode = tpo.RECIPES[c["packed"]]
        if mode == 1:
            x32 = decode_cf(data, dict(scale=scale, offset=offset, fill=fill, out=decoded)).astype(np.float32)
        else:
            assert scale > 0
            x32 = np.where(data == fill, np.nan, data.astype(np.float32)).astype(np.float32)
    else:
        x32 = data
    for a in (doy, data, x32):
        a.setflags(write=False)
    return c, doy, data, x32


@functools.lru_cache(maxsize=2)
def modelled(name):
    c, doy, _, x32 = load(name)
    return scm.model(x32, doy, c["q"], c["negate"])


def forced_nchunks(name):
    """the smallest forced chunk count (2..24) whose cuts make one proven row a chunk's first output row and another
    proven row a chunk's last (None: there is none); found from the kernel's own chunk table"""
    _, doy, _, _ = load(name)
    rows = modelled(name).proven.any(axis=1)
    for nch in range(2, 25):
        ch = scm.plan_lists(doy, nch)["chunks"]
        first = [int(b) for _, b, e, _ in ch if e - b > 1 and rows[b]]
        last = [int(e) - 1 for _, b, e, _ in ch if e - b > 1 and rows[e - 1]]
        if first and last and (len(set(first) | set(last)) > 1):
            return nch
    return None
