"""The detect-stage kernels (csrc/kernels_detect.hip, kernels_events.hip, event_walk.h) one by one through their
bindings, on the planted cases of tests/detect_cases.py, against the loop oracles -- with every array on a leading
dimension of its own (ld, ldt, ldc, ldo, ldv, ldb all different and all wider than the grid), poisoned pad columns
in the inputs and 0xFF canaries around the outputs, and once with offset pointers into wider resident arrays.
The end-to-end tests (test_gpu_detect.py, test_gpu_features.py, test_gpu_detect_api.py) always pass ld == C."""
import numpy as np
import numpy.testing as npt
import pytest

import detect_cases as dc

pytestmark = pytest.mark.gpu

CASES = dc.gpu_cases()
PITCH = dict(ld=3, ldt=5, ldc=6, ldo=7, ldv=9, ldb=2)          # columns added to C
DENSE = dict.fromkeys(PITCH, 0)
INTEGER_COLUMNS = (0, 1, 2, 3, 4, 5, 17, 18, 19, 20, 21, 27, 28)   # as test_gpu_detect_api._compare


@pytest.fixture(scope="module")
def h():
    from xmhw_amd._lib import hip, require_gpu
    require_gpu()
    return hip()


def _padded(a, ld, poison):
    out = np.empty((a.shape[0], ld), dtype=a.dtype)
    out[:, :a.shape[1]] = a
    out[:, a.shape[1]:] = poison
    return out


class _Out:
    def __init__(self, buf, rows, ld, dtype, c0, c1, what):
        self.buf, self.rows, self.ld, self.dtype, self.c0, self.c1, self.what = buf, rows, ld, np.dtype(dtype), c0, c1, what
        self.ptr = buf.ptr + self.dtype.itemsize * c0


class _Run:
    """The device side of one case: inputs laid out with the pitches C + extra[...] (pad columns poisoned: 1e30 in
    ts, -1e30 in thresh, NaN in seas, 0x7FFFFFFF in events), output buffers pre-filled with 0xFF bytes and one row
    longer than the call needs.  With ``block=(a, b)`` the arrays keep their width and cells [a, b) are addressed
    through offset pointers."""

    def __init__(self, h, r, case, extra, block=None):
        from xmhw_amd.device import DeviceBuffer
        self._new = DeviceBuffer
        self.h, self.bufs = h, []
        self.T, Cw, dtype, cold, (self.m, jg, self.gap) = case
        self.jg, self.neg = int(jg), int(cold)
        self.off, end = block if block else (0, Cw)
        self.C = end - self.off
        self.isz = np.dtype(dtype).itemsize
        self.rows = r["row_of_t"]
        self.D = r["thresh"].shape[0]
        for k, v in extra.items():
            setattr(self, k, Cw + v)
        self.ts = self._up(_padded(r["x"], self.ld, 1e30), self.isz)
        self.th_t = self._up(_padded(r["thresh"], self.ldt, -1e30), 8)
        self.se = self._up(_padded(r["seas"], self.ldc, np.nan), 8)
        self.th_c = self._up(_padded(r["thresh"], self.ldc, -1e30), 8)
        self.ev = self._up(_padded(r["events"], self.ldo, 0x7FFFFFFF), 4)
        offs = r["offsets"][self.off:end + 1] - r["offsets"][self.off]
        self.ntot = int(offs[-1])
        self.offsets = self._up(offs, 0)

    def _up(self, a, itemsize):
        b = self._new.from_array(a)
        self.bufs.append(b)
        return b.ptr + itemsize * self.off

    def out(self, rows, ld, dtype, what, cols=None):
        """(rows + 1, ld) elements of 0xFF bytes; the call may write columns [off, off + C) (or ``cols``) of the
        first ``rows`` rows"""
        c0, c1 = cols if cols else (self.off, self.off + self.C)
        b = self._new((rows + 1) * ld * np.dtype(dtype).itemsize)
        self.bufs.append(b)
        self.h.memset(b.ptr, 0xFF, b.nbytes)
        return _Out(b, rows, ld, dtype, c0, c1, what)

    def read(self, o):
        """the written region; every other byte of the buffer must still be 0xFF"""
        self.h.stream_sync(0)
        full = o.buf.to_array((o.rows + 1, o.ld), o.dtype)
        raw = full.view(np.uint8).reshape(o.rows + 1, o.ld, o.dtype.itemsize)
        outside = np.ones((o.rows + 1, o.ld), dtype=bool)
        outside[:o.rows, o.c0:o.c1] = False
        assert (raw[outside] == 0xFF).all(), f"{o.what}: written outside its {o.rows} rows / columns [{o.c0}, {o.c1})"
        return full[:o.rows, o.c0:o.c1].copy()

    def free(self):
        for b in self.bufs:
            b.free()
        self.bufs = []

    # ---- the kernels -------------------------------------------------------------------------------------------
    def detect_events(self, optional=True):
        T, C = self.T, self.C
        ev, st, en = (self.out(T, self.ldo, np.int32, k) for k in ("events", "start", "end"))
        b = self.out(T, self.ldo, np.uint8, "bthresh")
        n = self.out(1, self.off + C + 1, np.int32, "nevents")
        self.h.detect_events(self.ts, self.isz, T, C, self.ld, self.th_t, self.ldt, self.rows, self.m, self.jg, self.gap,
                             self.neg, ev.ptr, st.ptr, en.ptr, b.ptr if optional else 0, self.ldo, n.ptr if optional else 0)
        got = dict(events=self.read(ev), start=self.read(st), end=self.read(en), bthresh=self.read(b),
                   nevents=self.read(n)[0])
        return got, st

    def event_stats(self):
        tab = self.out(1, self.ntot * 31 + 1, np.float64, "event table", cols=(0, self.ntot * 31))
        self.h.event_stats(self.ts, self.isz, self.T, self.C, self.ld, self.se, self.th_c, self.ldc, self.rows, self.neg,
                           self.ev, self.ldo, self.offsets, tab.ptr)
        return self.read(tab).reshape(self.ntot, 31)

    def event_intermediate(self):
        T = self.T
        out = self.out(8 * T, self.ldv, np.float64, "intermediate planes")
        dur = self.out(4 * T, self.ldv, np.uint8, "duration planes")
        self.h.event_intermediate(self.ts, self.isz, T, self.C, self.ld, self.se, self.th_c, self.ldc, self.rows, self.neg,
                                  self.ev, self.ldo, out.ptr, self.ldv, dur.ptr)
        return self.read(out).reshape(8, T, self.C), self.read(dur).reshape(4, T, self.C)

    def bits_chain(self):
        """exceed_bits -> events_from_bits (count) -> offsets_from_counts -> events_from_bits (fill) ->
        event_stats_sparse: (words (W, C), counts, offsets, table).  The bit buffer has exactly W rows and the canary
        row behind them, all-ones words like the pad columns: a walk that read either would see exceedances."""
        T, C = self.T, self.C
        W = (T + 63) // 64
        bits = self.out(W, self.ldb, np.uint64, "bits")
        self.h.exceed_bits(self.ts, self.isz, T, C, self.ld, self.th_t, self.ldt, self.D, self.rows, self.neg, bits.ptr,
                           self.ldb)
        n = self.out(1, self.off + C + 1, np.int32, "nevents (bits)")
        self.h.events_from_bits(bits.ptr, T, C, self.ldb, self.m, self.jg, self.gap, 0, n.ptr, 0)
        off = self.out(1, C + 2, np.int64, "offsets", cols=(0, C + 1))
        self.h.offsets_from_counts(n.ptr, C, off.ptr)
        counts, offsets = self.read(n)[0], self.read(off)[0]
        ntot = int(offsets[-1])
        tab = self.out(1, ntot * 31 + 1, np.float64, "event table (bits)", cols=(0, ntot * 31))
        if ntot:
            self.h.events_from_bits(bits.ptr, T, C, self.ldb, self.m, self.jg, self.gap, off.ptr, 0, tab.ptr)
            self.h.event_stats_sparse(self.ts, self.isz, T, C, self.ld, self.se, self.th_c, self.ldc, self.rows, self.neg,
                                      ntot, tab.ptr)
        return self.read(bits), counts, offsets, self.read(tab).reshape(ntot, 31)


def _same_bits(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, what
    npt.assert_array_equal(a.view(np.uint64) if a.dtype == np.float64 else a,
                           b.view(np.uint64) if b.dtype == np.float64 else b, err_msg=what)


def _words(bthresh):
    T, C = bthresh.shape
    words = np.zeros(((T + 63) // 64, C), dtype=np.uint64)
    for t in range(T):
        words[t // 64] |= bthresh[t].astype(np.uint64) << np.uint64(t % 64)
    return words


def _assert_table(got, r, what):
    want = r["table"]
    assert got.shape == want.shape, what
    for k in INTEGER_COLUMNS:
        npt.assert_array_equal(got[:, k], want[:, k], err_msg=f"{what}: column {k}")
    npt.assert_allclose(got, want, rtol=1e-9, atol=1e-11, equal_nan=True, err_msg=what)


@pytest.mark.parametrize("case", CASES, ids=dc.case_id)
def test_detect_events_and_count_events_on_pitched_arrays(h, case):
    r = dc.case_with_oracle(case)
    run = _Run(h, r, case, PITCH)
    try:
        got, d_start = run.detect_events()
        for k in ("events", "start", "end", "bthresh"):
            npt.assert_array_equal(got[k], r[k], err_msg=k)
        npt.assert_array_equal(got["nevents"], r["counts"])
        # bthresh and nevents are optional outputs: null pointers change nothing else
        bare, _ = run.detect_events(optional=False)
        for k in ("events", "start", "end"):
            npt.assert_array_equal(bare[k], r[k], err_msg=f"{k} (bthresh = nevents = 0)")
        assert (bare["bthresh"] == 0xFF).all() and (bare["nevents"] == -1).all()
        n = run.out(1, run.C + 1, np.int32, "count_events")
        h.count_events(d_start.ptr, run.T, run.C, run.ldo, n.ptr)
        counted = run.read(n)[0]
        npt.assert_array_equal(counted, got["nevents"])
        npt.assert_array_equal(counted, np.sum(got["start"] >= 0, axis=0))
    finally:
        run.free()


@pytest.mark.parametrize("case", CASES, ids=dc.case_id)
def test_event_stats_on_pitched_arrays(h, case):
    r = dc.case_with_oracle(case)
    run, dense = _Run(h, r, case, PITCH), None
    try:
        got = run.event_stats()
        _assert_table(got, r, "event_stats")
        # per-cell arithmetic does not depend on the pitch: the same call on contiguous arrays, bit for bit
        dense = _Run(h, r, case, DENSE)
        _same_bits(got, dense.event_stats(), "pitched against contiguous")
    finally:
        run.free()
        if dense:
            dense.free()


@pytest.mark.parametrize("case", CASES, ids=dc.case_id)
def test_event_intermediate_on_pitched_arrays(h, case):
    """elementwise float64 in the oracle's order: identical values (NaN where the oracle has NaN, zeros of the same
    sign), as test_intermediate_kernel_matches_reference_mhw_df requires"""
    r = dc.case_with_oracle(case)
    run = _Run(h, r, case, PITCH)
    try:
        out, dur = run.event_intermediate()
    finally:
        run.free()
    npt.assert_array_equal(out, r["inter"])
    valued = ~np.isnan(r["inter"])
    npt.assert_array_equal(np.signbit(out[valued]), np.signbit(r["inter"][valued]))
    npt.assert_array_equal(dur, r["dur"])


@pytest.mark.parametrize("case", CASES, ids=dc.case_id)
def test_bit_path_on_pitched_arrays(h, case):
    r = dc.case_with_oracle(case)
    want_words = _words(r["bthresh"])
    run = _Run(h, r, case, PITCH)
    try:
        table = run.event_stats()
        for mode in (1, 2):                          # exceedance bits: per-step kernel, tiled kernel
            h.set_exceed_kernel(mode)
            words, counts, offsets, sparse = run.bits_chain()
            npt.assert_array_equal(words, want_words, err_msg=f"exceed_bits mode {mode}")
            npt.assert_array_equal(counts, r["counts"], err_msg=f"events_from_bits mode {mode}")
            npt.assert_array_equal(offsets, r["offsets"], err_msg=f"offsets_from_counts mode {mode}")
            # as test_table_only_path_equals_per_step_path: the same per-event arithmetic in the same order
            _same_bits(sparse, table, f"event_stats_sparse against event_stats, mode {mode}")
            _assert_table(sparse, r, f"event_stats_sparse mode {mode}")
    finally:
        h.set_exceed_kernel(0)
        run.free()


BLOCK_CASES = [c for c in CASES if c[:3] in ((129, 257, np.float32), (300, 257, np.float64))]


@pytest.mark.parametrize("case", BLOCK_CASES, ids=dc.case_id)
def test_a_column_block_through_offset_pointers_equals_the_block_alone(h, case):
    """cells [a, b) of wider resident arrays: every pointer advanced by a elements, the full width as the pitch.
    The block holds planted cells and crosses a 128-thread block boundary."""
    a, b = 5, 140
    wide = dc.case_with_oracle(case)
    T, _, dtype, cold, params = case
    alone = {k: (np.ascontiguousarray(v[:, a:b]) if k in ("x", "seas", "thresh", "events") else v) for k, v in wide.items()}
    alone["offsets"] = wide["offsets"][a:b + 1] - wide["offsets"][a]
    inside, outside = _Run(h, wide, case, DENSE, block=(a, b)), None
    try:
        outside = _Run(h, alone, (T, b - a, dtype, cold, params), DENSE)
        assert inside.ntot == outside.ntot > 0
        got, _ = inside.detect_events()
        ref, _ = outside.detect_events()
        for k in ref:
            npt.assert_array_equal(got[k], ref[k], err_msg=k)
            npt.assert_array_equal(got[k], (wide["counts"][a:b] if k == "nevents" else wide[k][:, a:b]), err_msg=k)
        _same_bits(inside.event_stats(), outside.event_stats(), "event_stats")
        for g, w, k in zip(inside.event_intermediate(), outside.event_intermediate(), ("planes", "durations")):
            _same_bits(g, w, f"event_intermediate {k}")
        for mode in (1, 2):
            h.set_exceed_kernel(mode)
            for g, w, k in zip(inside.bits_chain(), outside.bits_chain(), ("bits", "counts", "offsets", "table")):
                _same_bits(g, w, f"bit path, mode {mode}: {k}")
    finally:
        h.set_exceed_kernel(0)
        inside.free()
        if outside:
            outside.free()
