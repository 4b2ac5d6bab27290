"""The case generators shared by the host and the GPU tests of anomaly_distribution(): the series and class patterns of
lag_correlation_cases with the columns that can go wrong under bins (lo_q, width_q, B) made by construction.  TEST
INFRASTRUCTURE ONLY."""
import numpy as np

import lag_correlation_cases as lc

PATTERNS = lc.PATTERNS
ONE = 65536
FIRST = 8                                       # the first column made here (lag_correlation_cases makes 2 .. 7)
COLUMNS = 15                                    # the cells a case needs for all of them
# B: an odd number of bins (the last dword has one half), and both sides of each LDS size (32 / 64 / 128 KB)
BIN_COUNTS = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256)


def bins_for(B, odd_width=False):
    """bins of B bins that the anomalies of series() fill: a width of 2**k units, or an odd one"""
    width_q = 1 << (((16 * ONE) // max(B, 16)).bit_length() - 1)           # B >= 16: between -4 .. 4 and -8 .. 8 in all
    if odd_width:
        width_q += 1 if width_q % 2 == 0 else 2
    return -(B * width_q) // 2, width_q, B


def series(T, C, dtype, seed, lo_q, width_q, B, Dr=1, shift=0):
    """lag_correlation_cases.series() x (T, C) around base (Dr, C) -- anomalies of a few units, 3 % NaN, out-of-range values
    and +-2**7 exactly in columns 6 and 7 -- and, where C allows, over a base of zero, as exact multiples of the unit of the
    fixed point (after the shift), by column
       8  one sample exactly on the edge e = min(2, B) (step 3) and one a unit below it (step 4)
       9  samples exactly at lo_q, at lo_q - 1, at the last edge and one unit inside it (steps 5 .. 8)
      10  a constant column           11  every sample in UNDER          12  every sample in OVER
      13  all NaN                     14  +2**7 and -2**7 exactly and both infinities (steps 1, 2, 9, 10), and nine samples
                                          near +-127.5 (steps 20 .. 28: cubes and fourth powers past 64 bits)
    Returns x, base, rows, doy, doys."""
    d = lc.series(T, C, dtype, seed, Dr=Dr)
    x, base, rows = d["x"].astype(np.float64), d["base_x"].copy(), d["rows"]
    rng = np.random.default_rng(seed + 1000)
    unit = 2.0 ** shift / ONE                   # one unit of the fixed point in the units of x
    hi_q = lo_q + B * width_q
    lim = (1 << 23) - 1
    clip = lambda q: int(min(max(q, -lim), lim))                                                     # noqa: E731
    if C >= COLUMNS:
        base[:, FIRST:COLUMNS] = 0.0
        noise = np.rint(rng.normal(0.0, 2.0, (T, COLUMNS - FIRST)) * 4096.0) * 16                   # units of the fixed point
        x[:, FIRST:COLUMNS] = noise * unit
        if T > 10:
            x[3, 8], x[4, 8] = (lo_q + min(2, B) * width_q) * unit, (lo_q + min(2, B) * width_q - 1) * unit
            x[5:9, 9] = np.array([lo_q, clip(lo_q - 1), hi_q, hi_q - 1]) * unit
            x[:, 10] = clip(lo_q + (B // 2) * width_q + width_q // 3) * unit
            x[:, 11] = np.array([clip(lo_q - 1 - (t % 3)) for t in range(T)]) * unit
            x[:, 12] = np.array([clip(hi_q + (t % 3)) for t in range(T)]) * unit
            x[:, 13] = np.nan
            x[[1, 2, 9, 10], 14] = np.array([128.0, -128.0, np.inf, -np.inf]) * 2.0 ** shift
        if T > 30:
            x[20:29, 14] = np.array([127.5, 127.5, -127.75, 127.5, 127.5, -127.75, 127.5, -127.75, 127.5]) * 2.0 ** shift
    return {"x": x.astype(dtype), "base": base, "rows": rows, "doy": d["doy"], "doys": d["doys"]}
