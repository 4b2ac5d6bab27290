"""Generators of the synthetic region_series() cases shared by the host and the GPU tests.  TEST INFRASTRUCTURE ONLY.

The device kernel treats a wave of 64 consecutive cells in one of three ways, by the number of distinct region labels
(>= 0) among them: one (path A), 2..4 (path B), 5 and more (path C).  paths_of() counts them the same way and every
layout generator asserts which paths it produces, so that no path goes untested."""
import numpy as np

from coverage_cases import scattered_regions, wave_regions, weights_q      # noqa: F401  (re-exported)

WAVE = 64
LIST_MAX = 4                    # kRegListMax of csrc/kernels_region.hip


def paths_of(region):
    """The set of paths ("A", "B", "C") the waves of this layout take; a wave without a live cell takes none."""
    region = np.asarray(region)
    out = set()
    for lo in range(0, region.shape[0], WAVE):
        r = region[lo:lo + WAVE]
        k = np.unique(r[r >= 0]).shape[0]
        if k:
            out.add("A" if k == 1 else "B" if k <= LIST_MAX else "C")
    return out


def series(T, C, dtype=np.float32, seed=0, nan_frac=0.0, x0=0.0, spread=12.0):
    """(T, C) samples on both sides of x0, well within 2**7 of it."""
    rng = np.random.default_rng(seed)
    ts = (x0 + np.clip(rng.normal(scale=spread, size=(T, C)), -100.0, 100.0)).astype(dtype)
    if nan_frac:
        ts[rng.random((T, C)) < nan_frac] = np.nan
    return ts


def weights_i(C, bits=31, seed=2):
    """Integer weights in [0, 2**bits] with both ends present."""
    return weights_q(C, seed) >> (31 - bits)


def uniform_waves(C, R=7):
    """One region per wave: path A only."""
    reg = wave_regions(C, R)
    assert paths_of(reg) == {"A"}
    return reg


def few_per_wave(C, k, R):
    """Exactly k (2..4) regions in every full wave, the k of a wave changing from wave to wave: path B (a last wave
    shorter than k cells holds fewer)."""
    assert 2 <= k <= LIST_MAX <= R
    c = np.arange(C)
    reg = (((c // WAVE) * 3 + (c % k)) % R).astype(np.int32)
    if C >= 8:
        reg[5] = -1                                     # an excluded lane inside a wave
    for lo in range(0, C - WAVE + 1, WAVE):
        assert np.unique(reg[lo:lo + WAVE][reg[lo:lo + WAVE] >= 0]).shape[0] == k
    if C >= k:
        assert "B" in paths_of(reg)
    if C >= WAVE and C % WAVE == 0:
        assert paths_of(reg) == {"B"}
    return reg


def many_per_wave(C, R):
    """R >= 5 regions dealt cell by cell: every wave of 5 cells and more takes path C."""
    assert R > LIST_MAX
    reg = (np.arange(C) % R).astype(np.int32)
    if C >= R:
        assert "C" in paths_of(reg)
    if C % WAVE == 0 or C % WAVE > LIST_MAX:
        assert paths_of(reg) == {"C"}
    return reg
