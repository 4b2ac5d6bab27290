"""The class patterns and the case check shared by the host and the GPU tests of mhw_days_by().  TEST INFRASTRUCTURE
ONLY.  The series come from coverage_cases.synthetic()."""
import numpy as np


def one_class(T):
    return np.zeros(T, dtype=np.int32), 1


def runs_of_17(T):
    """Twelve classes in runs of 17 steps (needs T >= 204 - 17 + 1 for every class to have a step)."""
    return ((np.arange(T) // 17) % 12).astype(np.int32), 12


def every_step(T):
    """Labels that change every step, some -1: the flush-per-step worst case."""
    return np.random.default_rng(11).integers(-1, 7, T).astype(np.int32), 7


PATTERNS = (one_class, runs_of_17, every_step)


def check_case(want):
    """On the oracle's side: every class has event days and all four categories occur.  A case without them proves
    nothing."""
    days = want["days"] if isinstance(want, dict) else want[0]
    assert (days[:, 4].sum(axis=-1) > 0).all(), "a class without event days"
    assert (days[:, :4].sum(axis=(0, 2)) > 0).all(), "a category that never occurs"
