"""Write tests/golden/rank_cases.npz: the reference's rank fixture (test/xmhw_fixtures.py, rank_data):
five intensity_max values of one grid cell and the ranks xmhw.stats.mhw_rank gives them.

    python tools/make_golden_rank.py
"""
import os

import numpy as np

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "rank_cases.npz")

if __name__ == "__main__":
    np.savez(OUT,
             values=np.array([2.3, 1.2, 3.5, 2.4, 2.3]),
             events=np.array([8, 18, 29, 50, 89], dtype=np.int64),
             rank=np.array([4, 5, 1, 2, 3], dtype=np.int64))
    print("wrote", os.path.normpath(OUT))
