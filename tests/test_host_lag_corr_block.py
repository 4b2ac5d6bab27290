"""The automatic time block of lag_correlation() (xmhw_amd/csrc/stage_blocks.h, lag_corr_auto_block) pinned against values
worked out by hand from its rule: with least = max(256, 16 L) -- the L warm-up steps stay below 1/16 of a block -- and
cap = max(4096, least), as many blocks as bring the launch to about 2048 workgroups (a workgroup is 256 cells x one group
of lags: one group of 8 up to 8 lags, groups of 16 beyond), more where a block would exceed cap steps, never more than
T // least blocks, one at least; the block is the axis divided evenly.  The header is plain C++, so the program builds
with g++ and needs no device."""
import json
import os
import subprocess

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

# (T, C, L, block): wg = ceil(C / 256) * groups, groups = 1 for L < 8 and L // 16 + 1 beyond;
# blocks = clamp(max(ceil(2048 / wg), ceil(T / cap)), 1, T // least)
WANT = [
    (14610, 1036800, 0, 3653),      # wg 4050: 1 block would do, the cap of 4096 asks for 4; ceil(14610 / 4)
    (14610, 1036800, 63, 3653),     # wg 16200, least 1008: 14 blocks allowed, 4 wanted
    (14610, 65536, 7, 1827),        # wg 256: 8 blocks fill the chip; ceil(14610 / 8)
    (14610, 65536, 8, 1827),        # nine lags are one group of 16: the same
    (14610, 65536, 16, 3653),       # a second lag group, wg 512: 4 blocks fill the chip, and the cap asks for 4
    (14610, 256, 0, 257),           # wg 1: 2048 blocks wanted, 57 of 256 steps allowed; ceil(14610 / 57)
    (14610, 256, 63, 1044),         # wg 4: 512 blocks wanted, 14610 // 1008 = 14 allowed; ceil(14610 / 14)
    (131071, 64, 63, 1009),         # the longest series: 130 blocks allowed; ceil(131071 / 130)
    (10000, 1000000, 8, 3334),      # the cap alone: 3 blocks
    (4097, 1000000, 0, 2049),       # one step past the cap: 2 blocks
    (300, 600, 63, 300),            # shorter than the least block: one block, however few the cells
    (1, 1, 0, 1),
]


def test_lag_corr_block_lengths(tmp_path):
    exe = os.path.join(str(tmp_path), "lag_corr_block")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror",
                           os.path.join(ROOT, "tests", "c", "lag_corr_block.cpp"), "-o", exe])
    args = [str(v) for row in WANT for v in row[:3]]
    out = subprocess.run([exe] + args, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    assert [tuple(r) for r in json.loads(out.stdout)] == WANT
