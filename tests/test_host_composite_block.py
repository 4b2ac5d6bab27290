"""The automatic time block of mhw_composite() (xmhw_amd/csrc/stage_blocks.h, composite_auto_block) pinned against values
worked out by hand from its rule, which is that of index_regression(): as many blocks as bring the launch to about 2048
workgroups, more where a block would exceed 512 steps, never more than T // 256 blocks, one at least; the block is the
axis divided evenly; the window length D does not enter.  The header is plain C++, so the program builds with g++ and
needs no device."""
import json
import os
import subprocess

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

# (T, C, D, block): wg = ceil(C / 256) workgroups per block, blocks = clamp(max(ceil(2048 / wg), ceil(T / 512)), 1, T // 256)
WANT = [
    (14610, 1036800, 61, 504),      # wg 4050: 1 block would do, the cap asks for 29; ceil(14610 / 29)
    (14610, 1036800, 128, 504),     # the same for the longest window
    (14610, 65536, 61, 504),        # wg 256: 8 blocks would do, the cap asks for 29
    (14610, 256, 1, 257),           # wg 1: 2048 blocks wanted, 57 of 256 steps allowed; ceil(14610 / 57)
    (131071, 64, 128, 257),         # the longest series: 511 blocks allowed
    (1024, 1000000, 61, 512),       # the cap alone: 2 blocks
    (513, 1000000, 61, 257),        # one step past the cap: 2 blocks
    (512, 1000000, 61, 512),        # on the cap: 1 block
    (300, 600, 128, 300),           # fewer than 512 steps: one block, however few the cells
    (1, 1, 1, 1),
]


def test_composite_block_lengths(tmp_path):
    exe = os.path.join(str(tmp_path), "composite_block")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror",
                           os.path.join(ROOT, "tests", "c", "composite_block.cpp"), "-o", exe])
    args = [str(v) for row in WANT for v in row[:3]]
    out = subprocess.run([exe] + args, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    assert [tuple(r) for r in json.loads(out.stdout)] == WANT
