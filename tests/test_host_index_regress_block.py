"""The automatic time block of index_regression() (xmhw_amd/csrc/stage_blocks.h, index_regress_auto_block) pinned against
values worked out by hand from its rule: as many blocks as bring the launch to about 2048 workgroups, more where a block
would exceed 512 steps, never more than T // 256 blocks, one at least; the block is the axis divided evenly.  The header
is plain C++, so the program builds with g++ and needs no device."""
import json
import os
import subprocess

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

# (T, C, block): wg = ceil(C / 256) workgroups per block, blocks = clamp(max(ceil(2048 / wg), ceil(T / 512)), 1, T // 256)
WANT = [
    (14610, 1036800, 504),      # wg 4050: 1 block would do, the cap asks for 29; ceil(14610 / 29)
    (14610, 129600, 504),       # wg 507: 5 blocks would do, the cap asks for 29
    (14610, 256, 257),          # wg 1: 2048 blocks wanted, 57 of 256 steps allowed; ceil(14610 / 57)
    (131071, 64, 257),          # the longest series: 511 blocks allowed
    (1024, 1000000, 512),       # the cap alone: 2 blocks
    (513, 1000000, 257),        # one step past the cap: 2 blocks
    (512, 1000000, 512),        # on the cap: 1 block
    (300, 600, 300),            # fewer than 512 steps: one block, however few the cells
    (100, 10, 100),
    (1, 1, 1),
]


def test_index_regress_block_lengths(tmp_path):
    exe = os.path.join(str(tmp_path), "index_regress_block")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror",
                           os.path.join(ROOT, "tests", "c", "index_regress_block.cpp"), "-o", exe])
    args = [str(v) for T, C, _ in WANT for v in (T, C)]
    out = subprocess.run([exe] + args, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    assert [tuple(r) for r in json.loads(out.stdout)] == WANT
