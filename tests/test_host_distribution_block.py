"""The automatic time block of anomaly_distribution() (xmhw_amd/csrc/stage_blocks.h, distribution_auto_block) pinned against
values worked out by hand from its rule: as many blocks as bring the launch to about 2048 workgroups (a workgroup is 256
cells), more where a block would exceed 4096 steps, never more than ceil(T / 256) blocks, one at least; the block is the
axis divided evenly.  The header is plain C++, so the program builds with g++ and needs no device."""
import json
import os
import subprocess

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

# (T, C, block): wg = ceil(C / 256); blocks = clamp(max(ceil(2048 / wg), ceil(T / 4096)), 1, ceil(T / 256))
WANT = [
    (14610, 1036800, 3653),         # wg 4050: 1 block would do, the cap of 4096 asks for 4; ceil(14610 / 4)
    (14610, 65536, 1827),           # wg 256: 8 blocks fill the chip; ceil(14610 / 8)
    (14610, 256, 252),              # wg 1: 2048 blocks wanted, ceil(14610 / 256) = 58 allowed; ceil(14610 / 58)
    (131071, 64, 256),              # the longest series: 512 blocks allowed; ceil(131071 / 512)
    (70000, 64, 256),               # 274 blocks allowed; ceil(70000 / 274)
    (10000, 1000000, 3334),         # the cap alone: 3 blocks
    (4097, 1000000, 2049),          # one step past the cap: 2 blocks
    (300, 600, 150),                # wg 3: 683 blocks wanted, 2 allowed
    (400, 300, 200),                # the shape of the GPU tests: two blocks
    (256, 1, 256),                  # one block allowed
    (1, 1, 1),
]


def test_distribution_block_lengths(tmp_path):
    exe = os.path.join(str(tmp_path), "distribution_block")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror",
                           os.path.join(ROOT, "tests", "c", "distribution_block.cpp"), "-o", exe])
    args = [str(v) for row in WANT for v in row[:2]]
    out = subprocess.run([exe] + args, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    assert [tuple(r) for r in json.loads(out.stdout)] == WANT
