"""The automatic time block of spatial_correlation() (xmhw_amd/csrc/stage_blocks.h, spatial_corr_auto_block) and its
offset groups pinned against values worked out by hand from the rule: a workgroup is a tile of ``rows`` grid rows x 64
longitudes times one group of offsets (one group of 8 up to 8 offsets, groups of 16 beyond); as many blocks as bring the
launch to about 2048 workgroups, more where a block would exceed 256 steps, never more than one per step, one at least;
the block is the axis divided evenly.
The header is plain C++, so the program builds with g++ and needs no device."""
import json
import os
import subprocess

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

# (nt, ny, nx, rows, D, group, groups, block): wg = ceil(ny / rows) * ceil(nx / 64) * groups;
# blocks = clamp(max(ceil(2048 / wg), ceil(nt / 256)), 1, nt); block = ceil(nt / blocks)
WANT = [
    (14610, 720, 1440, 4, 13, 16, 1, 252),      # 180 x 23 tiles fill the chip: the cap of 256 asks for 58 blocks; ceil(14610 / 58)
    (14610, 720, 1440, 8, 64, 16, 4, 252),      # ... four groups and the 8-row tile all the more
    (14610, 64, 256, 4, 8, 8, 1, 252),          # 16 x 4 tiles, one group of 8: 32 blocks fill the chip, the cap asks for 58
    (14610, 64, 256, 4, 9, 16, 1, 252),         # nine offsets are one group of 16: the same
    (14610, 64, 256, 4, 17, 16, 2, 252),        # a second group, wg 128: 16 blocks would do
    (14610, 64, 256, 8, 8, 8, 1, 229),          # the 8-row tile halves the workgroups: 64 blocks fill the chip; ceil(14610 / 64)
    (2000, 8, 64, 8, 1, 8, 1, 1),               # one tile: 2048 blocks wanted, one step each
    (300, 1, 1, 4, 1, 8, 1, 1),                 # one tile: 2048 blocks wanted, 300 steps there are
    (1, 9, 130, 4, 64, 16, 4, 1),
    (0, 5, 5, 4, 1, 8, 1, 1),                   # no step: one, and nothing is launched
    (131071, 37, 33, 4, 16, 16, 1, 256),        # the longest series: 10 tiles want 205 blocks, the cap 512; ceil(131071 / 512)
]


def test_spatial_corr_block_lengths(tmp_path):
    exe = os.path.join(str(tmp_path), "spatial_corr_block")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror",
                           os.path.join(ROOT, "tests", "c", "spatial_corr_block.cpp"), "-o", exe])
    args = [str(v) for row in WANT for v in row[:5]]
    out = subprocess.run([exe] + args, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    assert [tuple(r) for r in json.loads(out.stdout)] == WANT
