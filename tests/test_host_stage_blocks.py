"""The automatic block lengths of the stage kernels (xmhw_amd/csrc/stage_blocks.h: one rule, four callers) pinned
against the values of the four separate functions they replaced (tests/golden/stage_blocks.json: [arguments..., block]
per entry, recorded from those functions).  The header is plain C++, so the program builds with g++ and needs no device."""
import json
import os
import subprocess

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_stage_block_lengths_are_the_recorded_ones(tmp_path):
    exe = os.path.join(str(tmp_path), "stage_blocks")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror",
                           os.path.join(ROOT, "tests", "c", "stage_blocks.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    got = json.loads(out.stdout)
    with open(os.path.join(ROOT, "tests", "golden", "stage_blocks.json")) as f:
        want = json.load(f)
    assert sorted(got) == sorted(want) == ["class_days", "cooccur", "displacement", "heat_stress"]
    for name in want:
        assert len(got[name]) == len(want[name]), name
        wrong = [(g, w) for g, w in zip(got[name], want[name]) if g != w]
        assert not wrong, f"{name}: {len(wrong)} of {len(want[name])} differ, first (got, recorded): {wrong[:3]}"
