"""The history arithmetic of lag_correlation() (xmhw_amd/csrc/lag_ring.h: the ring slot of a step at a lag, the warm-up
range of a block, the mask update) against a brute-force lookup of the series.  The header is plain integer code that the
kernel and this host program compile alike: tests/c/lag_ring.cpp is built with the host compiler under AddressSanitizer
and UBSan and run as a program of its own."""
import os
import subprocess

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_ring_and_mask_equal_the_series(tmp_path):
    exe = os.path.join(str(tmp_path), "lag_ring")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "c", "lag_ring.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    # 64 lag ranges x their ring depths x 8 series lengths x (3 block lengths + 5 starts): nothing was skipped
    assert int(out.stdout) > 10 ** 7
