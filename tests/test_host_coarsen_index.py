"""The index arithmetic of coarsen() (xmhw_amd/csrc/coarsen_index.h: flat cell to block origin, the in-grid extents of a
block, the alignment class that picks the instantiation, the window chunk of a workgroup; and the chunk rule of
stage_blocks.h) against brute force.  The header is plain integer code that the kernel and this host program compile
alike: tests/c/coarsen_index.cpp is built with the host compiler under AddressSanitizer and UBSan and run as a program
of its own."""
import os
import subprocess

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_blocks_classes_and_chunks_equal_brute_force(tmp_path):
    exe = os.path.join(str(tmp_path), "coarsen_index")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "c", "coarsen_index.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    # 400 grids x 81 factor pairs x 2 coarse grids: two checks per fine point and more per cell
    assert int(out.stdout) > 10 ** 7
