"""The index arithmetic of regrid() (xmhw_amd/csrc/regrid_index.h: workgroup to destination row and column tile, a
tile's source column span with the seam wrap, a lane's LDS offset, the fit test that picks the path, the layout of the
packed table, the step chunk) against brute-force tables.  The header is plain integer code that the kernel and this
host program compile alike: tests/c/regrid_index.cpp is built with the host compiler under AddressSanitizer and UBSan
and run as a program of its own."""
import os
import subprocess

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_tiles_spans_offsets_fit_and_chunks_equal_brute_force(tmp_path):
    exe = os.path.join(str(tmp_path), "regrid_index")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "c", "regrid_index.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    # 12 widths x 9 grids x 2 x 4 kinds x 3 draws: three checks per entry of every run and more per tile
    assert int(out.stdout) > 10 ** 6
