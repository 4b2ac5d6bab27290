"""The tile arithmetic of spatial_correlation() (xmhw_amd/csrc/halo_tile.h: the tile of a workgroup, the halo box of an
offset group, the LDS slot of a tile position, the grid point behind a slot with seam wrap and edge test, the slot a lane
reads for an offset) against a brute-force lookup of the grid.  The header is plain integer code that the kernel and this
host program compile alike: tests/c/halo_tile.cpp is built with the host compiler under AddressSanitizer and UBSan and
run as a program of its own."""
import os
import subprocess

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_slots_and_points_equal_the_grid(tmp_path):
    exe = os.path.join(str(tmp_path), "halo_tile")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "c", "halo_tile.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    # 49 grids x 2 seam settings x 2 tile shapes x 81 boxes (625 on the 6 grids of up to 2 x 33) x every tile: two
    # checks per slot of every tile and two per lane and offset of nine; a 9 x 200 grid alone has 12 tiles of 4 rows
    assert int(out.stdout) > 10 ** 8
