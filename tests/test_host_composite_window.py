"""The window arithmetic of mhw_composite() (xmhw_amd/csrc/composite_window.h: the block warm-up from bitmap words, the
shift-insert-mask step, the look-ahead cursor) against a brute-force lookup of the bits.  The header is plain integer
code that the kernel and this host program compile alike: tests/c/composite_window.cpp is built with the host compiler
under AddressSanitizer and UBSan and run as a program of its own."""
import os
import subprocess

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_rolled_window_equals_the_bits(tmp_path):
    exe = os.path.join(str(tmp_path), "composite_window")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "c", "composite_window.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    # 128 window lengths x 4 splits x 42 columns, 3 windows per block start: nothing was skipped
    assert int(out.stdout) > 5 * 10 ** 8
