"""The integer rules of anomaly_distribution() (xmhw_amd/csrc/hist_bin.h: the bin of a sample as the exact floor of an
integer division -- a shift, or a reciprocal and one correction step --, the packed 16-bit halves of a lane's column, the
rank of a probability) against plain integer arithmetic.  The header is plain integer code that the kernel and this host
program compile alike: tests/c/hist_bin.cpp is built with the host compiler under AddressSanitizer and UBSan and run as a
program of its own."""
import os
import subprocess

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_bins_halves_and_ranks_equal_integer_arithmetic(tmp_path):
    exe = os.path.join(str(tmp_path), "hist_bin")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "c", "hist_bin.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout + out.stderr
    # every q in (-2**23, 2**23) x 5 lo_q x 9 width_q, 256 halves, 5 p_q x 6 n: nothing was skipped
    assert int(out.stdout) == (2 ** 24 - 1) * 5 * 9 + 256 + 5 * 6
