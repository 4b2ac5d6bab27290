"""The 128-bit sums of anomaly_distribution() (xmhw_amd/csrc/wide_sum.h: the multiply-accumulate of q**3 and q**4 into a
(low, high) pair and the flush that adds such a pair to memory by an atomic add of the low word that returns the old value
and a carry derived from it) against __int128.  The header is plain integer code that the kernel and this host program
compile alike: tests/c/wide_sum.cpp is built with the host compiler under AddressSanitizer and UBSan and run as a program
of its own."""
import os
import subprocess

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_wide_sums_and_flushes_equal_int128(tmp_path):
    exe = os.path.join(str(tmp_path), "wide_sum")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "c", "wide_sum.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    # 5 series of 2**17 terms x 3 flush rhythms x 5 memory presets: nothing was skipped
    assert int(out.stdout) == 5 * 3 * 5 * 2 ** 17
