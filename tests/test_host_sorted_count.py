"""The sorted-list kernel counts the keys of a row's new list above the carried boundary from the position in the sorted run
(xmhw_amd/csrc/sorted_count.h: bit k of the count = XOR of the nested compares at the multiples of 2^k) instead of adding
one compare per key.  The rule is host and device code alike, so it is checked here without a device: tests/c/sorted_count.cpp
runs it against the plain count over every descending run of 2 .. 9 keys drawn from four distinct values and 0 (all tie
patterns, 0 = no key) at the thresholds 0, each value, each value - 1 and + 1, and all ones."""
import json
import os
import subprocess

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

# runs of N keys over 5 values: C(N + 4, 4); 14 thresholds each
RUNS = sum({2: 15, 3: 35, 4: 70, 5: 126, 6: 210, 7: 330, 8: 495, 9: 715}.values())


def test_count_of_a_sorted_run_equals_the_plain_count(tmp_path):
    exe = os.path.join(str(tmp_path), "sorted_count")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror",
                           os.path.join(ROOT, "tests", "c", "sorted_count.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    got = json.loads(out.stdout.strip().splitlines()[-1])
    assert got == {"cases": RUNS * 14, "wrong": 0}, got
