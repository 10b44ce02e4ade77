"""The rank tracker of the sliding-histogram order-statistic kernel (zignal_amd/csrc/zg_order_stat_track.h: add, remove, replace, settle,
midpoint, trimmed mean) on the CPU: tests/c/order_stat_track.cpp includes only that header, is built with plain g++ under
-fsanitize=address,undefined with the two HIP qualifiers defined away, and compares every step of a sliding window with a sort of the
window (radii 1, 2, 16, 127 with u16 counters and 128 with u32 counters; noise, a 0 / 255 checkerboard, constants, ramps)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "order_stat_track.cpp")
BIN = os.path.join(ROOT, "tests", "c", "order_stat_track")


def test_order_stat_tracker_against_a_sort_of_the_window():
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-D__host__=", "-D__device__=", "-o", BIN, SRC], check=True)
    out = subprocess.run([BIN], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "order-stat tracker ok" in out.stdout, out.stdout[-4000:] + out.stderr[-4000:]
