"""zignal_amd/csrc/zg_tracer_step.h on the CPU: tests/c/tracer_step.cpp includes only that header, is built with plain g++ under
-fsanitize=address,undefined with the two HIP qualifiers defined away and -ffp-contract=off, and checks the chosen neighbour for all 8
incoming directions plus "no history" and all 256 masks of open neighbours, the bits of all 64 scores, and distanceToSegment on a few
thousand integer triples that reach its four returns, against fixtures tests/tracer_ref.py wrote. Nothing is loaded into python under a
sanitizer."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests import tracer_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "tracer_step.cpp")
BIN = os.path.join(ROOT, "tests", "c", "tracer_step")
STEP = os.path.join(ROOT, "tests", "golden", "tracer_step.json")
DIST = os.path.join(ROOT, "tests", "golden", "tracer_step_dist.bin")


@pytest.fixture(scope="module")
def step():
    with open(STEP) as f:
        return json.load(f)


def test_the_fixtures_are_what_the_restatement_gives(step):
    assert step["choice"] == R.CHOICE and step["offsets"] == [list(o) for o in R.OFFSETS]
    assert step["score_bits"] == [["%08x" % int(np.float32(s).view(np.uint32)) for s in row] for row in R.SCORE]
    rec = np.fromfile(DIST, "<u4").reshape(-1, 8)
    assert 2000 <= len(rec) <= 8000 and set(rec[:, 7]) == {0, 1, 2, 3}
    assert np.array_equal(rec[:, :6].view(np.int32), R.dist_cases())
    for row in rec[:: 37]:
        v = row[:6].view(np.int32)
        d, which = R.distance_to_segment(v[0:2], v[2:4], v[4:6])
        assert d.view(np.uint32)[0] == row[6] and which[0] == row[7]
    # the scores take seven values, and the straight-on diagonal is not 1 in f32
    patterns = {b for row in step["score_bits"] for b in row}
    values = {float(np.array(int(b, 16), np.uint32).view(np.float32)) for b in patterns}  # 0.0 and -0.0 are one value
    assert len(values) == 7 and "3f7fffff" in patterns and "3f800000" in patterns


def test_header_equals_the_fixtures_under_sanitizers(step):
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-D__host__=", "-D__device__=", "-o", BIN, SRC], check=True)
    lines = ["C %d %d %x" % (pk - 1, m, step["choice"][pk][m] + 1) for pk in range(9) for m in range(256)]
    lines += ["S %d %d %s" % (pk, k, step["score_bits"][pk][k]) for pk in range(8) for k in range(8)]
    out = subprocess.run([BIN, DIST], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    n_rec = os.path.getsize(DIST) // 32
    assert out.returncode == 0 and f"tracer step ok {len(lines)} {n_rec}" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
