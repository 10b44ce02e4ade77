"""zignal_amd/csrc/zg_qr_geom.h on the CPU: tests/c/qr_geom.cpp includes only that header, is built with plain g++ under
-fsanitize=address,undefined and -ffp-contract=off, and compares bit for bit with records tests/qr_ref.py wrote (tests/golden/qr_geom.json indexes them: the seed, the number of records of each kind and
their SHA-256; the records themselves, a line of hexadecimal words each, and the checkRatio bits are kept deflated in the two .bin files
beside it, so that a few hundred kilobytes of digits are in no diff): the 8 x 8 solve and project
on a few hundred seeded quadruples, collinear sets and a zero-pivot system (which must answer "none"), checkRatio on every window with runs
in 0 .. 12 at the three tolerances, the triple score and its labels on seeded finders with forced ties, estimateVersion, the BCH codewords,
nearModule, Cross.center, timingOk and readVersion. Nothing is loaded into python under a sanitizer."""
import hashlib
import json
import os
import subprocess
import zlib

import numpy as np
import pytest

from tests import qr_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "qr_geom.cpp")
BIN = os.path.join(ROOT, "tests", "c", "qr_geom")
GEOM = os.path.join(ROOT, "tests", "golden", "qr_geom.json")
RECORDS = os.path.join(ROOT, "tests", "golden", "qr_geom_records.bin")
RATIO = os.path.join(ROOT, "tests", "golden", "qr_geom_ratio.bin")
SEED = 20


def inflate(path):
    with open(path, "rb") as f:
        return zlib.decompress(f.read())


def index_of(text):
    lines = text.decode().split("\n")
    return {"seed": SEED, "kinds": {k: sum(line[0] == k for line in lines) for k in "QSVBNCG"}, "sha256": hashlib.sha256(text).hexdigest()}


@pytest.fixture(scope="module")
def lines():
    return inflate(RECORDS).decode().split("\n")


def test_the_fixtures_are_what_the_restatement_gives(lines):
    assert lines == R.geom_records(SEED)
    with open(GEOM) as f:
        assert json.load(f) == index_of(inflate(RECORDS))
    ratio = np.frombuffer(inflate(RATIO), np.uint8)
    assert np.array_equal(ratio, R.ratio_bits())
    kinds = {k: sum(line[0] == k for line in lines) for k in "QSVBNCG"}
    assert kinds["Q"] >= 200 and kinds["S"] >= 400 and kinds["B"] == 34 and all(kinds.values())
    none = [line for line in lines if line[0] == "Q" and line.split()[17] == "0"]
    assert len(none) >= 4  # two collinear sets, a zero pivot, four equal points
    # the windows that pass grow with the tolerance, and 1:1:3:1:1 itself passes at each
    bits = np.unpackbits(ratio.reshape(3, -1), axis=1, bitorder="little")[:, :13 ** 5]
    assert 0 < bits[0].sum() < bits[1].sum() < bits[2].sum()
    w = ((((1 * 13 + 1) * 13 + 3) * 13 + 1) * 13) + 1
    assert bits[:, w].all() and not bits[:, 0].any()
    assert R.UNDEFINED_CASTS[0] == 0


def test_header_equals_the_fixtures_under_sanitizers(lines, tmp_path):
    ratio = tmp_path / "ratio.bin"
    ratio.write_bytes(inflate(RATIO))
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", BIN, SRC], check=True)
    out = subprocess.run([BIN, str(ratio)], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and f"qr geom ok {len(lines)} {3 * 13 ** 5}" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
