"""The host side of the track export (plastid_amd/csrc/track_host.h): the serial bedGraph / variableStep writers against the
reference's texts of tests/golden/track_export_fixture.npz, byte for byte; the ``repr(float)`` formatter against Python's
on the golden values, on 10^6 seeded bit patterns and on 10^5 short decimals; and tests/track_export_host_test.cpp --
formatter and writers over arrays with runs at position 0 and at the last cell -- compiled with the host compiler (under
the address and undefined-behaviour sanitizers where it has them) and run as a program.  No GPU needed."""
import io
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from plastid_amd import track  # noqa: E402
from tests import track_export_cases as xc  # noqa: E402


@pytest.mark.parametrize("name", xc.case_names())
def test_host_writers_give_the_reference_text(name):
    c = xc.case(name)
    ga = xc.host_array(name)
    for st in "+-":
        fh = io.StringIO()
        stats = track.write_bedgraph(ga, fh, xc.TRACKNAME, st, **xc.KWARGS)
        assert fh.getvalue() == c["bedgraph"][st]
        assert stats["bytes"] == len(fh.getvalue().split("\n", 1)[1].encode()) and stats["lines"] == fh.getvalue().count("\n") - 1
        fh = io.StringIO()
        stats = track.write_variable_step(ga, fh, xc.TRACKNAME, st, **xc.KWARGS)
        assert fh.getvalue() == c["variable_step"][st]
        assert stats["lines"] == fh.getvalue().count("\n") - 1


def test_host_writers_write_bytes_to_a_binary_file():
    ga = xc.host_array("values")
    fh = io.StringIO()
    track.write_bedgraph(ga, fh, "t", "+")
    assert fh.getvalue().startswith("track type=bedGraph name=t\nchr10\t0\t5\t0\n")


def _check_repr(values):
    got = track.float_repr(values)
    bad = [(float(v), g) for v, g in zip(values, got) if g != repr(float(v))]
    assert not bad, bad[:10]


def test_formatter_on_the_golden_values():
    vals = list(xc.ODD) + [1.7976931348623157e308, 5e-324, float("inf"), float("-inf"), float("nan"), 0.0, -0.0, 1e15, 1e16, 9999999999999998.0,
                           1e-4, 1e-5, 9.999999999999999e-05, 0.00010000000000000002, 123456789012345.6, 1e21, 1e22, 1e23, 2.0 ** 53, 2.0 ** 63, -2.0 ** 63,
                           2.2250738585072014e-308, 2.225073858507201e-308, 0.3, 2.0 / 3.0, 100.0, 1.5e16, -1.5e-7]
    vals += [-v for v in xc.ODD]
    _check_repr(np.array(vals, np.float64))
    assert track.float_repr([float("nan")]) == ["nan"] and track.float_repr([-0.0, 3.0, 1e16]) == ["-0.0", "3.0", "1e+16"]


def test_formatter_on_random_bit_patterns():
    rng = np.random.default_rng(20261019)
    bits = rng.integers(0, 2 ** 64, size=10 ** 6, dtype=np.uint64)
    _check_repr(bits.view(np.float64))


def test_formatter_on_short_decimals():
    rng = np.random.default_rng(7)
    k = rng.integers(-10 ** 9, 10 ** 9, size=10 ** 5)
    d = rng.integers(0, 12, size=10 ** 5)
    _check_repr(np.array([int(a) / 10 ** int(b) for a, b in zip(k, d)], np.float64))


def test_track_export_program(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "track_export_host_test")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    if subprocess.call([cxx] + san + [str(probe), "-o", str(tmp_path / "probe")], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL) != 0 \
            or subprocess.call([str(tmp_path / "probe")]) != 0:
        san = []
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror"] + san + ["-I", os.path.join(root, "plastid_amd", "csrc"),
                           os.path.join(root, "tests", "track_export_host_test.cpp"), "-o", exe])
    # the golden cases as a plain text file: name, cells, expected texts (hex), one record per contig and strand
    lines = []
    for name in xc.case_names():
        c = xc.case(name)
        for st in "+-":
            lines.append("case %s %s %d" % (name, st, len(c["chroms"])))
            for ch in sorted(c["chroms"]):
                v = xc.cells(name, ch, st)
                lines.append("contig %s %d" % (ch.encode().hex(), len(v)))
                lines.append(" ".join(float(x).hex() for x in v))
            for what in ("bedgraph", "variable_step"):
                lines.append("text %s" % c[what][st].split("\n", 1)[1].encode().hex())
    cases = tmp_path / "cases.txt"
    cases.write_text("\n".join(lines) + "\n")
    out = subprocess.run([exe, str(cases)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert out.returncode == 0, out.stdout.decode()
    assert b"track_export_host: ok" in out.stdout
