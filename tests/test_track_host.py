"""plastid_amd/csrc/track_host.h -- the bedGraph / wiggle line parser that the host reader (plastid_amd.read_wiggle) and
the device import share -- on the CPU: every case of tests/golden/track_fixture.npz (the reference's WiggleReader tuples,
bit for bit), the refused texts with their line numbers, and tests/track_host_test.cpp: the plain predicate and both
converters against strtod at their boundaries and lines that end at a buffer's last byte, compiled with the host compiler
(under the address and undefined-behaviour sanitizers where it has them) and run as a program.  No GPU needed."""
import io
import os
import shutil
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import plastid_amd as pa  # noqa: E402
from tests import track_cases as tc  # noqa: E402


@pytest.mark.parametrize("name", tc.case_names())
def test_host_reader_yields_the_reference_tuples(name):
    c = tc.case(name)
    for (text, _), exp in zip(c["adds"], c["tuples"]):
        t = pa.read_wiggle(io.StringIO(text))
        assert tc.same_tuples(t.tuples(), [tuple(x) for x in exp])
        assert t.stats["yielded"] == len(exp) == len(t)
        assert t.stats["lines"] == len(text.split("\n")) - (1 if text.endswith("\n") or not text else 0)
        assert t.stats["escaped"] == int(t.escaped.sum())


@pytest.mark.parametrize("name", tc.refused_names())
def test_host_reader_refuses_with_the_line(name):
    r = tc.refused(name)
    with pytest.raises(ValueError) as e:
        pa.read_wiggle(io.StringIO(r["text"]))
    assert str(e.value).startswith("<memory>: track line %d: " % r["line"]), str(e.value)


def test_host_reader_reads_a_path_and_names_it(tmp_path):
    p = tmp_path / "t.bedgraph"
    p.write_bytes(b"chrA 1 2 3\r\nchrA 5 x 3\r\n")
    with pytest.raises(ValueError) as e:
        pa.read_wiggle(str(p))
    assert str(e.value) == "%s: track line 2: a coordinate is not an integer" % p
    p.write_bytes(b"chrA 1 2 3\r\nchrB 5 6 3")
    t = pa.read_wiggle(p)
    assert t.tuples() == [("chrA", 1, 2, 3.0), ("chrB", 5, 6, 3.0)] and t.names == ["chrA", "chrB"] and t.stats["states"] == 2


def test_escapes_are_what_the_plain_predicate_names():
    # integer counts and short decimals never escape; Python-only spellings and long significands do
    t = pa.read_wiggle(io.StringIO("chrA 1 2 3\nchrA 2 3 0.125\nchrA 3 4 123456789012345\nchrA 4 5 1e22\nchrA 5 6 -2.5e-3\n"))
    assert not t.escaped.any()
    t = pa.read_wiggle(io.StringIO("chrA 1 2 1e23\nchrA 2 3 nan\nchrA 1_0 30 1\nchrA 4 5 0.12345678901234567\nchrA 5 6 1.\nchrA 6 7 7\n"))
    assert t.escaped.tolist() == [True, True, True, True, True, False]


def test_track_parser_program(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "track_host_test")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    if subprocess.call([cxx] + san + [str(probe), "-o", str(tmp_path / "probe")], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL) != 0 \
            or subprocess.call([str(tmp_path / "probe")]) != 0:
        san = []
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror"] + san + ["-I", os.path.join(root, "plastid_amd", "csrc"),
                           os.path.join(root, "tests", "track_host_test.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert out.returncode == 0, out.stdout.decode()
    assert b"track_host: ok" in out.stdout
