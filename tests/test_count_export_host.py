"""The host side of the export of count vectors (``BAMGenomeArray.to_bedgraph`` / ``to_variable_step``): the serial writers
of plastid_amd/csrc/track_host.h (``track.write_count_bedgraph`` / ``write_count_variable_step``) against the 36 texts the
reference itself wrote (tests/golden/export_regions.npz, vectors from the oracle) and against the reference's window loop
restated over seeded vectors; and tests/count_export_host_test.cpp -- the batch layout and the line -> run -> range mapping
of plastid_amd/csrc/track_table.h -- compiled with the host compiler (under the address and undefined-behaviour sanitizers
where it has them) and run as a program.  No GPU needed."""
import io
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from plastid_amd import track  # noqa: E402
from tests import count_export_cases as cc  # noqa: E402


def _write(what, vectors, window, **kwargs):
    fh = io.StringIO()
    fn = track.write_count_bedgraph if what == "bedgraph" else track.write_count_variable_step
    stats = fn(vectors, fh, "trk", window_size=window, **kwargs)
    return fh.getvalue(), stats


def test_there_are_36_golden_texts():
    assert len(cc.golden()[0]["exports"]) == 36


@pytest.mark.parametrize("k", range(36))
def test_host_writers_give_the_reference_text(k):
    ex = cc.golden()[0]["exports"][k]
    vectors = cc.oracle_vectors(ex)
    want_float = ex["normalize"] or ex["spec"]["kind"] == "center"
    assert all(v.dtype == (np.float64 if want_float else np.int64) for v in vectors.values())
    text, stats = _write(ex["what"], vectors, ex["window"], **ex["kwargs"])
    assert text == ex["text"], cc.export_id(ex)
    body = text.split("\n", 1)[1]
    assert stats["lines"] == body.count("\n") and stats["bytes"] == len(body.encode())
    if not want_float:
        assert stats["listed"] == 0


def _seeded_vectors(rng, dtype):
    """Contigs of 0, 1 and 2 positions, an all-zero contig between two others, runs across every window border."""
    if dtype == np.int64:
        pick = np.array([0, 0, 0, 9, 10, 99, 100, 10 ** 15], np.int64)
    else:
        pick = np.array([0.0, 0.0, 0.0, 0.5, 1e-05, 1.0 / 3.0, 1e16, 3.0], np.float64)
    v = {}
    v["chr10"] = np.repeat(pick[rng.integers(0, len(pick), 40)], rng.integers(1, 6, 40))
    v["chr2"] = np.zeros(23, dtype)
    v["chr3"] = np.repeat(pick[rng.integers(0, len(pick), 15)], rng.integers(1, 9, 15))
    v["e0"] = np.zeros(0, dtype)
    v["e1"] = pick[3:4].copy()
    v["e2"] = pick[[4, 4]].copy()
    v["z1"] = np.zeros(1, dtype)
    return v


@pytest.mark.parametrize("dtype", [np.int64, np.float64])
def test_host_writers_are_the_reference_window_loop(dtype):
    rng = np.random.default_rng(20261019)
    for _ in range(4):
        vectors = _seeded_vectors(rng, dtype)
        size = len(vectors["chr10"])
        for window in (1, 7, size, size + 1, 100000):
            text, stats = _write("bedgraph", vectors, window)
            want = cc.reference_bedgraph(vectors, window)
            assert text == "track type=bedGraph name=trk\n" + want, (dtype, window)
            assert stats["lines"] == want.count("\n") and stats["bytes"] == len(want)
            text, stats = _write("variable_step", vectors, window)
            want = cc.reference_variable_step(vectors, window)
            assert text == "track type=wiggle_0 name=trk\n" + want, (dtype, window)
            assert stats["lines"] == want.count("\n") and stats["runs"] == sum(int(np.count_nonzero(v)) for v in vectors.values())


def test_a_run_across_a_window_border_is_two_lines():
    v = {"c": np.array([0, 4, 4, 4, 4, 0, 10 ** 15], np.int64)}
    assert _write("bedgraph", v, 3)[0].split("\n", 1)[1] == "c\t1\t3\t4\nc\t3\t5\t4\nc\t6\t7\t1000000000000000\n"
    assert _write("bedgraph", v, 7)[0].split("\n", 1)[1] == "c\t1\t5\t4\nc\t6\t7\t1000000000000000\n"
    f = {"c": np.array([0.5, 1e-05, 1.0 / 3.0, 1e16, 3.0]), "b": np.zeros(0)}
    text, stats = _write("variable_step", f, 2, color="1,2,3")
    assert text == ("track type=wiggle_0 name=trk color=1,2,3\nvariableStep chrom=b span=1\nvariableStep chrom=c span=1\n"
                    "1\t0.5\n2\t1e-05\n3\t0.3333333333333333\n4\t1e+16\n5\t3.0\n")
    assert stats == {"lines": 7, "runs": 5, "listed": 4, "bytes": len(text.split("\n", 1)[1])}


def test_vectors_of_two_dtypes_are_refused():
    with pytest.raises(TypeError):
        _write("bedgraph", {"a": np.ones(3, np.int64), "b": np.ones(3, np.float64)}, 10)
    with pytest.raises(TypeError):
        _write("bedgraph", {"a": np.ones((2, 3), np.int64)}, 10)


def test_count_export_program(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "count_export_host_test")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    if subprocess.call([cxx] + san + [str(probe), "-o", str(tmp_path / "probe")], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL) != 0 \
            or subprocess.call([str(tmp_path / "probe")]) != 0:
        san = []
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror"] + san + ["-I", os.path.join(root, "plastid_amd", "csrc"),
                           os.path.join(root, "tests", "count_export_host_test.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert out.returncode == 0, out.stdout.decode()
    assert b"count_export_host: ok" in out.stdout
