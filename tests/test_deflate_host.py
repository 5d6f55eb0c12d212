"""plastid_amd/csrc/deflate_host.h -- the zlib ENCODER's model: the serial host encoder the kernel k_zlib_deflate must
match byte for byte -- on the CPU, over the inputs of tests/bigwig_write_cases.py: every stream inflates with zlib to its
input, carries zlib's Adler-32 and stays within input + 11 bytes; the inputs reach every length code from 4 up and every
distance code an input of 24 600 bytes can; count sections come out smaller than they went in, random bytes fall back to
the stored block; what is refused; and tests/deflate_host_test.cpp, the header as a program under the address and
undefined-behaviour sanitizers.  No GPU needed."""
import os
import shutil
import struct
import subprocess
import sys
import zlib

import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from plastid_amd import track  # noqa: E402
from tests import bigwig_write_cases as wc  # noqa: E402

INPUTS = wc.deflate_inputs()


@pytest.fixture(scope="module")
def streams():
    out, off, ln = track.deflate_zlib_host(list(INPUTS.values()))
    assert list(off) == [int(x) for x in (ln.cumsum() - ln)] and len(out) == int(ln.sum())       # back to back
    return {name: out[int(a):int(a) + int(n)] for name, a, n in zip(INPUTS, off, ln)}


@pytest.mark.parametrize("name", list(INPUTS))
def test_every_stream_inflates_to_its_input(streams, name):
    wc.check_stream(streams[name], INPUTS[name])
    tokens = wc.fixed_tokens(streams[name])
    if tokens is None:
        assert len(streams[name]) == len(INPUTS[name]) + 11
    else:
        assert wc.replay(tokens) == INPUTS[name] and len(streams[name]) < len(INPUTS[name]) + 11
        assert all(t[0] == "lit" or (4 <= t[1] <= 258 and 1 <= t[2]) for t in tokens)


def test_the_empty_input_is_an_empty_fixed_block(streams):
    assert streams["len0"] == b"\x78\x01\x03\x00\x00\x00\x00\x01" and zlib.decompress(streams["len0"]) == b""


def test_the_codes_the_inputs_reach(streams):
    tokens = [t for s in streams.values() for t in (wc.fixed_tokens(s) or []) if t[0] == "match"]
    lengths, dists = {t[1] for t in tokens}, {t[2] for t in tokens}
    assert lengths == set(range(4, 259))                                   # every length code but 257, every extra bit pattern
    assert set(wc.DIST_BASE) <= dists                                      # every distance code, 0 .. 29
    literals = {t[1] for s in streams.values() for t in (wc.fixed_tokens(s) or []) if t[0] == "lit"}
    assert literals == set(range(256))                                     # the 8-bit and the 9-bit literal codes


def test_runs_overlap_their_own_output(streams):
    for n in (257, 258, 259, 260, wc.MAX_INPUT):
        t = wc.fixed_tokens(streams["repeat%d" % n])
        assert t[0][0] == "lit" and all(x[0] == "match" and x[2] == 1 for x in t[1:-1] if x[0] == "match")
        assert t[1] == ("match", min(n - 1, 258), 1)
    assert len(streams["repeat%d" % wc.MAX_INPUT]) < 200


def test_count_sections_shrink_and_random_bytes_are_stored(streams):
    for n in (1023, 1024, 2048):
        assert len(streams["section%d" % n]) < len(INPUTS["section%d" % n])
    # (the prototype of the floor gave 6 856 .. 8 950 bytes for 12 312; zlib level 6 about two thirds of that)
    assert len(streams["section1024"]) < 0.8 * len(INPUTS["section1024"])
    for name in ("random12312", "random24600"):
        assert wc.fixed_tokens(streams[name]) is None and len(streams[name]) == len(INPUTS[name]) + 11


def test_many_inputs_in_one_call():
    many = wc.many_inputs()
    out, off, ln = track.deflate_zlib_host(many)
    ends = set()
    for raw, a, n in zip(many, off, ln):
        s = out[int(a):int(a) + int(n)]
        wc.check_stream(s, raw)
        ends.add(int(n) % 4)
    assert ends == {0, 1, 2, 3}


def test_refusals():
    with pytest.raises(ValueError, match="more than 24600 bytes"):
        track.deflate_zlib_host([b"x" * (wc.MAX_INPUT + 1)])
    with pytest.raises(ValueError, match="out_capacity"):
        track.deflate_zlib_host([b"abc", b"defg"], capacity=3 + 4 + 22 - 1)
    out, off, ln = track.deflate_zlib_host([b"abc", b"defg"], capacity=3 + 4 + 22)
    assert zlib.decompress(out[int(off[1]):]) == b"defg"
    out, off, ln = track.deflate_zlib_host([])
    assert out == b"" and len(off) == 0 and len(ln) == 0


def test_deflate_host_program(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "deflate_host_test")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    if subprocess.call([cxx] + san + [str(probe), "-o", str(tmp_path / "probe")], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL) != 0 \
            or subprocess.call([str(tmp_path / "probe")]) != 0:
        san = []
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror"] + san + ["-I", os.path.join(root, "plastid_amd", "csrc"),
                           os.path.join(root, "tests", "deflate_host_test.cpp"), "-lz", "-o", exe])
    inputs = list(INPUTS.values()) + wc.many_inputs(40)
    blob = tmp_path / "inputs.bin"
    blob.write_bytes(struct.pack("<I", len(inputs)) + b"".join(struct.pack("<I", len(x)) + x for x in inputs))
    out = subprocess.run([exe, str(blob)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert out.returncode == 0, out.stdout.decode()
    assert b"deflate_host: ok" in out.stdout
