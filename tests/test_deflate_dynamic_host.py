"""The DYNAMIC Huffman codes of the zlib encoder's model (plastid_amd/csrc/deflate_host.h, mode 2 of pb_deflate_zlib_mode;
codes="dynamic" of track.deflate_zlib_host) on the CPU, over the inputs of tests/bigwig_write_cases.py: every stream
inflates with zlib to its input and is never longer than the fixed-mode stream; the tokens are those of the fixed mode;
every code a stream carries is complete, within its limit and canonical, and optimal where no length reached the limit;
which block wins; the sizes against the fixed streams and zlib level 6; the length function (pb_huffman_lengths) past both
limits; mode 1 of the new seam is the old seam; what is refused; and tests/deflate_dynamic_host_test.cpp, the header as a
program under the address and undefined-behaviour sanitizers.  No GPU needed."""
import ctypes
import os
import shutil
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from plastid_amd import track  # noqa: E402
from tests import bigwig_write_cases as wc  # noqa: E402
from tests import deflate_dynamic_cases as dc  # noqa: E402

INPUTS = wc.deflate_inputs()
LENGTH_CASES = dc.length_cases()


def split(out, off, ln, names):
    assert list(off) == [int(x) for x in (ln.cumsum() - ln)] and len(out) == int(ln.sum())       # back to back
    return {name: out[int(a):int(a) + int(n)] for name, a, n in zip(names, off, ln)}


@pytest.fixture(scope="module")
def dynamic():
    return split(*track.deflate_zlib_host(list(INPUTS.values()), codes="dynamic"), INPUTS)


@pytest.fixture(scope="module")
def fixed():
    return split(*track.deflate_zlib_host(list(INPUTS.values()), codes="fixed"), INPUTS)


@pytest.fixture(scope="module")
def parsed(dynamic):
    return {name: dc.block_tokens(s) for name, s in dynamic.items()}


def check_dynamic_stream(stream, fixed_stream, raw):
    """What a dynamic-mode stream must satisfy against the fixed-mode stream of the same input."""
    wc.check_stream(stream, raw)
    assert len(stream) <= len(fixed_stream)
    btype, tokens, tables = dc.block_tokens(stream)
    fixed_tokens = wc.fixed_tokens(fixed_stream)
    if btype != 2:
        assert stream == fixed_stream                    # what the fixed mode gives, to the byte
        return btype
    assert len(stream) < len(fixed_stream) and len(stream) < len(raw) + 11     # the choice: strictly smaller than both
    assert wc.replay(tokens) == raw
    if fixed_tokens is not None:
        assert tokens == fixed_tokens                    # the parse did not change
    lit_lengths, dist_lengths, cl_lengths, hclen = tables
    lit_counts, dist_counts = dc.histograms(tokens)
    for counts, lengths, limit in ((lit_counts, lit_lengths, 15), (dist_counts, dist_lengths, 15)):
        lengths = lengths + [0] * (len(counts) - len(lengths))
        dc.check_lengths(counts, lengths, limit)         # complete, within the limit, monotone, optimal below the limit
    assert len(lit_lengths) >= 257 and (len(lit_lengths) == 257 or lit_lengths[-1]) and (len(dist_lengths) == 1 or dist_lengths[-1])     # HLIT, HDIST trimmed
    assert dc.kraft(cl_lengths, 7) == 1 << 7 and max(cl_lengths) <= 7
    assert hclen == 4 or cl_lengths[dc.CL_ORDER[hclen - 1]]                  # HCLEN trimmed
    return btype


@pytest.mark.parametrize("name", list(INPUTS))
def test_every_stream_inflates_and_its_codes_are_complete_and_optimal(dynamic, fixed, name):
    check_dynamic_stream(dynamic[name], fixed[name], INPUTS[name])


def test_the_code_length_code_is_optimal_for_what_the_header_holds(dynamic):
    """The header's run-length symbols, read back, under the code-length code: complete by the test above; here its cost
    against heapq's for the same symbols (no length at 7: optimal)."""
    seen = 0
    for name, s in dynamic.items():
        btype, _, tables = dc.block_tokens(s)
        if btype != 2:
            continue
        lit_lengths, dist_lengths, cl_lengths, _ = tables
        r = dc.BitReader(s[2:-4])
        r.at = 3 + 14 + 3 * tables[3]
        table, counts, got = dc.canonical(cl_lengths), [0] * 19, 0
        while got < len(lit_lengths) + len(dist_lengths):
            sym = r.symbol(table)
            counts[sym] += 1
            got += 1 if sym < 16 else (3 + r.take(2) if sym == 16 else (3 + r.take(3) if sym == 17 else 11 + r.take(7)))
        dc.check_lengths(counts, cl_lengths, 7)
        seen += 1
    assert seen >= 3                                     # (the three count sections at the least: their size conditions need the dynamic block)


def test_which_block_wins(parsed, dynamic, fixed):
    # a dynamic header alone (14 bits, 14 or more code-length code lengths of 3 bits, the coded lengths) outweighs the whole
    # fixed body of an input of 0 .. 5 bytes (at most 3 + 5 x 9 + 7 bits): the fixed block stays
    for n in range(6):
        assert parsed["len%d" % n][0] == 1 and dynamic["len%d" % n] == fixed["len%d" % n]
    assert dynamic["len0"] == b"\x78\x01\x03\x00\x00\x00\x00\x01"
    # random bytes: no code brings 8 bits a byte below 8, and the header comes on top: the stored block stays
    for name in ("random12312", "random24600"):
        assert parsed[name][0] == 0 and len(dynamic[name]) == len(INPUTS[name]) + 11 and dynamic[name] == fixed[name]
    # count sections, runs and the markers: the block's own codes win
    for name in ("section1023", "section1024", "section2048", "runs_3_180", "runs_181_259", "markers", "repeat24600"):
        assert parsed[name][0] == 2, name
    assert {p[0] for p in parsed.values()} == {0, 1, 2}


def test_fewer_than_two_symbols_are_padded(parsed):
    # one run: the byte, 95 matches of 258 at distance 1, the rest, the end of block.  ONE distance code is used: code 0;
    # code 1 is the lowest unused one, and both get one bit
    btype, tokens, tables = parsed["repeat24600"]
    assert btype == 2 and {t[2] for t in tokens if t[0] == "match"} == {1}
    assert tables[1] == [1, 1]
    lit_counts, _ = dc.histograms(tokens)
    assert [s for s, n in enumerate(tables[0]) if n] == [s for s, c in enumerate(lit_counts) if c]
    # the length function itself: no symbol used, one used
    assert list(track.huffman_lengths_host([0] * 30, 15)) == [1, 1] + [0] * 28
    assert list(track.huffman_lengths_host([0] * 7 + [12] + [0] * 22, 15)) == [1] + [0] * 6 + [1] + [0] * 22
    assert list(track.huffman_lengths_host([5] + [0] * 18, 7)) == [1, 1] + [0] * 17
    # a section of one item: whichever block it takes, a dynamic one would carry two distance lengths at least
    btype, tokens, tables = parsed["section1"]
    if btype == 2:
        assert len([n for n in tables[1] if n]) >= 2


def test_sizes_against_the_fixed_streams_and_zlib(dynamic, fixed):
    """Any optimal code meets both bounds with the largest header a block can carry (285 bytes): the token bits of the
    greedy parse under an optimal code are 6 423, 4 323 and 8 857 bytes for these inputs."""
    for name in ("section1023", "section1024", "section2048"):
        d, f, z = len(dynamic[name]), len(fixed[name]), len(zlib.compress(INPUTS[name], 6))
        print(name, "dynamic", d, "fixed", f, "zlib level 6", z)
        assert d <= 0.80 * f
        assert d <= 1.15 * z


def test_many_inputs_in_one_call():
    many = wc.many_inputs()
    out, off, ln = track.deflate_zlib_host(many, codes="dynamic")
    fout, foff, fln = track.deflate_zlib_host(many, codes="fixed")
    types = set()
    for raw, a, n, fa, fn in zip(many, off, ln, foff, fln):
        types.add(check_dynamic_stream(out[int(a):int(a) + int(n)], fout[int(fa):int(fa) + int(fn)], raw))
    assert types == {0, 1, 2}
    assert int(ln.sum()) < int(fln.sum())


@pytest.mark.parametrize("name", list(LENGTH_CASES))
def test_huffman_lengths_host(name):
    counts, limit = LENGTH_CASES[name]
    lengths = track.huffman_lengths_host(counts, limit)
    assert lengths.dtype == np.uint8 and len(lengths) == len(counts)
    dc.check_lengths(counts, lengths, limit)
    if name.startswith("fib") and name not in ("fib16_15",):
        assert max(lengths) == limit                         # the chain was cut: the limit was needed
    assert list(track.huffman_lengths_host(counts, limit)) == list(lengths)


def test_huffman_lengths_do_not_depend_on_where_equal_counts_stand():
    """The order is (count, symbol): equal counts take their lengths by symbol number, longest first."""
    lengths = list(track.huffman_lengths_host([1, 1, 1, 1, 1], 15))
    assert lengths == [3, 3, 2, 2, 2]
    assert list(track.huffman_lengths_host([4, 1, 1, 2], 15)) == [1, 3, 3, 2]
    assert list(track.huffman_lengths_host([1, 1, 2, 4], 2)) == [2, 2, 2, 2]      # depth 3 under limit 2


def test_huffman_lengths_refusals():
    for counts, limit in (([1], 15), ([1] * 287, 15), ([1, 2, 3], 0), ([1, 2, 3], 16), ([1] * 9, 3), ([1 << 31, 1 << 31], 15), ([3, -1], 15)):
        with pytest.raises(ValueError):
            track.huffman_lengths_host(counts, limit)


def raw_call(fn, inputs, *extra):
    lens = np.array([len(s) for s in inputs], np.int64)
    offs = (np.cumsum(lens) - lens).astype(np.int64)
    image = b"".join(inputs)
    cap = int(lens.sum()) + 11 * len(inputs)
    out, out_off, out_len = np.zeros(max(cap, 1), np.uint8), np.zeros(len(inputs), np.int64), np.zeros(len(inputs), np.int64)
    buf = ctypes.create_string_buffer(image, len(image))
    rc = fn(ctypes.cast(buf, ctypes.c_void_p), len(inputs), offs.ctypes.data, lens.ctypes.data, out.ctypes.data, cap, out_off.ctypes.data, out_len.ctypes.data, *extra)
    return rc, out[:int(out_len.sum())].tobytes(), list(out_len)


def test_mode_1_is_the_old_seam_and_other_modes_are_refused():
    from plastid_amd.bam import _load
    L = _load()
    inputs = list(INPUTS.values())
    old = raw_call(L.pb_deflate_zlib, inputs)
    assert old[0] == 0 and raw_call(L.pb_deflate_zlib_mode, inputs, 1) == old
    two = raw_call(L.pb_deflate_zlib_mode, inputs, 2)
    assert two[0] == 0 and two[1] == track.deflate_zlib_host(inputs, codes="dynamic")[0] and two[1] != old[1]
    assert track.deflate_zlib_host(inputs)[0] == old[1] and track.deflate_zlib_host(inputs, codes="fixed")[0] == old[1]
    for mode in (0, 3, -1):
        assert raw_call(L.pb_deflate_zlib_mode, inputs[:3], mode)[0] != 0
        assert b"mode" in L.pb_last_error()


def test_refusals():
    with pytest.raises(ValueError, match="more than 24600 bytes"):
        track.deflate_zlib_host([b"x" * (wc.MAX_INPUT + 1)], codes="dynamic")
    with pytest.raises(ValueError, match="out_capacity"):
        track.deflate_zlib_host([b"abc", b"defg"], capacity=3 + 4 + 22 - 1, codes="dynamic")
    with pytest.raises(ValueError, match="codes"):
        track.deflate_zlib_host([b"abc"], codes="optimal")
    out, off, ln = track.deflate_zlib_host([b"abc", b"defg"], capacity=3 + 4 + 22, codes="dynamic")
    assert zlib.decompress(out[int(off[1]):]) == b"defg"
    out, off, ln = track.deflate_zlib_host([], codes="dynamic")
    assert out == b"" and len(off) == 0 and len(ln) == 0


def test_deflate_dynamic_host_program(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "deflate_dynamic_host_test")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    if subprocess.call([cxx] + san + [str(probe), "-o", str(tmp_path / "probe")], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL) != 0 \
            or subprocess.call([str(tmp_path / "probe")]) != 0:
        san = []
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror"] + san + ["-I", os.path.join(root, "plastid_amd", "csrc"),
                           os.path.join(root, "tests", "deflate_dynamic_host_test.cpp"), "-lz", "-o", exe])
    inputs = list(INPUTS.values()) + wc.many_inputs(40)
    blob = tmp_path / "inputs.bin"
    blob.write_bytes(struct.pack("<I", len(inputs)) + b"".join(struct.pack("<I", len(x)) + x for x in inputs))
    cases = [c for c in LENGTH_CASES.values() if sum(c[0]) < 1 << 32]
    counts = tmp_path / "counts.bin"
    counts.write_bytes(struct.pack("<I", len(cases)) + b"".join(struct.pack("<II", len(c), limit) + np.array(c, np.uint32).tobytes() for c, limit in cases))
    out = subprocess.run([exe, str(blob), str(counts)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert out.returncode == 0, out.stdout.decode()
    assert b"deflate_dynamic_host: ok" in out.stdout
