"""pc_deflate_zlib_mode with mode 2 -- the DYNAMIC instantiation of k_zlib_deflate (csrc/deflate_kernels.hip.h: histograms,
rank sort, the trees of csrc/deflate_host.h on two lanes, the header, the choice of the block) -- against its model, the
serial host encoder (pb_deflate_zlib_mode, tested on the CPU by test_deflate_dynamic_host.py): over every input of
tests/bigwig_write_cases.py one per call and all in one call, over 200 inputs in ONE call and over inputs at odd offsets
of one image, the offsets, the lengths and the bytes are the model's; every stream inflates with zlib and with the GPU's
own k_zlib_inflate (pc_inflate_zlib, status 0) to its input; mode 1 of the new seam is pc_deflate_zlib; pc_huffman_lengths
(k_huffman_lengths) gives the host twin's lengths past both limits; refusals leave the engine working."""
import ctypes
import os
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from plastid_amd import _lib, track  # noqa: E402
from plastid_amd._lib import check  # noqa: E402
from plastid_amd.engine import Engine  # noqa: E402
from tests import bigwig_write_cases as wc  # noqa: E402
from tests import deflate_dynamic_cases as dc  # noqa: E402

pytestmark = pytest.mark.gpu
INPUTS = wc.deflate_inputs()
LENGTH_CASES = dc.length_cases()


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def compare(eng, inputs):
    """Device against model: offsets, lengths, bytes; then every stream on its own merits."""
    want, want_off, want_len = track.deflate_zlib_host(inputs, codes="dynamic")
    got, off, ln = track.deflate_zlib(eng, inputs, codes="dynamic")
    assert list(ln) == list(want_len) and list(off) == list(want_off)
    wrong = [k for k in range(len(inputs)) if got[int(off[k]):int(off[k] + ln[k])] != want[int(off[k]):int(off[k] + ln[k])]]
    assert not wrong, wrong[:10]
    assert got == want
    streams = [got[int(a):int(a + n)] for a, n in zip(off, ln)]
    for s, raw in zip(streams, inputs):
        assert zlib.decompress(s) == raw
    back = track.inflate_zlib(eng, streams, wc.MAX_INPUT)
    assert [st for _, st in back] == [0] * len(inputs)
    assert all(out == raw for (out, _), raw in zip(back, inputs))
    return streams


@pytest.mark.parametrize("name", list(INPUTS))
def test_one_input_equals_the_model(eng, name):
    compare(eng, [INPUTS[name]])


def test_all_inputs_in_one_call(eng):
    streams = compare(eng, list(INPUTS.values()))
    assert {(s[2] >> 1) & 3 for s in streams} == {0, 1, 2}           # stored, fixed and dynamic blocks side by side


def test_many_inputs_in_one_call(eng):
    many = wc.many_inputs()
    streams = compare(eng, many)
    assert {len(s) % 4 for s in streams} == {0, 1, 2, 3}
    assert {(s[2] >> 1) & 3 for s in streams} == {0, 1, 2}
    fixed, _, fixed_len = track.deflate_zlib(eng, many)
    assert all(len(s) <= int(n) for s, n in zip(streams, fixed_len))


def raw_call(fn, eng, image, off, ln, *extra):
    cap = int(ln.sum()) + 11 * len(ln)
    out, out_off, out_len = np.zeros(cap, np.uint8), np.zeros(len(ln), np.int64), np.zeros(len(ln), np.int64)
    buf = ctypes.create_string_buffer(image, len(image))
    rc = fn(eng._h, ctypes.cast(buf, ctypes.c_void_p), len(ln), off.ctypes.data, ln.ctypes.data, out.ctypes.data, cap, out_off.ctypes.data, out_len.ctypes.data, *extra)
    return rc, out[:int(out_len.sum())].tobytes(), list(out_len)


def test_inputs_anywhere_in_the_image(eng):
    """Inputs that overlap, repeat and stand at odd offsets of one image (the Python helper lays them back to back)."""
    image = INPUTS["section1024"] + INPUTS["runs_3_180"]
    off = np.array([1, 0, 1, 12000, len(image) - 5, 7], np.int64)
    ln = np.array([5000, 0, 5000, 12001, 5, wc.MAX_INPUT], np.int64)
    rc, out, out_len = raw_call(_lib.load().pc_deflate_zlib_mode, eng, image, off, ln, 2)
    check(rc, "pc_deflate_zlib_mode")
    want, _, want_len = track.deflate_zlib_host([image[a:a + n] for a, n in zip(off, ln)], codes="dynamic")
    assert out_len == list(want_len) and out == want


def test_mode_1_is_the_old_seam_and_other_modes_are_refused(eng):
    L = _lib.load()
    image = b"".join(INPUTS.values())
    ln = np.array([len(v) for v in INPUTS.values()], np.int64)
    off = (np.cumsum(ln) - ln).astype(np.int64)
    old = raw_call(L.pc_deflate_zlib, eng, image, off, ln)
    assert old[0] == 0 and raw_call(L.pc_deflate_zlib_mode, eng, image, off, ln, 1) == old
    assert old[1] == track.deflate_zlib_host(list(INPUTS.values()))[0] == track.deflate_zlib(eng, list(INPUTS.values()), codes="fixed")[0]
    for mode in (0, 3, -1):
        assert raw_call(L.pc_deflate_zlib_mode, eng, image, off, ln, mode)[0] == -1
    compare(eng, [INPUTS["section1"]])


@pytest.mark.parametrize("name", list(LENGTH_CASES))
def test_huffman_lengths_equal_the_host_twin(eng, name):
    counts, limit = LENGTH_CASES[name]
    want = track.huffman_lengths_host(counts, limit)
    got = track.huffman_lengths(eng, counts, limit)
    assert got.dtype == np.uint8 and list(got) == list(want)
    dc.check_lengths(counts, got, limit)


def test_refusals_leave_the_engine_working(eng):
    with pytest.raises(ValueError, match="more than 24600 bytes"):
        track.deflate_zlib(eng, [b"abc", b"x" * (wc.MAX_INPUT + 1)], codes="dynamic")
    with pytest.raises(ValueError, match="out_capacity"):
        track.deflate_zlib(eng, [b"abc", b"defg"], capacity=3 + 4 + 22 - 1, codes="dynamic")
    with pytest.raises(ValueError, match="codes"):
        track.deflate_zlib(eng, [b"abc"], codes="optimal")
    for counts, limit in (([1], 15), ([1] * 287, 15), ([1, 2, 3], 0), ([1, 2, 3], 16), ([1] * 9, 3), ([1 << 31, 1 << 31], 15)):
        with pytest.raises(ValueError):
            track.huffman_lengths(eng, counts, limit)
    # the library's own refusals, under the Python checks
    L = _lib.load()
    c, out = np.ones(9, np.uint32), np.zeros(9, np.uint8)
    assert L.pc_huffman_lengths(eng._h, c.ctypes.data, 9, 3, out.ctypes.data) == -1
    assert L.pc_huffman_lengths(eng._h, c.ctypes.data, 1, 15, out.ctypes.data) == -1
    assert L.pc_huffman_lengths(eng._h, None, 9, 15, out.ctypes.data) == -1
    big = np.full(2, 1 << 31, np.uint32)
    assert L.pc_huffman_lengths(eng._h, big.ctypes.data, 2, 15, out.ctypes.data) == -1
    out, off, ln = track.deflate_zlib(eng, [], codes="dynamic")
    assert out == b"" and len(off) == 0
    assert list(track.huffman_lengths(eng, [4, 1, 1, 2], 15)) == [1, 3, 3, 2]
    compare(eng, [b"abc", b"defg" * 100])
