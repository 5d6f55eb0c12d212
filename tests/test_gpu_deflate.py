"""pc_deflate_zlib -- k_zlib_deflate and k_deflate_compact (csrc/deflate_kernels.hip.h), the zlib ENCODER on the GPU --
against its model, the serial host encoder of csrc/deflate_host.h (pb_deflate_zlib): over every input of
tests/bigwig_write_cases.py, and over 200 inputs in ONE call (more streams than compute units, the compaction across the
blocks of the scan, streams that end on and off byte and dword borders), the offsets, the lengths and the bytes are the
model's; every stream inflates with zlib to its input and passes pc_inflate_zlib with status 0; an over-long input and a
short capacity are refused and the engine goes on working."""
import os
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from plastid_amd import track  # noqa: E402
from plastid_amd.engine import Engine  # noqa: E402
from tests import bigwig_write_cases as wc  # noqa: E402

pytestmark = pytest.mark.gpu
INPUTS = wc.deflate_inputs()


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def compare(eng, inputs):
    """Device against model: offsets, lengths, bytes; then every stream on its own merits."""
    want, want_off, want_len = track.deflate_zlib_host(inputs)
    got, off, ln = track.deflate_zlib(eng, inputs)
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
    compare(eng, list(INPUTS.values()))


def test_many_inputs_in_one_call(eng):
    many = wc.many_inputs()
    streams = compare(eng, many)
    assert {len(s) % 4 for s in streams} == {0, 1, 2, 3}
    kinds = {wc.fixed_tokens(s) is None for s in streams[:40]}
    assert kinds == {True, False}                       # stored and coded streams side by side


def test_inputs_anywhere_in_the_image(eng):
    """Inputs that overlap, repeat and stand at odd offsets of one image (the Python helper lays them back to back)."""
    import ctypes
    from plastid_amd import _lib
    from plastid_amd._lib import check
    image = INPUTS["section1024"] + INPUTS["runs_3_180"]
    off = np.array([1, 0, 1, 12000, len(image) - 5, 7], np.int64)
    ln = np.array([5000, 0, 5000, 12001, 5, wc.MAX_INPUT], np.int64)
    cap = int(ln.sum()) + 11 * len(ln)
    out, out_off, out_len = np.zeros(cap, np.uint8), np.zeros(len(ln), np.int64), np.zeros(len(ln), np.int64)
    buf = ctypes.create_string_buffer(image, len(image))
    check(_lib.load().pc_deflate_zlib(eng._h, ctypes.cast(buf, ctypes.c_void_p), len(ln), off.ctypes.data, ln.ctypes.data, out.ctypes.data, cap,
                                      out_off.ctypes.data, out_len.ctypes.data), "pc_deflate_zlib")
    want, _, want_len = track.deflate_zlib_host([image[a:a + n] for a, n in zip(off, ln)])
    assert list(out_len) == list(want_len) and out[:int(out_len.sum())].tobytes() == want


def test_refusals_leave_the_engine_working(eng):
    with pytest.raises(ValueError, match="more than 24600 bytes"):
        track.deflate_zlib(eng, [b"abc", b"x" * (wc.MAX_INPUT + 1)])
    with pytest.raises(ValueError, match="out_capacity"):
        track.deflate_zlib(eng, [b"abc", b"defg"], capacity=3 + 4 + 22 - 1)
    out, off, ln = track.deflate_zlib(eng, [])
    assert out == b"" and len(off) == 0
    compare(eng, [b"abc", b"defg" * 100])
