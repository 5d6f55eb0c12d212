"""pc_inflate_zlib -- the zlib instantiation of k_bgzf_inflate (csrc/bam_kernels.hip.h) and k_zlib_adler
(csrc/bigwig_kernels.hip.h) -- on the hand-built DEFLATE streams of tests/inflate_cases.py: the raw stream of every case's
member wrapped again as ``78 9c`` + stream + Adler-32 of the modelled payload.  Bytes AND produced length must be the
payload's, with a capacity above every payload (65 536 + 16) and with the capacity exactly the payload's length; every
rejected stream is refused with a status and the engine goes on working; a wrong Adler-32 is refused; Adler-32 at the
lengths that pass the lane split and the reduction of the sums."""
import os
import struct
import sys
import zlib

import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from plastid_amd.engine import Engine  # noqa: E402
from plastid_amd.track import inflate_zlib  # noqa: E402
from tests import inflate_cases as ic  # noqa: E402

pytestmark = pytest.mark.gpu
CAPACITY = 65536 + 16


def rewrap(c):
    """The case's raw DEFLATE stream as a zlib stream with the Adler-32 of its modelled payload.  (A BGZF member may hold
    bytes between the end of its stream and its trailer -- some of the random members do -- and a zlib stream may not: the
    trailer stands where the stream ends, which zlib finds for the valid members.)"""
    (_, at, _), = ic.member_offsets(c.member)
    raw = c.member[at:len(c.member) - 8]
    if c.valid:
        d = zlib.decompressobj(-15)
        assert d.decompress(raw) == c.payload and d.eof
        raw = raw[:len(raw) - len(d.unused_data)]
    return b"\x78\x9c" + raw + struct.pack(">I", zlib.adler32(c.payload))


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def valid_cases():
    return [c for fn in ic.GROUPS.values() for c in fn()]


def health(eng):
    data = bytes(range(256)) * 40
    assert inflate_zlib(eng, [zlib.compress(data, 9), zlib.compress(b"", 6)], len(data)) == [(data, 0), (b"", 0)]


def test_valid_streams_bytes_and_length(eng, valid_cases):
    got = inflate_zlib(eng, [rewrap(c) for c in valid_cases], CAPACITY)
    bad = [(c.name, st, len(out), len(c.payload)) for c, (out, st) in zip(valid_cases, got) if st != 0 or out != c.payload]
    assert not bad, bad[:10]


def test_capacity_exactly_the_payload(eng, valid_cases):
    """Every stream alone with its payload's length as the capacity (grouped by length: one call per distinct length)."""
    by_len = {}
    for c in valid_cases:
        by_len.setdefault(len(c.payload), []).append(c)
    bad = []
    for n, cases in sorted(by_len.items()):
        got = inflate_zlib(eng, [rewrap(c) for c in cases], n)
        bad += [(c.name, st, len(out), n) for c, (out, st) in zip(cases, got) if st != 0 or out != c.payload]
    assert not bad, bad[:10]
    # one byte less is one byte too few
    c = max(valid_cases, key=lambda c: len(c.payload))
    (out, st), = inflate_zlib(eng, [rewrap(c)], len(c.payload) - 1)
    assert st != 0 and out == b""
    health(eng)


def test_rejected_streams_are_a_status(eng):
    rejected = ic.rejected()
    got = inflate_zlib(eng, [rewrap(c) for c in rejected], CAPACITY)
    taken = [c.name for c, (out, st) in zip(rejected, got) if st == 0]
    assert not taken, taken
    assert all(out == b"" for out, _ in got)
    health(eng)


def test_wrong_adler_and_header(eng):
    data = bytes(range(251)) * 50
    good = zlib.compress(data, 6)
    wrong = good[:-1] + bytes([good[-1] ^ 1])
    fdict = b"\x78\xbb" + good[2:]          # FDICT set (and FCHECK right for it)
    cm = b"\x79\x9c" + good[2:]
    slack = good[:-4] + b"\x00" + good[-4:]    # a byte between the stream's end and the trailer
    got = inflate_zlib(eng, [good, wrong, fdict, cm, slack, good[:5], b""], len(data))
    assert (0x78bb % 31, got[0]) == (0, (data, 0))
    assert [st for _, st in got[1:]] == [10, 12, 12, 11, 12, 12] and all(out == b"" for out, _ in got[1:])
    health(eng)


@pytest.mark.parametrize("level", [0, 6])
def test_adler_lengths(eng, level):
    """0xff bytes maximise both sums; the lengths pass the lane split (64 slices) and zlib's NMAX; 400 000 bytes give
    every lane more than NMAX bytes: the sums are reduced inside a slice."""
    lengths = [0, 1, 63, 64, 65, 5551, 5552, 5553, 65536, 400000]
    streams = [zlib.compress(b"\xff" * n, level) for n in lengths]
    got = inflate_zlib(eng, streams, max(lengths))
    assert [(len(out), st) for out, st in got] == [(n, 0) for n in lengths]
    assert all(out == b"\xff" * n for (out, _), n in zip(got, lengths))
    broken = [s[:-4] + struct.pack(">I", (zlib.adler32(b"\xff" * n) + 65521 * 0 + 1) & 0xffffffff) for s, n in zip(streams, lengths)]
    assert [st for _, st in inflate_zlib(eng, broken, max(lengths))] == [10] * len(lengths)
