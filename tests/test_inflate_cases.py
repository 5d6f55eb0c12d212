"""The conformance cases of tests/inflate_cases.py, made trustworthy without a GPU: zlib inflates every valid member
to exactly the modelled payload and refuses every rejected one; the host decoder loads every valid group's file with
the expected columns and raises on every rejected case's file; and the list holds what it is meant to hold.

The reference is zlib.  The host decoder prefers libdeflate where the machine has it (csrc/bam_stager.cpp raw_inflate;
PB_ZLIB=1 keeps it to zlib), and libdeflate is more lenient than zlib and RFC 1951 in three places: it takes HLIT and
HDIST fields of 30 and 31 (as long as the symbols beyond 285 / 29 are not used), a repeat code that runs past
HLIT + HDIST, and the unused half of a single one-bit distance code (it decodes as the used half).  So every check
against the host decoder runs with PB_ZLIB=1; the valid files also run with the decoder's own choice of inflater, and
the rejected ones too, where LIBDEFLATE_TAKES names the six it may then load."""
import os
import sys
import zlib

import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from plastid_amd.bam import read_bam  # noqa: E402
from tests import inflate_cases as ic  # noqa: E402

GROUPS = list(ic.GROUPS)
LIBDEFLATE_TAKES = {"R.hlit30", "R.hlit31", "R.hdist30", "R.hdist31", "R.repeat.past", "R.dist.unusedhalf"}


def zlib_inflate(c):
    """What zlib makes of the member's DEFLATE stream, asked for ISIZE bytes as the host decoder asks:
    (bytes, finished)."""
    (_, at, isize), = ic.member_offsets(c.member)
    d = zlib.decompressobj(-15)
    out = d.decompress(c.member[at:-8], isize + 1) if isize else d.decompress(c.member[at:-8])
    return out, d.eof


@pytest.mark.parametrize("group", GROUPS)
def test_zlib_inflates_every_valid_case_to_the_model(group):
    cases = ic.GROUPS[group]()
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    for c in cases:
        assert c.valid
        out, eof = zlib_inflate(c)
        assert eof and out == c.payload, c.name
        (_, _, isize), = ic.member_offsets(c.member)
        assert isize == len(c.payload) and len(c.member) <= 65536, c.name
    print("group %s: %d members, %d listed items, %d bytes, %d inflated" % (group, len(cases), sum(len(c.covers) for c in cases),
                                                                            sum(len(c.member) for c in cases), sum(len(c.payload) for c in cases)))


def test_zlib_refuses_every_rejected_case():
    for c in ic.rejected():
        assert not c.valid and c.doc.startswith("kInf"), c.name
        (_, _, isize), = ic.member_offsets(c.member)
        assert isize > 0, c.name              # (both decoders pass over empty members)
        try:
            out, eof = zlib_inflate(c)
        except zlib.error:
            continue
        assert not eof or len(out) != isize, c.name


def columns_are_the_expected(r):
    assert r.n == len(ic.EXPECT_POS) and r.pos.tolist() == ic.EXPECT_POS and r.flag16.tolist() == ic.EXPECT_FLAG16
    assert r.mapped == len(ic.TAIL) and list(r.references) == ic.REFS and list(r.lengths) == ic.LENS


@pytest.mark.parametrize("inflater", ["zlib", "own"])
@pytest.mark.parametrize("group", GROUPS)
def test_the_host_decoder_loads_every_valid_group(tmp_path, monkeypatch, group, inflater):
    if inflater == "zlib":
        monkeypatch.setenv("PB_ZLIB", "1")
    path = str(tmp_path / "group.bam")
    open(path, "wb").write(ic.group_file(ic.GROUPS[group]()))
    columns_are_the_expected(read_bam(path))
    columns_are_the_expected(read_bam(path, threads=3))


def test_the_host_decoder_raises_on_every_rejected_case(tmp_path, monkeypatch):
    path = str(tmp_path / "rejected.bam")
    for c in ic.rejected():
        open(path, "wb").write(ic.rejected_file(c))
        monkeypatch.setenv("PB_ZLIB", "1")
        with pytest.raises(ValueError, match="BGZF"):
            read_bam(path)
        monkeypatch.delenv("PB_ZLIB")
        try:
            r = read_bam(path)
        except ValueError as e:
            assert "BGZF" in str(e), c.name
            continue
        assert c.name in LIBDEFLATE_TAKES, c.name       # (loaded: only where libdeflate is known to be lenient ...)
        columns_are_the_expected(r)                     # (... and then as the bytes of the trailer's CRC)


def test_the_list_holds_what_it_should():
    """The names of the issue's list, written out here once more: a case dropped from tests/inflate_cases.py fails."""
    def covers(*groups):
        return sorted(x for g in groups for c in ic.GROUPS[g]() for x in c.covers)
    lens = ["len%d.%s" % (s, w) for s in range(257, 285) for w in ("min", "max")] + ["len284.extra31", "len285.min"]
    dists = ["dist%d.%s" % (s, w) for s in range(30) for w in ("min", "max")]
    assert covers("A") == sorted("%s.%s" % (k, x) for k in ("fixed", "dynamic") for x in lens + dists)
    bd = list(range(1, 71)) + [127, 128, 129]
    bl = [3, 4, 63, 64, 65, 127, 128, 129, 257, 258]
    assert covers("B") == sorted("%s.d%d.l%d.%s" % (k, d, ln, w) for k in ("fixed", "dynamic") for d in bd for ln in bl for w in ("lit", "match"))
    cd = [1789, 1790, 1791, 1792, 2047, 2048, 2049, 2305, 2306, 3837, 3838, 3839, 4096, 32767, 32768]
    assert covers("C") == sorted("%s.d%d.l%d.p%d" % (h, d, ln, p) for h in ("stored", "huffman") for d in cd for ln in (3, 258)
                                 for p in (0, 1, 15, 16, 17, 511))
    assert covers("D") == sorted(["D.one.s%d" % s for s in range(601)] + ["D.two.g%d" % g for g in range(71)])
    e = ["hclen5", "hclen19.padded", "hclen19.len15", "cl.7bit", "hlit257.hdist1", "hlit286.padded", "hlit286.sym285", "hdist30.padded",
         "hdist30.sym29", "rle16.count3", "rle16.count6", "rle17.count3", "rle17.count10", "rle18.count11", "rle18.count138", "rle16.across",
         "rle.none", "dist.single.used", "dist.all.zero", "long.prefixes", "long.random0", "long.random1", "long.random2", "long.random3"]
    assert covers("E") == sorted("E." + x for x in e)
    f = ["stored.%s.bit%d.sp%d" % (w, b, sp) for w in ("empty", "onebyte") for b in range(8) for sp in range(4)]
    f += ["fixed.empty.middle", "fixed.empty.final", "dynamic.fixed.stored.dynamic", "blocks1000", "stored.largest", "stored.twowindows.match"]
    f += ["window%d.then.stored" % k for k in (1605, 1620, 1635)]
    assert covers("F") == sorted("F." + x for x in f)
    g = ["isize%d.%s" % (n, w) for n in (1, 2, 15, 16, 17, 63, 64, 65, 1055, 1056, 1057, 2112, 65535, 65536) for w in ("one", "many")]
    g += ["empty.fixed", "between.1", "empty.stored", "between.2"] + ["extra.b%s.a%s" % (b, a) for b in (None, 0, 1, 2, 3) for a in (None, 0, 1, 3)]
    g += ["align16.%d" % k for k in range(18)] + ["align16.tail"]
    assert covers("G") == sorted("G." + x for x in g)
    for k in range(3):
        assert covers("H%d" % k) == sorted("H%d.m%d" % (k, m) for m in range(200))
    r = ["blocktype3", "stored.nlen", "stored.beyond", "hlit30", "hlit31", "hdist30", "hdist31", "first16", "repeat.past", "no256", "ll.over",
         "ll.incomplete", "dist.incomplete2", "cl.over", "dist.unusedhalf", "hclen4", "fixed286", "fixed287", "fixed.dist30", "fixed.dist31",
         "dist.beyond.later", "dist.beyond.first", "over.literal", "over.match", "over.stored", "short", "ends.in.eob", "ends.in.literal"]
    assert sorted(c.name for c in ic.rejected()) == sorted("R." + x for x in r)


def test_the_members_lie_where_the_cases_say():
    """What a case claims about the place of its member in the file or in the inflated stream, checked on the file."""
    blob = ic.group_file(ic.group_g())
    at = ic.member_offsets(blob)[1:]                      # (behind the first member; one entry per case, then the tail)
    names = [c.name for c in ic.group_g()]
    assert {a % 4 for (_, a, _), nm in zip(at, names) if nm.startswith("G.extra.")} == {0, 1, 2, 3}
    uoff, starts = len(ic.lead_payload(0)), {}
    for (_, _, isize), nm in zip(at, names):
        starts[nm] = uoff
        uoff += isize
    assert {starts[nm] % 16 for nm in names if nm.startswith("G.align16.")} == set(range(16))
    assert [isize for (_, _, isize), nm in zip(at, names) if nm.startswith("G.empty.")] == [0, 0]
    # group H: members of 300 bytes and of 64 KiB, stored / fixed / dynamic blocks, 15-bit codes
    for k in range(3):
        sizes = [len(c.payload) for c in ic.group_h(k)]
        assert min(sizes) == 300 and max(sizes) == 65536
