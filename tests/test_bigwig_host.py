"""plastid_amd/csrc/bigwig_host.h -- the bigWig container the host reader (plastid_amd.read_bigwig) and the device import
share -- on the CPU, against tests/golden/bigwig_fixture.npz (Kent's own writer and readers, and the reference's
BigWigGenomeArray over them: tests/golden/make_bigwig_golden.py): the contigs in bbiChromList's order, the block table, the
item table (assigned in file order it gives bigWigValsOnChromFetchData's values and bigWigIntervalQuery's intervals), the
refusals word for word; the files of tests/bigwig_writer.py re-read by a reader of the test's own (struct + zlib); a
host-only model of BigWigReader / BigWigGenomeArray (numpy over read_bigwig) against the fixture, the sum() quirk included;
and tests/bigwig_host_test.cpp: the header under the address and undefined-behaviour sanitizers, as a program, over the
fixture's files and every truncation and single-byte damage of a small one.  No GPU needed."""
import os
import shutil
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import plastid_amd as pa  # noqa: E402
from plastid_amd import track  # noqa: E402
from tests import bigwig_cases as bc  # noqa: E402
from tests import bigwig_writer as bw  # noqa: E402

S = bw.Section


@pytest.fixture(scope="module")
def fx():
    return bc.load_fixture()


@pytest.fixture(scope="module")
def files(fx):
    return bc.fixture_files(fx)


@pytest.fixture(scope="module")
def tables(files):
    return {n: pa.read_bigwig(image) for n, image in files.items()}


def file_names():
    return list(bc.kent_texts()) + list(bc.python_files())


def test_the_fixture_holds_the_cases(fx):
    assert [str(n) for n in fx["files"]] == file_names() and [str(a) for a in fx["arrays"]] == list(bc.ARRAYS)


@pytest.mark.parametrize("name", file_names())
def test_info_and_block_table(fx, files, tables, name):
    info = track.bigwig_info(files[name])
    chroms, sizes = [str(c) for c in fx[name + "_chroms"]], [int(x) for x in fx[name + "_sizes"]]
    assert list(info["chroms"].items()) == list(zip(chroms, sizes))          # bbiChromList's order
    t = tables[name]
    assert t.names == chroms and t.lengths == sizes
    # Kent lists the blocks per contig, each list in index order: per contig, the table's blocks in order
    kent = [(int(c), int(o), int(s)) for c, o, s in fx[name + "_blocks"]]
    first_chrom = {}
    for b, c in zip(t.block, t.chrom):
        first_chrom.setdefault(int(b), int(c))
    mine = sorted(((first_chrom[b], b) for b in first_chrom))
    assert [(c, int(t.block_off[b]), int(t.block_size[b])) for c, b in mine] == kent
    assert info["blocks"] == list(zip(t.block_off.tolist(), t.block_size.tolist())) and len(info["blocks"]) == t.stats["blocks"]
    assert (info["uncompress_buf_size"] == 0) == (name == "kent_stored") and info["version"] >= 3
    assert t.stats["compressed_blocks"] == (0 if name == "kent_stored" else t.stats["blocks"])


@pytest.mark.parametrize("name", file_names())
def test_items_give_kents_values(fx, tables, name):
    t = tables[name]
    for ci, c in enumerate(t.names):
        exp = np.zeros(t.lengths[ci])
        for (k, a, b), v in zip(fx[name + "_runs"], fx[name + "_run_values"]):
            if k == ci:
                exp[a:b] = v
        assert np.array_equal(t.chromosome_counts(c), exp), c
    off = fx[name + "_region_off"]
    for r, (ci, a, b) in enumerate(fx[name + "_regions"]):
        got = np.zeros(b - a)
        for k in range(off[r], off[r + 1]):
            s, e = fx[name + "_ivs"][k]
            got[s - a:e - a] = fx[name + "_iv_values"][k]
        assert np.array_equal(t.chromosome_counts(t.names[ci])[a:b], got), r
    total = sum(float(t.chromosome_counts(c)[lo:hi].sum()) for c, (lo, hi) in zip(t.names, track.sum_ranges(t.lengths)))
    assert total == float(fx[name + "_sum"])


def test_the_sum_quirk_shows(fx, tables):
    t = tables["kent_mixed"]
    assert track.sum_ranges([3000, 1200, 2500]) == [(0, 3000), (1200, 1200), (2500, 2500)]
    assert float(fx["kent_mixed_sum"]) == float(t.chromosome_counts("chrA").sum()) < sum(float(t.chromosome_counts(c).sum()) for c in t.names)


@pytest.mark.parametrize("name", list(bc.python_files()))
def test_writer_is_read_by_a_reader_of_its_own(files, tables, name):
    image = bc.python_files()[name]
    chroms, blocks, items = bw.read_model(image)
    assert (chroms, blocks, items) == bw.read_model(files[name])              # what the fixture's bytes hold
    t = pa.read_bigwig(image)
    assert [(n, s) for n, _, s in chroms] == list(zip(t.names, t.lengths))
    assert blocks == list(zip(t.block_off.tolist(), t.block_size.tolist()))
    by_id = {cid: k for k, (_, cid, _) in enumerate(chroms)}
    assert [(by_id[c], a, e, v, b) for c, a, e, v, b in items] == list(zip(t.chrom.tolist(), t.start.tolist(), t.stop.tolist(), t.value.tolist(), t.block.tolist()))
    assert pa.read_bigwig(image).tuples() == tables[name].tuples()


# ---------------------------------------------------------------------------------------------------------------------
# a host-only model of the two classes: numpy over read_bigwig

class HostArray(object):
    def __init__(self, tables, adds):
        self.by_strand = {}
        for strand, f in adds:
            self.by_strand.setdefault(strand, []).append(tables[f])
        self.readers = [t for r in self.by_strand.values() for t in r]

    def lengths(self):
        out = {}
        for t in self.readers:
            for c, n in zip(t.names, t.lengths):
                out[c] = max(out.get(c, 0), n)
        return out

    def sum(self):
        return sum([sum(float(t.chromosome_counts(c)[lo:hi].sum()) for c, (lo, hi) in zip(t.names, track.sum_ranges(t.lengths))) for t in self.readers], 0)

    def get_genome_order(self, chrom, a, b, strand, norm):
        v = np.zeros(b - a)
        for t in self.by_strand.get(strand, []):
            r = np.zeros(b - a)
            if chrom in t.names:
                whole = t.chromosome_counts(chrom)
                lo, hi = max(a, 0), min(b, len(whole))
                if hi > lo:
                    r[lo - a:hi - a] = whole[lo:hi]
            v += r
        return v / float(self.sum()) * 1e6 if norm else v


def expected_gets(fx, aname, norm):
    off, flat = fx[aname + "_get_off"], fx[aname + ("_get_norm" if norm else "_get")]
    return [flat[off[k]:off[k + 1]] for k in range(len(off) - 1)]


@pytest.mark.parametrize("aname", list(bc.ARRAYS))
def test_host_model_of_the_array(fx, tables, aname):
    arr = HostArray(tables, bc.ARRAYS[aname])
    assert sorted(arr.lengths()) == [str(c) for c in fx[aname + "_chroms"]]
    assert arr.lengths() == dict(zip([str(c) for c in fx[aname + "_length_names"]], [int(x) for x in fx[aname + "_lengths"]]))
    assert sorted(arr.by_strand) == [str(s) for s in fx[aname + "_strands"]]
    assert arr.sum() == float(fx[aname + "_sum"])
    segs, chains = bc.query_segments(20261020)
    for norm in (False, True):
        exp = iter(expected_gets(fx, aname, norm))
        for strand in "+-.":
            for c, a, b in segs:
                v = arr.get_genome_order(c, a, b, strand, norm)
                assert np.array_equal(v[::-1] if strand == "-" else v, next(exp), equal_nan=True), (strand, c, a, b)
        for strand in "+-.":
            for ch in chains:
                v = np.concatenate([arr.get_genome_order(c, a, b, strand, norm) for c, a, b in ch])
                assert np.array_equal(v[::-1] if strand == "-" else v, next(exp), equal_nan=True), (strand, ch)
    # to_genome_array: every reader added onto its strand; every contig 10000 longer than lengths() (the first write that
    # ends at a contig's length grows it)
    strands = sorted(arr.by_strand)
    names = [str(c) for c in fx[aname + "_ga_names"]]
    assert dict(zip(names, [int(x) for x in fx[aname + "_ga_lengths"]])) == {c: n + 10000 for c, n in arr.lengths().items()}
    total = 0.0
    for c in names:
        for si, st in enumerate(strands):
            exp = fx["%s_ga_%s_%d" % (aname, c, si)]
            got = np.zeros(len(exp))
            got[:arr.lengths()[c]] = arr.get_genome_order(c, 0, arr.lengths()[c], st, False)
            assert np.array_equal(got, exp), (c, st)
            total += float(got.sum())
    assert total == float(fx[aname + "_ga_sum"])


# ---------------------------------------------------------------------------------------------------------------------
# refusals

CHROMS = [("chrA", 1000), ("chrB", 500)]
GOOD = [S(0, "bedgraph", [(0, 5, 1.5), (5, 9, 2.0)]), S(1, "variable", [(3, 1.0), (10, 2.0)], span=4), S(1, "fixed", [1.0, 2.0, 3.0], span=2, step=3, start=100)]


def put(fmt, off, value):
    def damage(image, layout):
        struct.pack_into(fmt, image, off(layout) if callable(off) else off, value)
    return damage


def reblock(k, change):
    """Block k's section rewritten before it is compressed: change(bytearray) -> bytes."""
    return {"edit_raw": {k: change}}


def setb(off, value):
    def change(raw):
        raw[off:off + len(value)] = value
        return raw
    return change


REFUSED = [
    ("bigbed", put("<I", 0, 0x8789F2EB), "this is a bigBed file (magic 0x8789F2EB), not a bigWig"),
    ("swapped", put(">I", 0, 0x888FFC26), "byte-swapped (big-endian) files are not read"),
    ("magic", put("<I", 0, 0x12345678), "not a bigWig file (magic is not 0x888FFC26)"),
    ("version", put("<H", 4, 2), "version below 3"),
    ("chrom_tree_outside", put("<Q", 8, 1 << 40), "the chromosome tree lies outside the file"),
    ("chrom_tree_magic", put("<I", lambda l: l.chrom_tree, 1), "the chromosome tree has a wrong magic"),
    ("chrom_node_outside", put("<H", lambda l: l.chrom_tree + 32 + 2, 60000), "a node of the chromosome tree lies outside the file"),
    ("index_outside", put("<Q", 24, 1 << 40), "the unzoomed index lies outside the file"),
    ("index_magic", put("<I", lambda l: l.index, 1), "the unzoomed index has a wrong magic"),
    ("index_node_outside", put("<H", lambda l: l.index + 48 + 2, 60000), "a node of the unzoomed index lies outside the file"),
    ("block_outside", put("<Q", lambda l: l.index + 48 + 4 + 32 + 16, 1 << 40), "block 1: the block lies outside the file"),
    ("block_end_outside", put("<Q", lambda l: l.index + 48 + 4 + 32 + 24, (1 << 28) + 1), "block 1: the block lies outside the file"),
    ("zlib_cm", put("<B", lambda l: l.blocks[1][0], 0x79), "block 1: not a zlib stream of CM = 8 without FDICT"),
    ("zlib_fdict", put("<H", lambda l: l.blocks[2][0], 0x3d78), "block 2: not a zlib stream of CM = 8 without FDICT"),
    ("adler", put("<B", lambda l: l.blocks[1][0] + l.blocks[1][1] - 1, 0), "block 1: Adler-32 mismatch"),
    ("deflate", put("<B", lambda l: l.blocks[0][0] + 2, 0x07), "block 0: DEFLATE error"),
    ("type", reblock(1, setb(20, b"\x04")), "block 1: section of unknown type"),
    ("type0", reblock(0, setb(20, b"\x00")), "block 0: section of unknown type"),
    ("count", reblock(2, setb(22, struct.pack("<H", 4))), "block 2: the items do not end where the block does"),
    ("short", reblock(0, lambda raw: raw[:20]), "block 0: shorter than a section header"),
    ("chrom_id", reblock(1, setb(0, struct.pack("<I", 2))), "block 1: chromId outside the chromosome tree"),
    ("empty_item", reblock(0, setb(24 + 12, struct.pack("<II", 9, 9))), "block 0 item 1: end <= start"),
    ("beyond", reblock(1, setb(24 + 8, struct.pack("<I", 497))), "block 1 item 1: end beyond the contig's size"),
    ("beyond_fixed", reblock(2, setb(4, struct.pack("<I", 493))), "block 2 item 2: end beyond the contig's size"),
    ("span0", reblock(1, setb(16, struct.pack("<I", 0))), "block 1 item 0: end <= start"),
    ("lowest_first", {"edit_raw": {2: setb(20, b"\x09"), 0: setb(24 + 12, struct.pack("<II", 9, 9))}}, "block 0 item 1: end <= start"),
]


def refused_image(name):
    how = [d for n, d, _ in REFUSED if n == name][0]
    return bw.write_bigwig(CHROMS, GOOD, fanout=256, level=6, **(how if isinstance(how, dict) else {"damage": how}))


def test_the_undamaged_file_reads():
    t = pa.read_bigwig(bw.write_bigwig(CHROMS, GOOD))
    assert t.tuples() == [("chrA", 0, 5, 1.5), ("chrA", 5, 9, 2.0), ("chrB", 3, 7, 1.0), ("chrB", 10, 14, 2.0), ("chrB", 100, 102, 1.0),
                          ("chrB", 103, 105, 2.0), ("chrB", 106, 108, 3.0)]


@pytest.mark.parametrize("name", [n for n, _, _ in REFUSED])
def test_refusals_word_for_word(name, tmp_path):
    what = [w for n, _, w in REFUSED if n == name][0]
    image = refused_image(name)
    with pytest.raises(ValueError) as e:
        pa.read_bigwig(image)
    assert str(e.value) == "<memory>: bigWig: " + what
    if what.startswith("block") and "block lies" not in what and "zlib stream" not in what:
        track.bigwig_info(image)                     # (the container is whole: only reading the blocks finds it)
    else:
        with pytest.raises(ValueError) as e2:
            track.bigwig_info(image)
        assert str(e2.value) == "<memory>: bigWig: " + what
    p = tmp_path / "refused.bw"
    p.write_bytes(image)
    with pytest.raises(ValueError) as e3:
        pa.read_bigwig(str(p))
    assert str(e3.value) == "%s: bigWig: %s" % (p, what)


def test_capacity_and_stored_files():
    # uncompressBufSize is a bound, not a size: three times too large reads the same; too small is a DEFLATE error
    a = pa.read_bigwig(bw.write_bigwig(CHROMS, GOOD, buf_factor=3))
    assert a.tuples() == pa.read_bigwig(bw.write_bigwig(CHROMS, GOOD)).tuples() and a.stats["uncompress_buf_size"] == 3 * 48
    with pytest.raises(ValueError) as e:
        pa.read_bigwig(bw.write_bigwig(CHROMS, GOOD, damage=put("<I", 52, 47)))
    assert str(e.value) == "<memory>: bigWig: block 0: DEFLATE error"
    s = pa.read_bigwig(bw.write_bigwig(CHROMS, GOOD, level=None))
    assert s.tuples() == a.tuples() and s.stats["compressed_blocks"] == 0 and s.stats["bytes_inflated"] == 0
    empty = pa.read_bigwig(bw.write_bigwig(CHROMS, []))
    assert len(empty) == 0 and empty.names == ["chrA", "chrB"]


def test_bigwig_host_program(tmp_path, files):
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "bigwig_host_test")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    if subprocess.call([cxx] + san + [str(probe), "-o", str(tmp_path / "probe")], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL) != 0 \
            or subprocess.call([str(tmp_path / "probe")]) != 0:
        san = []
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror"] + san + ["-I", os.path.join(root, "plastid_amd", "csrc"),
                           os.path.join(root, "tests", "bigwig_host_test.cpp"), "-lz", "-o", exe])
    paths = []
    for n, image in files.items():
        p = tmp_path / (n + ".bw")
        p.write_bytes(image)
        paths.append("%s:%d" % (p, len(pa.read_bigwig(image))))
    small = tmp_path / "small.bw"
    small.write_bytes(bw.write_bigwig(CHROMS, GOOD, fanout=2, chrom_fanout=2, items_per_block=2))
    out = subprocess.run([exe, str(small)] + paths, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert out.returncode == 0, out.stdout.decode()
    assert b"bigwig_host: ok" in out.stdout
