"""BigWigReader / BigWigGenomeArray on the GPU (csrc/bigwig_kernels.hip.h, csrc/bigwig_decoder.hip.h).

Against tests/golden/bigwig_fixture.npz -- Kent's own writer and readers and the reference's BigWigGenomeArray over them
(tests/golden/make_bigwig_golden.py) -- bit for bit: every file's cells, chroms, sum and region reads; every array's chroms,
lengths, strands, sum, segment and chain reads, normalised reads, the warnings of a missing strand and a missing contig,
and to_genome_array().  Against the host reader (plastid_amd.read_bigwig, pinned to the fixture by
tests/test_bigwig_host.py): the kernel seams, files of tests/bigwig_writer.py.  The refused files of
tests/test_bigwig_host.py are refused with the host reader's words and leave a filled array as it was."""
import os
import random
import struct
import sys
import warnings
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import plastid_amd as pa  # noqa: E402
from plastid_amd import _lib  # noqa: E402
from plastid_amd.engine import Engine  # noqa: E402
from plastid_amd.exceptions import DataWarning  # noqa: E402
from plastid_amd.roitools import GenomicSegment, SegmentChain  # noqa: E402
from tests import bigwig_cases as bc  # noqa: E402
from tests import bigwig_writer as bw  # noqa: E402
from tests import test_bigwig_host as host  # noqa: E402
from tests.deflate_writer import M, Stream  # noqa: E402

pytestmark = pytest.mark.gpu
S = bw.Section
SEED = 20261020


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def fx():
    return bc.load_fixture()


@pytest.fixture(scope="module")
def paths(fx, tmp_path_factory):
    d = tmp_path_factory.mktemp("bigwig_fixture")
    out = {}
    for n, image in bc.fixture_files(fx).items():
        out[n] = str(d / (n + ".bw"))
        open(out[n], "wb").write(image)
    return out


def overlapping(t):
    """Items of `t` (a BigWigTable) in clusters of several: sorted by (contig, start), a cluster goes on while an item
    starts below the furthest end so far."""
    n = 0
    for ci in range(len(t.names)):
        idx = np.flatnonzero(t.chrom == ci)
        idx = idx[np.argsort(t.start[idx], kind="stable")]
        size, far = 0, -1
        for k in idx:
            if size and t.start[k] < far:
                size += 1
            else:
                n += size if size > 1 else 0
                size = 1
            far = max(far, int(t.stop[k]))
        n += size if size > 1 else 0
    return n


def same_as_table(reader, t):
    """The reader's cells, chroms and statistics against the host reader's table of the same file."""
    assert list(reader.chroms.items()) == list(zip(t.names, t.lengths))
    dense = reader._ga.to_host()
    for c in t.names:
        exp = t.chromosome_counts(c)
        assert np.array_equal(dense._chroms[c]["."], exp), c
        assert np.array_equal(reader.get_chromosome_counts(c), exp), c
    st = reader.import_stats()
    assert st["blocks"] == t.stats["blocks"] and st["inflated_blocks"] == t.stats["compressed_blocks"]
    assert (st["bedgraph_items"], st["variable_step_items"], st["fixed_step_items"]) == (t.stats["bedgraph_items"], t.stats["variable_step_items"], t.stats["fixed_step_items"])
    assert st["bytes_inflated"] == t.stats["bytes_inflated"] and st["overlapping"] == overlapping(t)
    assert st["bytes_in"] == (int((t.block_off + t.block_size).max() - t.block_off.min()) if len(t.block_off) else 0)
    assert set(reader.import_timing()) == {"upload", "inflate_adler", "sections_items", "sort_apply"}


# ---------------------------------------------------------------------------------------------------------------------
# the fixture

@pytest.mark.parametrize("name", host.file_names())
def test_fixture_files(eng, fx, paths, name):
    r = pa.BigWigReader(paths[name], engine=eng)
    try:
        chroms = [str(c) for c in fx[name + "_chroms"]]
        assert list(r.chroms.items()) == list(zip(chroms, [int(x) for x in fx[name + "_sizes"]])) and r.filename == paths[name]
        dense = r._ga.to_host()
        for ci, c in enumerate(chroms):
            exp = np.zeros(r.chroms[c])
            for (k, a, b), v in zip(fx[name + "_runs"], fx[name + "_run_values"]):
                if k == ci:
                    exp[a:b] = v
            assert np.array_equal(dense._chroms[c]["."], exp) and np.array_equal(r.get_chromosome_counts(c), exp), c
        off = fx[name + "_region_off"]
        for k, (ci, a, b) in enumerate(fx[name + "_regions"]):
            exp = np.zeros(b - a)
            for j in range(off[k], off[k + 1]):
                s, e = fx[name + "_ivs"][j]
                exp[s - a:e - a] = fx[name + "_iv_values"][j]
            assert np.array_equal(r.get(GenomicSegment(chroms[ci], int(a), int(b), "+")), exp)
            assert np.array_equal(r[GenomicSegment(chroms[ci], int(a), int(b), "-")], exp[::-1])
            assert np.array_equal(r.get(GenomicSegment(chroms[ci], int(a), int(b), "-"), roi_order=False), exp)
        with pytest.warns(DataWarning, match="Summing over a large BigWig file"):
            assert r.sum() == float(fx[name + "_sum"])
        same_as_table(r, pa.read_bigwig(paths[name]))
        # what the file lacks
        with pytest.warns(DataWarning) as w:
            assert np.array_equal(r.get(GenomicSegment("chrZ", 5, 25, "+")), np.zeros(20))
        assert [str(x.message) for x in w] == ["No data for chromosome 'chrZ' in file '%s'." % paths[name]]
        with pytest.warns(DataWarning, match="No data for chromosome 'chrZ'"):
            z = r.get_chromosome_counts("chrZ")
        assert z.shape == () and z == 0.0 and z.dtype == np.float64
        with pytest.raises(NotImplementedError):
            r.get(GenomicSegment("chrA", 0, 5, "+"), fill=1.0)
        assert np.array_equal(r.get(GenomicSegment("chrA", 0, 5, "+"), fill=0.0), r.get(GenomicSegment("chrA", 0, 5, "+")))
    finally:
        r.close()


@pytest.mark.parametrize("aname", list(bc.ARRAYS))
def test_fixture_arrays(eng, fx, paths, aname):
    arr = pa.BigWigGenomeArray(engine=eng)
    try:
        for strand, f in bc.ARRAYS[aname]:
            arr.add_from_bigwig(paths[f], strand)
        assert sorted(arr.chroms()) == [str(c) for c in fx[aname + "_chroms"]] and isinstance(arr.chroms(), set)
        assert list(arr.lengths().items()) == list(zip([str(c) for c in fx[aname + "_length_names"]], [int(x) for x in fx[aname + "_lengths"]]))
        assert list(arr.strands()) == [str(s) for s in fx[aname + "_strands"]]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", DataWarning)
            assert arr.sum() == float(fx[aname + "_sum"])
            segs, chains = bc.query_segments(SEED)
            for norm in (False, True):
                arr.set_normalize(norm)
                exp = iter(host.expected_gets(fx, aname, norm))
                for strand in "+-.":
                    for c, a, b in segs:
                        e = next(exp)
                        assert np.array_equal(arr.get(GenomicSegment(c, a, b, strand)), e, equal_nan=True), (norm, strand, c, a, b)
                        assert np.array_equal(arr[GenomicSegment(c, a, b, strand)], e, equal_nan=True)
                        assert np.array_equal(arr.get(GenomicSegment(c, a, b, strand), roi_order=False), e[::-1] if strand == "-" else e, equal_nan=True)
                made, want = [], []
                for strand in "+-.":
                    for ch in chains:
                        made.append(SegmentChain(*[GenomicSegment(c, a, b, strand) for c, a, b in ch]))
                        want.append(next(exp))
                        assert np.array_equal(made[-1].get_counts(arr), want[-1], equal_nan=True), (norm, strand, ch)
                for got, e in zip(arr.get_counts_batch(made), want):
                    assert np.array_equal(got, e, equal_nan=True)
                assert np.array_equal(made[0].get_masked_counts(arr).data, want[0], equal_nan=True)
            arr.set_normalize(False)
        # the warnings' texts
        have = list(dict.fromkeys(s for s, _ in bc.ARRAYS[aname]))
        with pytest.warns(DataWarning) as w:
            assert np.array_equal(arr.get(GenomicSegment("chrA", 0, 10, ".")), np.zeros(10))
        assert [str(x.message) for x in w] == ["Strand '.' not in BigWigGenomeArray (has %s)." % ", ".join(have)]
        with pytest.warns(DataWarning) as w:
            arr.get(GenomicSegment("chrZ", 0, 10, have[0]))
        assert [str(x.message) for x in w] == ["No data for chromosome 'chrZ' in file '%s'." % paths[f] for s, f in bc.ARRAYS[aname] if s == have[0]]
        # to_genome_array: on the same engine, bit for bit
        ga = arr.to_genome_array()
        assert isinstance(ga, pa.GenomeArray) and ga._engine is eng
        assert list(ga.lengths().items()) == list(zip([str(c) for c in fx[aname + "_ga_names"]], [int(x) for x in fx[aname + "_ga_lengths"]]))
        assert list(ga.strands()) == list(arr.strands()) and ga.sum() == float(fx[aname + "_ga_sum"])
        dense = ga.to_host()
        for c in ga.chroms():
            for si, st in enumerate(ga.strands()):
                assert np.array_equal(dense._chroms[c][st], fx["%s_ga_%s_%d" % (aname, c, si)]), (c, st)
        ga.close()
        # set_sum, reset_sum
        arr.set_sum(1000.0)
        arr.set_normalize(True)
        seg = GenomicSegment("chrA", 100, 140, have[0])
        arr.set_normalize(False)
        plain = arr.get(seg)
        arr.set_normalize(True)
        assert np.array_equal(arr.get(seg), plain / 1000.0 * 1e6)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", DataWarning)
            assert arr.reset_sum() == float(fx[aname + "_sum"]) == arr.sum()
    finally:
        arr.close()


# ---------------------------------------------------------------------------------------------------------------------
# the kernel seams, files of tests/bigwig_writer.py held to read_bigwig

BIG = [("chr1", 250000), ("chr2", 5000)]


def far_match_file():
    """One fixedStep block of 37 928 bytes whose last 5 160 bytes are twenty matches of length 258 at distance 32 768, the
    longest DEFLATE has (zlib's own deflate stops at 32 506): a stored block, then a fixed-Huffman block of the matches."""
    rng = random.Random(3)
    count = 8186 + 6 + 1284
    first = [bc.val(rng) for _ in range(8186)]
    probe, _ = bw.section_bytes(S(0, "fixed", [0.0] * count, span=1, step=2, start=10))
    head = list(struct.unpack("<6f", probe[:24]))                       # items 8186 .. 8191 repeat the header's bytes
    items = first + head + first[:1284]
    sec = S(0, "fixed", items, span=1, step=2, start=10)
    raw, _ = bw.section_bytes(sec)
    assert len(raw) == 32768 + 20 * 258 and raw[32768:] == raw[:20 * 258] and not np.isnan(np.array(head)).any()
    s = Stream().stored(raw[:32768]).fixed([M(258, 32768)] * 20, final=True)
    assert bytes(s.out) == raw
    stream = b"\x78\x9c" + s.cdata() + struct.pack(">I", zlib.adler32(raw))
    return bw.write_bigwig(BIG, [sec], packed={0: stream})


def seam_files():
    rng = random.Random(11)

    def bed(n, at=0, gap=3, chrom=0, ln=2):
        return [(at + k * (ln + gap), at + k * (ln + gap) + ln, bc.val(rng)) for k in range(n)]

    many = [S(0, "bedgraph", bed(3, at=100 * k)) for k in range(300)]
    out = {
        "blocks_1": bw.write_bigwig(BIG, [S(0, "bedgraph", bed(5))]),
        "blocks_65": bw.write_bigwig(BIG, many[:65], fanout=256),
        "blocks_300_fanout_4": bw.write_bigwig(BIG, many, fanout=4),
        "count_1": bw.write_bigwig(BIG, [S(1, "variable", [(7, 2.5)], span=3)]),
        "count_65535": bw.write_bigwig(BIG, [S(0, "fixed", [bc.val(rng) for _ in range(65535)], span=2, step=3, start=5)]),
        "beyond_lds_window": bw.write_bigwig(BIG, [S(0, "bedgraph", bed(300))], level=9),
        "far_match": far_match_file(),
        "levels_0_1_9": bw.write_bigwig(BIG, many[:30] + [S(1, "fixed", [bc.val(rng) for _ in range(700)], span=1, step=1, start=0)], level=[0, 1, 9], items_per_block=200),
        "buf_3x": bw.write_bigwig(BIG, many[:10], buf_factor=3),
        "stored": bw.write_bigwig(BIG, many[:40] + [S(1, "variable", [(a, bc.val(rng)) for a in range(0, 4000, 9)], span=4)], level=None, fanout=4),
        "fill_classes": bw.write_bigwig(BIG, [S(0, "bedgraph", [(10, 11, 1.5), (20, 52, 2.5), (60, 93, 3.5), (100, 2149, 4.5), (3000, 3000 + 4097, 5.5)])]),
        "cluster_of_3": bw.write_bigwig(BIG, [S(0, "bedgraph", [(500, 520, 1.0), (490, 3000, 2.0), (510, 515, 3.0)]), S(1, "bedgraph", [(0, 5000, 7.0)])]),
        "overlap_across_blocks": bw.write_bigwig(BIG, [S(0, "bedgraph", [(0, 100, 1.0), (50, 150, 2.0), (140, 400, 3.0), (399, 2500, 4.0), (2, 3, 5.0)])], items_per_block=1),
        "no_items": bw.write_bigwig(BIG, []),
    }
    return out


@pytest.fixture(scope="module")
def seams(tmp_path_factory):
    d = tmp_path_factory.mktemp("bigwig_seams")
    out = {}
    for n, image in seam_files().items():
        out[n] = str(d / (n + ".bw"))
        open(out[n], "wb").write(image)
    return out


SEAMS = ["blocks_1", "blocks_65", "blocks_300_fanout_4", "count_1", "count_65535", "beyond_lds_window", "far_match", "levels_0_1_9", "buf_3x", "stored",
         "fill_classes", "cluster_of_3", "overlap_across_blocks", "no_items"]


@pytest.mark.parametrize("name", SEAMS)
def test_seams(eng, seams, name):
    t = pa.read_bigwig(seams[name])
    shape = {"blocks_1": 1, "blocks_65": 65, "blocks_300_fanout_4": 300, "count_1": 1, "count_65535": 1, "far_match": 1, "no_items": 0}
    if name in shape:
        assert t.stats["blocks"] == shape[name]
    if name == "count_65535":
        assert len(t) == 65535
    if name == "beyond_lds_window":
        assert t.stats["bytes_inflated"] > 2048
    if name == "far_match":
        assert t.stats["bytes_inflated"] == 37928
    if name == "buf_3x":
        assert t.stats["uncompress_buf_size"] == 3 * 60
    if name == "cluster_of_3":
        assert overlapping(t) == 3 and t.chromosome_counts("chr1")[488:522].tolist() == [0.0] * 2 + [2.0] * 20 + [3.0] * 5 + [2.0] * 7
    if name == "fill_classes":
        assert sorted((t.stop - t.start).tolist()) == [1, 32, 33, 2049, 4097]
    r = pa.BigWigReader(seams[name], engine=eng)
    try:
        same_as_table(r, t)
    finally:
        r.close()


def test_two_files_interleave_on_one_strand(eng, tmp_path):
    rng = random.Random(5)
    a = [S(0, "bedgraph", [(k * 10, k * 10 + 6, bc.val(rng)) for k in range(0, 400, 2)])]
    b = [S(0, "bedgraph", [(k * 10 + 3, k * 10 + 9, bc.val(rng)) for k in range(1, 400, 2)]), S(1, "fixed", [bc.val(rng) for _ in range(50)], span=2, step=2, start=0)]
    pa_, pb = str(tmp_path / "a.bw"), str(tmp_path / "b.bw")
    open(pa_, "wb").write(bw.write_bigwig(BIG, a, items_per_block=7))
    open(pb, "wb").write(bw.write_bigwig(BIG + [("chr3", 10)], b, level=None))
    ta, tb = pa.read_bigwig(pa_), pa.read_bigwig(pb)
    arr = pa.BigWigGenomeArray(engine=eng)
    try:
        arr.add_from_bigwig(pa_, "+")
        arr.add_from_bigwig(pb, "+")
        assert arr.chroms() == {"chr1", "chr2", "chr3"} and arr.lengths() == {"chr1": 250000, "chr2": 5000, "chr3": 10}
        exp = ta.chromosome_counts("chr1")[:4100] + tb.chromosome_counts("chr1")[:4100]
        assert np.array_equal(arr.get(GenomicSegment("chr1", 0, 4100, "+")), exp)
        chain = SegmentChain(GenomicSegment("chr1", 5, 50, "+"), GenomicSegment("chr1", 1000, 1200, "+"))
        assert np.array_equal(chain.get_counts(arr), np.concatenate([exp[5:50], exp[1000:1200]]))
        assert np.array_equal(arr.get(GenomicSegment("chr2", 0, 120, "+")), ta.chromosome_counts("chr2")[:120] + tb.chromosome_counts("chr2")[:120])
    finally:
        arr.close()


# ---------------------------------------------------------------------------------------------------------------------
# refusals: error returns, not faults

def test_refused_files_leave_the_array_as_it_was(eng, tmp_path):
    L = _lib.load()
    ga = pa.GenomeArray({"chrA": 1000}, strands=("+",), engine=eng)
    try:
        good = tmp_path / "good.bw"
        good.write_bytes(bw.write_bigwig(host.CHROMS, host.GOOD))
        _lib.check(L.pc_track_add_bigwig_path(ga._h, os.fsencode(str(good)), 0))
        before_lengths, before = ga.lengths(), ga.to_host()
        assert before_lengths == {"chrA": 1000, "chrB": 500} and before._chroms["chrB"]["+"][100:108].tolist() == [1.0, 1.0, 0.0, 2.0, 2.0, 0.0, 3.0, 3.0]
        path = tmp_path / "refused.bw"
        for name, _, what in host.REFUSED:
            path.write_bytes(host.refused_image(name))
            with pytest.raises(ValueError) as e:
                _lib.check(L.pc_track_add_bigwig_path(ga._h, os.fsencode(str(path)), 0))
            assert str(e.value) == "%s: bigWig: %s" % (path, what), name
            with pytest.raises(ValueError) as e2:
                pa.BigWigReader(str(path), engine=eng)
            assert str(e2.value) == str(e.value)
        # uncompressBufSize one byte too small: the block does not fit its slot
        path.write_bytes(bw.write_bigwig(host.CHROMS, host.GOOD, damage=host.put("<I", 52, 47)))
        with pytest.raises(ValueError) as e:
            _lib.check(L.pc_track_add_bigwig_path(ga._h, os.fsencode(str(path)), 0))
        assert str(e.value) == "%s: bigWig: block 0: DEFLATE error" % path
        after = ga.to_host()
        assert ga.lengths() == before_lengths
        for c in before_lengths:
            assert np.array_equal(after._chroms[c]["+"], before._chroms[c]["+"])
        # and the engine goes on working
        _lib.check(L.pc_track_add_bigwig_path(ga._h, os.fsencode(str(good)), 0))
        assert np.array_equal(ga.to_host()._chroms["chrB"]["+"], before._chroms["chrB"]["+"])     # (assigned again: the same cells)
    finally:
        ga.close()
