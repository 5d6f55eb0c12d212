"""Coordinate sort at decode on the GPU (``PC_BAM_SORT``: csrc/sort_kernels.hip.h, one stable radix sort in
``decode_columns``): ``read_bam_gpu(path, sort=True)``, ``Engine.add_bam(path, sort=True)`` and
``BAMGenomeArray(path, sort=True)`` on files in shuffled record order against the TWIN of tests/bam_sort_cases.py -- the
same records written in the contract's order and read by the code path without ``sort`` -- and against the oracle on the
twin.  Needs a real MI355X: ``pytest -m gpu``.

Shapes: record counts at workgroup (256) and k_bam_scan_inputs (2 048) borders; 200 000 records for a radix sort of many
blocks; 1, 3 and 70 000 references (33, 35 and 50 key bits), one record at POS 2^31 - 2; a tie of 6 000 records that
spans many workgroups; wide reads; members of 700 bytes, so that records cross member borders."""
import ctypes
import gzip
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import plastid_amd as pa  # noqa: E402
from plastid_amd import synth  # noqa: E402
from plastid_amd.bam import read_bam, read_bam_gpu  # noqa: E402
from plastid_amd.engine import Engine  # noqa: E402
from tests import bam_sort_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu

REFS3, LENS3 = ["chrA", "chrB", "chrC"], [5000000, 3000000, 100000]
SIZE = (22, 36)


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as o
    o.lib()
    return o


def case_records(name):
    """(references, lengths, records in file order, block bytes, key bits the sort has to look at)"""
    if name == "wide":
        return REFS3, LENS3, cases.wide_records(), 20000, 35
    if name == "pile":
        return REFS3, LENS3, cases.tie_pile(6000), 60000, 35
    if name == "big":      # many radix-sort blocks; one reference: 33 key bits
        return ["chr1"], [250000000], cases.random_records(200000, 1, seed=11, span=5000000, rich=False), 60000, 33
    if name == "ref1":
        return ["chr1"], [250000000], cases.random_records(3000, 1, seed=12), 700, 33
    if name == "ref70000":   # 17 bits of reference id: 50 key bits; the last reference holds a record at POS 2^31 - 2
        n_ref = 70000
        recs = cases.random_records(90000, n_ref, seed=13, span=40, rich=False)
        recs.insert(100, (n_ref - 1, 2**31 - 2, [(0, 1)], 16, cases.nh_aux(1), 17))
        recs.insert(50000, (n_ref - 1, 2**31 - 2, [], 4, b"", 3))
        return ["c%d" % i for i in range(n_ref)], [1000] * (n_ref - 1) + [2**31 - 1], recs, 60000, 50
    return REFS3, LENS3, cases.random_records(int(name), 3, seed=int(name) + 7), 700, 35


_written = {}


@pytest.fixture(scope="module")
def written(tmp_path_factory):
    """Each case is written (and its records kept) once per module."""
    def get(name):
        if name not in _written:
            refs, lens, recs, block, bits = case_records(name)
            tmp = tmp_path_factory.mktemp("sort_" + name)
            path, twin = cases.write_pair(tmp, name, refs, lens, recs, block_bytes=block)
            _written[name] = (path, twin, recs, bits)
        return _written[name]
    yield get
    _written.clear()


@pytest.mark.parametrize("name", ["0", "1", "2", "255", "256", "257", "2047", "2049", "4097", "ref1", "wide", "pile", "big", "ref70000"])
def test_shuffled_file_equals_its_twin(eng, written, name):
    """Column for column the twin read without ``sort``, and the host decoder's ``sort=True``, ``file_order`` included."""
    path, twin, recs, bits = written(name)
    timing = {}
    got = read_bam_gpu(path, eng, sort=True, timing=timing)
    cases.same_columns(got, read_bam_gpu(twin, eng), name)
    host = read_bam(path, sort=True)
    cases.same_columns(got, host, name)
    cases.same_file_order(got, recs, name)
    cases.same_file_order(host, recs, name)
    order, moved = cases.model_order(recs)
    disorder = not cases.in_order(recs)
    assert timing["records_moved"] == moved and timing["sorted_input"] == (not disorder) and timing["sort_ms"] >= 0.0
    assert timing["sort_key_bits"] == (bits if disorder else 0)
    if len(getattr(got, "wide_idx", ())):
        assert np.all(np.diff(got.wide_idx) > 0)
    if disorder:
        for reader in (lambda: read_bam_gpu(path, eng), lambda: read_bam(path)):
            with pytest.raises(ValueError) as e:
                reader()
            assert str(e.value) == "%s: %s" % (cases.UNSORTED, path)
    if name == "pile":
        at = got.pos == 3000
        fo, rev = got.file_order[at], got.flags[at] & 1
        assert at.sum() == 6000 and 0 < rev.sum() < 6000
        assert np.all(np.diff(rev) >= 0) and np.all(np.diff(fo[rev == 0]) > 0) and np.all(np.diff(fo[rev == 1]) > 0)
    if name == "ref70000":
        assert got.tid[-1] == 69999 and got.pos[-1] == 2**31 - 2 and got.n == len(order)


def names_of(name):
    return ["chr1"] if name in ("big", "ref1") else REFS3


def segments_of(recs, ntid=3):
    """Every reference from 0 to behind its last read on each strand selection (at most 60 000 positions: the 200 000
    records of "big" lie over 5 x 10^6)."""
    top = min(int(max([r[1] for r in recs if r[1] < 2**30] + [0])) + 4000, 60000)
    return [(t, 0, top, st) for t in range(ntid) for st in (1, 2, 3)]


def engine_counts(e, rule, segs):
    seg_tid = np.array([s[0] for s in segs], np.int32)
    seg_start = np.array([s[1] for s in segs], np.int64)
    seg_end = np.array([s[2] for s in segs], np.int64)
    seg_strand = np.array([s[3] for s in segs], np.uint8)
    synth.mapping_factory(rule)._configure(e)
    e.set_size_filter(*SIZE)
    e.set_nh_filter(1)
    rows = e.rows
    lens = seg_end - seg_start
    out_off = np.concatenate([[0], np.cumsum(lens * rows)[:-1]])
    plan = e.plan(seg_tid, seg_start, seg_end, seg_strand, out_off, np.ones(len(lens), np.int8), lens, int((lens * rows).sum()), rows)
    got = plan.count(np.float64 if rule[0] == "center" else np.int64).copy()
    plan.close()
    return got


def bits(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint64)


PA_RULES = [lambda: pa.FivePrimeMapFactory(12), lambda: pa.ThreePrimeMapFactory(0), lambda: pa.VariableFivePrimeMapFactory(cases.RULES[2][1]),
            lambda: pa.StratifiedVariableFivePrimeMapFactory(cases.RULES[3][1], 25, 35), lambda: pa.CenterMapFactory(0)]


@pytest.mark.parametrize("name", ["257", "2049", "4097", "ref1", "wide", "pile", "big"])
def test_counts_equal_the_oracle_on_the_twin(oracle, written, name):
    """``Engine.add_bam(sort=True)`` and ``BAMGenomeArray(sort=True, keep_reads=False)`` under all five rules, with a size
    filter and the unique-mapper filter: element for element the oracle's counts over the twin's reads that pass (the
    center rule bit for bit: its float64 sums follow the record order, ties included)."""
    path, twin, recs, _ = written(name)
    ref = read_bam(twin)
    kept = ref.subset(np.nonzero(ref.nh == 1)[0])
    names = names_of(name)
    segs = segments_of(recs, len(names))
    e = Engine(0)
    assert e.add_bam(path, sort=True) == ref.mapped
    ga = pa.BAMGenomeArray(path, sort=True, keep_reads=False)
    ga.add_filter("size", pa.SizeFilterFactory(*SIZE))
    ga.add_filter("nh", pa.FlagFilterFactory(max_nh=1))
    total = 0.0
    for rule, factory in zip(cases.RULES, PA_RULES):
        want = cases.oracle_counts(oracle, [kept], rule, segs, size_filter=SIZE)
        exp = np.concatenate([np.asarray(a).reshape(-1) for a in want])
        total += float(exp.sum())
        assert np.array_equal(bits(engine_counts(e, rule, segs)), bits(exp)), (name, rule[0])
        ga.set_mapping(factory())
        for (t, s, en, st), w in zip(segs, want):
            g = ga.get(pa.GenomicSegment(names[t], s, en, "+-."[st - 1]), roi_order=False)
            assert np.array_equal(bits(np.asarray(g, np.float64)), bits(np.asarray(w, np.float64))), (name, rule[0], t, st)
    assert total > 0
    e.close()


@pytest.mark.parametrize("name,chrom,start,end,least", [("4097", "chrB", 100, 900, 50), ("257", "chrA", 0, 200, 10), ("ref1", "chr1", 100, 900, 50),
                                                        ("big", "chr1", 1000000, 1100000, 500), ("pile", "chrA", 2900, 3100, 1000)])
def test_get_reads_returns_the_twins_reads_in_the_twins_order(written, name, chrom, start, end, least):
    path, twin, recs, _ = written(name)
    a, b = pa.BAMGenomeArray(path, sort=True, decode="gpu"), pa.BAMGenomeArray(twin, decode="gpu")
    seg = pa.GenomicSegment(chrom, start, end, "+")
    ra, rb = a.get_reads(seg), b.get_reads(seg)
    key = lambda r: (r.reference_id, r.reference_start, r.is_reverse, r.flag, r.mapping_quality, tuple(r._runs))  # noqa: E731
    assert len(rb) > least and [key(r) for r in ra] == [key(r) for r in rb]
    assert len(set(r.mapping_quality for r in rb)) > 5   # (a MAPQ column permuted out of step would show)


def test_sorted_input_is_not_touched(eng, written, tmp_path):
    """The twin itself, and a file sorted by (tid, POS) with reverse before forward in its ties, with ``sort=True``: the
    arrays of ``sort=False``; pc_bam_sort_stats reports in-order and nothing moved, and there is no file order to read."""
    from plastid_amd import _lib as clib
    ties = str(tmp_path / "ties.bam")
    cases.bam_writer.write_bam(ties, REFS3, LENS3, [(0, 10, [(0, 30)], 16), (0, 10, [(0, 31)], 0), (0, 10, [(0, 32)], 16), (0, 11, [(0, 25)], 16),
                                                  (0, 11, [(0, 26)], 0), (1, 5, [(0, 27)], 16), (1, 5, [(0, 28), (3, 10), (0, 5)], 0), (-1, -1, [], 4)])
    L = clib.load()
    for path in (written("4097")[1], written("pile")[1], ties):
        timing = {}
        got = read_bam_gpu(path, eng, sort=True, timing=timing)
        cases.same_columns(got, read_bam_gpu(path, eng))
        assert got.file_order is None and timing["sorted_input"] is True and timing["records_moved"] == 0
        h = ctypes.c_void_p()
        clib.check(L.pc_bam_open_path_flags(eng._h, os.fsencode(path), clib.PC_BAM_SORT, ctypes.byref(h)))
        try:
            st, ms = np.zeros(4, np.int64), ctypes.c_double(-1.0)
            clib.check(L.pc_bam_sort_stats(h, st.ctypes.data_as(ctypes.c_void_p), ctypes.byref(ms)))
            assert st.tolist() == [1, 1, 0, 0] and ms.value >= 0.0
            rec_no = np.zeros(max(got.n, 1), np.int64)
            assert L.pc_bam_read_file_order(h, rec_no.ctypes.data_as(ctypes.c_void_p)) != 0
        finally:
            L.pc_bam_close(h)
        h = ctypes.c_void_p()
        clib.check(L.pc_bam_open_path(eng._h, os.fsencode(path), ctypes.byref(h)))
        try:
            st = np.ones(4, np.int64)
            clib.check(L.pc_bam_sort_stats(h, st.ctypes.data_as(ctypes.c_void_p), None))
            assert st.tolist() == [0, 1, 0, 0]
        finally:
            L.pc_bam_close(h)
    with pytest.raises(ValueError):   # a flag the library does not know
        clib.check(L.pc_bam_open_path_flags(eng._h, os.fsencode(ties), 2, ctypes.byref(h)))


def test_sort_with_regions_raises(eng, tmp_path):
    path = str(tmp_path / "absent.bam")   # refused before any file is opened
    for call in (lambda: read_bam_gpu(path, eng, regions=[("chrA", 0, 10)], sort=True), lambda: eng.add_bam(path, regions=[("chrA", 0, 10)], sort=True),
                 lambda: pa.BAMGenomeArray(path, regions=[("chrA", 0, 10)], sort=True), lambda: pa.BAMGenomeArray(path, regions=[("chrA", 0, 10)], sort=True, keep_reads=False)):
        with pytest.raises(ValueError) as e:
            call()
        assert "sort" in str(e.value) and "regions" in str(e.value)


def test_defects_are_ordinary_errors(eng, tmp_path):
    """With ``sort``: a deletion-first read that the sorted order puts out of first-aligned-position order, a corrupt
    CIGAR and a file cut in half are refused with the messages of an open without it; both decoders agree."""
    def both(path):
        msgs = []
        for reader in (lambda: read_bam_gpu(path, eng, sort=True), lambda: read_bam(path, sort=True)):
            with pytest.raises(ValueError) as e:
                reader()
            msgs.append(str(e.value))
        assert msgs[0] == msgs[1]
        return msgs[0]
    filler = cases.random_records(600, 3, seed=21, rich=False)
    path = str(tmp_path / "del.bam")
    cases.write_fast(path, REFS3, LENS3, filler[:300] + [(2, 90100, [(2, 50), (0, 20)], 0), (2, 90120, [(0, 30)], 0)] + filler[300:], block_bytes=900)
    assert "starting with a deletion" in both(path)
    raw = bytearray(cases.bam_writer.encode_record(1, 77, [(0, 30)], 0))
    raw[16:18] = b"\xff\xff"                       # n_cigar_op: the CIGAR overruns the record
    path = str(tmp_path / "cigar.bam")
    cases.write_fast(path, REFS3, LENS3, filler[:400] + [bytes(raw)] + filler[400:], block_bytes=900)
    assert both(path) == "corrupt BAM record (cigar overruns block)"
    whole = str(tmp_path / "whole.bam")
    cases.write_fast(whole, REFS3, LENS3, filler, block_bytes=100000)
    data = gzip.decompress(open(whole, "rb").read())
    cut = str(tmp_path / "cut.bam")
    with open(cut, "wb") as fh:
        fh.write(cases.bam_writer.bgzf_block(data[:len(data) // 2]) + cases.bam_writer.BGZF_EOF)
    assert both(cut) == "truncated BAM record"
    with pytest.raises(ValueError) as e:           # without sort it stops at the disorder first (or at the same truncation)
        read_bam_gpu(cut, eng)
    assert str(e.value) in ("truncated BAM record", "%s: %s" % (cases.UNSORTED, cut))


def test_a_shuffled_and_a_sorted_file_in_one_array(oracle, written):
    """Two files named by path, one out of order: the counts are the oracle's over the two twins, file-major (the center
    rule adds the files' reads in file order)."""
    path, twin, recs, _ = written("4097")
    other = written("2049")[1]                      # in order already
    files = [read_bam(twin), read_bam(other)]
    segs = segments_of(recs)
    for keep in (False, True):
        ga = pa.BAMGenomeArray(path, other, sort=True, keep_reads=keep, decode="gpu")
        for rule, factory in ((cases.RULES[0], PA_RULES[0]), (cases.RULES[4], PA_RULES[4])):
            ga.set_mapping(factory())
            want = cases.oracle_counts(oracle, files, rule, segs)
            assert sum(float(np.asarray(w).sum()) for w in want) > 0
            for (t, s, en, st), w in zip(segs, want):
                g = ga.get(pa.GenomicSegment(REFS3[t], s, en, "+-."[st - 1]), roi_order=False)
                assert np.array_equal(bits(np.asarray(g, np.float64)), bits(np.asarray(w, np.float64))), (keep, rule[0], t, st)
