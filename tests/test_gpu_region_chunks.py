"""Region reads on the GPU decoder from the index's chunk list (``pc_bam_open_chunks`` / ``pc_add_alignment_bam_chunks``):
only the members the regions' chunks touch are uploaded and inflated, and the columns are those of the host region
reader (itself pinned to htslib's ``sam_itr_queryi``, tests/test_hts_golden.py), record for record."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import plastid_amd as pa  # noqa: E402
from plastid_amd import synth  # noqa: E402
from plastid_amd.bam import read_bam, read_bam_gpu, resolve_regions  # noqa: E402
from plastid_amd.engine import Engine  # noqa: E402
from tests import bam_writer  # noqa: E402
from tests.test_region_chunks import bgzf_members, ends_regions, touched  # noqa: E402

pytestmark = pytest.mark.gpu
FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hts_fixture.npz")
COLS = ("tid", "pos", "alen", "flags", "nblk", "blk_start", "blk_len", "wide_idx", "wide_alen", "wide_nblk", "flag16", "mapq", "qlen", "nh")
HEADER_SLICE = 256 << 10     # compressed bytes from the start of the file the reader first searches for the header


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def same(a, b):
    for k in COLS:
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    assert a.references == b.references and a.lengths == b.lengths and a.mapped == b.mapped and a.n == b.n


def count_all_rules(eng, tx):
    out = []
    for mapping, dtype in ((("fiveprime", 12), np.int64), (("threeprime", 0), np.int64), (("center", 2), np.float64),
                           (("variable", synth.VARIABLE_OFFSETS), np.int64), (("stratified", synth.VARIABLE_OFFSETS, 25, 35), np.int64)):
        f = synth.mapping_factory(mapping)
        f._configure(eng)
        rows = getattr(f, "_numlengths", 1)
        p = tx.plan_arrays(rows=rows)
        plan = eng.plan(p["tid"], p["start"], p["end"], p["strand"], p["out_off"], p["out_step"], p["row_stride"], p["out_elems"], rows)
        out.append(plan.count(dtype).copy().view(np.uint64))
        plan.close()
    return out


def indexed_bam(path, reads, block_bytes, header_lines=0):
    recs = bam_writer.packed_to_records(reads)
    text = "@HD\tVN:1.6\tSO:coordinate\n" + "".join("@CO\tpadding line %06d %s\n" % (k, "x" * 60) for k in range(header_lines))
    bam_writer.write_bam(path, list(reads.references), [int(x) for x in reads.lengths], recs, block_bytes=block_bytes, header_text=text, index=True)


def test_chunk_reads_match_hts_itr_query(eng, tmp_path):
    """(a) each of the fixture's 400 regions, and the 40-region set: the host region reader's arrays and htslib's own
    result sets (FLAG, MAPQ, l_seq, file order)."""
    hts = np.load(FIX)
    path = str(tmp_path / "htslib.bam")
    open(path, "wb").write(hts["bam"].tobytes())
    open(path + ".bai", "wb").write(hts["bai"].tobytes())
    refs = [str(x) for x in hts["references"]]
    nonempty = 0
    for q in range(len(hts["regions"])):
        t, b, e = (int(x) for x in hts["regions"][q])
        reg = [(refs[t], b, e)]
        got = read_bam_gpu(path, eng, regions=reg)
        same(got, read_bam(path, regions=reg))
        want = hts["region_records"][hts["region_off"][q]:hts["region_off"][q + 1]]
        assert got.n == len(want), (q, reg)
        nonempty += got.n > 0
        assert np.array_equal(got.flag16, hts["flag"][want]) and np.array_equal(got.mapq, hts["mapq"][want]) and np.array_equal(got.qlen, hts["l_qseq"][want])
    assert nonempty > 300
    many = [(refs[int(t)], int(b), int(e)) for t, b, e in hts["regions"][:40]]
    timing = {}
    same(read_bam_gpu(path, eng, regions=many, timing=timing), read_bam(path, regions=many))
    assert timing["runs"] >= 1 and 0 < timing["uploaded_bytes"] <= os.path.getsize(path)


@pytest.mark.parametrize("block_bytes,header_lines", [(3000, 0), (20000, 0), (2500, 9000)])
def test_chunk_reads_over_many_members(eng, tmp_path, monkeypatch, block_bytes, header_lines):
    """(b) twelve random multi-region sets -- chunks that share members, touch, or lie far apart; records that straddle
    members -- give the host region reader's arrays; so does a header of a dozen members longer than the first slice
    searched for it."""
    genome, tx, reads, _ = synth.make_config("C4", scale=0.00006, tx_scale=0.002)
    path = str(tmp_path / "idx.bam")
    rng = np.random.default_rng(block_bytes + header_lines)
    if header_lines:
        monkeypatch.setenv("PC_BAM_HEADER_BYTES", "600")
    indexed_bam(path, reads, block_bytes, header_lines)
    refs, lens = list(reads.references), [int(x) for x in reads.lengths]
    multi_run = 0
    for trial in range(12):
        regs = []
        for _ in range(int(rng.integers(2, 12))):
            t = int(rng.integers(0, len(refs)))
            b = int(rng.integers(0, max(lens[t] - 10, 1)))
            regs.append((refs[t], b, b + int(rng.choice([1, 50, 3000, 200000, lens[t]]))))
        timing = {}
        got, want = read_bam_gpu(path, eng, regions=regs, timing=timing), read_bam(path, regions=regs)
        same(got, want)
        multi_run += timing["runs"] > 2
    assert multi_run > 0


def test_far_apart_regions_upload_only_their_members(eng, tmp_path):
    """(c) one region on the first contig and one on the last of a file of thousands of members: what goes to HBM is the
    header's slice plus the members the chunks touch (at most twice their bytes), not the file between them."""
    genome, tx, reads, _ = synth.make_config("C2", scale=0.004, tx_scale=0.002)
    path = str(tmp_path / "far.bam")
    indexed_bam(path, reads, 3000)
    offs, lens = bgzf_members(path)
    assert len(offs) >= 2000
    regs = ends_regions(reads)
    sp = resolve_regions(path, regs)
    hit = touched(offs, sp["chunks"])
    head = np.nonzero(offs < min(HEADER_SLICE, int(sp["chunks"][0, 0]) >> 16))[0]
    timing = {}
    got = read_bam_gpu(path, eng, regions=regs, timing=timing)
    same(got, read_bam(path, regions=regs))
    assert got.n > 0
    assert timing["uploaded_bytes"] <= lens[head].sum() + 2 * lens[hit].sum(), (timing, lens[head].sum(), lens[hit].sum())
    assert timing["members"] <= len(head) + 2 * len(hit), (timing["members"], len(head), len(hit))
    assert timing["uploaded_bytes"] < os.path.getsize(path) / 5


def test_chunk_reads_count_like_host_staged_ones(tmp_path):
    """(d) staged without leaving the device (``Engine.add_bam(path, regions)``, ``BAMGenomeArray(path, keep_reads=False,
    regions=...)``): counts under all five rules equal those of the host-staged region read, the center rule bit for bit."""
    genome, tx, reads, _ = synth.make_config("C4", scale=0.00006, tx_scale=0.002)
    path = str(tmp_path / "cnt.bam")
    indexed_bam(path, reads, 3000)
    chains = tx.chains(limit=60)
    regs = [(c.chrom, c.spanning_segment.start, c.spanning_segment.end) for c in chains[:25]]
    host = read_bam(path, regions=regs)
    a, b = Engine(0), Engine(0)
    a.set_alignments([host])
    kept = b.add_bam(path, regions=regs)
    assert kept == int(((host.flag16 & 4) == 0).sum()) and b.num_records(0) == host.n
    sub = tx.subset(np.arange(25))
    for x, y in zip(count_all_rules(a, sub), count_all_rules(b, sub)):
        assert np.array_equal(x, y)
    a.close()
    b.close()
    ha = pa.BAMGenomeArray(path, regions=regs, mapping=pa.FivePrimeMapFactory(12))
    da = pa.BAMGenomeArray(path, keep_reads=False, regions=regs, mapping=pa.FivePrimeMapFactory(12))
    for factory in (pa.FivePrimeMapFactory(12), pa.CenterMapFactory(0)):
        for ga in (ha, da):
            ga.set_mapping(factory)
        for x, y in zip(ha.get_counts_batch(chains[:25]), da.get_counts_batch(chains[:25])):
            assert np.array_equal(np.asarray(x).view(np.uint64), np.asarray(y).view(np.uint64))


def test_foreign_index_and_empty_region_sets(eng, tmp_path):
    """(e) an index that does not belong to the file is a ValueError; a region set that matches nothing reads the header
    alone (every reference, no record, the index's mapped count)."""
    genome, tx, reads, _ = synth.make_config("C2", scale=0.00005, tx_scale=0.002)
    path, other = str(tmp_path / "a.bam"), str(tmp_path / "b.bam")
    indexed_bam(path, reads, 3000)
    indexed_bam(other, reads.slice(57, reads.n // 2), 7000)
    for regs in ([], [("nope", 0, 100)]):
        none = read_bam_gpu(path, eng, regions=regs)
        assert none.n == 0 and list(none.references) == list(reads.references)
        assert none.mapped == resolve_regions(path, [])["mapped"]
        e = Engine(0)
        assert e.add_bam(path, regions=regs) == 0 and e.num_records(0) == 0
        e.close()
    os.replace(path + ".bai", other + ".bai")
    outcomes = []
    for t in range(len(reads.references)):
        on = reads.pos[reads.tid == t]
        if not len(on):
            continue
        for b in (int(np.quantile(on, f)) for f in (0.1, 0.5, 0.9)):
            try:
                got = read_bam_gpu(other, eng, regions=[(reads.references[t], b, b + 50000)])
                outcomes.append("ok")
                assert got.n >= 0
            except ValueError as e:
                outcomes.append("error")
                assert any(k in str(e) for k in ("index", "BGZF", "BAM", "sorted")), str(e)
    assert outcomes.count("error") >= len(outcomes) // 2, outcomes


def open_span(eng, path, voff_begin, voff_end, sp):
    """The columns, references and lengths of one ``pc_bam_open_span`` read (straight through ctypes: no Python caller is left)."""
    from plastid_amd import _lib as clib
    L = clib.load()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    h = ctypes.c_void_p()
    clib.check(L.pc_bam_open_span(eng._h, os.fsencode(path), int(voff_begin), int(voff_end), len(sp["tid"]), p(sp["tid"]), p(sp["beg"]), p(sp["end"]),
                                  ctypes.byref(h)))
    try:
        counts = np.zeros(8, np.int64)
        clib.check(L.pc_bam_counts(h, p(counts)))
        n, nrun, nw = int(counts[0]), int(counts[1]), int(counts[4])
        refs = [L.pc_bam_ref_name(h, i).decode() for i in range(L.pc_bam_nref(h))]
        lens = [int(L.pc_bam_ref_length(h, i)) for i in range(len(refs))]
        c = dict(tid=np.empty(n, np.int32), pos=np.empty(n, np.int32), alen=np.empty(n, np.uint16), flags=np.empty(n, np.uint8),
                 nblk=np.empty(n, np.uint8), blk_start=np.empty(nrun, np.int32), blk_len=np.empty(nrun, np.int32),
                 wide_idx=np.empty(nw, np.int64), wide_alen=np.empty(nw, np.int32), wide_nblk=np.empty(nw, np.int32),
                 flag16=np.empty(n, np.uint16), mapq=np.empty(n, np.uint8), qlen=np.empty(n, np.int32), nh=np.empty(n, np.uint16))
        clib.check(L.pc_bam_read(h, *(p(c[k]) for k in COLS[:10])))
        clib.check(L.pc_bam_read_sam(h, p(c["flag16"]), p(c["mapq"]), p(c["qlen"])))
        clib.check(L.pc_bam_read_nh(h, p(c["nh"])))
    finally:
        L.pc_bam_close(h)
    return c, refs, lens


def test_span_reads_are_one_chunk_reads(eng, tmp_path):
    """(g) ``pc_bam_open_span`` over the span that encloses the regions' chunks: the host region reader's columns, for the
    htslib fixture's 40-region set and for a multi-region set on a file of many members; the span 0, 0 reads the header
    alone (every reference, no record)."""
    hts = np.load(FIX)
    fix = str(tmp_path / "htslib.bam")
    open(fix, "wb").write(hts["bam"].tobytes())
    open(fix + ".bai", "wb").write(hts["bai"].tobytes())
    refs = [str(x) for x in hts["references"]]
    many = [(refs[int(t)], int(b), int(e)) for t, b, e in hts["regions"][:40]]
    genome, tx, reads, _ = synth.make_config("C4", scale=0.00006, tx_scale=0.002)
    syn = str(tmp_path / "span.bam")
    indexed_bam(syn, reads, 3000)
    assert len(bgzf_members(syn)[0]) > 20
    chains = tx.chains(limit=60)
    some = [(c.chrom, c.spanning_segment.start, c.spanning_segment.end) for c in chains[5:45:4]]
    for path, regs in ((fix, many), (syn, some)):
        sp = resolve_regions(path, regs)
        want = read_bam(path, regions=regs)
        assert want.n > 0 and len(sp["tid"]) > 1 and sp["voff_end"] > sp["voff_begin"]
        got, grefs, glens = open_span(eng, path, sp["voff_begin"], sp["voff_end"], sp)
        for k in COLS:
            assert np.array_equal(got[k], getattr(want, k)), (path, k)
        assert grefs == list(want.references) and glens == [int(x) for x in want.lengths]
        none, nrefs, nlens = open_span(eng, path, 0, 0, sp)
        assert all(len(none[k]) == 0 for k in COLS)
        assert nrefs == list(want.references) and nlens == [int(x) for x in want.lengths]


def test_two_identical_calls_give_identical_arrays(eng, tmp_path):
    """(f) the same region read twice: the same arrays."""
    genome, tx, reads, _ = synth.make_config("C4", scale=0.00006, tx_scale=0.002)
    path = str(tmp_path / "rep.bam")
    indexed_bam(path, reads, 3000)
    chains = tx.chains(limit=60)
    regs = [(c.chrom, c.spanning_segment.start, c.spanning_segment.end) for c in chains[:40]]
    same(read_bam_gpu(path, eng, regions=regs), read_bam_gpu(path, eng, regions=regs))


UPLOAD_SETTINGS = {"default": {}, "pieces": {"PC_BAM_PIECE": "7000"}, "pieces.no_ring": {"PC_BAM_PIECE": "7000", "PC_BAM_NO_RING": "1"},
                   "pieces.one_stream": {"PC_BAM_PIECE": "7000", "PC_BAM_STREAMS": "1"}, "pieces.four_streams": {"PC_BAM_PIECE": "7000", "PC_BAM_STREAMS": "4"}}


def test_every_upload_path_of_a_region_read(eng, tmp_path, monkeypatch):
    """(h) a region read whose image is cut into pieces of a few members: the page-locked ring with pieces that lie in one
    run and pieces gathered from several short runs, the same pieces straight from the mapping (PC_BAM_NO_RING), and the
    inflate launches on one, two and four streams -- every setting gives the columns and counts of the default one (one
    gathered piece) and of the host region reader."""
    rng = np.random.default_rng(7000)
    n = 4000
    tid = np.sort(rng.integers(0, 2, n)).astype(np.int32)
    pos = rng.integers(0, 190000, n).astype(np.int32)
    cigars = [("%dM" % L) if k % 7 else ("%dM%dN12M" % (L, 40 + k % 300)) for k, L in enumerate(rng.integers(20, 60, n))]
    reads = pa.PackedAlignments.from_cigars(tid, pos, cigars, rng.integers(0, 2, n).astype(bool), references=["a", "b"], lengths=[200000, 200000],
                                            sort=True)
    path = str(tmp_path / "pieces.bam")
    indexed_bam(path, reads, 3000)
    regs = [("a", 60000, 62000), ("a", 150000, 152000), ("b", 100000, 102000)]
    want = read_bam(path, regions=regs)
    assert want.n > 20
    first = None
    for name, env in UPLOAD_SETTINGS.items():
        for k in ("PC_BAM_PIECE", "PC_BAM_NO_RING", "PC_BAM_STREAMS"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        timing = {}
        got = read_bam_gpu(path, eng, regions=regs, timing=timing)
        same(got, want)
        assert timing["runs"] >= 3 and timing["uploaded_bytes"] >= 2 * 7000, (name, timing)
        counts = {k: timing[k] for k in ("runs", "uploaded_bytes", "members", "inflated_bytes")}
        if first is None:
            first = (got, counts)
        same(got, first[0])
        assert counts == first[1], (name, counts, first[1])
