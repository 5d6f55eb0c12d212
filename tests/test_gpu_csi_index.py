"""The CSI index built on the GPU (``build_index(fmt="csi")`` / ``pc_bam_index_build_csi``) against the CSI htslib wrote
(tests/golden/csi_fixture.npz) and the record-by-record model (tests/csi_model.py); region reads and counts beyond 2^29
through the built index."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import plastid_amd as pa  # noqa: E402
from plastid_amd import bam as pbam  # noqa: E402
from plastid_amd.bam import BamIndex, build_index, read_bam, read_bam_gpu  # noqa: E402
from plastid_amd.engine import Engine  # noqa: E402
from plastid_amd.roitools import GenomicSegment, SegmentChain  # noqa: E402
from tests import bam_writer  # noqa: E402
from tests import csi_cases as cc  # noqa: E402
from tests import csi_model as cm  # noqa: E402

pytestmark = pytest.mark.gpu

P29, P30, TOP = 1 << 29, 1 << 30, (1 << 31) - 1


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def built_equals_model(path, eng, min_shift, walked=None):
    """Build the CSI of `path` beside it; the file written, the returned object and the model agree.  Returns
    ``(walk, pre-finish arrays of the model, parsed index)``."""
    w = walked or cm.walk(open(path, "rb").read())
    pre = cm.prefinish(w, min_shift)
    refs, nn = cm.finish(pre)
    timing = {}
    idx = build_index(path, engine=eng, overwrite=True, timing=timing, fmt="csi", min_shift=min_shift)
    data = open(path + ".csi", "rb").read()
    assert data[:4] == b"\x1f\x8b\x08\x04" and data[-28:] == pbam._BGZF_EOF
    payload = pbam._bgzf_unwrap(data)
    got = cm.parse_csi(payload)
    assert got == (min_shift, pre["n_lvls"], refs, nn)
    assert idx == BamIndex.from_file(path + ".csi") and (idx.fmt, idx.min_shift, idx.depth, idx.n_no_coor) == ("csi", min_shift, pre["n_lvls"], nn)
    for ids in cm.bin_order(payload):
        assert ids == sorted(ids) and (not ids or ids[-1] == cm.meta_bin(pre["n_lvls"]))
    assert timing["records"] == len(w["recs"]) and timing["n_no_coor"] == nn and timing["index_bytes"] == len(data)
    assert timing["mapped"] == sum(1 for r in w["recs"] if r[1] >= 0 and r[4]) and timing["total_ms"] > 0
    assert (timing["min_shift"], timing["depth"]) == (min_shift, pre["n_lvls"]) and timing["linear"] == sum(pre["n_intv"])
    assert timing["runs"] == len(pre["run_tid"])
    return w, pre, got


@pytest.mark.parametrize("case,min_shift", cc.case_shapes())
def test_the_index_of_every_fixture_case(eng, tmp_path, case, min_shift):
    d = cc.case_data(case, min_shift)
    path = cc.write_case(tmp_path, case)
    _, pre, got = built_equals_model(path, eng, min_shift, cc.case_walk(case))
    want = cm.parse_csi(d["csi"])
    assert got == want and pre["n_lvls"] == want[1]
    idx = BamIndex.from_file(path + ".csi")
    assert idx == BamIndex.from_bytes(d["csi"]) and idx.mapped == int(d["stat"][:, 1].sum())
    assert not [f for f in os.listdir(str(tmp_path)) if "tmp" in f]


@pytest.mark.parametrize("n", [1, 255, 256, 257, 513])
def test_run_heads_on_workgroup_borders(eng, tmp_path, n):
    """The bin changes at records 255 and 256 (leaves of 1 kb): run heads in the last thread of one workgroup and the
    first of the next; the loff of the runs on both sides is the offset of the run's own first record."""
    recs = [(0, 10 + (k if k < 255 else 20000 if k == 255 else 40000 + k), [(0, 25)], 0) for k in range(n)]
    path = str(tmp_path / "wg.bam")
    bam_writer.write_bam(path, ["c1"], [100_000], recs, block_bytes=5000)
    w, pre, (_, depth, refs, _) = built_equals_model(path, eng, 10)
    assert depth == 3 and len(pre["run_tid"]) == (1 if n <= 255 else 2 if n == 256 else 3)
    bins, loff = refs[0]
    leaf = cm.level_first(3)
    heads = [0] + ([255] if n > 255 else []) + ([256] if n > 256 else [])
    for k in heads:
        b = leaf + (recs[k][1] >> 10)
        assert loff[b] == w["recs"][k][0] == bins[b][0][0], k


DEGENERATE = {
    "header-only": [],
    "unplaced-only": [(-1, -1, [], 4)] * 7,
    "one-read": [(1, 9000, [(0, 2)], 0)],
    "no-reference-base": [(0, 0, [(4, 20)], 0), (0, 9000, [(1, 5)], 16)],
    "reference-without-records": [(1, 100, [(0, 30)], 0), (1, 4000, [(0, 30)], 16)],
    "placed-unmapped-only": [(0, 50, [(0, 30)], 0), (1, 10, [], 4), (1, 9000, [], 4), (-1, -1, [], 4)],
}


@pytest.mark.parametrize("depth,length", [(0, 16_000), (1, 40_000)])
@pytest.mark.parametrize("name", sorted(DEGENERATE))
def test_degenerate_files(eng, tmp_path, name, depth, length):
    recs = DEGENERATE[name]
    path = str(tmp_path / "d.bam")
    bam_writer.write_bam(path, ["c1", "c2"], [length, length], recs)
    w, pre, (_, got_depth, refs, nn) = built_equals_model(path, eng, 14)
    assert got_depth == depth and nn == sum(1 for r in recs if r[0] < 0)
    idx = BamIndex.from_file(path + ".csi")
    assert idx.n_ref == 2
    # (bins as pushed, before small ones move into an existing parent)
    assert {(int(t), int(b)) for t, b in zip(pre["run_tid"], pre["run_bin"])} == {(r[1], cm.reg2bin(r[2], r[3], 14, depth)) for r in w["recs"] if r[1] >= 0}
    assert [len(b) for b in idx.bins] == [len([b for b in refs[t][0] if b != cm.meta_bin(depth)]) for t in range(2)]
    if name == "placed-unmapped-only":
        assert pre["n_intv"][1] == 0 and idx.loff[1] and all(v == 0 for v in idx.loff[1].values()) and idx.meta[1][2:] == (0, 2)
        assert all(v == w["recs"][0][0] for v in idx.loff[0].values())
    if name == "reference-without-records":
        assert idx.bins[0] == {} and idx.meta[0] is None


def test_member_boundaries(eng, tmp_path):
    refs, lens = ["c1", "c2"], [3_000_000, 50_000]
    recs = [(0, 500 * k, [(0, 30)], 0) for k in range(400)] + [(1, 7 * k, [(0, 20), (3, 40), (0, 20)], 16) for k in range(100)] + [(-1, -1, [], 4)] * 3
    path = str(tmp_path / "b.bam")
    bam_writer.write_bam(path, refs, lens, recs, block_bytes=60000)
    w0 = cm.walk(open(path, "rb").read())
    # a record starts exactly where a member begins: its offset is that member's with 0 inside, and a loff carries it
    at = w0["starts"][137]
    bam_writer.write_bam(path, refs, lens, recs, block_bytes=at)
    w = cm.walk(open(path, "rb").read())
    assert w["starts"] == w0["starts"] and w["recs"][137][0] & 0xffff == 0 and w["recs"][137][0] >> 16 == w["members"][1][0] > 0
    _, pre, (_, depth, irefs, _) = built_equals_model(path, eng, 8, w)      # (leaves of 256: every read of c1 is a run of its own)
    leaf = cm.level_first(depth) + (500 * 137 >> 8)
    assert irefs[0][1][leaf] == w["recs"][137][0] and w["recs"][137][0] in pre["run_loff"].tolist()
    # every record spans several members; members without a record start
    long_recs = [(0, 100 + 40 * k, [(0, 300)], 16 if k & 1 else 0) for k in range(60)] + [(1, 5, [(0, 200), (2, 7)], 0)]
    bam_writer.write_bam(path, refs, lens, long_recs, block_bytes=100)
    w = cm.walk(open(path, "rb").read())
    assert all(b - a > 300 for a, b in zip(w["starts"], w["starts"][1:]))
    _, pre, _ = built_equals_model(path, eng, 8, w)
    assert len(set(pre["run_loff"].tolist())) >= 3 and all(v & 0xffff for v in pre["run_loff"].tolist()[1:])     # offsets inside members
    built_equals_model(path, eng, 14, w)


def test_forward_fill_across_references(eng, tmp_path):
    """Reference 0 ends in covered windows; reference 1 begins with a placed-unmapped read and uncovered windows: their
    loff is the offset of reference 1's first record, not the last offset of reference 0."""
    recs = [(0, 1000 * k, [(0, 50)], 0) for k in range(90)] + [(0, 89_500, [(0, 10), (3, 9000), (0, 10)], 0)]
    recs += [(1, 5, [], 4), (1, 2100, [], 4), (1, 50_000, [(0, 40)], 16), (1, 50_010, [(0, 40)], 0), (1, 70_000, [(0, 30)], 0)]
    path = str(tmp_path / "ff.bam")
    bam_writer.write_bam(path, ["c1", "c2"], [100_000, 100_000], recs, block_bytes=900)
    w, pre, (_, depth, refs, _) = built_equals_model(path, eng, 10)
    first1 = w["recs"][91][0]
    last0 = w["recs"][90][0]
    assert depth == 3 and pre["n_intv"][0] == (89_500 + 9020 - 1 >> 10) + 1 and pre["filled"][0][-1] == last0
    leaf = cm.level_first(3)
    bins, loff = refs[1]
    assert loff[leaf + 0] == first1 == loff[leaf + 2] and first1 > last0
    assert loff[leaf + (50_000 >> 10)] == w["recs"][93][0] and loff[leaf + (70_000 >> 10)] == w["recs"][95][0]


def test_refusals(eng, tmp_path):
    path = str(tmp_path / "r.bam")
    clean = lambda: not os.path.exists(path + ".csi") and not [f for f in os.listdir(str(tmp_path)) if "tmp" in f]  # noqa: E731
    # reference 100 000, min_shift 14 -> depth 1, reach 131 072: a read at 99 990 with a 40 000 N ends beyond it
    bam_writer.write_bam(path, ["c1"], [100_000], [(0, 99_990, [(0, 5), (3, 40_000), (0, 5)], 0)])
    with pytest.raises(ValueError, match=r"CSI index of min_shift 14 and depth 1 cannot hold .* beyond 131072"):
        build_index(path, engine=eng, fmt="csi")
    assert clean()
    bam_writer.write_bam(path, ["c1"], [100_000], [(0, 99_990, [(0, 5), (3, 31_072), (0, 5)], 0)])      # ends at 131 072: fits
    built_equals_model(path, eng, 14)
    os.remove(path + ".csi")
    for ms in (7, 31):
        with pytest.raises(ValueError, match="min_shift"):
            build_index(path, engine=eng, fmt="csi", min_shift=ms)
    with pytest.raises(ValueError, match="min_shift 14"):
        build_index(path, engine=eng, fmt="bai", min_shift=12)
    assert clean()
    # the window cap: 33 references with a read at the end of 2^31 - 1 have 33 * 2^23 windows of 256 positions
    many = ["c%d" % t for t in range(33)]
    cc.write_bam(path, many, [TOP] * 33, [(t, TOP - 30, [(0, 30)], 0) for t in range(33)])
    with pytest.raises(ValueError, match="more than 2\\^28: use a larger min_shift"):
        build_index(path, engine=eng, fmt="csi", min_shift=8)
    assert clean()
    _, pre, _ = built_equals_model(path, eng, 20)
    assert sum(pre["n_intv"]) == 33 << 11
    open(path + ".csi", "wb").write(b"someone else's bytes")
    with pytest.raises(FileExistsError):
        build_index(path, engine=eng, fmt="csi")
    assert open(path + ".csi", "rb").read() == b"someone else's bytes"
    bam_writer.write_bam(path, ["c1"], [100_000], [(0, 500, [(0, 30)], 0), (0, 100, [(0, 30)], 0)])
    with pytest.raises(ValueError, match="not coordinate sorted"):
        build_index(path, engine=eng, fmt="csi", overwrite=True)
    assert open(path + ".csi", "rb").read() == b"someone else's bytes" and not [f for f in os.listdir(str(tmp_path)) if "tmp" in f]


def test_region_reads_through_the_built_index(eng, tmp_path):
    d = cc.case_data("long", 14)
    path = cc.write_case(tmp_path, "long", 14)
    build_index(path, engine=eng, fmt="csi", out=path + ".built.csi")
    high = [q for q in range(len(d["regions"])) if d["regions"][q, 1] >= P29 and d["region_off"][q + 1] > d["region_off"][q]][:40]
    rest = [q for q in range(len(d["regions"])) if q not in high][:20]
    assert len(high) >= 30
    stager = Engine(0)
    for q in high + rest:
        reg, want = cc.region_want(d, q)
        got = read_bam_gpu(path, eng, regions=[reg], index=path + ".built.csi")
        cc.same(got, read_bam(path, regions=[reg], index=path + ".hts.csi"))
        cc.assert_records(got, d, want)
        stager.clear_alignments()
        stager.add_bam(path, regions=[reg], index=path + ".built.csi")
        assert stager.num_records(0) == len(want)
    stager.close()
    regs = [cc.region_want(d, q)[0] for q in high]
    cc.same(read_bam_gpu(path, eng, regions=regs, index=path + ".built.csi"), read_bam(path, regions=regs, index=path + ".hts.csi"))


def _aligned_positions(aln):
    """Per record of a PackedAlignments the aligned reference positions, from its runs."""
    out, r = [], 0
    for k in range(aln.n):
        if aln.nblk[k] <= 1:
            out.append(np.arange(aln.pos[k], int(aln.pos[k]) + int(aln.alen[k]), dtype=np.int64))
        else:
            nb = int(aln.nblk[k])
            out.append(np.concatenate([np.arange(s, int(s) + int(l), dtype=np.int64) for s, l in zip(aln.blk_start[r:r + nb], aln.blk_len[r:r + nb])]))
            r += nb
    return out


def test_counts_beyond_2_29_through_a_built_csi(tmp_path):
    """``index="build-csi"`` on the long case: the region-limited array counts what the whole-file array, the oracle and a
    plain bincount of the mapped positions count, for chains at the read clusters up to 2^31 - 2^17."""
    from oracle import oracle
    from plastid_amd.packing import concat_file_major
    path = cc.write_case(tmp_path, "long")
    seg = lambda c, s, e, st: GenomicSegment(c, s, e, st)  # noqa: E731
    chains = [SegmentChain(seg("big", 0, 900, "+")), SegmentChain(seg("big", 50, 400, "-")),
              SegmentChain(seg("big", P29 - 300, P29 + 900, "+")), SegmentChain(seg("big", P29 - 300, P29 - 5, "-"), seg("big", P29 + 5, P29 + 600, "-")),
              SegmentChain(seg("big", P30 - 200, P30 + 700, "-")), SegmentChain(seg("big", P30 - 100, P30 - 1, "+"), seg("big", P30 + 1, P30 + 300, "+")),
              SegmentChain(seg("big", 2_000_000_000, 2_000_001_500, "+")), SegmentChain(seg("big", 2_000_000_100, 2_000_000_900, "-")),
              SegmentChain(seg("big", (1 << 31) - (1 << 17) - 5000, (1 << 31) - (1 << 17), "+")),
              SegmentChain(seg("mid", P29 - 200, P29 + 800, "+")), SegmentChain(seg("mid", 100, 700, "-")), SegmentChain(seg("small", 0, 9000, "+"))]
    regs = [(c.chrom, c.spanning_segment.start, c.spanning_segment.end) for c in chains]
    part = pa.BAMGenomeArray(path, regions=regs, index="build-csi", keep_reads=False, mapping=pa.FivePrimeMapFactory(12))
    assert os.path.isfile(path + ".csi") and not os.path.exists(path + ".bai")
    assert BamIndex.from_file(path + ".csi") == BamIndex.from_bytes(cc.case_data("long", 14)["csi"])
    stamp = os.stat(path + ".csi").st_mtime_ns
    again = pa.BAMGenomeArray(path, regions=regs[:3], index="build-csi", keep_reads=False)
    assert os.stat(path + ".csi").st_mtime_ns == stamp and again.bamfiles[0].mapped == part.bamfiles[0].mapped
    whole = pa.BAMGenomeArray(path, keep_reads=False, mapping=pa.FivePrimeMapFactory(12))
    assert part.bamfiles[0].mapped == whole.bamfiles[0].mapped == int(cc.case_data("long", 14)["stat"][:, 1].sum())
    host = read_bam(path)
    aln = concat_file_major([host])
    positions = _aligned_positions(host)
    names = list(host.references)
    total = 0
    for kind, factory, spec in (("fiveprime", pa.FivePrimeMapFactory(12), oracle.mapping_spec("fiveprime", 12)),
                                ("center", pa.CenterMapFactory(0), oracle.mapping_spec("center", 0))):
        for ga in (part, whole):
            ga.set_mapping(factory)
        got_part, got_whole = part.get_counts_batch(chains), whole.get_counts_batch(chains)
        for c, x, y in zip(chains, got_part, got_whole):
            x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
            assert np.array_equal(x.view(np.uint64), y.view(np.uint64)), (kind, str(c))
            tid, strand = names.index(c.spanning_segment.chrom), c.spanning_segment.strand
            segs = [(s.start, s.end) for s in c]
            want = oracle.chain_get_counts(aln, spec, tid, segs, strand)
            assert np.array_equal(x, np.asarray(want, np.float64).reshape(x.shape)), (kind, str(c))
            # independent of both: a bincount over the chain's positions
            where = np.concatenate([np.arange(s, e, dtype=np.int64) for s, e in segs])
            slot = {int(p): i for i, p in enumerate(where)}
            acc = np.zeros(len(where), np.float64)
            for k in np.flatnonzero((host.tid == tid) & ((host.flags & 1) == (1 if strand == "-" else 0)) & (host.alen > 0)):
                p = positions[k]
                if kind == "fiveprime":
                    hit, wt = ([p[12]] if strand == "+" else [p[-13]]), 1.0
                else:
                    hit, wt = p, 1.0 / len(p)
                for q in hit:
                    i = slot.get(int(q))
                    if i is not None:
                        acc[i] += wt
            if strand == "-":
                acc = acc[::-1]
            if kind == "fiveprime":
                assert np.array_equal(x.ravel(), acc), (kind, str(c))
            else:   # (sums of 1 / length in another order: a few units in the last place)
                assert np.allclose(x.ravel(), acc, rtol=1e-12, atol=0), (kind, str(c))
            total += x.sum()
    assert total > 100
