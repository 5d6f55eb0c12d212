"""The BAI index built on the GPU (``plastid_amd.bam.build_index`` / ``pc_bam_index_build``) against the record-by-record
model (tests/index_model.py, itself pinned to the index htslib wrote for the fixture by tests/test_bam_index.py), and
region reads through the built index."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import plastid_amd as pa  # noqa: E402
from plastid_amd import synth  # noqa: E402
from plastid_amd.bam import BamIndex, build_index, read_bam, read_bam_gpu  # noqa: E402
from plastid_amd.engine import Engine  # noqa: E402
from tests import bam_writer  # noqa: E402
from tests import index_cases as ic  # noqa: E402
from tests import index_model as im  # noqa: E402

pytestmark = pytest.mark.gpu

COLS = ("tid", "pos", "alen", "flags", "nblk", "blk_start", "blk_len", "wide_idx", "wide_alen", "wide_nblk", "flag16", "mapq", "qlen", "nh")


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def same(a, b):
    for k in COLS:
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    assert a.references == b.references and a.lengths == b.lengths and a.mapped == b.mapped and a.n == b.n


def built_equals_model(path, eng, walked=None):
    """Build the index of `path` beside it; the bytes written, the returned object and the model agree.  Returns the walk."""
    w = walked or im.walk(open(path, "rb").read())
    want = im.finish(im.prefinish(w))
    timing = {}
    idx = build_index(path, engine=eng, overwrite=True, timing=timing)
    data = open(path + ".bai", "rb").read()
    assert im.parse_bai(data) == want
    assert idx == BamIndex.from_bytes(data) and idx.n_no_coor == want[1]
    for ids in im.bin_order(data):
        assert ids == sorted(ids)
    assert timing["records"] == len(w["recs"]) and timing["n_no_coor"] == want[1] and timing["index_bytes"] == len(data)
    assert timing["mapped"] == sum(1 for r in w["recs"] if r[1] >= 0 and r[4]) and timing["total_ms"] > 0
    return w


def test_the_index_of_the_htslib_fixture(eng, tmp_path):
    """The built index equals the one htslib wrote, parsed; the fixture's 400 regions read through it give htslib's own
    result sets, record for record."""
    hts = np.load(ic.FIX)
    path = str(tmp_path / "htslib.bam")
    open(path, "wb").write(hts["bam"].tobytes())
    idx = build_index(path, engine=eng)
    assert idx == BamIndex.from_bytes(hts["bai"].tobytes())
    assert im.parse_bai(open(path + ".bai", "rb").read()) == im.parse_bai(hts["bai"].tobytes())
    assert idx.mapped == int(hts["index_stat"][:, 1].sum())
    refs = [str(x) for x in hts["references"]]
    nonempty = 0
    for q in range(len(hts["regions"])):
        t, b, e = (int(x) for x in hts["regions"][q])
        got = read_bam_gpu(path, eng, regions=[(refs[t], b, e)])
        want = hts["region_records"][hts["region_off"][q]:hts["region_off"][q + 1]]
        assert got.n == len(want), q
        nonempty += got.n > 0
        assert np.array_equal(got.flag16, hts["flag"][want]) and np.array_equal(got.mapq, hts["mapq"][want]) and np.array_equal(got.qlen, hts["l_qseq"][want])
        assert got.mapped == idx.mapped
    assert nonempty > 300


def test_a_multi_level_file(eng, tmp_path):
    """Bins of levels 0, 4 and 5, a pile of 12 000 reads in one window whose bin stays (it spans more than 0x10000 file
    bytes) with several chunks, bins that move into their parents, a reference without records, reads that end in N and D,
    placed-unmapped and unplaced reads; then random region sets through the built index against the writer's own."""
    path = str(tmp_path / "synth.bam")
    ic.write_synth(path, index=True)
    os.replace(path + ".bai", path + ".writer.bai")
    w, _, model = ic.synth_model(path)
    ic.assert_synth_shape(model)
    built_equals_model(path, eng, w)
    rng = np.random.default_rng(11)
    a, b = Engine(0), Engine(0)
    for trial in range(8):
        regs = []
        for _ in range(int(rng.integers(1, 6))):
            t = int(rng.choice([0, 0, 2, 3, 1]))
            lo = int(rng.choice([0, ic.PILE_AT - 30000, ic.PILE_AT, 99_000, int(rng.integers(0, ic.SYNTH_LENS[t]))]))
            lo = min(lo, ic.SYNTH_LENS[t] - 1)
            regs.append((ic.SYNTH_REFS[t], lo, lo + int(rng.choice([1, 50, 3000, 200000, 70_000_000]))))
        got, want = read_bam_gpu(path, eng, regions=regs), read_bam_gpu(path, eng, regions=regs, index=path + ".writer.bai")
        same(got, want)
        same(got, read_bam(path, regions=regs))
        a.clear_alignments()
        b.clear_alignments()
        assert a.add_bam(path, regions=regs) == b.add_bam(path, regions=regs, index=path + ".writer.bai")
        assert a.num_records(0) == b.num_records(0) == got.n
        if got.n:
            ra, rb = a.read_records(0, np.arange(got.n)), b.read_records(0, np.arange(got.n))
            assert all(np.array_equal(ra[k], rb[k]) for k in ra)
    a.close()
    b.close()


def _long_reads(n, step=40, length=300):
    return [(0, 100 + step * k, [(0, length)], 16 if k & 1 else 0) for k in range(n)]


def test_member_boundaries(eng, tmp_path):
    refs, lens = ["c1", "c2"], [3_000_000, 50_000]
    recs = [(0, 500 * k, [(0, 30)], 0) for k in range(400)] + [(1, 7 * k, [(0, 20), (3, 40), (0, 20)], 16) for k in range(100)] + [(-1, -1, [], 4)] * 3
    path = str(tmp_path / "b.bam")
    bam_writer.write_bam(path, refs, lens, recs, block_bytes=60000)
    w0 = im.walk(open(path, "rb").read())
    total = w0["members"][-1][1]          # bytes of the inflated stream (where the EOF block begins)
    # a record starts exactly where a member begins
    at = w0["starts"][137]
    bam_writer.write_bam(path, refs, lens, recs, block_bytes=at)
    w = im.walk(open(path, "rb").read())
    assert w["starts"] == w0["starts"] and w["recs"][137][0] & 0xffff == 0 and w["recs"][137][0] >> 16 == w["members"][1][0] > 0
    built_equals_model(path, eng, w)
    # the last record ends exactly where the last data member ends: the final offset is the EOF block's
    div = next(d for d in range(300, total + 1) if total % d == 0)
    bam_writer.write_bam(path, refs, lens, recs, block_bytes=div)
    w = im.walk(open(path, "rb").read())
    assert w["members"][-1][2] == 0 and w["members"][-2][1] + w["members"][-2][2] == total == w["members"][-1][1]
    assert w["final"] == w["members"][-1][0] << 16
    idx_end = im.finish(im.prefinish(w))[0][1][0][37450][0][1]
    assert idx_end == w["recs"][500][0]          # the last reference's range ends at the first unplaced record
    built_equals_model(path, eng, w)
    # every record spans several members; members without a record start
    long_recs = _long_reads(60) + [(1, 5, [(0, 200), (2, 7)], 0)]
    bam_writer.write_bam(path, refs, lens, long_recs, block_bytes=100)
    w = im.walk(open(path, "rb").read())
    begins = np.array([m[1] for m in w["members"]])
    per_member = np.histogram(w["starts"], bins=np.append(begins, begins[-1] + 1))[0]
    assert (per_member[:-1] == 0).sum() > len(long_recs) and all(b - a > 300 for a, b in zip(w["starts"], w["starts"][1:]))
    built_equals_model(path, eng, w)
    # a header of a dozen members
    text = "@HD\tVN:1.6\tSO:coordinate\n" + "".join("@CO\tpadding line %06d %s\n" % (k, "x" * 60) for k in range(400))
    bam_writer.write_bam(path, refs, lens, recs, block_bytes=2500, header_text=text)
    w = im.walk(open(path, "rb").read())
    assert sum(1 for m in w["members"] if m[1] + m[2] <= w["first_record"]) >= 12
    built_equals_model(path, eng, w)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 513])
def test_run_heads_on_workgroup_borders(eng, tmp_path, n):
    """The bin changes at records 255 and 256: run heads in the last thread of one workgroup and the first of the next."""
    recs = [(0, 10 + (k if k < 255 else 20000 if k == 255 else 40000 + k), [(0, 25)], 0) for k in range(n)]
    path = str(tmp_path / "wg.bam")
    bam_writer.write_bam(path, ["c1"], [100_000], recs, block_bytes=5000)
    w = im.walk(open(path, "rb").read())
    pre = im.prefinish(w)
    assert len(pre["run_tid"]) == (1 if n <= 255 else 2 if n == 256 else 3)
    built_equals_model(path, eng, w)


@pytest.mark.parametrize("recs", [[], [(-1, -1, [], 4)] * 7, [(1, 16383, [(0, 2)], 0)], [(0, 0, [(4, 20)], 0), (0, 16384, [(1, 5)], 16)]],
                         ids=["header-only", "unplaced-only", "one-read", "no-reference-base"])
def test_degenerate_files(eng, tmp_path, recs):
    path = str(tmp_path / "d.bam")
    bam_writer.write_bam(path, ["c1", "c2"], [40_000, 40_000], recs)
    w = built_equals_model(path, eng)
    idx = BamIndex.from_file(path + ".bai")
    assert idx.n_ref == 2 and idx.n_no_coor == sum(1 for r in recs if r[0] < 0)
    assert [len(b) for b in idx.bins] == [len({im.reg2bin(r[2], r[3]) for r in w["recs"] if r[1] == t}) for t in range(2)]


def test_refusals(eng, tmp_path):
    path = str(tmp_path / "r.bam")
    bam_writer.write_bam(path, ["c1"], [100_000], [(0, 500, [(0, 30)], 0), (0, 100, [(0, 30)], 0)])
    with pytest.raises(ValueError, match="not coordinate sorted"):
        build_index(path, engine=eng)
    assert not os.path.exists(path + ".bai")
    bam_writer.write_bam(path, ["c1"], [(1 << 29) + 1], [(0, 500, [(0, 30)], 0)])
    with pytest.raises(ValueError, match="BAI index cannot hold"):
        build_index(path, engine=eng)
    bam_writer.write_bam(path, ["c1"], [1 << 29], [(0, (1 << 29) - 10, [(0, 5), (3, 10), (0, 5)], 0)])
    with pytest.raises(ValueError, match="BAI index cannot hold"):
        build_index(path, engine=eng)
    assert not os.path.exists(path + ".bai") and not [f for f in os.listdir(str(tmp_path)) if "tmp" in f]
    bam_writer.write_bam(path, ["c1"], [1 << 29], [(0, (1 << 29) - 10, [(0, 5), (3, 2), (0, 3)], 0)])     # ends at 2^29: fits
    built_equals_model(path, eng)
    open(path + ".bai", "wb").write(b"someone else's bytes")
    with pytest.raises(FileExistsError):
        build_index(path, engine=eng)
    assert open(path + ".bai", "rb").read() == b"someone else's bytes"
    with pytest.raises(IOError):
        build_index(str(tmp_path / "missing.bam"), engine=eng)


def test_index_build_keyword(tmp_path):
    """``index="build"``: a file without an index gets one, and the region-limited array counts what the whole-file array
    counts; without the keyword the same file raises the error of a missing index."""
    genome, tx, reads, _ = synth.make_config("C4", scale=0.00006, tx_scale=0.002)
    path = str(tmp_path / "noidx.bam")
    bam_writer.write_bam(path, list(reads.references), [int(x) for x in reads.lengths], bam_writer.packed_to_records(reads), block_bytes=3000)
    chains = tx.chains(limit=60)[:25]
    regs = [(c.chrom, c.spanning_segment.start, c.spanning_segment.end) for c in chains]
    with pytest.raises(ValueError, match="cannot read the index of"):
        pa.BAMGenomeArray(path, regions=regs, keep_reads=False)
    assert not os.path.exists(path + ".bai")
    part = pa.BAMGenomeArray(path, regions=regs, index="build", keep_reads=False, mapping=pa.FivePrimeMapFactory(12))
    assert os.path.isfile(path + ".bai")
    assert im.parse_bai(open(path + ".bai", "rb").read()) == im.model(open(path, "rb").read())
    whole = pa.BAMGenomeArray(path, keep_reads=False, mapping=pa.FivePrimeMapFactory(12))
    assert part.bamfiles[0].mapped == whole.bamfiles[0].mapped
    for factory in (pa.FivePrimeMapFactory(12), pa.CenterMapFactory(0)):
        for ga in (part, whole):
            ga.set_mapping(factory)
        for x, y in zip(part.get_counts_batch(chains), whole.get_counts_batch(chains)):
            assert np.array_equal(np.asarray(x).view(np.uint64), np.asarray(y).view(np.uint64))
    stamp = os.path.getmtime(path + ".bai")
    again = read_bam_gpu(path, part._engine, regions=regs[:3], index="build")     # found: not built again
    assert os.path.getmtime(path + ".bai") == stamp
    same(again, read_bam(path, regions=regs[:3], index="build"))
