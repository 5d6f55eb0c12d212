"""``BAMGenomeArray.to_bedgraph`` / ``to_variable_step`` on the format kernels (``pc_counts_export``) and
``to_genome_array(array_type=GenomeArray)`` device to device (``pc_track_set_counts``): the 36 texts the reference itself
wrote; designed count vectors sized to the kernels' seams (the run-head tile of 2048 elements, the 256 lines a workgroup
formats, window borders) against the host writers (``track.write_count_bedgraph``: the same line functions, serial) over
``ga.get(..., roi_order=False)``; batches; a staged BAM file; the error paths."""
import io
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import plastid_amd as pa  # noqa: E402
from plastid_amd import synth, track  # noqa: E402
from plastid_amd._lib import EngineError  # noqa: E402
from plastid_amd.genome_array import DenseGenomeArray  # noqa: E402
from tests import count_export_cases as cc  # noqa: E402

pytestmark = pytest.mark.gpu


def device_text(ga, what, strand, window=100000, **kwargs):
    fh = io.StringIO()
    (ga.to_bedgraph if what == "bedgraph" else ga.to_variable_step)(fh, "trk", strand, window_size=window, **kwargs)
    return fh.getvalue()


def vectors_of(ga, strand):
    return {c: ga.get(pa.GenomicSegment(c, 0, int(n), strand), roi_order=False) for c, n in ga.lengths().items()}


def host_text(ga, what, strand, window=100000, vectors=None):
    vectors = vectors_of(ga, strand) if vectors is None else vectors
    fh = io.StringIO()
    (track.write_count_bedgraph if what == "bedgraph" else track.write_count_variable_step)(vectors, fh, "trk", window_size=window)
    return fh.getvalue()


# ------------------------------------------------------------------ the reference's own texts
@pytest.fixture(scope="module")
def golden_arrays():
    made = {}

    def get(ex):
        key = (str(sorted(ex["spec"].items())), ex["normalize"])
        if key not in made:
            made[key] = pa.BAMGenomeArray(cc.golden_packed(pa), mapping=cc.factory(pa, ex["spec"]))
            made[key].set_normalize(ex["normalize"])
        return made[key]
    return get


@pytest.mark.parametrize("k", range(36))
def test_device_export_gives_the_reference_text(golden_arrays, k):
    ex = cc.golden()[0]["exports"][k]
    ga = golden_arrays(ex)
    text = device_text(ga, ex["what"], ex["strand"], ex["window"], **ex["kwargs"])
    assert text == ex["text"], cc.export_id(ex)
    stats = ga.export_stats()
    assert stats["lines"] == text.count("\n") - 1 and stats["bytes"] == len(text.split("\n", 1)[1].encode()) and stats["batches"] == 1
    if not (ex["normalize"] or ex["spec"]["kind"] == "center"):
        assert stats["listed"] == 0
    assert set(ga.export_timing()) == {"run_heads", "runs", "listed_values", "lengths", "format", "read_back"}


# ------------------------------------------------------------------ geometry
SEAM_LENGTHS = {"c0001": 1, "c2047": 2047, "c2048": 2048, "c2049": 2049, "c4097": 4097, "quiet": 300}


def _seam_counts():
    """Runs that begin in one tile of 2048 export elements and end in the next (the contigs stand one behind the other in
    the export, so the borders fall inside c2048, c2049 and c4097 too), runs at position 0 and at the last position,
    counts of every digit width up to four."""
    counts = {"c0001": {0: 3}}
    counts["c2047"] = {0: 1, 1: 1, 2: 10, 1000: 99, 1001: 100, 2045: 7, 2046: 7}
    counts["c2048"] = {**{p: 5 for p in range(2040, 2048)}, 0: 9, 254: 2, 255: 2, 256: 2, 257: 3}
    counts["c2049"] = {**{p: 4 for p in range(2046, 2049)}, 3: 1000, 510: 1, 511: 1}
    counts["c4097"] = {**{p: 6 for p in range(2040, 2060)}, **{p: 2 for p in range(4090, 4097)}}
    counts["c4097"].update({0: 12, 2047: 6, 2048: 6, 4095: 8, 4096: 8})
    return counts


@pytest.fixture(scope="module")
def seam_reads():
    return cc.designed_packed(pa, SEAM_LENGTHS, _seam_counts(), reverse=("c2049",))


@pytest.mark.parametrize("rule", ["fiveprime", "threeprime-norm", "center"])
def test_export_across_tiles_and_windows(seam_reads, rule):
    reads = seam_reads
    if rule == "center":   # reads of 3 nt: a third of a read per position, sums of thirds where they overlap
        reads = cc.designed_packed(pa, SEAM_LENGTHS, {c: {p: n for p, n in d.items() if p + 3 <= SEAM_LENGTHS[c]} for c, d in _seam_counts().items()},
                                   reverse=("c2049",), alen=3)
    mapping = {"fiveprime": pa.FivePrimeMapFactory(0), "threeprime-norm": pa.ThreePrimeMapFactory(0), "center": pa.CenterMapFactory()}[rule]
    ga = pa.BAMGenomeArray(reads, mapping=mapping)
    ga.set_normalize(rule == "threeprime-norm")
    for strand in ("+", "-", "."):
        vectors = vectors_of(ga, strand)
        for window in (1, 255, 2048, 2049, 100000):
            got = device_text(ga, "bedgraph", strand, window)
            assert got == host_text(ga, "bedgraph", strand, window, vectors), (rule, strand, window)
            assert ga.export_stats()["lines"] == got.count("\n") - 1
        got = device_text(ga, "variable_step", strand)
        assert got == host_text(ga, "variable_step", strand, vectors=vectors), (rule, strand)
        assert got.count("variableStep chrom=") == len(SEAM_LENGTHS)
    listed = ga.export_stats()["listed"]
    assert listed == 0 if rule == "fiveprime" else listed > 0
    # the designed counts themselves, once
    if rule == "fiveprime":
        plus = device_text(ga, "bedgraph", "+", 100000)
        assert "c2048\t2040\t2048\t5\n" in plus and "c4097\t2040\t2060\t6\n" in plus and "c2047\t1001\t1002\t100\n" in plus and "c2049" not in plus
        assert "c2049\t3\t4\t1000\n" in device_text(ga, "bedgraph", "-", 100000)
        assert "c4097\t2040\t2048\t6\nc4097\t2048\t2060\t6\n" in device_text(ga, "bedgraph", "+", 2048)


@pytest.mark.parametrize("nlines", [254, 255, 256, 257, 513])
def test_export_of_exactly_this_many_lines(nlines):
    """256 lines per workgroup of the length and format kernels: one line short of a workgroup, exactly one, one more."""
    lengths = {"a": 700, "b": 1500}
    counts = {"a": {2 * i + 1: 1 + i % 11 for i in range(min(nlines, 300))}, "b": {3 * i: 7 for i in range(max(nlines - 300, 0))}}
    ga = pa.BAMGenomeArray(cc.designed_packed(pa, lengths, counts), mapping=pa.FivePrimeMapFactory(0))
    bed = device_text(ga, "bedgraph", "+")
    assert bed.count("\n") - 1 == nlines and ga.export_stats()["lines"] == nlines
    assert bed == host_text(ga, "bedgraph", "+")
    # variableStep: two headers and nlines - 2 positions
    counts["a"].pop(1)
    counts["a"].pop(3)
    ga = pa.BAMGenomeArray(cc.designed_packed(pa, lengths, counts), mapping=pa.FivePrimeMapFactory(0))
    var = device_text(ga, "variable_step", "+")
    assert var.count("\n") - 1 == nlines and ga.export_stats()["lines"] == nlines and ga.export_stats()["runs"] == nlines - 2
    assert var == host_text(ga, "variable_step", "+")


# ------------------------------------------------------------------ batches
def test_batches_give_the_text_of_one_batch():
    lengths = {"chrA": 5000, "chrB": 3000, "chrC": 900, "chrD": 1}
    rng = np.random.default_rng(5)
    counts = {c: {int(p): int(rng.integers(1, 120)) for p in rng.integers(0, n, min(n, 200))} for c, n in lengths.items()}
    ga = pa.BAMGenomeArray(cc.designed_packed(pa, lengths, counts, reverse=("chrB",)), mapping=pa.FivePrimeMapFactory(0))
    for what in ("bedgraph", "variable_step"):
        for strand in ("+", "."):
            whole = device_text(ga, what, strand, 777)
            assert ga.export_stats()["batches"] == 1
            one = ga.export_stats()
            assert whole == host_text(ga, what, strand, 777)
            assert device_text(ga, what, strand, 777, _batch_elems=3000) == whole      # chrA alone (over budget), chrB, chrC + chrD
            cut = ga.export_stats()
            assert cut["batches"] == 3 and [cut[k] for k in ("lines", "runs", "listed", "bytes")] == [one[k] for k in ("lines", "runs", "listed", "bytes")]
            assert device_text(ga, what, strand, 777, _batch_elems=1) == whole and ga.export_stats()["batches"] == 4
            assert device_text(ga, what, strand, 777, _batch_elems=901) == whole and ga.export_stats()["batches"] == 3
    messages = []

    class Printer(object):
        def write(self, msg):
            messages.append(msg)
    fh = io.StringIO()
    ga.to_bedgraph(fh, "trk", "+", printer=Printer(), _batch_elems=3000)
    assert messages == ["Writing chromosome %s..." % c for c in sorted(lengths)]


def test_a_batch_of_more_contigs_than_16_bits_count():
    """A transcriptome or a scaffold-level assembly: 70 000 contigs of one or two positions are ONE batch of the default
    budget (a batch is bounded by its positions, not by its contigs), and cut ones give the same text."""
    n = 70000
    lengths = {"t%05d" % k: 1 + k % 2 for k in range(n)}
    counts = {"t%05d" % k: {k % 2: 1 + k % 13} for k in range(0, n, 7)}
    ga = pa.BAMGenomeArray(cc.designed_packed(pa, lengths, counts), mapping=pa.FivePrimeMapFactory(0))
    bed = "track type=bedGraph name=trk\n" + "".join("t%05d\t%d\t%d\t%d\n" % (k, k % 2, k % 2 + 1, 1 + k % 13) for k in range(0, n, 7))
    var = "track type=wiggle_0 name=trk\n" + "".join(
        "variableStep chrom=t%05d span=1\n" % k + ("%d\t%d\n" % (k % 2 + 1, 1 + k % 13) if k % 7 == 0 else "") for k in range(n))
    assert device_text(ga, "bedgraph", "+") == bed
    assert ga.export_stats()["batches"] == 1 and ga.export_stats()["lines"] == len(range(0, n, 7))
    assert device_text(ga, "variable_step", ".") == var
    assert ga.export_stats()["batches"] == 1 and ga.export_stats()["lines"] == n + len(range(0, n, 7))
    assert device_text(ga, "bedgraph", "+", _batch_elems=40000) == bed and ga.export_stats()["batches"] == 3
    assert device_text(ga, "bedgraph", "-") == "track type=bedGraph name=trk\n"


# ------------------------------------------------------------------ a staged BAM file
def test_a_staged_bam_file_exports_the_same_bytes(tmp_path):
    from tests import bam_writer
    reads = cc.golden_packed(pa)
    path = str(tmp_path / "reads.bam")
    bam_writer.write_bam(path, list(reads.references), list(reads.lengths), bam_writer.packed_to_records(reads))
    for mapping in (pa.FivePrimeMapFactory(12), pa.CenterMapFactory(3)):
        staged = pa.BAMGenomeArray(path, keep_reads=False, mapping=mapping)
        packed = pa.BAMGenomeArray(reads, mapping=mapping)
        for what, strand, window in (("bedgraph", "+", 777), ("bedgraph", ".", 100000), ("variable_step", "-", 100000)):
            text = device_text(staged, what, strand, window)
            assert text == device_text(packed, what, strand, window) and text.count("\n") > 10


# ------------------------------------------------------------------ to_genome_array(array_type=GenomeArray)
def _dyadic_reads():
    """1024 reads of 1 nt: normalised counts are c / 1024 * 10^6 = c * 976.5625 and center counts whole numbers, so every
    sum of them is exact in any order -- numpy's pairwise sum of the host path and the fixed tree of the device agree bit
    for bit, as the test below asks."""
    lengths = {"chrA": 5000, "chrB": 2049, "chrC": 2}
    counts = {"chrA": {p: 2 for p in range(0, 450, 3)}, "chrB": {p: 4 for p in range(1000, 1100)}, "chrC": {0: 24}}
    counts["chrA"][4998] = 200
    counts["chrA"][4999] = 1024 - sum(sum(d.values()) for d in counts.values())   # (the last position: to_genome_array stops short of it)
    reads = cc.designed_packed(pa, lengths, counts, reverse=("chrB",))
    assert reads.n == 1024
    return reads


@pytest.mark.parametrize("rule", ["fiveprime", "threeprime-norm", "center"])
def test_to_genome_array_device_to_device(rule):
    mapping = {"fiveprime": pa.FivePrimeMapFactory(0), "threeprime-norm": pa.ThreePrimeMapFactory(0), "center": pa.CenterMapFactory()}[rule]
    bga = pa.BAMGenomeArray(_dyadic_reads(), mapping=mapping)
    bga.set_normalize(rule == "threeprime-norm")
    dense = bga.to_genome_array()
    ga = bga.to_genome_array(array_type=pa.GenomeArray)
    assert isinstance(dense, DenseGenomeArray) and isinstance(ga, pa.GenomeArray)
    assert ga._engine is bga._engine
    assert ga.strands() == dense.strands() == ("+", "-", ".")
    assert ga.chroms() == dense.chroms() and dict(ga.lengths()) == dict(dense.lengths())
    host = ga.to_host()
    for c in dense.chroms():
        for st in dense.strands():
            assert np.array_equal(host._chroms[c][st], dense._chroms[c][st]), (c, st)
    assert dense.sum() > 0 and ga.sum() == dense.sum()
    assert host._chroms["chrA"]["+"][4999] == 0 and host._chroms["chrA"]["+"][4998] != 0      # the reference's off-by-one
    # the parent's path -- every vector through the host and __setitem__, an engine of the array's own -- writes the same track
    old = pa.GenomeArray(chr_lengths=bga.lengths(), strands=bga.strands())
    for c in bga.chroms():
        for st in bga.strands():
            seg = pa.GenomicSegment(c, 0, bga.lengths()[c] - 1, st)
            old[seg] = bga[seg]
    assert old._engine is not bga._engine
    for st in bga.strands():
        texts = []
        for arr in (ga, old):
            fh = io.StringIO()
            arr.to_bedgraph(fh, "trk", st)
            texts.append(fh.getvalue())
        assert texts[0] == texts[1] and (st == "-" or texts[0].count("\n") > 100)
    old.close()
    want = dense._chroms["chrB"]["-"][990:1010]
    del bga
    import gc
    gc.collect()
    assert np.array_equal(ga.get(pa.GenomicSegment("chrB", 990, 1010, "-"), roi_order=False), want)   # the array holds the engine
    ga.close()


# ------------------------------------------------------------------ errors
def test_errors_write_nothing():
    reads = _dyadic_reads()
    bga = pa.BAMGenomeArray(reads, mapping=pa.FivePrimeMapFactory(0))
    eng = bga._engine
    bga._sync_engine()
    plan = eng.plan([0], [0], [5000], [1], [0], np.ones(1, np.int8), [5000], 5000, 1)
    with pytest.raises(EngineError, match="nothing counted yet"):      # PC_ERR_STATE
        plan.export_text(0, ["chrA"], [0], [5000], period=100)
    ga = pa.GenomeArray(chr_lengths=bga.lengths(), strands=bga.strands(), engine=eng)
    with pytest.raises(EngineError, match="nothing counted yet"):
        plan.set_track(ga, "chrA", 0, 0, 0, 100)
    plan.launch(np.int64)
    for bad in (dict(period=0), dict(period=-5)):
        with pytest.raises(ValueError):                                  # PC_ERR_ARG
            plan.export_text(0, ["chrA"], [0], [5000], **bad)
    with pytest.raises(ValueError, match="outside"):
        plan.export_text(1, ["chrA"], [1], [5000])
    with pytest.raises(ValueError, match="outside"):
        plan.set_track(ga, "chrA", 0, 0, 4000, 1001)
    other = pa.GenomeArray(chr_lengths=bga.lengths(), strands=bga.strands())      # an engine of its own
    with pytest.raises(ValueError, match="another engine"):
        plan.set_track(other, "chrA", 0, 0, 0, 100)
    for arr in (ga, other):
        assert arr.sum() == 0.0 and all(n == 0 for per in arr.extents().values() for n in per.values())
        assert dict(arr.lengths()) == dict(bga.lengths())
    plan.set_track(ga, "chrA", 0, 10, 0, 100)                             # (and the call itself works)
    assert ga.sum() == float(sum(2 for p in range(0, 100, 3))) and ga.extents()["chrA"]["+"] == 110
    assert len(plan.export_text(0, ["chrA"], [0], [5000], period=100)) > 0
    # summed slices and several rows are no source
    summed = eng.plan([0], [0], [5000], [1], [0], np.zeros(1, np.int8), [1], 1, 1)
    summed.launch(np.int64)
    with pytest.raises(ValueError, match="one row"):
        summed.export_text(1, ["chrA"], [0], [1])
    for p in (plan, summed):
        p.close()
    other.close()
    ga.close()
    # a stratified rule: TypeError before the track line
    bga.set_mapping(pa.StratifiedVariableFivePrimeMapFactory(synth.VARIABLE_OFFSETS, 25, 35))
    for what in (bga.to_bedgraph, bga.to_variable_step):
        fh = io.StringIO()
        with pytest.raises(TypeError):
            what(fh, "trk", "+")
        assert fh.getvalue() == ""
    with pytest.raises(TypeError):
        bga.to_genome_array(array_type=pa.GenomeArray)
