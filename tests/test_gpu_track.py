"""plastid_amd.GenomeArray on the GPU: bedGraph / wiggle text parsed and applied by the kernels of
csrc/track_kernels.hip.h, read back through k_track_gather.  Every case of tests/golden/track_fixture.npz against the
reference's arrays, tuples, lengths, sums and counts; generated files sized to the kernels' seams against the host reader
(plastid_amd.read_wiggle, the same parser source) applied in file order with numpy; a round trip through
BAMGenomeArray.to_bedgraph; the import statistics (the GPU path really parses: no escaped line where every token is
plain); overlapping lines; and the refused texts, word for word as the host reader refuses them."""
import io
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import plastid_amd as pa  # noqa: E402
from plastid_amd import synth  # noqa: E402
from tests import track_cases as tc  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    from plastid_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def model_arrays(texts_and_strands, lengths):
    """The host reader's rows applied in file order: {(chrom, strand): vector of lengths[chrom]}."""
    out = {}
    for text, strand in texts_and_strands:
        t = pa.read_wiggle(io.StringIO(text))
        for name, a, b, v in t.tuples():
            vec = out.setdefault((name, strand), np.zeros(lengths[name]))
            vec[a:b] = vec[a:b] + v
    return out


def overlapping_lines(text):
    """Rows of the text that share a cluster with another row (clusters: runs of rows, by start, that begin below the
    furthest end so far on their contig); empty intervals write nothing and belong to none."""
    t = pa.read_wiggle(io.StringIO(text))
    n = 0
    for c in range(len(t.names)):
        rows = sorted((int(a), int(b)) for k, a, b in zip(t.chrom, t.start, t.stop) if k == c and b > a)
        size, far = 0, -1
        for a, b in rows:
            if size and a < far:
                size += 1
            else:
                n += size if size > 1 else 0
                size = 1
            far = max(far, b)
        n += size if size > 1 else 0
    return n


def assert_matches_model(ga, adds):
    host = ga.to_host()
    lengths = ga.lengths()
    model = model_arrays(adds, lengths)
    for c in ga.chroms():
        for st in ga.strands():
            exp = model.get((c, st), np.zeros(lengths[c]))
            assert tc.same_bits(host._chroms[c][st], exp), (c, st)
    return host


# ------------------------------------------------------------------ the reference's cases
@pytest.mark.parametrize("name", tc.case_names())
def test_fixture_case(engine, name):
    manifest, arrays = tc.fixture()
    c = tc.case(name)
    ga = pa.GenomeArray(c["chr_lengths"], min_chr_size=manifest["min_chr_size"], engine=engine)
    escaped = []
    for text, strand in c["adds"]:
        ga.add_from_wiggle(io.StringIO(text), strand)
        st, host = ga.import_stats(), pa.read_wiggle(io.StringIO(text))
        assert (st["lines"], st["yielded"], st["states"]) == (host.stats["lines"], host.stats["yielded"], host.stats["states"])
        assert st["overlapping"] == overlapping_lines(text)
        escaped.append((st["escaped"], host.stats["escaped"]))
    assert all(a == b for a, b in escaped), escaped       # exactly the lines the host's plain predicate names
    assert ga.chroms() == c["chroms"] and dict(ga.lengths()) == c["lengths"]
    assert len(ga) == len(c["chroms"]) and all(ch in ga for ch in c["chroms"]) and "nope" not in ga
    host = assert_matches_model(ga, [tuple(a) for a in c["adds"]])
    for ch in c["chroms"]:
        for st in ("+", "-"):
            assert tc.same_bits(host._chroms[ch][st], arrays["%s|%s|%s" % (name, ch, st)]), (ch, st)
    ref_sum = float(c["sum"])
    if not np.isfinite(ref_sum):
        assert not np.isfinite(ga.sum())
    elif c["integer"]:
        assert ga.sum() == ref_sum
    else:
        assert abs(ga.sum() - ref_sum) <= tc.sum_bound(arrays, c)
    assert tc.same_bits([ga.sum()], [ga.sum()])
    for s in c["segments"]:
        ch, a, b, st = s["seg"]
        seg = pa.GenomicSegment(ch, a, b, st)
        assert tc.same_bits(ga[seg], arrays[s["key"]])
        assert tc.same_bits(ga.get(seg, roi_order=False), arrays[s["key"]][::-1] if st == "-" else arrays[s["key"]])
    for ci in c["chains"]:
        chain = pa.SegmentChain(*[pa.GenomicSegment(ci["chrom"], s, e, ci["strand"]) for s, e in ci["segments"]])
        if ci["masks"]:
            chain.add_masks(*[pa.GenomicSegment(ci["chrom"], s, e, ci["strand"]) for s, e in ci["masks"]])
        assert tc.same_bits(chain.get_counts(ga), arrays[ci["key"]])
        assert tc.same_bits(ga[chain], arrays[ci["key"]])
        masked = chain.get_masked_counts(ga)
        assert tc.same_bits(masked.data, arrays[ci["key"] + "|masked"])
        assert np.array_equal(np.ma.getmaskarray(masked), arrays[ci["key"] + "|mask"].astype(bool))
    if c["normalised"]:
        ga.set_normalize(True)
        for s in c["segments"]:
            ch, a, b, st = s["seg"]
            assert tc.same_bits(ga[pa.GenomicSegment(ch, a, b, st)], arrays[s["key"] + "|norm"])
        with pytest.raises(ValueError):
            ga.add_from_wiggle(io.StringIO("chrA 1 2 3\n"), "+")
        ga.set_normalize(False)
    ga.close()


# ------------------------------------------------------------------ the kernels' seams
def seam_text():
    """About 10 KiB (line-start tiles are 4 KiB): a bedGraph block whose last line straddles the first tile border, a
    fixedStep block that spans the second, values with up to 15 significant digits."""
    rng = np.random.default_rng(7)
    lines = ["track type=bedGraph name=seams"]
    pos = 0
    while sum(len(x) + 1 for x in lines) < 4096 - 40:
        n = int(rng.integers(1, 9))
        lines.append("chrA\t%d\t%d\t%s" % (pos, pos + n, repr(round(float(rng.uniform(0, 50)), int(rng.integers(0, 6))))))
        pos += n + int(rng.integers(0, 3))
    lines.append("chrSeam_%s\t5\t9\t2.5" % ("x" * 60))          # straddles byte 4096
    assert sum(len(x) + 1 for x in lines[:-1]) < 4096 < sum(len(x) + 1 for x in lines)
    lines.append("fixedStep chrom=chrB start=101 step=3 span=2")
    while sum(len(x) + 1 for x in lines) < 2 * 4096 + 600:          # the block runs across byte 8192
        lines.append(str(int(rng.integers(0, 1000))))
    lines.append("variableStep chrom=chrA span=5")
    at = 20000
    for _ in range(120):
        at += int(rng.integers(5, 40))
        lines.append("%d %d" % (at, int(rng.integers(1, 99))))
    return "\n".join(lines) + "\n"


def test_line_start_tiles_and_blocks_across_them(engine):
    text = seam_text()
    assert 2 * 4096 < len(text) < 3 * 4096
    ga = pa.GenomeArray(min_chr_size=30000, engine=engine)
    ga.add_from_wiggle(io.StringIO(text), "+")
    st = ga.import_stats()
    host = pa.read_wiggle(io.StringIO(text))
    assert st["escaped"] == 0 and st["overlapping"] == 0 and st["states"] == host.stats["states"] == 4
    assert st["yielded"] == len(host) and st["lines"] == host.stats["lines"]
    assert_matches_model(ga, [(text, "+")])
    ga.close()


ITEM_LENGTHS = (1, 2047, 2048, 2049, 4097)


def test_intervals_and_segments_around_the_item_length(engine):
    lines, at, spans = [], 3, []
    for k, n in enumerate(ITEM_LENGTHS):
        lines.append("chrA\t%d\t%d\t%d" % (at, at + n, k + 1))
        spans.append((at, at + n))
        at += n + 7
    text = "\n".join(lines) + "\n"
    ga = pa.GenomeArray({"chrA": at + 100}, engine=engine)
    ga.add_from_wiggle(io.StringIO(text), "-")
    assert ga.extents()["chrA"] == {"+": 0, "-": spans[-1][1]}
    host = assert_matches_model(ga, [(text, "-")])
    for strand in ("+", "-"):
        for (a, b) in spans:
            for lo, hi in ((a, b), (a - 1, b + 1), (a + 1, b)):
                seg = pa.GenomicSegment("chrA", lo, hi, strand)
                assert np.array_equal(ga[seg], host[seg]) and len(ga[seg]) == hi - lo
    # before 0, beyond the extent, beyond the length, an unknown contig: zeros where there are no cells
    for seg in (pa.GenomicSegment("chrA", -50, 40, "-"), pa.GenomicSegment("chrA", spans[-1][1] - 10, at + 5000, "-"),
                pa.GenomicSegment("chrA", at + 200, at + 300, "-"), pa.GenomicSegment("chrA", -9, 0, "+")):
        got = ga.get(seg, roi_order=False)
        exp = np.zeros(len(seg))
        vec = host._chroms["chrA"][seg.strand]
        lo, hi = max(seg.start, 0), min(seg.end, len(vec))
        if hi > lo:
            exp[lo - seg.start:hi - seg.start] = vec[lo:hi]
        assert np.array_equal(got, exp)
    assert np.array_equal(ga[pa.GenomicSegment("chrNope", 5, 2100, "+")], np.zeros(2095))
    assert ga.chroms() == ["chrA"] and dict(ga.lengths()) == {"chrA": at + 100}     # a read grows nothing
    ga.close()


def test_batch_of_chains_against_the_host_array(engine):
    rng = np.random.default_rng(11)
    lines = []
    for chrom, n in (("chrA", 9000), ("chrB", 5000)):
        pos = 0
        while pos < n:
            w = int(rng.integers(1, 30))
            if rng.random() < 0.6:
                lines.append("%s\t%d\t%d\t%d" % (chrom, pos, pos + w, int(rng.integers(1, 500))))
            pos += w
    text = "\n".join(lines) + "\n"
    ga = pa.GenomeArray(min_chr_size=12000, engine=engine)
    ga.add_from_wiggle(io.StringIO(text), "+")
    ga.add_from_wiggle(io.StringIO(text.replace("\t", " ")[: len(text) // 2].rsplit("\n", 1)[0] + "\n"), "-")
    host = ga.to_host()
    chains = []
    for k in range(300):
        chrom = ("chrA", "chrB", "chrNope")[k % 3 if k % 50 else 2]
        strand = "+-"[int(rng.integers(0, 2))]
        cuts = np.sort(rng.choice(np.arange(-40, 9500), size=2 * int(rng.integers(1, 5)), replace=False))
        chains.append(pa.SegmentChain(*[pa.GenomicSegment(chrom, int(a), int(b), strand) for a, b in zip(cuts[0::2], cuts[1::2])]))
    chains.append(pa.SegmentChain(pa.GenomicSegment("chrA", 100, 100 + 4097, "-"), pa.GenomicSegment("chrA", 5000, 5000 + 2049, "-")))
    for stranded in (True, False):
        got = ga.get_counts_batch(chains, stranded=stranded)
        for c, g in zip(chains, got):
            exp = c.get_counts(host, stranded) if c.chrom != "chrNope" else np.zeros(c.length)
            assert g.dtype == np.float64 and np.array_equal(g, exp)
    for c in chains[:5] + chains[-1:]:
        assert np.array_equal(c.get_counts(ga), ga.get_counts_batch([c])[0])
    ga.close()


# ------------------------------------------------------------------ round trip through the exporter
def test_round_trip_of_a_staged_bam(engine, tmp_path):
    from tests import bam_writer
    genome, tx, reads, _ = synth.make_config("C2", scale=0.0004, tx_scale=0.004)
    path = str(tmp_path / "reads.bam")
    bam_writer.write_bam(path, list(reads.references), list(reads.lengths), bam_writer.packed_to_records(reads))
    bga = pa.BAMGenomeArray(path, mapping=pa.FivePrimeMapFactory(12))
    ga = pa.GenomeArray(dict(zip(reads.references, (int(x) for x in reads.lengths))), engine=engine)
    for strand in ("+", "-"):
        buf = io.StringIO()
        bga.to_bedgraph(buf, "trk", strand)
        ga.add_from_wiggle(io.StringIO(buf.getvalue()), strand)
        st = ga.import_stats()
        assert st["escaped"] == 0 and st["overlapping"] == 0 and st["yielded"] == st["lines"] - 1
    lengths = bga.lengths()
    chains = [pa.SegmentChain(pa.GenomicSegment(c, 0, int(lengths[c]), s)) for c in bga.chroms() for s in "+-"]
    total = 0.0
    for a, b in zip(ga.get_counts_batch(chains), bga.get_counts_batch(chains)):
        assert np.array_equal(a, b)
        total += float(b.sum())
    assert ga.sum() == total and total > 0
    ga.close()


# ------------------------------------------------------------------ the GPU path really parses
def test_plain_values_never_escape(engine):
    rng = np.random.default_rng(5)
    lines = ["variableStep chrom=chrA"]
    for k in range(3000):
        digits = int(rng.integers(1, 16))
        sig = int(rng.integers(10 ** (digits - 1), 10 ** digits))
        frac = int(rng.integers(0, digits + 1))
        tok = str(sig) if frac == 0 else ("%0*d" % (frac + 1, sig))[:-frac] + "." + ("%0*d" % (frac + 1, sig))[-frac:]
        if k % 7 == 0:
            tok += "e%d" % int(rng.integers(-5, 6))
        lines.append("%d %s%s" % (k + 1, "-" if k % 5 == 0 else "", tok))
    text = "\n".join(lines) + "\n"
    ga = pa.GenomeArray(min_chr_size=5000, engine=engine)
    ga.add_from_wiggle(io.StringIO(text), "+")
    assert ga.import_stats()["escaped"] == 0 and ga.import_stats()["yielded"] == 3000
    assert_matches_model(ga, [(text, "+")])
    ga.close()


def test_mixed_tokens_escape_exactly_as_the_host_says(engine):
    text = ("chrA 1 2 1e23\nchrA 2 3 nan\nchrA 1_0 30 1\nchrA 40 41 0.12345678901234567\nchrA 50 51 1.\nchrA 60 61 7\n"
            "variableStep chrom=chrB\n+5 1e22\n0_7 2\n9 .5\n10 3\n")
    host = pa.read_wiggle(io.StringIO(text))
    ga = pa.GenomeArray(min_chr_size=100, engine=engine)
    ga.add_from_wiggle(io.StringIO(text), "+")
    assert ga.import_stats()["escaped"] == int(host.escaped.sum()) == 7
    assert_matches_model(ga, [(text, "+")])
    ga.close()


def test_overlaps_in_file_order_and_across_calls(engine):
    c = tc.case("overlap_order")
    text = c["adds"][0][0]
    ga = pa.GenomeArray(min_chr_size=400, engine=engine)
    ga.add_from_wiggle(io.StringIO(text), "+")
    assert ga.import_stats()["overlapping"] == overlapping_lines(text) == 11
    # a long cluster: 40 lines over one stretch, sums that depend on the order
    rng = np.random.default_rng(3)
    lines = ["chrL %d %d %s" % (int(a), int(a) + int(rng.integers(1, 5000)), repr(float(v)))
             for a, v in zip(rng.integers(0, 3000, 40), rng.choice([0.1, 0.2, 0.3, 1e16, -1e16, 7.0], 40))]
    text2 = "\n".join(lines) + "\n"
    ga.add_from_wiggle(io.StringIO(text2), "+")
    assert ga.import_stats()["overlapping"] == overlapping_lines(text2)
    assert_matches_model(ga, [(text, "+"), (text2, "+")])
    ga.close()


# ------------------------------------------------------------------ errors
@pytest.mark.parametrize("name", tc.refused_names())
def test_refused_text_same_message_and_nothing_written(engine, name):
    r = tc.refused(name)
    with pytest.raises(ValueError) as host:
        pa.read_wiggle(io.StringIO(r["text"]))
    ga = pa.GenomeArray({"chrA": 100}, min_chr_size=50, engine=engine)
    ga.add_from_wiggle(io.StringIO("chrA 1 5 2\n"), "+")
    with pytest.raises(ValueError) as dev:
        ga.add_from_wiggle(io.StringIO(r["text"]), "+")
    assert str(dev.value) == str(host.value) and ("track line %d: " % r["line"]) in str(dev.value)
    assert ga.chroms() == ["chrA"] and ga.sum() == 8.0 and dict(ga.lengths()) == {"chrA": 100}
    ga.close()


def test_engine_closed_before_its_array():
    """An engine takes its tracks with it: closing the array afterwards touches nothing."""
    from plastid_amd.engine import Engine
    e = Engine(0)
    ga = pa.GenomeArray(min_chr_size=50, engine=e)
    ga.add_from_wiggle(io.StringIO("chrA 1 5 2\n"), "+")
    assert ga.sum() == 8.0
    e.close()
    ga.close()
    own = pa.GenomeArray(min_chr_size=50)      # an engine of its own goes with the array
    own.add_from_wiggle(io.StringIO("chrA 1 5 2\n"), "-")
    assert own[pa.GenomicSegment("chrA", 0, 7, "-")].tolist() == [0, 0, 2, 2, 2, 2, 0]
    own.close()
    own.close()


def test_path_input_and_bad_strand(engine, tmp_path):
    p = tmp_path / "t.wig"
    p.write_bytes(b"fixedStep chrom=chrA start=3 step=2\r\n1\r\n2\r\n3")
    ga = pa.GenomeArray(min_chr_size=20, engine=engine)
    ga.add_from_wiggle(str(p), "-")
    assert ga[pa.GenomicSegment("chrA", 0, 8, "-")].tolist() == [0, 3, 0, 2, 0, 1, 0, 0]
    with pytest.raises(ValueError):
        ga.add_from_wiggle(str(p), ".")
    p.write_bytes(b"chrA 1 2 3\nchrA 1 2 x\n")
    with pytest.raises(ValueError) as e:
        ga.add_from_wiggle(str(p), "+")
    assert str(e.value) == "%s: track line 2: the value is not a number" % p
    ga.close()
