"""The mutable plastid_amd.GenomeArray on the GPU: writes (k_track_set), arithmetic (k_track_op), nonzero, ``==`` and the
bedGraph / variableStep export whose text is formatted by the kernels of csrc/track_kernels.hip.h.  Every case of
tests/golden/track_export_fixture.npz, built by its recorded steps, against the reference's cells, lengths, nonzero and
texts; arrays sized to the kernels' seams (the run-head tile T, the R lines a workgroup formats, every digit-count change
of a coordinate) against the host writers (plastid_amd.track.write_bedgraph, the same line functions, serial); the plain
predicate through export_stats; round trips through add_from_wiggle; seeded writes and arithmetic against numpy."""
import io
import operator
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import plastid_amd as pa  # noqa: E402
from plastid_amd import synth, track  # noqa: E402
from plastid_amd.genome_array import DenseGenomeArray  # noqa: E402
from tests import track_export_cases as xc  # noqa: E402

pytestmark = pytest.mark.gpu

ITEM = 2048   # positions of an item of k_track_gather / k_track_set


@pytest.fixture(scope="module")
def engine():
    from plastid_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def geometry():
    return track.EXPORT_TILE, track.FORMAT_RUNS


def device_texts(ga, strand, **kwargs):
    out = []
    for what in (ga.to_bedgraph, ga.to_variable_step):
        fh = io.StringIO()
        what(fh, "t", strand, **kwargs)
        out.append(fh.getvalue())
    return out


def host_texts(host, strand, **kwargs):
    out = []
    for what in (track.write_bedgraph, track.write_variable_step):
        fh = io.StringIO()
        what(host, fh, "t", strand, **kwargs)
        out.append(fh.getvalue())
    return out


def assert_texts_match_host(ga, strands=("+", "-")):
    host = ga.to_host()
    for st in strands:
        assert device_texts(ga, st) == host_texts(host, st)
    return host


def from_vectors(engine, vectors, lengths=None):
    """An array with `vectors` ({(chrom, strand): cells from position 0}) written through __setitem__."""
    lengths = lengths or {}
    chroms = []
    for c, _ in vectors:
        if c not in chroms:
            chroms.append(c)
    ga = pa.GenomeArray({c: lengths.get(c, max(len(v) for (cc, _), v in vectors.items() if cc == c) + 1) for c in chroms}, min_chr_size=xc.MIN_CHR,
                        engine=engine)
    for (c, st), v in vectors.items():
        v = np.asarray(v, float)
        if len(v):
            ga[pa.GenomicSegment(c, 0, len(v), st)] = v[::-1] if st == "-" else v       # (a vector is 5'->3' of its segment)
    return ga


# ------------------------------------------------------------------ the golden cases
@pytest.mark.parametrize("name", xc.case_names())
def test_golden_case(engine, name):
    c = xc.case(name)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        arrays = xc.replay(c["steps"], lambda lengths: pa.GenomeArray(lengths, min_chr_size=xc.MIN_CHR, engine=engine))
    ga = arrays[c["result"]]
    last = c["steps"][-1]
    if last["op"] == "arith" and isinstance(last["right"], str) and (last["mode"] == "all" or last["how"] == "operator"):
        # (the reference takes the order of its `all` result from a set; here it is the left operand's)
        assert sorted(ga.chroms()) == sorted(c["chroms"]) and ga.chroms() == arrays[last["left"]].chroms()
    else:
        assert ga.chroms() == c["chroms"]
    # (the strand order of the reference's `all` result comes from a set too)
    assert dict(ga.lengths()) == c["lengths"] and sorted(ga.strands()) == sorted(c["strands"]) and list(ga.strands()) == ["+", "-"]
    host = ga.to_host()
    nz = ga.nonzero()
    for ch in c["chroms"]:
        for st in c["strands"]:
            exp = xc.cells(name, ch, st)
            got = host._chroms[ch][st]
            assert got.shape == exp.shape and np.array_equal(got.view(np.uint64), exp.view(np.uint64)), (ch, st)
            assert nz[ch][st].dtype == np.int64 and np.array_equal(nz[ch][st], xc.nonzero(name, ch, st)), (ch, st)
    for st in "+-":
        bed, var = device_texts(ga, st, **xc.KWARGS)
        assert bed.replace("name=t ", "name=%s " % xc.TRACKNAME, 1) == c["bedgraph"][st]
        assert var.replace("name=t ", "name=%s " % xc.TRACKNAME, 1) == c["variable_step"][st]
    for a in arrays.values():
        a.close()


@pytest.mark.parametrize("name", xc.case_names(raised=True))
def test_all_over_differing_contig_sets(engine, name):
    """Where the reference raises (genome_array.py:1789): the behaviour its docstring describes, against a numpy model."""
    c = xc.case(name)
    last = c["steps"][-1]
    arrays = xc.replay(c["steps"][:-1], lambda lengths: pa.GenomeArray(lengths, min_chr_size=xc.MIN_CHR, engine=engine))
    a, b = arrays[last["left"]], arrays[last["right"]]
    r = a.apply_operation(b, xc.FUNCS[last["func"]], mode=last["mode"])
    chroms, strands, cells = xc.combine_model(a.to_host(), b.to_host(), xc.FUNCS[last["func"]], last["mode"])
    assert r.chroms() == chroms and list(r.strands()) == strands
    assert chroms[:len(a.chroms())] == a.chroms() and set(chroms) == set(a.chroms()) | set(b.chroms())
    host = r.to_host()
    for ch in chroms:
        assert r.lengths()[ch] == max(x.lengths().get(ch, 0) for x in (a, b))
        for st in strands:
            assert np.array_equal(host._chroms[ch][st], cells[ch][st])
    for x in (a, b, r):
        x.close()


# ------------------------------------------------------------------ tile borders
def test_tile_borders(engine, geometry):
    T, R = geometry
    vec = {}
    for k, n in enumerate((T - 1, T, T + 1, 3 * T + 5)):
        v = np.zeros(n)
        v[0], v[n - 1] = 2.0, 3.0                     # first and last non-zero at cells 0 and extent - 1
        vec[("ext%d" % k, "+")] = v
    v = np.zeros(3 * T)
    v[T - 1:T + 2] = 4.0                              # a run from cell T - 1 to T + 1, first non-zero at T - 1
    vec[("straddle", "+")] = v
    v = np.zeros(3 * T + 9)
    v[T:3 * T] = 6.0                                  # one run over two whole tiles, first non-zero at T
    v[3 * T + 8] = 1.0
    vec[("two_tiles", "+")] = v
    v = np.zeros(2 * T)
    v[T - 1] = 5.0                                    # first and last non-zero at T - 1
    vec[("at_T_minus_1", "+")] = v
    v = np.zeros(2 * T)
    v[T] = 5.0
    vec[("at_T", "+")] = v
    vec[("alternating", "+")] = np.tile([1.0, 2.0], 2 * R)[:3 * R + 1]           # 3R + 1 runs of alternating values
    ga = from_vectors(engine, vec)
    host = assert_texts_match_host(ga, "+")
    assert np.array_equal(host._chroms["two_tiles"]["+"][:len(vec[("two_tiles", "+")])], vec[("two_tiles", "+")])
    ga.to_bedgraph(io.StringIO(), "t", "+")
    assert ga.export_stats()["runs"] == sum(1 + int(np.count_nonzero(np.diff(np.trim_zeros(v)))) for v in vec.values())
    ga.close()


def test_coordinates_around_every_digit_count_change(engine):
    n = 100010
    v = np.zeros(n)
    for p in (9, 10, 99, 100, 999, 1000, 9999, 10000, 99999, 100000):
        v[p - 1:p + 1] += np.array([1.0, 2.0])        # runs that start and end on both sides of the change
    v[8] = 7.0
    ga = from_vectors(engine, {("chr1", "+"): v, ("chr1", "-"): v[::-1].copy()}, {"chr1": n})
    assert_texts_match_host(ga)
    ga.close()


# ------------------------------------------------------------------ the plain predicate
def test_plain_values_never_reach_the_host(engine):
    rng = np.random.default_rng(11)
    ints = np.where(rng.random(5000) < 0.5, 0.0, rng.integers(-5, 1000, 5000).astype(float))
    ints[17], ints[18], ints[19] = 9999999999999998.0, -0.0, 2.0 ** 53
    halves = np.arange(1, 3001) + 0.5
    mixed = np.array([3.0, 0.5, 1e16, 1e15, 0.1, -2.0, float("inf"), 1e-5, 7.0, 2.0 ** 60])
    ga = from_vectors(engine, {("ints", "+"): ints, ("halves", "-"): halves, ("mixed", "+"): mixed, ("pad", "-"): np.array([1.0])})
    host = ga.to_host()
    for kind, (dev, ref) in enumerate(((ga.to_bedgraph, track.write_bedgraph), (ga.to_variable_step, track.write_variable_step))):
        for st in "+-":
            fh, fr = io.StringIO(), io.StringIO()
            dev(fh, "t", st)
            model = ref(host, fr, "t", st)
            assert fh.getvalue() == fr.getvalue()
            got = ga.export_stats()
            assert got == model
            # '+': the integer track lists nothing, `mixed` exactly what the predicate names (0.5, 1e16, 0.1, 1e-5, 2^60);
            # '-': every k + 0.5 is listed
            assert got["listed"] == (5 if st == "+" else 3000)
            assert got["bytes"] == len(fh.getvalue().split("\n", 1)[1].encode())
    t = ga.export_timing()
    assert set(t) == {"slot_sums", "runs", "listed_values", "lengths", "format", "read_back"} and all(x >= 0 for x in t.values())
    ga.close()


# ------------------------------------------------------------------ round trips
def test_round_trip_through_both_exports(engine):
    rng = np.random.default_rng(3)
    vec = {}
    for c, n in (("chr2", 5000), ("chr10", 2049), ("chrA", 700)):
        for st in "+-":
            bits = rng.integers(0, 2 ** 64, n, dtype=np.uint64).view(np.float64)
            v = np.where(np.isfinite(bits) & (bits != 0), np.abs(bits), 1.0)          # finite, non-zero, positive sums
            v = np.minimum(v, 1e300)
            v[rng.random(n) < 0.3] = 0.0
            v[rng.random(n) < 0.3] = 12.0
            vec[(c, st)] = v
    a = from_vectors(engine, vec, {"chr2": 6000, "chr10": 3000, "chrA": 701})
    ha = a.to_host()
    for what in ("to_bedgraph", "to_variable_step"):
        b = pa.GenomeArray.like(a)
        assert b._engine is a._engine and dict(b.lengths()) == dict(a.lengths())
        for st in "+-":
            fh = io.StringIO()
            getattr(a, what)(fh, "t", st)
            b.add_from_wiggle(io.StringIO(fh.getvalue()), st)
        hb = b.to_host()
        for c in ha.chroms():
            for st in "+-":
                assert np.array_equal(ha._chroms[c][st].view(np.uint64), hb._chroms[c][st].view(np.uint64)), (what, c, st)
        assert a == b
        b.close()
    a.close()


# ------------------------------------------------------------------ writes
def test_seeded_writes_against_numpy(engine):
    rng = np.random.default_rng(21)
    lengths = {"chrA": 3 * ITEM + 100, "chrB": 900}
    ga = pa.GenomeArray(lengths, min_chr_size=xc.MIN_CHR, engine=engine)
    model = {(c, st): np.zeros(n) for c, n in lengths.items() for st in "+-"}
    for k in range(60):
        c = "chrA" if rng.random() < 0.7 else "chrB"
        st = "+-"[int(rng.integers(2))]
        n = lengths[c]
        if k % 3 == 0:
            # a chain of three segments; every fifth one straddles an item border of the set kernel
            cuts = np.sort(rng.choice(np.arange(1, n - 1), 6, replace=False))
            if k % 5 == 0 and c == "chrA":
                cuts = np.array([ITEM - 7, ITEM + 9, 2 * ITEM - 1, 2 * ITEM + 1, 3 * ITEM - 3, 3 * ITEM + 50])
            segs = [(int(cuts[0]), int(cuts[1])), (int(cuts[2]), int(cuts[3])), (int(cuts[4]), int(cuts[5]))]
        else:
            a = int(rng.integers(0, n - 1))
            segs = [(a, int(rng.integers(a + 1, min(n - 1, a + 2 * ITEM + 50) + 1)))]
        total = sum(e - s for s, e in segs)
        roi = pa.SegmentChain(*[pa.GenomicSegment(c, s, e, st) for s, e in segs]) if len(segs) > 1 else pa.GenomicSegment(c, segs[0][0], segs[0][1], st)
        if k % 2:
            val = float(rng.integers(-3, 9))
            for s, e in segs:
                model[(c, st)][s:e] = val
        else:
            val = rng.normal(size=total)
            g = val[::-1] if st == "-" else val          # genome order
            x = 0
            for s, e in segs:
                model[(c, st)][s:e] = g[x:x + e - s]
                x += e - s
        ga[roi] = val
    host = ga.to_host()
    for (c, st), v in model.items():
        assert np.array_equal(host._chroms[c][st], v), (c, st)
        assert np.array_equal(ga[pa.GenomicSegment(c, 0, lengths[c] - 1, st)], v[:-1][::-1] if st == "-" else v[:-1])
    assert dict(ga.lengths()) == lengths and abs(ga.sum() - sum(float(v.sum()) for v in model.values())) <= 1e-12 * sum(float(np.abs(v).sum()) for v in model.values())
    ga.close()


def test_a_wrong_vector_length_changes_nothing(engine):
    ga = pa.GenomeArray({"chrA": 500}, min_chr_size=xc.MIN_CHR, engine=engine)
    ga[pa.GenomicSegment("chrA", 10, 20, "+")] = np.arange(10.0)
    before, total, lengths = ga.to_host(), ga.sum(), dict(ga.lengths())
    chain = pa.SegmentChain(pa.GenomicSegment("chrA", 5, 8, "-"), pa.GenomicSegment("chrA", 30, 900, "-"))
    for roi, val in ((pa.GenomicSegment("chrA", 12, 18, "+"), np.ones(7)), (chain, np.ones(872)), (pa.GenomicSegment("chrNew", 0, 4, "+"), np.ones(3))):
        with pytest.raises(ValueError):
            ga[roi] = val
    after = ga.to_host()
    assert ga.sum() == total and dict(ga.lengths()) == lengths and ga.chroms() == ["chrA"]
    for st in "+-":
        assert np.array_equal(before._chroms["chrA"][st], after._chroms["chrA"][st])
    ga.close()


def test_a_write_invalidates_the_sum_and_warns_when_normalised(engine):
    ga = pa.GenomeArray({"chrA": 100}, min_chr_size=xc.MIN_CHR, engine=engine)
    ga[pa.GenomicSegment("chrA", 0, 10, "+")] = 2.0
    assert ga.sum() == 20.0
    ga.set_normalize(True)
    with pytest.warns(pa.DataWarning):
        ga[pa.GenomicSegment("chrA", 0, 10, "-")] = 1.0
    ga.set_normalize(False)
    assert ga.sum() == 30.0
    # growth and birth by the rule of the import
    ga[pa.GenomicSegment("chrA", 95, 100, "+")] = 1.0
    ga[pa.GenomicSegment("chrB", 5, 6, "-")] = 1.0
    assert dict(ga.lengths()) == {"chrA": 10100, "chrB": xc.MIN_CHR} and ga.extents()["chrA"] == {"+": 100, "-": 10}
    ga.close()


# ------------------------------------------------------------------ arithmetic
@pytest.fixture(scope="module")
def operands(engine):
    rng = np.random.default_rng(8)
    a = pa.GenomeArray({"chrA": 5000, "chrB": 300, "chrC": 50}, min_chr_size=xc.MIN_CHR, engine=engine)
    b = pa.GenomeArray({"chrA": 5000, "chrB": 300, "chrC": 50}, min_chr_size=xc.MIN_CHR, engine=engine)      # a's dimensions, other extents
    c = pa.GenomeArray({"chrA": 2600, "chrB": 700, "chrC": 50}, min_chr_size=xc.MIN_CHR, engine=engine)      # unequal lengths
    for ga, spans in ((a, (("chrA", 0, 4100), ("chrB", 10, 200))), (b, (("chrA", 300, 2300), ("chrB", 0, 299), ("chrC", 3, 9))),
                      (c, (("chrA", 100, 2599), ("chrB", 150, 650)))):
        for ch, s, e in spans:
            for st in "+-":
                if ch == "chrB" and st == "-" and ga is a:
                    continue                                                                                  # (a slot without cells)
                ga[pa.GenomicSegment(ch, s, e, st)] = np.round(rng.normal(size=e - s) * 8) / 4
    yield a, b, c
    for ga in (a, b, c):
        ga.close()


@pytest.mark.parametrize("func", [operator.add, operator.sub, operator.mul])
@pytest.mark.parametrize("mode", ["same", "all", "truncate"])
def test_array_arithmetic_against_numpy(operands, func, mode):
    a, b, c = operands
    other = b if mode == "same" else c
    ha, ho = a.to_host(), other.to_host()
    r = a.apply_operation(other, func, mode=mode)
    chroms, strands, cells = xc.combine_model(ha, ho, func, mode)
    assert r.chroms() == chroms and list(r.strands()) == strands
    hr = r.to_host()
    for ch in chroms:
        assert r.lengths()[ch] == len(cells[ch]["+"])
        for st in strands:
            assert np.array_equal(hr._chroms[ch][st], cells[ch][st]), (ch, st)
    # the operands are unchanged
    for ga, h in ((a, ha), (other, ho)):
        now = ga.to_host()
        assert all(np.array_equal(now._chroms[ch][st], h._chroms[ch][st]) for ch in h.chroms() for st in "+-")
    r.close()


@pytest.mark.parametrize("func", [operator.add, operator.sub, operator.mul])
@pytest.mark.parametrize("mode", ["same", "all", "truncate"])
def test_scalar_arithmetic_against_numpy(operands, func, mode):
    a = operands[0]
    ha = a.to_host()
    r = a.apply_operation(-1.5, func, mode=mode)
    hr = r.to_host()
    assert r.chroms() == a.chroms() and dict(r.lengths()) == dict(a.lengths())
    for ch in a.chroms():
        for st in "+-":
            assert np.array_equal(hr._chroms[ch][st], func(ha._chroms[ch][st], -1.5))
            assert r.extents()[ch][st] == a.lengths()[ch]           # a scalar acts on every cell up to the length
    r.close()


def test_operators_and_refusals(operands):
    a, b, c = operands
    ha, hc = a.to_host(), c.to_host()
    for r, func in ((a + c, operator.add), (a - c, operator.sub), (a * c, operator.mul)):
        _, _, cells = xc.combine_model(ha, hc, func, "all")
        hr = r.to_host()
        assert all(np.array_equal(hr._chroms[ch][st], cells[ch][st]) for ch in cells for st in "+-")
        r.close()
    with pytest.raises(AssertionError):
        a.apply_operation(c, operator.add, mode="same")
    with pytest.raises(TypeError):
        a.apply_operation(b, lambda x, y: x + y)
    with pytest.raises(TypeError):
        a.apply_operation(2.0, np.maximum)
    with pytest.raises(ValueError):
        a.apply_operation(b, operator.add, mode="some")
    other = pa.GenomeArray({"chrA": 5000}, min_chr_size=xc.MIN_CHR)      # an engine of its own
    with pytest.raises(ValueError):
        a + other
    with pytest.raises(ValueError):
        a == other
    other.close()


# ------------------------------------------------------------------ equality
def test_equality(engine):
    def make(length, edits=()):
        ga = pa.GenomeArray({"chrA": length, "chrB": 40}, min_chr_size=xc.MIN_CHR, engine=engine)
        ga[pa.GenomicSegment("chrA", 5, 10, "+")] = np.array([1.0, 2.0, 3.0, 4.0, 5.0])
        ga[pa.GenomicSegment("chrA", 50, 53, "-")] = np.array([1.0, 2.0, 3.0])
        for pos, v in edits:
            ga[pa.GenomicSegment("chrA", pos, pos + 1, "+")] = v
        return ga
    a, longer = make(100), make(3000)
    assert a == longer and longer == a and not (a != longer)                       # lengths need not be equal
    close_up, close_down = make(100, [(7, 3.0 + 1e-11)]), make(100, [(7, 3.0 - 1e-11)])
    assert a == close_up and close_up == a and a == close_down and close_down == a
    far_up, far_down = make(100, [(7, 3.0 + 1e-9)]), make(100, [(7, 3.0 - 1e-9)])
    # (the reference's one-sided test, self - other <= tol, calls a == far_up equal)
    assert a != far_up and far_up != a and a != far_down and far_down != a
    last = make(100, [(9, 5.5)])                                                   # the last non-zero position alone
    assert a != last and last != a
    # what the reference computes for that pair: its segment ends at max(), so position 9 is never compared
    idx = np.arange(5, 10)
    assert ((np.array([1.0, 2.0, 3.0, 4.0, 5.0]) - np.array([1.0, 2.0, 3.0, 4.0, 5.5]))[:idx.max() - idx.min()] <= 1e-10).all()
    assert a != make(100, [(20, 1.0)]) and a != make(100, [(7, 0.0)])               # other index sets
    assert a.__eq__(far_up, tol=1e-8)
    extra = make(100)
    extra[pa.GenomicSegment("chrZ", 0, 3, "+")] = 0.0                               # a contig of zeros changes nothing
    assert a == extra and extra == a
    extra[pa.GenomicSegment("chrZ", 1, 2, "-")] = float("nan")                      # NaN is non-zero
    assert a != extra


# ------------------------------------------------------------------ BAMGenomeArray.to_genome_array
def test_to_genome_array_of_a_staged_bam(tmp_path):
    from tests import bam_writer
    genome, tx, reads, _ = synth.make_config("C2", scale=0.0004, tx_scale=0.004)
    path = str(tmp_path / "reads.bam")
    bam_writer.write_bam(path, list(reads.references), list(reads.lengths), bam_writer.packed_to_records(reads))
    bga = pa.BAMGenomeArray(path, mapping=pa.FivePrimeMapFactory(12))
    dense = bga.to_genome_array()
    ga = bga.to_genome_array(array_type=pa.GenomeArray)
    assert isinstance(dense, DenseGenomeArray) and isinstance(ga, pa.GenomeArray)
    assert ga.chroms() == dense.chroms() and dict(ga.lengths()) == dict(dense.lengths())
    host = ga.to_host()
    total = 0.0
    assert ga.strands() == dense.strands()
    for c in dense.chroms():
        for st in dense.strands():
            assert np.array_equal(host._chroms[c][st], dense._chroms[c][st])
            total += float(dense._chroms[c][st].sum())
    assert total > 0 and ga.sum() == total
    back = pa.GenomeArray.like(ga)
    for st in "+-":
        fh = io.StringIO()
        ga.to_bedgraph(fh, "trk", st)
        assert ga.export_stats()["listed"] == 0
        back.add_from_wiggle(io.StringIO(fh.getvalue()), st)
    lengths = bga.lengths()
    chains = [pa.SegmentChain(pa.GenomicSegment(c, 0, int(lengths[c]) - 1, s)) for c in bga.chroms() for s in "+-"]
    for x, y in zip(back.get_counts_batch(chains), bga.get_counts_batch(chains)):
        assert np.array_equal(x, y)
    back.close()
    ga.close()
