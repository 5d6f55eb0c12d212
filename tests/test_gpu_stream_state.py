"""The two derived streams of a staged file across the life of ONE engine: the compact stream (rebuilt behind every rewrite
of the stream words) and the canonical stream (built at the first count of an eligible plan, kept under a signature).
tests/test_gpu_compact_stream.py and tests/test_gpu_canonical_stream.py build a fresh engine per case; here the engine
lives on while rules, filters, flags, files and knobs change under two open plans, and every count is the oracle's, every
``stream_entries`` / ``canonical_entries`` the number tests/stream_models.py predicts.  The steps are those of
tests/stateful_cases.py, so a failure prints a trace that ``run_sequence`` replays (docs/stateful_fuzz.md).
Needs a real MI355X: ``pytest -m gpu``."""
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import stateful_cases as sc  # noqa: E402
import stream_models as sm  # noqa: E402

pytestmark = pytest.mark.gpu

A, D, B = 0, 1, 2            # plan ids: `stranded`, `stranded_dot`, a second `stranded` (and 3: a third)
F1 = (0, 0x100, 10)


@pytest.fixture(scope="module")
def env():
    import plastid_amd as pa
    from oracle import oracle
    return pa, oracle


def table_world(pa):
    """A stream world (stateful_cases.stream_world): pool files `dups`, `ends`, `one_length`, `other_range`."""
    return sc.stream_world(np.random.default_rng(4343), pa, 4343)


# ------------------------------------------------------------------------------------------ every ordered pair of transitions
def _knobs(knobs, **change):
    out = dict(knobs)
    for k, v in change.items():
        if v is None:
            out.pop(k, None)
        else:
            out[k] = v
    return out


#: name -> (apply, undo): functions of (world, knobs in force, 0 for the pair's first transition and 1 for its second) that
#: return the steps and the knobs in force afterwards
TRANSITIONS = {
    "rule": (lambda w, k, slot: ([("set_mapping", ("threeprime", 3))], k), lambda w, k, slot: ([("set_mapping", w["mapping0"])], k)),
    "center and back": (lambda w, k, slot: ([("set_mapping", ("center", 2)), ("canonical_entries", A), ("set_mapping", ("variable", ((28, 12), (30, 14), ("default", 13))))], k),
                        lambda w, k, slot: ([("set_mapping", w["mapping0"])], k)),
    # (set, counted, then CHANGED: the signature of the canonical stream must hold the bounds, not only "a filter is on")
    "size filter": (lambda w, k, slot: ([("set_size_filter", (26, 34)), ("canonical_entries", A), ("set_size_filter", (24, 30))], k),
                    lambda w, k, slot: ([("set_size_filter", None)], k)),
    "update_flags": (lambda w, k, slot: ([("update_flags", 0, 311, 30)], k), lambda w, k, slot: ([("update_flags", 0, 311, 0)], k)),
    "FLAG filter": (lambda w, k, slot: ([("set_flag_filter", F1)], k), lambda w, k, slot: ([("set_flag_filter", None)], k)),
    "late NH column": (lambda w, k, slot: ([("set_nh_filter", 2), ("set_alignments", ((0, True, False),)), ("canonical_entries", A), ("set_alignment_nh", 0)], k),
                       lambda w, k, slot: ([("set_nh_filter", 0)], k)),
    "second file": (lambda w, k, slot: ([("add_file", 1, True, True)], k), lambda w, k, slot: ([("set_alignments", ((0, True, True),))], k)),
    "other file": (lambda w, k, slot: ([("set_alignments", ((3, True, True),))], k), lambda w, k, slot: ([("set_alignments", ((0, True, True),))], k)),
    "PC_NO_CANON": (lambda w, k, slot: ([("reload_knobs", _knobs(k, PC_NO_CANON="1"))], _knobs(k, PC_NO_CANON="1")),
                    lambda w, k, slot: ([("reload_knobs", _knobs(k, PC_NO_CANON=None))], _knobs(k, PC_NO_CANON=None))),
    "PC_NO_COMPACT, re-filter": (lambda w, k, slot: ([("reload_knobs", _knobs(k, PC_NO_COMPACT="1")), ("update_flags", 0, 977, 10)], _knobs(k, PC_NO_COMPACT="1")),
                                 lambda w, k, slot: ([("reload_knobs", _knobs(k, PC_NO_COMPACT=None)), ("update_flags", 0, 977, 0)], _knobs(k, PC_NO_COMPACT=None))),
    "PC_COMPACT_KEEP, re-filter": (lambda w, k, slot: ([("reload_knobs", _knobs(k, PC_COMPACT_KEEP="0.5")), ("update_flags", 0, 613, 10)], _knobs(k, PC_COMPACT_KEEP="0.5")),
                                   lambda w, k, slot: ([("reload_knobs", _knobs(k, PC_COMPACT_KEEP=None)), ("update_flags", 0, 613, 0)], _knobs(k, PC_COMPACT_KEEP=None))),
    "second stranded plan": (lambda w, k, slot: ([("open_plan", B + slot, sc.SET_STRANDED), ("canonical_entries", B + slot), ("canonical_entries", A), ("canonical_entries", B + slot)], k),
                             lambda w, k, slot: ([("close_plan", B + slot)], k)),
}
PAIRS = list(itertools.product(sorted(TRANSITIONS), repeat=2))
COUNTS = [("canonical_entries", A), ("canonical_entries", D), ("canonical_entries", A), ("stream_entries", 0)]   # (the '.' twin in between, always)


def pair_steps(world, first, second):
    """Apply `first`, apply `second`, undo `second`, undo `first`; both plans are counted and both entry numbers read
    after each of the four."""
    steps = [("add_file", 0, True, True), ("open_plan", A, sc.SET_STRANDED), ("open_plan", D, sc.SET_DOT)] + COUNTS
    knobs = {}
    for name, way, slot in ((first, 0, 0), (second, 0, 1), (second, 1, 1), (first, 1, 0)):
        more, knobs = TRANSITIONS[name][way](world, knobs, slot)
        steps += more + COUNTS
    return steps


@pytest.fixture(scope="module")
def world(env):
    return table_world(env[0])


@pytest.mark.parametrize("first,second", PAIRS, ids=[" / ".join(p) for p in PAIRS])
def test_every_ordered_pair_of_transitions(env, world, first, second):
    """The whole table (12 x 12), nothing cut: one engine, pool file `dups`, plans `stranded` and `stranded_dot` open."""
    pa, oracle = env
    sc.run_sequence(pa, oracle, dict(seed=4343, world=world, steps=pair_steps(world, first, second)))


# ------------------------------------------------------------------------------------------ the weigh-in against the compact stream
def ungapped(pa, rows, names, lens):
    """rows: (pos, L, reverse, copies) on contig 0, sorted by position."""
    rows = sorted(rows, key=lambda r: r[0])
    pos = np.concatenate([np.full(r[3], r[0], np.int64) for r in rows])
    alen = np.concatenate([np.full(r[3], r[1], np.int64) for r in rows])
    rev = np.concatenate([np.full(r[3], bool(r[2])) for r in rows])
    return pa.PackedAlignments.from_ungapped(0, pos, alen, rev, references=names, lengths=lens)


def plain_world(pa, files, names, lens, segments, mapping0):
    """A world for ``run_sequence`` from hand-made files and '+' / '-' segments (segment set 0; set 1 is one '.' window)."""
    pool = []
    for f in files:
        flag16 = np.where(f.flags & 1, 16, 0).astype(np.uint16)
        mapq, nh = np.full(f.n, 30, np.uint8), np.ones(f.n, np.uint16)
        pool.append(dict(file=f, flag16=flag16, mapq=mapq, nh=nh, full=sc._with_columns(pa, f, flag16, mapq, nh)))
    ns = len(segments)
    stranded = dict(name="stranded", tid=np.array([s[0] for s in segments], np.int32), start=np.array([s[1] for s in segments], np.int64),
                    end=np.array([s[2] for s in segments], np.int64), strand=np.array([s[3] for s in segments], np.uint8), layout="forward",
                    step=np.ones(ns, np.int8), several_windows=True)
    single = dict(name="single", tid=np.zeros(1, np.int32), start=np.array([0], np.int64), end=np.array([200], np.int64),
                  strand=np.array([3], np.uint8), layout="forward", step=np.ones(1, np.int8))
    return dict(seed=0, names=names, lens=lens, pool=pool, segsets=[stranded, single], strat=(25, 30), big=False, stream=True, mapping0=mapping0)


WEIGH_NAMES, WEIGH_LENS = ["w", "far"], [30000, 5000]
WEIGH_SEGMENTS = [(0, 0, 30000, 1), (0, 0, 30000, 2), (0, 5000, 5200, 1), (1, 0, 5000, 2)]


def weigh_in_files(pa):
    """`merges`: 300 sites, three lengths with a common start, three copies each -- 901 compact entries of 2 700 records
    (900 groups, one of them cut by the edge of a compaction tile), 300 canonical ones under fiveprime(12).  `same`: 300
    sites of one length and 20 of two, three copies each -- 340 compact entries of 1 020 records and 320 canonical ones:
    more than 0.9 x 340, less than 0.9 x 1 020."""
    merges = ungapped(pa, [(100 + 90 * s, L, 0, 3) for s in range(300) for L in (26, 30, 34)], WEIGH_NAMES, WEIGH_LENS)
    same = ungapped(pa, [(100 + 90 * s, 30, 0, 3) for s in range(300)] + [(140 + 90 * s, L, 0, 3) for s in range(20) for L in (27, 33)],
                    WEIGH_NAMES, WEIGH_LENS)
    return merges, same


def test_weigh_in_against_the_compact_stream(env):
    """The canonical stream is weighed against the stream it replaces -- the compact one where the file keeps one: built at
    no more than 0.9 of it, not built between 0.9 x compact and 0.9 x records (the counts are the oracle's all the same),
    and built with the same entries against the records when PC_NO_COMPACT has kept the compact stream away."""
    pa, oracle = env
    merges, same = weigh_in_files(pa)
    rule = ("fiveprime", 12)
    none = np.zeros(merges.n, bool)
    # (conditions on the fixtures)
    assert sm.compact_prediction(merges, none) == 901 and sm.model_entries(merges, merges.flags, rule) == 300 <= 0.9 * 901
    cn, kn = sm.compact_prediction(same, np.zeros(same.n, bool)), sm.model_entries(same, same.flags, rule)
    assert cn == 340 and kn == 320 and 0.9 * cn < kn <= 0.9 * same.n
    world = plain_world(pa, [merges, same], WEIGH_NAMES, WEIGH_LENS, WEIGH_SEGMENTS, rule)
    steps = [("add_file", 0, True, True), ("open_plan", 0, 0), ("canonical_entries", 0), ("stream_entries", 0), ("count_twice", 0, "int64"),
             ("set_alignments", ((1, True, True),)), ("canonical_entries", 0), ("stream_entries", 0), ("count_twice", 0, "int64"),
             ("reload_knobs", {"PC_NO_COMPACT": "1"}), ("set_alignments", ((0, True, True),)), ("canonical_entries", 0), ("stream_entries", 0),
             ("reload_knobs", {}), ("canonical_entries", 0), ("stream_entries", 0)]
    seq = dict(seed=0, world=world, steps=steps)
    walk = list(sc.model_walk(oracle, seq, streams=True))
    assert [w[4] for w in walk if w[1][0] == "canonical_entries"] == [(("built", 300), 300), (("none", "weigh-in"), -1), (("built", 300), 300),
                                                                       (("built", 300), 300)]
    assert [int(w[3][0]) for w in walk if w[1][0] == "stream_entries"] == [901, 340, 2700, 2700]
    sc.run_sequence(pa, oracle, seq)


# ------------------------------------------------------------------------------------------ one engine, one plan, other files
def test_engine_reuse_across_files(env, world):
    """A plan opened and counted on `ends` (the stream is built: the file's first), then ``set_alignments`` to
    `other_range` -- same contigs, other reads, another range of aligned lengths -- and back: the same plan object each
    time, on a new staged file whose stream numbering starts over."""
    pa, oracle = env
    ends, other = world["pool"][1]["file"], world["pool"][3]["file"]
    assert sm.stream_ranges(ends) != sm.stream_ranges(other)
    steps = [("add_file", 1, True, True), ("open_plan", A, sc.SET_STRANDED), ("canonical_entries", A), ("stream_entries", 0),
             ("set_alignments", ((3, True, True),)), ("canonical_entries", A), ("stream_entries", 0),
             ("set_alignments", ((1, True, True),)), ("canonical_entries", A), ("count_twice", A, "int64")]
    seq = dict(seed=4343, world=world, steps=steps)
    built = [canon[0] for at, step, why, exp, canon, m in sc.model_walk(oracle, seq, streams=True) if canon is not None]
    assert [b[0] for b in built] == ["built"] * 4 and built[0] == built[2] == built[3] != built[1], built
    sc.run_sequence(pa, oracle, seq)


# ------------------------------------------------------------------------------------------ files staged by the GPU decoder
BAM_NAMES, BAM_LENS = ["chrA", "chrEmpty", "chrB"], [40000, 2000, 9000]
BAM_RULES = [("fiveprime", 12), ("threeprime", 3), ("variable", {26: 12, 27: 12, 28: 13, 30: 14, 31: 13, 33: 12, "default": 13})]
BAM_SEGMENTS = [(t, a, e, st) for (t, a, e) in [(0, 0, 40000), (0, 0, 5), (0, 120, 136), (0, 20000, 20100), (0, 39950, 40000), (1, 0, 2000), (2, 0, 9000),
                                               (2, 4000, 4100)] for st in (1, 2)]
PILE = 20040                                        # a pile of reads on chrA that the regions cut in two
BAM_REGIONS = [("chrA", 100, PILE + 10), ("chrA", PILE + 300, 30000), ("chrB", 3900, 4500)]


def bam_reads(pa):
    """About 3 000 reads of 20 .. 44 nt: sites with common starts and common ends on both strands (the canonical stream
    merges them), exact duplicates (the compact stream), a pile, a few two-run reads, the first and last positions."""
    rng = np.random.default_rng(77)
    reads = []         # (tid, reverse, runs)
    for t, n, ln in ((0, 170, 40000), (2, 50, 9000)):
        for a in rng.integers(50, ln - 100, n):
            for rev in (0, 1):
                for L in rng.choice(np.arange(20, 45), 3, replace=False):
                    reads += [(t, bool(rev), [(int(a), int(L))])] * int(rng.integers(2, 4))
                    reads.append((t, bool(rev), [(int(a) + 45 - int(L), int(L))]))
    for c in range(200):
        reads.append((0, bool(c & 1), [(PILE - 20 + (c * 7) % 41, 22 + (c * 5) % 20)]))
    for c in range(10):
        reads.append((0, bool(c & 1), [(10000 + 11 * c, 14), (10000 + 11 * c + 25, 15)]))
    for L in (20, 30, 44):
        reads += [(0, False, [(0, L)]), (0, True, [(0, L)]), (0, False, [(40000 - L, L)]), (2, True, [(9000 - L, L)])]
    return pa.PackedAlignments.from_runs([r[0] for r in reads], [r[1] for r in reads], [r[2] for r in reads], references=BAM_NAMES,
                                         lengths=BAM_LENS, sort=True)


def test_canonical_stream_on_gpu_staged_files(env, tmp_path):
    """One coordinate-sorted BAM file and its shuffled twin, staged on the host, by ``Engine.add_bam`` (whole file, regions
    that cut a pile in two, ``sort=True`` on the twin): the GPU stager writes the stream words and the linear index with
    other kernels than the host path.  Under three point rules a `stranded` plan gives the oracle's counts four times, and
    ``canonical_entries`` is the model's on the records the host readers return; once more after ``update_flags``."""
    pa, oracle = env
    from plastid_amd.bam import read_bam
    from plastid_amd.engine import Engine
    from plastid_amd.packing import concat_file_major
    from tests import bam_writer
    from test_gpu_canonical_stream import configure, make_plan, seg_arrays, spec_for
    reads = bam_reads(pa)
    recs = bam_writer.packed_to_records(reads)
    path, twin = str(tmp_path / "sorted.bam"), str(tmp_path / "shuffled.bam")
    bam_writer.write_bam(path, BAM_NAMES, BAM_LENS, recs, block_bytes=20000, index=True)
    order = np.random.default_rng(78).permutation(len(recs))
    bam_writer.write_bam(twin, BAM_NAMES, BAM_LENS, [recs[i] for i in order], block_bytes=20000, header_text="@HD\tVN:1.6\tSO:unsorted\n")
    whole, part = read_bam(path), read_bam(path, regions=BAM_REGIONS)
    resorted = read_bam(twin, sort=True)       # (the twin's order within a position: it decides which groups a compaction tile's edge cuts)
    assert resorted.n == whole.n and np.array_equal(resorted.pos, whole.pos) and np.array_equal(resorted.tid, whole.tid)
    assert whole.n == reads.n and 0.3 * whole.n < part.n < whole.n and sm.certain_halo(whole)
    pile = (whole.tid == 0) & (whole.pos >= PILE - 20) & (whole.pos <= PILE + 20)
    in_part = (part.tid == 0) & (part.pos >= PILE - 20) & (part.pos <= PILE + 20)
    assert 0 < in_part.sum() < pile.sum()                                     # (the regions cut the pile)
    ways = [("host", whole, lambda e: e.set_alignments([whole])), ("add_bam", whole, lambda e: e.add_bam(path)),
            ("regions", part, lambda e: e.add_bam(path, regions=BAM_REGIONS)), ("sort=True", resorted, lambda e: e.add_bam(twin, sort=True))]
    tid, start, end, strand = seg_arrays(BAM_SEGMENTS)
    expected = {}

    def check(eng, plan, f, flags, mapping, what):
        key = (id(f), flags.tobytes(), repr(mapping))
        if key not in expected:
            kept = f.subset(np.nonzero((flags & 0x80) == 0)[0])
            arrays, _ = oracle.count_segments(concat_file_major([kept]), spec_for(oracle, mapping), tid, start, end, strand)
            entries, compact = sm.model_entries(f, flags, mapping), sm.compact_prediction(f, (flags & 0x80) != 0)
            assert 0 < entries <= 0.9 * (f.n if compact is None else compact), "the fixture must make the canonical stream worth building"
            expected[key] = (np.concatenate([np.asarray(a).reshape(-1) for a in arrays]), entries, f.n if compact is None else compact)
        exp, entries, compact = expected[key]
        got = plan.count(np.int64)
        assert got.dtype == np.int64 and np.array_equal(got, exp), (what, sc.first_difference(got, exp))
        assert eng.stream_entries(0) == compact, (what, eng.stream_entries(0), compact)
        assert eng.canonical_entries(0) == entries, (what, eng.canonical_entries(0), entries)

    for name, f, stage in ways:
        eng = Engine(0)
        plan = None
        try:
            stage(eng)
            assert eng.num_records(0) == f.n, name
            configure(eng, BAM_RULES[0])
            plan = make_plan(eng, BAM_SEGMENTS)
            for mapping in BAM_RULES:
                configure(eng, mapping)
                check(eng, plan, f, f.flags, mapping, (name, mapping[0]))
            third = f.flags.copy()
            third[::3] |= 0x80
            eng.update_flags(0, third)
            check(eng, plan, f, third, BAM_RULES[2], (name, "update_flags"))
        finally:
            if plan is not None:       # (before its engine: a plan outliving a closed engine is destroyed into freed memory)
                plan.close()
            eng.close()
