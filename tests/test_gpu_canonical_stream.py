"""The canonical stream: under a point rule (fiveprime, threeprime, variable) and a size filter, a plan over ONE file
whose segments are '+' / '-' only streams one entry per (contig, strand, MAPPED position) -- up to 16 reads per entry --
instead of one per (position, aligned length, strand).  Every count must stay what the oracle says and what the same
engine gives under ``PC_NO_CANON=1``; ``Engine.canonical_entries`` must agree with a numpy model of the grouping, change
when the rule, the filter or the flags change, and say -1 where a plan is not eligible.  Needs a real MI355X:
``pytest -m gpu``.

The fixture is one contig of 70 000 positions, an empty contig and a short one, about 5 000 reads.  Two facts shape it:
* the stream is used only when it has at most 90 % of the entries of the stream it replaces, so every anchor carries
  reads that share a 5' end (they merge under fiveprime / variable) and reads that share a 3' end (threeprime);
* reads whose span lies beyond the 99.5 % quantile of all spans leave the record stream for the long-read lists, so the
  sixty reads of 250 aligned positions (the variable rule with offsets 0 and 200: shifts beyond one 128-nt bucket) all
  have the same length."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stream_models import model_entries  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES, LENS = ["long", "empty", "short"], [70000, 1000, 300]
EXCLUDED = 0x80
CAP = 16
VAR_MISSING = {26: 12, 27: 12, 28: 13, 30: 14, 31: 13, 33: 12, 36: 15, 40: 12}    # no default: other lengths are not mapped
VAR_FAR = {25: 0, 30: 3, 250: 200}                                                 # largest shift 200: two buckets back
RULES = [("fiveprime", 0), ("fiveprime", 12), ("threeprime", 3), ("variable", VAR_MISSING), ("variable", VAR_FAR)]
RULE_IDS = ["fiveprime0", "fiveprime12", "threeprime3", "variable_missing", "variable_far"]
STRATIFIED = ("stratified", {26: 12, 27: 12, 28: 13, 29: 13, 30: 14, 31: 13, "default": 13}, 25, 35)
# '+' (1) and '-' (2) over: the whole contig, its first and last positions, both sides of a bucket edge, 65 535 / 65 536,
# the piles, the contig without reads and the short one
SPANS = [(0, 0, 70000), (0, 0, 3), (0, 100, 140), (0, 120, 130), (0, 65500, 65560), (0, 29990, 30110), (0, 69950, 70000),
         (1, 0, 1000), (2, 0, 300), (2, 250, 300)]
SEGMENTS = [(t, a, e, st) for (t, a, e) in SPANS for st in (1, 2)]


@pytest.fixture(scope="module")
def pa():
    import plastid_amd
    return plastid_amd


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as o
    o.lib()
    return o


def build_reads(pa):
    rng = np.random.default_rng(20240607)
    reads = []   # (tid, reverse, runs)

    def one(tid, pos, L, rev, copies=1):
        for _ in range(copies):
            reads.append((tid, bool(rev), [(int(pos), int(L))]))

    # anchors: per strand four reads with a common start and four with a common end, lengths all different
    anchors = np.unique(np.concatenate([rng.integers(200, 69700, 230), [65480, 65500, 65520, 65535, 65536]]))
    for a in anchors:
        for rev in (0, 1):
            for L in rng.choice(np.arange(20, 41), 4, replace=False):
                one(0, a, L, rev)
            for L in rng.choice(np.arange(20, 41), 4, replace=False):
                one(0, a + 45 - L, L, rev)
    # the first positions of the contig and its last ones
    for p in (0, 1, 2):
        for L in (20, 27, 33, 40):
            one(0, p, L, 0)
            one(0, p, L, 1)
    for L in range(20, 41, 3):
        one(0, 70000 - L, L, 0)
        one(0, 70000 - L, L, 1)
        one(0, 70000 - L - 1, L, L & 1)
    # every length on both strands around a bucket edge (positions 100 .. 130) and around 65 535 / 65 536
    for p in list(range(100, 131, 2)) + list(range(65505, 65540, 3)):
        for L in range(20, 41, 5):
            one(0, p, L, (p + L) & 1)
    for p in (126, 127, 128):
        for L in (26, 27, 28, 30, 31):
            one(0, p, L, 0)
            one(0, p, L, 1)
    # 15, 16, 17 and 300 reads of mixed lengths in one bin: common start (fiveprime: forward; threeprime: reverse) and common end
    for base, copies in ((30000, 15), (30020, 16), (30040, 17), (30060, 300)):
        for c in range(copies):
            L = 20 + (c * 7) % 21
            one(0, base, L, c & 1)
            one(0, base + 45 - L, L, (c >> 1) & 1)
    # lengths the rules do not map (L <= offset), and the long ones of VAR_FAR
    for L in (2, 3, 5, 10, 12, 13):
        one(0, 40000, L, 0, 2)
        one(0, 40000 + L, L, 1, 2)
    for c in range(60):
        one(0, 50000 + 37 * (c // 6), 250, c & 1)
    one(0, 50000, 25, 0, 3)
    one(0, 50170, 25, 1, 3)
    # two-run reads (binned from the run stream, never from the canonical one)
    for c in range(12):
        reads.append((0, bool(c & 1), [(20000 + 9 * c, 14), (20000 + 9 * c + 30, 15)]))
    # the short contig
    for p in (0, 5, 250, 262, 270):
        for L in (22, 30, 38):
            one(2, p, min(L, 300 - p), 0)
            one(2, p, min(L, 300 - p), 1)
    f = pa.PackedAlignments.from_runs([r[0] for r in reads], [r[1] for r in reads], [r[2] for r in reads], references=NAMES,
                                      lengths=LENS, sort=True)
    flags = f.flags.copy()
    flags[rng.choice(f.n, 40, replace=False)] |= EXCLUDED
    return f, flags


@pytest.fixture(scope="module")
def data(pa):
    f, flags = build_reads(pa)
    assert 4500 <= f.n <= 6000 and int((f.nblk >= 2).sum()) == 12
    return f, flags


def with_flags(f, flags):
    """What the oracle is given for `f` under the caller's `flags`: excluded records are absent from its input."""
    return f.subset(np.nonzero((flags & EXCLUDED) == 0)[0])


def spec_for(oracle, mapping, size_filter=None):
    kind = mapping[0]
    if kind in ("fiveprime", "threeprime"):
        return oracle.mapping_spec(kind, mapping[1], size_filter=size_filter)
    if kind == "variable":
        return oracle.mapping_spec(kind, 0, mapping[1], size_filter=size_filter)
    return oracle.mapping_spec(kind, 0, mapping[1], mapping[2], mapping[3], size_filter=size_filter)


def seg_arrays(segments):
    return (np.array([s[0] for s in segments], np.int32), np.array([s[1] for s in segments], np.int64),
            np.array([s[2] for s in segments], np.int64), np.array([s[3] for s in segments], np.uint8))


_EXPECTED = {}


def expected(oracle, files, mapping, size_filter, segments, key):
    """The oracle's counts in the plan's layout; computed once per `key` and shared."""
    if key not in _EXPECTED:
        from plastid_amd.packing import concat_file_major
        tid, start, end, strand = seg_arrays(segments)
        arrays, _ = oracle.count_segments(concat_file_major(files), spec_for(oracle, mapping, size_filter), tid, start, end, strand)
        exp = np.concatenate([np.asarray(a).reshape(-1) for a in arrays])
        exp.setflags(write=False)
        _EXPECTED[key] = exp
    return _EXPECTED[key]


def make_plan(eng, segments):
    tid, start, end, strand = seg_arrays(segments)
    lens = end - start
    rows = eng.rows
    out_off = np.concatenate([[0], np.cumsum(lens * rows)[:-1]])
    return eng.plan(tid, start, end, strand, out_off, np.ones(len(lens), np.int8), lens, int((lens * rows).sum()), rows)


def configure(eng, mapping, size_filter=None):
    from plastid_amd import synth
    synth.mapping_factory(mapping)._configure(eng)
    if size_filter:
        eng.set_size_filter(*size_filter)
    else:
        eng.set_size_filter(None)


def staged(files, flags=None):
    from plastid_amd.engine import Engine
    eng = Engine(0)
    eng.set_alignments(files)
    if flags is not None:
        eng.update_flags(0, flags)
    return eng


def forbid(eng, monkeypatch, on):
    if on:
        monkeypatch.setenv("PC_NO_CANON", "1")
    else:
        monkeypatch.delenv("PC_NO_CANON", raising=False)
    eng.reload_knobs()


def count_both_ways(eng, monkeypatch, segments, exp, what):
    """One plan counted with the canonical stream allowed, then forbidden: both equal `exp`.  Returns the entries the
    engine reported while it was allowed."""
    plan = make_plan(eng, segments)
    try:
        got = plan.count(np.int64)
        entries = eng.canonical_entries(0)
        assert got.dtype == np.int64 and np.array_equal(got, exp), what
        forbid(eng, monkeypatch, True)
        assert eng.canonical_entries(0) == -1
        assert np.array_equal(plan.count(np.int64), exp), (what, "PC_NO_CANON")
    finally:
        forbid(eng, monkeypatch, False)
        plan.close()
    return entries


@pytest.fixture(scope="module")
def engine(data):
    f, flags = data
    eng = staged([f], flags)
    yield eng
    eng.close()


@pytest.mark.parametrize("mapping", RULES, ids=RULE_IDS)
def test_rules(pa, oracle, data, engine, monkeypatch, mapping):
    f, flags = data
    configure(engine, mapping)
    exp = expected(oracle, [with_flags(f, flags)], mapping, None, SEGMENTS, ("base", RULE_IDS[RULES.index(mapping)]))
    model = model_entries(f, flags, mapping)
    assert 0 < model <= 0.9 * engine.stream_entries(0), "the fixture must make the canonical stream worth building"
    assert count_both_ways(engine, monkeypatch, SEGMENTS, exp, mapping[0]) == model
    assert engine.canonical_entries(0) == model   # (allowed again: the stream is still the file's)


def test_one_plan_through_rule_filter_and_flag_changes(pa, oracle, data, monkeypatch):
    """The same plan is counted after every change; no knob is touched in between, so only the signature of the
    canonical stream can make the engine rebuild the stream and the plan's work lists."""
    f, flags = data
    third = flags.copy()
    third[::3] |= EXCLUDED
    steps = [(("fiveprime", 12), None, flags), (("fiveprime", 12), (25, 30), flags), (("fiveprime", 12), None, flags),
             (("threeprime", 3), None, flags), (("threeprime", 3), None, third)]
    eng = staged([f], flags)
    try:
        outs = {}
        for allowed in (True, False):
            forbid(eng, monkeypatch, not allowed)
            eng.update_flags(0, flags)
            configure(eng, steps[0][0])
            plan = make_plan(eng, SEGMENTS)
            entries = []
            for i, (mapping, size_filter, fl) in enumerate(steps):
                if i == 4:
                    eng.update_flags(0, fl)
                configure(eng, mapping, size_filter)
                exp = expected(oracle, [with_flags(f, fl)], mapping, size_filter, SEGMENTS, ("steps", i))
                got = plan.count(np.int64)
                assert np.array_equal(got, exp), (allowed, i)
                outs[(allowed, i)] = got
                entries.append(eng.canonical_entries(0))
                if allowed:
                    assert entries[-1] == model_entries(f, fl, mapping, size_filter), i
                else:
                    assert entries[-1] == -1
            plan.close()
            if allowed:
                assert entries[1] < entries[0] == entries[2] and entries[4] < entries[3]
        for i in range(len(steps)):
            assert np.array_equal(outs[(True, i)], outs[(False, i)]), i
    finally:
        forbid(eng, monkeypatch, False)
        eng.close()


def test_plans_that_are_not_eligible_keep_their_streams(pa, oracle, data, monkeypatch):
    """A '.' segment, the stratified rule and two files: same counts, and no canonical stream is built."""
    f, flags = data
    kept = with_flags(f, flags)
    dot = SEGMENTS + [(0, 29990, 30110, 3)]
    eng = staged([f], flags)
    try:
        configure(eng, ("fiveprime", 12))
        exp = expected(oracle, [kept], ("fiveprime", 12), None, dot, "dot")
        assert count_both_ways(eng, monkeypatch, dot, exp, "'.' segment") == -1
        configure(eng, STRATIFIED)
        exp = expected(oracle, [kept], STRATIFIED, None, SEGMENTS, "stratified")
        assert count_both_ways(eng, monkeypatch, SEGMENTS, exp, "stratified") == -1
    finally:
        eng.close()
    f2 = f.subset(np.arange(0, f.n, 2))
    eng = staged([kept, f2])
    try:
        configure(eng, ("fiveprime", 12))
        exp = expected(oracle, [kept, f2], ("fiveprime", 12), None, SEGMENTS, "two files")
        assert count_both_ways(eng, monkeypatch, SEGMENTS, exp, "two files") == -1
        assert eng.canonical_entries(1) == -1
    finally:
        eng.close()


def test_windows_cut_into_128_wide_sub_windows(pa, oracle, monkeypatch):
    """PC_WORK_R=1024 and 12 288 reads in one 2 048-position window: sixteen sub-windows of 128 positions, each with an
    exact lower bound looked up in the canonical stream's index; shifts carry reads across every sub-window edge."""
    monkeypatch.setenv("PC_TILE_G", "2048")
    monkeypatch.setenv("PC_WORK_R", "1024")
    w0 = 10240
    p = np.repeat(np.arange(2048), 6)
    j = np.arange(len(p))
    f = pa.PackedAlignments.from_ungapped(0, w0 + p, 20 + (j * 5) % 21, (j // 3) & 1, references=NAMES, lengths=LENS)
    segments = [(0, w0, w0 + 2048, 1), (0, w0, w0 + 2048, 2), (0, w0 + 500, w0 + 1030, 1), (0, 60000, 60100, 2)]
    eng = staged([f])
    try:
        for mapping in (("fiveprime", 12), ("threeprime", 3)):
            configure(eng, mapping)
            exp = expected(oracle, [f], mapping, None, segments, ("cut", mapping[0]))
            assert count_both_ways(eng, monkeypatch, segments, exp, mapping[0]) == model_entries(f, f.flags, mapping)
    finally:
        eng.close()


def test_windows_of_256_positions(pa, oracle, data, monkeypatch):
    monkeypatch.setenv("PC_TILE_G", "256")
    f, flags = data
    eng = staged([f], flags)
    try:
        for mapping in (RULES[1], RULES[4]):
            configure(eng, mapping)
            exp = expected(oracle, [with_flags(f, flags)], mapping, None, SEGMENTS, ("base", RULE_IDS[RULES.index(mapping)]))
            assert count_both_ways(eng, monkeypatch, SEGMENTS, exp, mapping[0]) == model_entries(f, flags, mapping)
    finally:
        eng.close()


def test_short_segments_on_a_long_contig(pa, oracle, monkeypatch):
    """Read clusters up to 650 M on one contig -- more linear-index entries than the build launches workgroups, positions
    beyond 2^29 -- under a sparse plan of short segments: exact bounds at both ends of every window (looked up in the
    canonical stream's index) and the single-wave class of sparse windows."""
    names, lens = ["huge", "tail"], [700000000, 5000]
    tid, pos, alen, rev = [], [], [], []
    for c in (1000, (1 << 29) - 40, (1 << 29) + 70, 650000000):
        for j in range(48):
            L = 22 + (j * 5) % 17
            r = (j >> 2) & 1
            tid.append(0); alen.append(L); rev.append(r)
            pos.append(c + (j % 3) if (j & 1) else c + 50 - L + (j % 3))   # common starts and common ends
    for j in range(10):
        tid.append(1); pos.append(100 + j // 3); alen.append(25 + j); rev.append(j & 1)
    order = np.lexsort((np.array(pos), np.array(tid)))
    f = pa.PackedAlignments.from_ungapped(np.array(tid)[order], np.array(pos)[order], np.array(alen)[order], np.array(rev, bool)[order],
                                          references=names, lengths=lens)
    spans = []
    for c in (1000, (1 << 29) - 40, (1 << 29) + 70, 650000000):
        spans += [(0, c - 5, c + 20), (0, c + 12, c + 13), (0, c + 30, c + 75), (0, c - 300, c - 200)]
    spans += [(0, 300000000, 300000100), (1, 0, 200)]
    segments = [(t, a, e, st) for (t, a, e) in spans for st in (1, 2)]
    eng = staged([f])
    try:
        for mapping in (("fiveprime", 12), ("threeprime", 0), ("variable", VAR_MISSING)):
            configure(eng, mapping)
            exp = expected(oracle, [f], mapping, None, segments, ("long contig", mapping[0]))
            model = model_entries(f, f.flags, mapping)
            assert 0 < model <= 0.9 * eng.stream_entries(0)
            assert count_both_ways(eng, monkeypatch, segments, exp, mapping[0]) == model
    finally:
        eng.close()
