"""The dense vector: under a point rule (fiveprime, threeprime, variable) the count at a position does not depend on the
query, so a file whose genome is small beside its reads keeps one 16-bit cell per (contig, strand, position) and a plan of
'+' / '-' segments is served by one gather kernel.  Every comparison here is made three ways: against the oracle, against
the same engine under ``PC_NO_DENSE=1`` (bit-identical), and ``Engine.dense_cells`` must say which path ran.  Needs a real
MI355X: ``pytest -m gpu``.

The genomes are three contigs of 5 000 to 70 000 positions with a few 10^4 reads, dense enough that the vector (2 bytes per
cell) is no larger than the stream it replaces (4 bytes per entry).  The oracle is asked once per (file, rule, filter) for
both strands of every whole contig; what a segment must give -- clipped at 0 and at the contig's end, zero on an unknown
contig, reversed for out_step -1 -- is cut from those arrays with numpy."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

pytestmark = pytest.mark.gpu

NAMES, LENS = ["a", "b", "c"], [20000, 5000, 7000]
EXCLUDED = 0x80
VARIABLE = {26: 12, 27: 12, 28: 13, 30: 14, 31: 13, 33: 12, 36: 15, "default": 11}
RULES = [("fiveprime", 12), ("threeprime", 3), ("variable", VARIABLE)]
RULE_IDS = ["fiveprime12", "threeprime3", "variable"]
FWD, REV, DOT = 1, 2, 3

# (tid, start, end, strand, out_step): the item lengths 1, 2 047, 2 048, 2 049 and 4 097 on both strands and in both output
# directions, a three-exon chain, overlapping segments, starts below 0, ends past the contig, segments wholly outside,
# unknown contigs
SEGS = []
for k, n in enumerate((1, 2047, 2048, 2049, 4097)):
    SEGS += [(0, 300 + 37 * k, 300 + 37 * k + n, FWD, 1), (0, 9000 - 11 * k, 9000 - 11 * k + n, REV, -1),
             (2, 100 + k, min(100 + k + n, 7000), REV, 1), (0, 15000 + k, 15000 + k + n, FWD, -1)]
SEGS += [(1, 100, 400, FWD, 1), (1, 900, 1300, FWD, 1), (1, 2000, 2100, FWD, 1),        # a chain on '+'
         (1, 2000, 2100, REV, -1), (1, 900, 1300, REV, -1), (1, 100, 400, REV, -1),     # ... and on '-', laid out 3' to 5'
         (0, 5000, 8000, FWD, 1), (0, 6000, 9000, FWD, 1), (0, 6000, 9000, REV, 1),     # overlapping
         (0, -50, 300, FWD, 1), (0, -50, 300, REV, -1), (0, -3000, 2500, FWD, -1), (0, -400, -100, REV, 1),
         (1, 4900, 5300, FWD, 1), (1, 4900, 5300, REV, -1), (2, 6999, 9100, FWD, 1), (2, 7000, 7010, REV, 1), (1, 3000, 9000, REV, 1),
         (7, 100, 2300, FWD, 1), (-1, 0, 50, REV, -1), (3, 0, 10, FWD, 1)]


@pytest.fixture(scope="module")
def pa():
    import plastid_amd
    return plastid_amd


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as o
    o.lib()
    return o


def ungapped_file(pa, seed, n=90000, lens=LENS, sam=False):
    rng = np.random.default_rng(seed)
    tid = rng.choice(len(lens), n, p=np.array(lens) / float(sum(lens))).astype(np.int32)
    alen = rng.integers(20, 41, n)
    pos = (rng.random(n) * (np.array(lens)[tid] - alen + 1)).astype(np.int64)
    for t, L in enumerate(lens):   # a read at the very first and the very last positions of every contig
        k = np.nonzero(tid == t)[0][:4]
        pos[k[:2]] = 0
        pos[k[2:]] = L - alen[k[2:]]
    rev = rng.random(n) < 0.5
    order = np.lexsort((pos, tid))
    kw = {}
    if sam:
        flag16 = np.where(rev, 0x10, 0).astype(np.uint16)
        flag16[rng.random(n) < 0.2] |= 0x400
        kw = dict(flag16=flag16[order], mapq=rng.integers(0, 61, n).astype(np.uint8)[order])
    return pa.PackedAlignments.from_ungapped(tid[order], pos[order], alen[order], rev[order], references=NAMES, lengths=lens, **kw)


@pytest.fixture(scope="module")
def data(pa):
    return ungapped_file(pa, 20241019)


def spec_for(oracle, mapping, size_filter=None):
    if mapping[0] in ("fiveprime", "threeprime", "center"):
        return oracle.mapping_spec(mapping[0], mapping[1], size_filter=size_filter)
    if mapping[0] == "variable":
        return oracle.mapping_spec("variable", 0, mapping[1], size_filter=size_filter)
    return oracle.mapping_spec(mapping[0], 0, mapping[1], mapping[2], mapping[3], size_filter=size_filter)


_CONTIGS = {}


def contig_counts(oracle, key, files, mapping, size_filter=None, lens=LENS):
    """{(tid, strand): the oracle's counts of the whole contig on that strand}; computed once per `key` and left unchanged."""
    if key not in _CONTIGS:
        from plastid_amd.packing import concat_file_major
        tid = np.repeat(np.arange(len(lens)), 2).astype(np.int32)
        strand = np.tile([FWD, REV], len(lens)).astype(np.uint8)
        arrays, _ = oracle.count_segments(concat_file_major(files), spec_for(oracle, mapping, size_filter), tid, np.zeros(len(tid), np.int64),
                                          np.array(lens, np.int64)[tid], strand)
        out = {}
        for t, st, a in zip(tid, strand, arrays):
            a = np.asarray(a).reshape(-1).astype(np.int64)
            a.setflags(write=False)
            out[(int(t), int(st))] = a
        _CONTIGS[key] = out
    return _CONTIGS[key]


def expected(cc, segs, lens=LENS):
    parts = []
    for t, a, e, st, step in segs:
        arr = np.zeros(e - a, np.int64)
        if 0 <= t < len(lens):
            lo, hi = max(a, 0), min(e, lens[t])
            if hi > lo:
                arr[lo - a:hi - a] = cc[(t, st)][lo:hi]
        parts.append(arr[::-1] if step == -1 else arr)
    return np.concatenate(parts)


def make_plan(eng, segs):
    tid = np.array([s[0] for s in segs], np.int32)
    start = np.array([s[1] for s in segs], np.int64)
    end = np.array([s[2] for s in segs], np.int64)
    strand = np.array([s[3] for s in segs], np.uint8)
    step = np.array([s[4] for s in segs], np.int8)
    lens = end - start
    base = np.concatenate([[0], np.cumsum(lens)[:-1]])
    out_off = np.where(step == -1, base + lens - 1, base)
    return eng.plan(tid, start, end, strand, out_off, step, lens, int(lens.sum()), eng.rows)


def configure(eng, mapping, size_filter=None):
    from plastid_amd import synth
    synth.mapping_factory(mapping)._configure(eng)
    eng.set_size_filter(*size_filter) if size_filter else eng.set_size_filter(None)


def staged(files):
    from plastid_amd.engine import Engine
    eng = Engine(0)
    eng.set_alignments(files)
    return eng


def forbid(eng, monkeypatch, on):
    monkeypatch.setenv("PC_NO_DENSE", "1") if on else monkeypatch.delenv("PC_NO_DENSE", raising=False)
    eng.reload_knobs()


def model_cells(f):
    """2 strands x the furthest aligned end of every contig"""
    end = f.ref_end()
    return 2 * sum(int(end[f.tid == t].max(initial=0)) for t in range(len(f.references)))


def count_three_ways(eng, monkeypatch, plan, exp, dtype, cells, what):
    """`plan` counted with the vector allowed and forbidden: both equal `exp` bit for bit, and dense_cells says which ran."""
    got = plan.count(dtype)
    assert eng.dense_cells(0) == cells, (what, eng.dense_cells(0), cells)
    assert got.dtype == np.dtype(dtype) and np.array_equal(got, exp), what
    try:
        forbid(eng, monkeypatch, True)
        other = plan.count(dtype)
        assert eng.dense_cells(0) == -1, what
        assert np.array_equal(other, exp) and other.tobytes() == got.tobytes(), (what, "PC_NO_DENSE")
    finally:
        forbid(eng, monkeypatch, False)


@pytest.fixture(scope="module")
def engine(data):
    eng = staged([data])
    yield eng
    eng.close()


@pytest.mark.parametrize("mapping", RULES, ids=RULE_IDS)
def test_rules_and_output_modes(oracle, data, engine, monkeypatch, mapping):
    configure(engine, mapping)
    exp = expected(contig_counts(oracle, ("base", mapping[0]), [data], mapping), SEGS)
    assert exp.max() > 0 and len(exp) == sum(s[2] - s[1] for s in SEGS)
    cells = model_cells(data)
    assert cells == 2 * sum(LENS)
    plan = make_plan(engine, SEGS)
    try:
        count_three_ways(engine, monkeypatch, plan, exp, np.int64, cells, "int64")
        count_three_ways(engine, monkeypatch, plan, exp.astype(np.float64), np.float64, cells, "float64")
        total = float(data.n)
        engine.set_normalize(True, total)
        count_three_ways(engine, monkeypatch, plan, exp.astype(np.float64) / total * 1e6, np.float64, cells, "normalised")
    finally:
        engine.set_normalize(False)
        plan.close()


def test_gapped_and_spliced_reads(pa, oracle, monkeypatch):
    """Reads with a deletion, spliced reads and a few whose span leaves the halo of the record stream: the build counts them
    with the engine's own kernels, so the cells hold them."""
    rng = np.random.default_rng(7)
    base = ungapped_file(pa, 11, n=80000)
    tids = list(base.tid)
    revs = list((base.flags & 0x01) != 0)
    runs = [[(int(p), int(a))] for p, a in zip(base.pos, base.alen)]
    for j in range(3000):   # a deletion of 1 .. 3, or an intron of 60 .. 400
        t = int(rng.integers(0, 3))
        gap = int(rng.integers(1, 4)) if j & 1 else int(rng.integers(60, 400))
        a, b = int(rng.integers(8, 20)), int(rng.integers(8, 20))
        p = int(rng.integers(0, LENS[t] - a - b - gap))
        tids.append(t); revs.append(bool(j & 2)); runs.append([(p, a), (p + gap + a, b)])
    for j in range(12):     # introns of 3 000: beyond the span quantile, binned from the long-read lists
        p = 200 + 1100 * j
        tids.append(0); revs.append(bool(j & 1)); runs.append([(p, 15), (p + 3015, 10), (p + 3100, 8)])
    f = pa.PackedAlignments.from_runs(tids, revs, runs, references=NAMES, lengths=LENS, sort=True)
    assert int((f.nblk >= 2).sum()) == 3012
    eng = staged([f])
    try:
        for mapping in RULES:
            configure(eng, mapping)
            exp = expected(contig_counts(oracle, ("gapped", mapping[0]), [f], mapping), SEGS)
            plan = make_plan(eng, SEGS)
            try:
                count_three_ways(eng, monkeypatch, plan, exp, np.int64, model_cells(f), mapping[0])
            finally:
                plan.close()
    finally:
        eng.close()


def test_cells_beyond_16_bits(pa, oracle, monkeypatch):
    """65 534, 65 535, 65 536 and 200 000 reads on four neighbouring positions of either strand: 65 534 fits a cell, the
    others escape to the overflow list; every element exact."""
    rng = np.random.default_rng(3)
    piles = (65534, 65535, 65536, 200000)
    tid, pos, rev = [], [], []
    for k, n in enumerate(piles):
        tid.append(np.full(2 * n, 1)); pos.append(np.full(n, 1000 + k)); rev.append(np.zeros(n, bool))   # fiveprime 0: mapped at 1000 + k
        pos.append(np.full(n, 2000 + k - 24)); rev.append(np.ones(n, bool))                                # ... and at 2000 + k on '-'
    bg = 30000
    btid = rng.integers(0, 3, bg)
    tid.append(btid); pos.append((rng.random(bg) * (np.array(LENS)[btid] - 25)).astype(np.int64)); rev.append(rng.random(bg) < 0.5)
    tid, pos, rev = np.concatenate(tid), np.concatenate(pos), np.concatenate(rev)
    order = np.lexsort((pos, tid))
    f = pa.PackedAlignments.from_ungapped(tid[order], pos[order], np.full(len(tid), 25), rev[order], references=NAMES, lengths=LENS)
    segs = [(1, 0, 5000, FWD, 1), (1, 0, 5000, REV, -1), (1, 990, 1010, FWD, -1), (1, 1995, 2010, REV, 1), (1, 1001, 1002, FWD, 1),
            (0, 0, 20000, FWD, 1), (2, 0, 7000, REV, 1)]
    mapping = ("fiveprime", 0)
    cc = contig_counts(oracle, "piles", [f], mapping)
    for k, n in enumerate(piles):
        assert n <= cc[(1, FWD)][1000 + k] < n + 40 and n <= cc[(1, REV)][2000 + k] < n + 40
    exp = expected(cc, segs)
    eng = staged([f])
    try:
        configure(eng, mapping)
        plan = make_plan(eng, segs)
        try:
            count_three_ways(eng, monkeypatch, plan, exp, np.int64, model_cells(f), "piles")
            count_three_ways(eng, monkeypatch, plan, exp.astype(np.float64), np.float64, model_cells(f), "piles float64")
        finally:
            plan.close()
    finally:
        eng.close()


def test_vector_follows_filter_flag_rule_and_file_changes(pa, oracle, monkeypatch):
    """One plan, counted after each change with no knob touched in between: only the vector's signature can make the engine
    rebuild it, and a stale vector would give the counts of the step before."""
    f = ungapped_file(pa, 5, n=300000, sam=True)
    g = ungapped_file(pa, 6, n=250000, lens=[19000, 5000, 7000])
    g = pa.PackedAlignments(g.tid, g.pos, g.alen, g.flags, g.nblk, references=NAMES, lengths=LENS)   # (same contigs, shorter extent)
    third = f.flags.copy()
    third[::3] |= EXCLUDED
    keep_flag = ((f.flag16 & 0x400) == 0) & (f.mapq >= 10)
    eng = staged([f])
    try:
        configure(eng, RULES[0])
        plan = make_plan(eng, SEGS)
        prev = None

        def step(what, files, mapping, size_filter, cells):
            nonlocal prev
            exp = expected(contig_counts(oracle, ("steps", what), files, mapping, size_filter), SEGS)
            assert prev is None or not np.array_equal(exp, prev), what   # (the step must change the counts, or it proves nothing)
            count_three_ways(eng, monkeypatch, plan, exp, np.int64, cells, what)
            prev = exp

        cells = model_cells(f)
        step("base", [f], RULES[0], None, cells)
        configure(eng, RULES[0], (25, 30))
        step("size filter", [f], RULES[0], (25, 30), cells)
        eng.update_flags(0, third)
        step("update_flags", [f.subset((third & EXCLUDED) == 0)], RULES[0], (25, 30), cells)
        eng.update_flags(0, f.flags)
        eng.set_flag_filter(exclude=0x400, min_mapq=10)
        step("FLAG filter", [f.subset(keep_flag)], RULES[0], (25, 30), cells)
        eng.set_flag_filter(enabled=False)
        configure(eng, RULES[1], (25, 30))
        step("rule", [f], RULES[1], (25, 30), cells)
        eng.set_alignments([g])
        assert model_cells(g) < cells
        step("set_alignments", [g], RULES[1], (25, 30), model_cells(g))
        plan.close()
    finally:
        eng.close()


def direct(oracle, files, mapping, segs, size_filter=None):
    """The oracle on the segments themselves (all inside their contigs), in the plan's layout."""
    from plastid_amd.packing import concat_file_major
    arrays, _ = oracle.count_segments(concat_file_major(files), spec_for(oracle, mapping, size_filter), np.array([s[0] for s in segs], np.int32),
                                      np.array([s[1] for s in segs], np.int64), np.array([s[2] for s in segs], np.int64), np.array([s[3] for s in segs], np.uint8))
    return [np.asarray(a) for a in arrays]


def test_plans_and_files_that_are_not_eligible(pa, oracle, data, monkeypatch):
    """A '.' segment, a summed slice, two files, the stratified and the center rule, and a sparse file on a 50 M-nt contig
    (the vector would be larger than the stream): the window kernels serve them, with the same results."""
    inside = [s for s in SEGS if 0 <= s[0] < 3 and s[1] >= 0 and s[2] <= LENS[s[0]] and s[4] == 1]
    eng = staged([data])
    try:
        configure(eng, RULES[0])
        dot = inside + [(0, 1000, 3100, DOT, 1)]
        exp = np.concatenate([a.reshape(-1) for a in direct(oracle, [data], RULES[0], dot)]).astype(np.int64)
        plan = make_plan(eng, dot)
        count_three_ways(eng, monkeypatch, plan, exp, np.int64, -1, "'.' segment")
        plan.close()
        # a summed slice: out_step 0, one element per segment
        arrays = direct(oracle, [data], RULES[0], inside)
        n = len(inside)
        lens = np.array([s[2] - s[1] for s in inside], np.int64)
        step = np.ones(n, np.int8)
        step[0] = 0
        off = np.concatenate([[0], np.cumsum(np.where(step == 0, 1, lens))[:-1]])
        plan = eng.plan(np.array([s[0] for s in inside], np.int32), np.array([s[1] for s in inside], np.int64), np.array([s[2] for s in inside], np.int64),
                        np.array([s[3] for s in inside], np.uint8), off, step, lens, int(np.where(step == 0, 1, lens).sum()), 1)
        exp = np.concatenate([[a.sum()] if st == 0 else a.reshape(-1) for a, st in zip(arrays, step)]).astype(np.int64)
        count_three_ways(eng, monkeypatch, plan, exp, np.int64, -1, "summed slice")
        plan.close()
        # rules with rows, and the center rule
        strat = ("stratified", VARIABLE, 25, 35)
        configure(eng, strat)
        rows = eng.rows
        arrays = direct(oracle, [data], strat, inside)
        off = np.concatenate([[0], np.cumsum(lens * rows)[:-1]])
        plan = eng.plan(np.array([s[0] for s in inside], np.int32), np.array([s[1] for s in inside], np.int64), np.array([s[2] for s in inside], np.int64),
                        np.array([s[3] for s in inside], np.uint8), off, np.ones(n, np.int8), lens, int((lens * rows).sum()), rows)
        exp = np.concatenate([a.reshape(-1) for a in arrays]).astype(np.int64)
        count_three_ways(eng, monkeypatch, plan, exp, np.int64, -1, "stratified")
        plan.close()
        configure(eng, ("center", 2))
        exp = np.concatenate([a.reshape(-1) for a in direct(oracle, [data], ("center", 2), inside)]).astype(np.float64)
        plan = make_plan(eng, inside)
        count_three_ways(eng, monkeypatch, plan, exp, np.float64, -1, "center")
        plan.close()
    finally:
        eng.close()
    half = data.subset(np.arange(0, data.n, 2))
    eng = staged([data, half])
    try:
        configure(eng, RULES[0])
        exp = expected(contig_counts(oracle, "two files", [data, half], RULES[0]), SEGS)
        plan = make_plan(eng, SEGS)
        count_three_ways(eng, monkeypatch, plan, exp, np.int64, -1, "two files")
        assert eng.dense_cells(1) == -1
        plan.close()
    finally:
        eng.close()
    # 600 reads on 50 M positions
    big = [50000000, 5000, 7000]
    rng = np.random.default_rng(9)
    pos = np.sort(np.concatenate([rng.integers(0, 49999000, 300), rng.integers(1000000, 1002000, 300)]))
    f = pa.PackedAlignments.from_ungapped(0, pos, rng.integers(20, 41, 600), rng.random(600) < 0.5, references=NAMES, lengths=big)
    segs = [(0, 1000000, 1002100, FWD, 1), (0, 1000000, 1002100, REV, 1), (0, 0, 4097, FWD, 1), (0, 49990000, 50000000, REV, 1)]
    eng = staged([f])
    try:
        configure(eng, RULES[0])
        exp = np.concatenate([a.reshape(-1) for a in direct(oracle, [f], RULES[0], segs)]).astype(np.int64)
        plan = make_plan(eng, segs)
        count_three_ways(eng, monkeypatch, plan, exp, np.int64, -1, "sparse file")
        plan.close()
    finally:
        eng.close()


def test_two_plans_share_one_vector(oracle, data, monkeypatch):
    eng = staged([data])
    try:
        configure(eng, RULES[2])
        cc = contig_counts(oracle, ("base", "variable"), [data], RULES[2])
        first = make_plan(eng, SEGS[:9])
        count_three_ways(eng, monkeypatch, first, expected(cc, SEGS[:9]), np.int64, model_cells(data), "first plan")
        second = make_plan(eng, SEGS[9:])
        got = second.count(np.int64)   # its first count: items cut for this plan, cells as they are
        assert eng.dense_cells(0) == model_cells(data)
        assert np.array_equal(got, expected(cc, SEGS[9:]))
        assert np.array_equal(first.count(np.int64), expected(cc, SEGS[:9]))
        count_three_ways(eng, monkeypatch, second, expected(cc, SEGS[9:]), np.int64, model_cells(data), "second plan")
        first.close()
        second.close()
    finally:
        eng.close()
