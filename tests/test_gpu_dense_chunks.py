"""k_dense_gather_chunks: a plan whose output ranges do not overlap is served by aligned chunks of the output (1 024
elements; the layouts here also suit 2 048), one workgroup each, which write every element of the output -- gaps too, so no zero fill runs.  The plans here go
through the rows of a chunk that read through one, two and three spans, a pair of elements shared by two segments of
opposite direction, a chunk with more spans than its descriptor holds, a chunk that is all gap, outputs that end inside
a pair, a row and a chunk, clipped segments, unknown contigs and positions beyond the extent inside one row, escaped
cells at the ends of spans and in either half of a pair, and overlapping output ranges, which keep the item kernel.
Every plan is counted by chunks, under ``PC_DENSE_ITEMS=1`` and under ``PC_NO_DENSE=1``: all equal the oracle bit for
bit, and ``Engine.dense_path`` names the kernel.  Needs a real MI355X: ``pytest -m gpu``.

The file, the genome, the layouts and the oracle's whole-contig counts are those of tests/test_gpu_dense_vector.py and
tests/test_gpu_dense_gather_wide.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import test_gpu_dense_vector as dv            # noqa: E402  (helpers only)
from test_gpu_dense_gather_wide import Layout  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES, LENS, FWD, REV = dv.NAMES, dv.LENS, dv.FWD, dv.REV
RULE = dv.RULES[0]
# CHUNK: TWO chunks of the product (1 024 elements each), one of the other size that was measured: every boundary of
# the latter is one of the former, so "a chunk" below is 2 048 elements that the product serves as two
CHUNK, ROW, INLINE_SPANS = 2048, 128, 7


@pytest.fixture(scope="module")
def pa():
    import plastid_amd
    return plastid_amd


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as o
    o.lib()
    return o


@pytest.fixture(scope="module")
def data(pa):
    return dv.ungapped_file(pa, 20241019)


@pytest.fixture(scope="module")
def engine(data):
    eng = dv.staged([data])
    yield eng
    eng.close()


def knob(eng, monkeypatch, name, on):
    monkeypatch.setenv(name, "1") if on else monkeypatch.delenv(name, raising=False)
    eng.reload_knobs()


def count_by_every_path(eng, monkeypatch, plan, exp, dtype, what, path="chunks"):
    """`plan` counted by the default path (`path` must be the one), by items and by the window kernels: all `exp`, bit for bit"""
    got = plan.count(dtype)
    assert eng.dense_path() == path, (what, eng.dense_path())
    assert got.dtype == np.dtype(dtype) and np.array_equal(got, exp), what
    for name, want in (("PC_DENSE_ITEMS", "items" if path else None), ("PC_NO_DENSE", None)):
        try:
            knob(eng, monkeypatch, name, True)
            other = plan.count(dtype)
            assert eng.dense_path() == want, (what, name, eng.dense_path())
            assert np.array_equal(other, exp) and other.tobytes() == got.tobytes(), (what, name)
        finally:
            knob(eng, monkeypatch, name, False)
    return got


def spans_per_chunk(lay, size):
    """segments that meet each aligned chunk of `size` output elements"""
    n = np.zeros(-(-lay.elems // size), np.int64)
    for (t, a, e, st, step), off in zip(lay.segs, lay.off):
        lo = off if step == 1 else off - (e - a) + 1
        n[lo // size:(lo + e - a - 1) // size + 1] += 1
    return n


def poison(plan):
    """every byte of the plan's output block in HBM becomes 0x5A"""
    import torch
    from plastid_amd import multigpu
    multigpu.device_tensor(plan.device_ptr, plan.out_elems, "int64").fill_(0x5A5A5A5A5A5A5A5A)
    torch.cuda.synchronize()


def test_rows_of_one_two_and_three_spans_in_every_output_mode(oracle, data, engine, monkeypatch):
    """[0, 301) up, [301, 321) down, [321, 2321) up, [2321, 3821) down: row 2 (elements 256 to 383) reads through three
    spans, the pair (300, 301) belongs to an up and a down segment, rows 0 and 1 read through one span, the third segment
    crosses the boundaries at 1 024 and 2 048, and the row from 2 304 to 2 431 reads through two."""
    dv.configure(engine, RULE)
    cc = dv.contig_counts(oracle, ("base", RULE[0]), [data], RULE)
    lay = Layout()
    lay.add((0, 501, 802, FWD, 1)).add((1, 700, 720, REV, -1)).add((0, 3001, 5001, REV, 1)).add((2, 1000, 2500, FWD, -1))
    assert lay.off == [0, 320, 321, 3820] and lay.elems == 3821
    exp, seen = lay.expected(cc)
    assert seen.all() and exp[:CHUNK].max() > 0 and exp[CHUNK:].max() > 0
    plan = lay.plan(engine)
    try:
        count_by_every_path(engine, monkeypatch, plan, exp, np.int64, "int64")
        count_by_every_path(engine, monkeypatch, plan, exp.astype(np.float64), np.float64, "float64")
        total = float(data.n)
        engine.set_normalize(True, total)
        count_by_every_path(engine, monkeypatch, plan, exp.astype(np.float64) / total * 1e6, np.float64, "normalised")
    finally:
        engine.set_normalize(False)
        plan.close()


def test_overflow_spans_and_a_chunk_of_gap_without_a_zero_fill(oracle, data, engine, monkeypatch):
    """40 segments of 30 to 60 positions in the first 2 048 elements (the product's first two chunks, about 20 spans each;
    a descriptor holds 7), nothing in the next 2 048 (two chunks of gap), one segment behind them.  The output block is filled with 0x5A bytes between two counts: no memset runs on the chunk path,
    so every zero of the second count was stored by the kernel."""
    dv.configure(engine, RULE)
    cc = dv.contig_counts(oracle, ("base", RULE[0]), [data], RULE)
    rng = np.random.default_rng(41)
    lay = Layout()
    for k in range(40):
        n = int(rng.integers(30, 61))
        t = k % 3
        a = int(rng.integers(0, LENS[t] - n))
        lay.add((t, a, a + n, FWD if k % 2 else REV, 1 if k % 5 else -1), gap=int(k % 7 == 3))
    assert lay.elems <= CHUNK and spans_per_chunk(lay, CHUNK // 2)[:2].min() > INLINE_SPANS
    lay.add((0, 9000, 9100, FWD, -1), gap=2 * CHUNK - lay.elems + 11)
    exp, seen = lay.expected(cc, extra=3)
    assert not seen[CHUNK:2 * CHUNK].any() and seen[2 * CHUNK + 11] and exp[:CHUNK].max() > 0
    plan = lay.plan(engine, extra=3)
    try:
        first = plan.count(np.int64)
        assert engine.dense_path() == "chunks" and np.array_equal(first, exp)
        poison(plan)
        assert (plan.read() == 0x5A5A5A5A5A5A5A5A).all()
        count_by_every_path(engine, monkeypatch, plan, exp, np.int64, "overflow spans, gap chunk")
    finally:
        plan.close()


@pytest.mark.parametrize("out_elems", [1, 2, 127, 129, 1023, 1025, 2047, 2049, 4097])
def test_outputs_that_end_inside_a_pair_a_row_and_a_chunk(oracle, data, engine, monkeypatch, out_elems):
    """two segments on different contigs fill the output.  (One element holds one segment: a plan of ONE window is served
    by the single-window kernel whatever the vector offers.)"""
    dv.configure(engine, RULE)
    cc = dv.contig_counts(oracle, ("base", RULE[0]), [data], RULE)
    lay = Layout()
    n0 = (out_elems + 1) // 2
    lay.add((0, 777, 777 + n0, FWD, -1))
    if out_elems > n0:
        lay.add((2, 4000, 4000 + out_elems - n0, REV, 1))
    assert lay.elems == out_elems
    exp, seen = lay.expected(cc)
    assert seen.all()
    plan = lay.plan(engine)
    try:
        count_by_every_path(engine, monkeypatch, plan, exp, np.int64, "%d elements" % out_elems, path="chunks" if out_elems > 1 else None)
        count_by_every_path(engine, monkeypatch, plan, exp.astype(np.float64), np.float64, "%d elements, float64" % out_elems,
                            path="chunks" if out_elems > 1 else None)
    finally:
        plan.close()


def test_clips_unknown_contigs_and_the_extent_inside_one_row(oracle, data, engine, monkeypatch):
    dv.configure(engine, RULE)
    cc = dv.contig_counts(oracle, ("base", RULE[0]), [data], RULE)
    segs = [(0, -10, 20, FWD, 1), (7, 5, 25, FWD, 1), (2, LENS[2] - 10, LENS[2] + 15, REV, -1), (1, LENS[1] - 9, LENS[1] + 6, FWD, 1),
            (0, -8, -1, REV, 1), (-1, 0, 9, FWD, -1), (1, -3, 4, REV, -1)]
    assert sum(s[2] - s[1] for s in segs) < ROW
    for lead in (0, 1, ROW - 5, CHUNK // 2 - 40, CHUNK - 40):      # inside row 0, off by one, across a row boundary, across a chunk boundary
        lay = Layout()
        if lead:
            lay.add((0, 100, 100 + lead, FWD, 1))
        for s in segs:
            lay.add(s)
        lay.add((2, 0, 300, FWD, 1))
        exp, seen = lay.expected(cc)
        assert seen.all() and exp.max() > 0
        plan = lay.plan(engine)
        try:
            count_by_every_path(engine, monkeypatch, plan, exp, np.int64, "clips behind %d elements" % lead)
        finally:
            plan.close()


def test_escaped_cells_at_span_ends_in_pairs_and_in_overflow_chunks(pa, oracle, monkeypatch):
    """Piles of 65 534 to 70 000 reads on four neighbouring positions of either strand of contig 1 (counts from 65 535 on
    are escaped cells), queried so that a pile is the first and the last element of a span, of a short one among many in a
    chunk and of a long one that is alone in its rows, on both parities of the output, in both directions."""
    rng = np.random.default_rng(3)
    piles = (65534, 65535, 65536, 70000)
    tid, pos, rev = [], [], []
    for k, n in enumerate(piles):
        tid.append(np.full(2 * n, 1)); pos.append(np.full(n, 1000 + k)); rev.append(np.zeros(n, bool))
        pos.append(np.full(n, 2000 + k - 24)); rev.append(np.ones(n, bool))
    bg = 30000
    btid = rng.integers(0, 3, bg)
    tid.append(btid); pos.append((rng.random(bg) * (np.array(LENS)[btid] - 25)).astype(np.int64)); rev.append(rng.random(bg) < 0.5)
    tid, pos, rev = np.concatenate(tid), np.concatenate(pos), np.concatenate(rev)
    order = np.lexsort((pos, tid))
    f = pa.PackedAlignments.from_ungapped(tid[order], pos[order], np.full(len(tid), 25), rev[order], references=NAMES, lengths=LENS)
    mapping = ("fiveprime", 0)
    cc = dv.contig_counts(oracle, "piles 70000", [f], mapping)
    for k, n in enumerate(piles):
        assert n <= cc[(1, FWD)][1000 + k] < n + 40 and n <= cc[(1, REV)][2000 + k] < n + 40
    lay = Layout()
    for strand, at in ((FWD, 1000), (REV, 2000)):
        for step in (1, -1):
            for parity in (0, 1):
                for a in range(at - 2, at + 5):           # a pile at the first elements of a span ...
                    for n in (1, 2, 3, 5, 300, 2049):
                        lay.add((1, a, a + n, strand, step), parity=parity)
                for e in range(at, at + 6):               # ... and at the last ones
                    for n in (4, 301, 2050):
                        lay.add((1, e - n, e, strand, step), parity=parity)
    # ... and in chunks with more spans than a descriptor holds: runs of tiny segments over the piles, from a chunk boundary on
    tiny_from = -(-lay.elems // CHUNK) * CHUNK
    first = True
    for strand, at in ((FWD, 1000), (REV, 2000)):
        for step in (1, -1):
            for a in range(at - 1, at + 4):
                for n in (1, 2, 3, 5):
                    lay.add((1, a, a + n, strand, step), gap=tiny_from - lay.elems if first else (a + n) % 2)
                    first = False
    exp, _ = lay.expected(cc)
    assert (exp >= 65535).sum() > 500
    for size in (CHUNK // 2, CHUNK):      # the product's chunk and the other size measured: the first tiny chunk overflows, with piles
        assert spans_per_chunk(lay, size)[tiny_from // size] > INLINE_SPANS and (exp[tiny_from:tiny_from + size] >= 65535).sum() > 40
    eng = dv.staged([f])
    try:
        dv.configure(eng, mapping)
        plan = lay.plan(eng)
        try:
            count_by_every_path(eng, monkeypatch, plan, exp, np.int64, "piles")
            count_by_every_path(eng, monkeypatch, plan, exp.astype(np.float64), np.float64, "piles float64")
        finally:
            plan.close()
    finally:
        eng.close()


def test_overlapping_output_ranges_keep_the_items(oracle, data, engine, monkeypatch):
    """Equal ranges, one shared element and a range inside another.  Where two segments write one element they write the
    same value (the same position of the genome), so the result does not depend on which store lands last."""
    dv.configure(engine, RULE)
    cc = dv.contig_counts(oracle, ("base", RULE[0]), [data], RULE)
    segs = [(0, 100, 150, FWD, 1, 0), (0, 100, 150, FWD, 1, 0),                # (..., out_off)
            (0, 149, 200, FWD, 1, 49),
            (2, 500, 3000, REV, 1, 100), (2, 1000, 1200, REV, 1, 600),
            (1, 10, 60, FWD, -1, 2649)]
    out_elems = 2650
    exp = np.zeros(out_elems, np.int64)
    for t, a, e, st, step, off in segs:
        exp[off + step * np.arange(e - a)] = cc[(t, st)][a:e]
    assert exp.max() > 0
    plan = engine.plan(np.array([s[0] for s in segs], np.int32), np.array([s[1] for s in segs], np.int64), np.array([s[2] for s in segs], np.int64),
                       np.array([s[3] for s in segs], np.uint8), np.array([s[5] for s in segs], np.int64), np.array([s[4] for s in segs], np.int8),
                       np.array([s[2] - s[1] for s in segs], np.int64), out_elems, engine.rows)
    try:
        count_by_every_path(engine, monkeypatch, plan, exp, np.int64, "overlapping output ranges", path="items")
    finally:
        plan.close()
