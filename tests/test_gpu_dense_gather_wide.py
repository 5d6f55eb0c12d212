"""k_dense_gather as it serves an item: 16-byte stores of aligned pairs of output elements with a head and a tail of one
element, 4-byte loads of the 16-bit cells at even cell indices, one item or a batch of items per workgroup.  The plans here go through
every case of that arithmetic: both parities of the output offset and of the cell address, both output directions and
strands, lengths around one wave, one workgroup pass and one item; the first and the last cell of the block; escaped
cells in either half of a pair and at the ends of items and batches; plans around the batch size; output slices in any
order, with gaps of one element.  Every plan is counted with the vector allowed and under ``PC_NO_DENSE=1``: both equal
the oracle bit for bit, and ``Engine.dense_cells`` names the path.  Needs a real MI355X: ``pytest -m gpu``.

The file, the genome and the oracle's whole-contig counts are those of tests/test_gpu_dense_vector.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import test_gpu_dense_vector as dv   # noqa: E402  (helpers only)

pytestmark = pytest.mark.gpu

NAMES, LENS, FWD, REV = dv.NAMES, dv.LENS, dv.FWD, dv.REV
RULE = dv.RULES[0]
LENGTHS = (1, 2, 3, 255, 256, 257, 2047, 2048, 2049, 4097)


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


class Layout:
    """Segments (tid, start, end, strand, out_step) with the output element of each one's position 0."""

    def __init__(self):
        self.segs, self.off, self.elems = [], [], 0

    def add(self, seg, parity=None, gap=0):
        """Behind what is there, after `gap` free elements; parity: of the element position 0 goes to (one more free
        element where it does not come out that way)."""
        n = seg[2] - seg[1]
        at = self.elems + gap
        first = at if seg[4] == 1 else at + n - 1
        if parity is not None and first % 2 != parity:
            at += 1
            first += 1
        self.segs.append(seg)
        self.off.append(first)
        self.elems = at + n
        return self

    def permuted(self, order):
        out = Layout()
        out.segs = [self.segs[k] for k in order]
        out.off = [self.off[k] for k in order]
        out.elems = self.elems
        return out

    def plan(self, eng, extra=0):
        s = self.segs
        lens = np.array([x[2] - x[1] for x in s], np.int64)
        return eng.plan(np.array([x[0] for x in s], np.int32), np.array([x[1] for x in s], np.int64), np.array([x[2] for x in s], np.int64),
                        np.array([x[3] for x in s], np.uint8), np.array(self.off, np.int64), np.array([x[4] for x in s], np.int8), lens,
                        self.elems + extra, eng.rows)

    def expected(self, cc, extra=0, lens=LENS):
        out = np.zeros(self.elems + extra, np.int64)
        seen = np.zeros(self.elems + extra, bool)
        for (t, a, e, st, step), off in zip(self.segs, self.off):
            arr = np.zeros(e - a, np.int64)
            if 0 <= t < len(lens):
                lo, hi = max(a, 0), min(e, lens[t])
                if hi > lo:
                    arr[lo - a:hi - a] = cc[(t, st)][lo:hi]
            idx = off + step * np.arange(e - a, dtype=np.int64)
            assert not seen[idx].any()          # (the layouts here never overlap)
            seen[idx] = True
            out[idx] = arr
        return out, seen


def alignment_matrix():
    """output-offset parity x cell-address parity x out_step x strand x length; contig 0, whose strands start at even
    cells (0 and 20 000)"""
    lay = Layout()
    k = 0
    for n in LENGTHS:
        for strand in (FWD, REV):
            for step in (1, -1):
                for cell_parity in (0, 1):
                    for out_parity in (0, 1):
                        start = 200 + 2 * (k % 3000) + cell_parity
                        lay.add((0, start, start + n, strand, step), parity=out_parity)
                        k += 7
    return lay


def test_alignment_matrix_and_output_modes(oracle, data, engine, monkeypatch):
    dv.configure(engine, RULE)
    cc = dv.contig_counts(oracle, ("base", RULE[0]), [data], RULE)
    lay = alignment_matrix()
    assert len(lay.segs) == 16 * len(LENGTHS)
    exp, seen = lay.expected(cc)
    assert exp.max() > 0 and not seen.all()     # (the parity padding leaves gaps)
    cells = dv.model_cells(data)
    plan = lay.plan(engine)
    try:
        dv.count_three_ways(engine, monkeypatch, plan, exp, np.int64, cells, "int64")
        dv.count_three_ways(engine, monkeypatch, plan, exp.astype(np.float64), np.float64, cells, "float64")
        total = float(data.n)
        engine.set_normalize(True, total)
        dv.count_three_ways(engine, monkeypatch, plan, exp.astype(np.float64) / total * 1e6, np.float64, cells, "normalised")
    finally:
        engine.set_normalize(False)
        plan.close()


def test_edges_of_the_block(oracle, data, engine, monkeypatch):
    """Cell 0, the last cell of the last strand, starts below 0 and ends past the extent at odd offsets, unknown contigs
    and empty clips between them (inside a batch), on both output parities and directions."""
    dv.configure(engine, RULE)
    cc = dv.contig_counts(oracle, ("base", RULE[0]), [data], RULE)
    last = LENS[2]
    segs = []
    for n in (1, 2, 3, 256, 257, 2049):
        segs += [(0, 0, n, FWD, 1), (0, 0, n, FWD, -1), (2, last - n, last, REV, 1), (2, last - n, last, REV, -1),
                 (7, 10, 10 + n, FWD, 1), (0, -n - 5, -5, REV, -1),                        # unknown contig, wholly below 0
                 (0, -n, n + 1, FWD, 1), (0, -n - 1, n, REV, -1), (2, last - n, last + n + 1, FWD, -1), (2, last - n - 1, last + n, REV, 1),
                 (1, LENS[1], LENS[1] + n, FWD, 1), (-1, 0, n, REV, 1),                     # starts at the end, unknown contig
                 (0, LENS[0] - 1, LENS[0] + 2, REV, 1), (1, -1, 2, REV, -1)]
    for first_parity in (0, 1):
        lay = Layout()
        for k, s in enumerate(segs):
            lay.add(s, parity=(first_parity + k) % 2 if k % 3 == 0 else None)
        exp, _ = lay.expected(cc)
        plan = lay.plan(engine)
        try:
            dv.count_three_ways(engine, monkeypatch, plan, exp, np.int64, dv.model_cells(data), "edges %d" % first_parity)
        finally:
            plan.close()


def test_escaped_cells_in_pairs_items_and_batches(pa, oracle, monkeypatch):
    """The piles of test_cells_beyond_16_bits (65 534 to 200 000 reads on four neighbouring positions of either strand of
    contig 1), queried so that an escaped cell is the first and the second element of a pair, alone in a head or a tail,
    the first and the last position of an item, of a 2 048-position item, and of the first and last item of a batch."""
    rng = np.random.default_rng(3)
    piles = (65534, 65535, 65536, 200000)
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
    cc = dv.contig_counts(oracle, "piles", [f], mapping)
    for k, n in enumerate(piles):
        assert n <= cc[(1, FWD)][1000 + k] < n + 40 and n <= cc[(1, REV)][2000 + k] < n + 40
    lay = Layout()
    for strand, at in ((FWD, 1000), (REV, 2000)):
        for step in (1, -1):
            for parity in (0, 1):
                for a in range(at - 2, at + 5):                       # the piles at the first positions of a segment ...
                    for n in (1, 2, 3, 5, 2048, 2049):
                        lay.add((1, a, a + n, strand, step), parity=parity)
                for e in range(at, at + 6):                           # ... and at the last ones, of one item and of two
                    for n in (4, 2047, 2048, 2050):
                        lay.add((1, e - n, e, strand, step), parity=parity)    # (the longest start below 0)
    exp, _ = lay.expected(cc)
    assert (exp >= 65535).sum() > 500
    eng = dv.staged([f])
    try:
        dv.configure(eng, mapping)
        for shift in range(4):     # every segment comes to lie at every place of a batch of 2, 4 or 8 items
            sub = lay.permuted(list(range(shift, len(lay.segs))) + list(range(shift)))
            e2, _ = sub.expected(cc)
            assert np.array_equal(e2, exp)
            plan = sub.plan(eng)
            try:
                dv.count_three_ways(eng, monkeypatch, plan, exp, np.int64, dv.model_cells(f), "piles, plan order shifted by %d" % shift)
                if shift == 0:
                    dv.count_three_ways(eng, monkeypatch, plan, exp.astype(np.float64), np.float64, dv.model_cells(f), "piles float64")
            finally:
                plan.close()
    finally:
        eng.close()


@pytest.mark.parametrize("n_items", [1, 2, 3, 4, 5, 7, 8, 9, 13, 17, 25])
def test_plans_around_the_batch_size(oracle, data, engine, monkeypatch, n_items):
    """1, B - 1, B, B + 1 and 3 B + 1 items for B = 2, 4 and 8: the last batch is short, or full, or one item."""
    dv.configure(engine, RULE)
    cc = dv.contig_counts(oracle, ("base", RULE[0]), [data], RULE)
    lay = Layout()
    for k in range(n_items):
        n = (301, 2048, 77, 1500)[k % 4]
        lay.add((k % 3, 50 + 61 * k, 50 + 61 * k + n, FWD if k % 2 else REV, 1 if k % 3 else -1))
    exp, seen = lay.expected(cc)
    assert seen.all()
    plan = lay.plan(engine)
    try:
        # (a plan of ONE window is served by the single-window kernel whatever the vector offers: pc_count)
        dv.count_three_ways(engine, monkeypatch, plan, exp, np.int64, dv.model_cells(data) if n_items > 1 else -1, "%d items" % n_items)
    finally:
        plan.close()


def test_thousands_of_tiny_segments(oracle, data, engine, monkeypatch):
    dv.configure(engine, RULE)
    cc = dv.contig_counts(oracle, ("base", RULE[0]), [data], RULE)
    rng = np.random.default_rng(17)
    lay = Layout()
    for k in range(5003):
        t = int(rng.integers(0, 3))
        a = int(rng.integers(-2, LENS[t] + 1))
        lay.add((t, a, a + int(rng.integers(1, 4)), FWD if rng.random() < 0.5 else REV, 1 if rng.random() < 0.5 else -1))
    exp, seen = lay.expected(cc)
    assert seen.all() and exp.max() > 0
    plan = lay.plan(engine)
    try:
        dv.count_three_ways(engine, monkeypatch, plan, exp, np.int64, dv.model_cells(data), "tiny segments")
    finally:
        plan.close()


def test_layouts_with_gaps_in_any_order(pa, oracle, monkeypatch):
    """Slices in permuted and in reversed order, one free element between slices and at both ends of the output, and an
    output longer than the slices need.  The plan is counted under one size filter and then under another: a gap element
    that is not 0 then was either left over or hit by a store wider than its slice.  A file of 300 000 reads: under
    either filter its stream stays larger than the vector, so the vector serves both counts (dense_host.h, size_rule)."""
    filters = ((25, 30), (31, 40))
    data = dv.ungapped_file(pa, 5, n=300000)
    cc = [dv.contig_counts(oracle, ("wide", sf), [data], RULE, sf) for sf in filters]
    engine = dv.staged([data])
    lay = Layout()
    k = 0
    for n in (1, 2, 3, 4, 255, 256, 257, 2047, 2048, 2049, 4097):
        for strand, step in ((FWD, 1), (FWD, -1), (REV, 1), (REV, -1)):
            lay.add((k % 3, 40 + 13 * k, 40 + 13 * k + n, strand, step), gap=1)     # (gap 1: also before the first slice)
            k += 1
    extra = 5                                                                        # free elements behind the last slice
    rng = np.random.default_rng(23)
    orders = {"plan order": list(range(len(lay.segs))), "reversed": list(range(len(lay.segs)))[::-1],
              "permuted": [int(x) for x in rng.permutation(len(lay.segs))]}
    try:
        for what, order in orders.items():
            sub = lay.permuted(order)
            plan = sub.plan(engine, extra=extra)
            try:
                prev = None
                for sf, c in zip(filters, cc):
                    dv.configure(engine, RULE, sf)
                    exp, seen = sub.expected(c, extra=extra)
                    assert not seen[0] and not seen[-extra:].any() and (~seen).sum() == len(lay.segs) + extra
                    assert prev is None or not np.array_equal(exp, prev)
                    got = plan.count(np.int64)
                    assert not got[~seen].any(), (what, sf)
                    dv.count_three_ways(engine, monkeypatch, plan, exp, np.int64, dv.model_cells(data), "%s, size filter %s" % (what, sf))
                    prev = exp
            finally:
                plan.close()
    finally:
        engine.close()
