"""The compact record stream: duplicate reads -- same contig, position, aligned length and strand -- are staged a second
time as ONE entry with a multiplicity (up to 16 reads per entry) and binned once.  Every count must stay what the oracle
says, and ``Engine.stream_entries`` must show that the compaction is on.  Needs a real MI355X: ``pytest -m gpu``.

Shapes are the smallest at which the paths can go wrong.  Two facts shape them:
* a plan of ONE window over one file is counted by the single-launch kernel, which streams the records -- so every plan
  here carries a second, far segment (``FAR``) and goes through the work lists;
* a compaction tile is 2 048 consecutive records; a tile that spans a contig change or more than 32 766 positions is
  left as it is (nothing merges there), and a file that keeps more than 90 % of its records as entries keeps no compact
  stream at all.  The cases that need such a tile put it behind a tile of duplicates, so that the compaction stays on."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stream_models import entries_of_sorted_tiles  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES, LENS = ["a", "b"], [200000, 100000]
FAR = (0, 180000, 180100)            # a segment without reads, in a window of its own
TILE, CAP = 2048, 16
OFFSETS = {26: 12, 27: 12, 28: 13, 29: 13, 30: 14, 31: 13, "default": 13}
MAPPINGS = [("fiveprime", 12), ("threeprime", 0), ("variable", OFFSETS), ("stratified", OFFSETS, 25, 35)]
EXCLUDED = 0x80


@pytest.fixture(scope="module")
def pa():
    import plastid_amd
    return plastid_amd


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as o
    o.lib()
    return o


def packed(pa, reads, **kw):
    """reads: iterable of (tid, pos, L, reverse, copies) -> PackedAlignments sorted by (tid, pos), the order given kept
    within a position."""
    tid = np.concatenate([np.full(r[4], r[0], np.int32) for r in reads])
    pos = np.concatenate([np.full(r[4], r[1], np.int32) for r in reads])
    alen = np.concatenate([np.full(r[4], r[2], np.int64) for r in reads])
    rev = np.concatenate([np.full(r[4], bool(r[3])) for r in reads])
    order = np.lexsort((pos, tid))   # stable
    return pa.PackedAlignments.from_ungapped(tid[order], pos[order], alen[order], rev[order], references=NAMES,
                                             lengths=LENS, **kw)


def with_flags(pa, f, flags):
    """What the oracle is given for `f` under the caller's `flags`: excluded records are simply absent from its input."""
    return f.subset(np.nonzero((flags & EXCLUDED) == 0)[0])


def spec_for(oracle, mapping, size_filter=None):
    kind = mapping[0]
    if kind in ("fiveprime", "threeprime"):
        return oracle.mapping_spec(kind, mapping[1], size_filter=size_filter)
    if kind == "variable":
        return oracle.mapping_spec(kind, 0, mapping[1], size_filter=size_filter)
    return oracle.mapping_spec(kind, 0, mapping[1], mapping[2], mapping[3], size_filter=size_filter)


def check_counts(pa, oracle, eng, oracle_files, segments, mappings=MAPPINGS, size_filter=None, what=""):
    """Every segment under strands + - . (and the far segment), every mapping: int64 counts equal the oracle's."""
    from plastid_amd import synth
    from plastid_amd.packing import concat_file_major
    segs = [(t, s, e, st) for (t, s, e) in list(segments) + [FAR] for st in (1, 2, 3)]
    seg_tid = np.array([s[0] for s in segs], np.int32)
    seg_start = np.array([s[1] for s in segs], np.int64)
    seg_end = np.array([s[2] for s in segs], np.int64)
    seg_strand = np.array([s[3] for s in segs], np.uint8)
    lens = seg_end - seg_start
    aln = concat_file_major(oracle_files)
    for mapping in mappings:
        synth.mapping_factory(mapping)._configure(eng)
        if size_filter:
            eng.set_size_filter(*size_filter)
        else:
            eng.set_size_filter(None)
        rows = eng.rows
        out_off = np.concatenate([[0], np.cumsum(lens * rows)[:-1]])
        plan = eng.plan(seg_tid, seg_start, seg_end, seg_strand, out_off, np.ones(len(lens), np.int8), lens,
                        int((lens * rows).sum()), rows)
        arrays, _ = oracle.count_segments(aln, spec_for(oracle, mapping, size_filter), seg_tid, seg_start, seg_end, seg_strand)
        exp = np.concatenate([np.asarray(a).reshape(-1) for a in arrays])
        got = plan.count(np.int64)
        plan.close()
        assert got.dtype == np.int64 and np.array_equal(got, exp), (what, mapping[0], size_filter)


def engine_with(pa, files):
    from plastid_amd.engine import Engine
    eng = Engine(0)
    eng.set_alignments(files)
    return eng


def test_cap_boundaries(pa, oracle):
    """Groups of exactly cap, cap + 1 and 2 cap + 1 identical reads next to groups of one: 1, 2 and 3 entries."""
    f = packed(pa, [(0, 1000, 30, 0, 1), (0, 1010, 30, 0, CAP), (0, 1020, 30, 1, CAP + 1), (0, 1030, 30, 0, 2 * CAP + 1),
                    (0, 1040, 30, 0, 1)])
    eng = engine_with(pa, [f])
    assert eng.num_records(0) == 4 + 4 * CAP
    assert eng.stream_entries(0) == 1 + 1 + 2 + 3 + 1
    check_counts(pa, oracle, eng, [f], [(0, 900, 1200), (0, 1020, 1021)])
    eng.close()


def test_group_across_compaction_tiles(pa, oracle):
    """10 000 identical reads: one group over five tiles, cut at every tile edge and every 16 reads."""
    f = packed(pa, [(0, 4990, 28, 1, 3), (0, 5000, 28, 0, 10000), (0, 5003, 31, 0, 5)])
    eng = engine_with(pa, [f])
    assert eng.stream_entries(0) == entries_of_sorted_tiles(f) < eng.num_records(0) // 15
    check_counts(pa, oracle, eng, [f], [(0, 4900, 5200)])
    eng.close()


@pytest.mark.parametrize("no_small", [False, True], ids=["small-window class", "PC_NO_SMALL"])
def test_every_quad_alignment_of_an_item(pa, oracle, monkeypatch, no_small):
    """One entry (two reads) per position, so the entry of position 2000 + k has index `shift` + k.  A window this short
    (span <= 1 024) gets exact bounds, in the single-wave class and -- PC_NO_SMALL -- in the general one: its item
    starts at the entry of a - Ws + 1 (Ws = 30, the longest read) and ends before that of e, so a = 2040 .. 2043 and
    e = 2060 .. 2063 give lo & 3 and hi & 3 every value 0 .. 3, the alignments of the 16-byte quads the kernel loads.
    Nothing here can observe the bounds themselves; should windows like these ever get bucket-floor bounds instead,
    the `shift` entries in front still move both ends of the item through every alignment."""
    if no_small:
        monkeypatch.setenv("PC_NO_SMALL", "1")
    for shift in range(4):
        f = packed(pa, [(0, 1900 + k, 30, 0, 2) for k in range(shift)] + [(0, 2000 + k, 30, k & 1, 2) for k in range(100)])
        eng = engine_with(pa, [f])
        assert eng.stream_entries(0) == 100 + shift and eng.num_records(0) == 200 + 2 * shift
        for a in (range(2040, 2044) if shift == 0 else [2040]):
            for e in (range(2060, 2064) if shift == 0 else [2061]):
                check_counts(pa, oracle, eng, [f], [(0, a, e)], mappings=[MAPPINGS[0], MAPPINGS[3]], what=(shift, a, e))
        eng.close()


def test_partly_different_keys_do_not_merge(pa, oracle):
    """Same position, different length / strand, and one copy excluded by update_flags."""
    f = packed(pa, [(0, 3000, 28, 0, 3), (0, 3000, 29, 0, 2), (0, 3000, 28, 1, 2), (0, 3010, 28, 0, 8)])
    eng = engine_with(pa, [f])
    assert eng.stream_entries(0) == 4
    flags = f.flags.copy()
    flags[1] |= EXCLUDED                      # one of the three (3000, 28, +)
    eng.update_flags(0, flags)
    assert eng.stream_entries(0) == 4         # (the group is one read smaller, not gone)
    check_counts(pa, oracle, eng, [with_flags(pa, f, flags)], [(0, 2900, 3100)])
    eng.close()


def test_positions_65536_apart_do_not_merge(pa, oracle):
    """p and p + 65 536 with nothing between them share the 16 bits a stream word carries."""
    f = packed(pa, [(0, 1000 + k, 30, 0, 4) for k in range(600)] + [(0, 70000, 30, 0, 1), (0, 70000 + 65536, 30, 0, 1)])
    eng = engine_with(pa, [f])
    assert eng.stream_entries(0) < eng.num_records(0)
    check_counts(pa, oracle, eng, [f], [(0, 69900, 70100), (0, 135436, 135636), (0, 1000, 1700)], mappings=MAPPINGS[:2])
    eng.close()


def test_same_key_on_two_contigs_does_not_merge(pa, oracle):
    """The last records of one contig and the first of the next: same position, length and strand."""
    f = packed(pa, [(0, 100 + k, 30, 0, 4) for k in range(700)] + [(0, 5000, 30, 0, 3), (1, 5000, 30, 0, 2)] +
               [(1, 6000 + k, 30, 1, 4) for k in range(700)])
    eng = engine_with(pa, [f])
    assert eng.stream_entries(0) < eng.num_records(0)
    check_counts(pa, oracle, eng, [f], [(0, 4900, 5100), (1, 4900, 5100), (1, 6000, 6300)], mappings=MAPPINGS[:2])
    eng.close()


def test_position_sorted_only_is_grouped_by_the_tile_sort(pa, oracle):
    """Within a position the reads alternate length and strand, as in a file sorted by position alone: run-length
    encoding in file order would merge nothing."""
    reads = []
    for k in range(50):
        for _ in range(4):
            reads += [(0, 4000 + k, 28, 0, 1), (0, 4000 + k, 30, 1, 1)]
    f = packed(pa, reads)
    eng = engine_with(pa, [f])
    assert eng.num_records(0) == 400 and eng.stream_entries(0) == 100
    check_counts(pa, oracle, eng, [f], [(0, 3900, 4200)])
    eng.close()


def test_exact_bound_windows(pa, oracle):
    """Duplicate groups at the first position the halo of a short window admits (a - Ws + 1), one before it, at the
    last queried position and one past it."""
    a, e, Ws = 6000, 6500, 30
    reads = []
    for p in (a - Ws + 1, a - Ws, e - 1, e):
        reads += [(0, p, Ws, 0, 3), (0, p, Ws, 1, 3), (0, p, 26, 0, 2)]
    f = packed(pa, reads)
    eng = engine_with(pa, [f])
    assert eng.stream_entries(0) == 12 < eng.num_records(0)
    check_counts(pa, oracle, eng, [f], [(0, a, e)])
    eng.close()


def test_window_cut_into_sub_windows(pa, oracle, monkeypatch):
    """A 2 048-position window that a dense region cuts into sub-windows (PC_WORK_R=1024): duplicate groups on both
    sides of a sub-window edge, and one exactly on an edge."""
    monkeypatch.setenv("PC_TILE_G", "2048")
    monkeypatch.setenv("PC_WORK_R", "1024")
    w0 = 10240
    reads = [(0, w0 + 2 * k, 28 + (k % 3), k & 1, 3) for k in range(1000)]           # 3 000 records over the window
    for edge in (w0 + 512, w0 + 1024, w0 + 1536):
        reads += [(0, edge - 1, 30, 0, 5), (0, edge, 30, 0, 7), (0, edge, 30, 1, 4), (0, edge + 1, 30, 1, 5)]
    f = packed(pa, reads)
    eng = engine_with(pa, [f])
    assert eng.stream_entries(0) < eng.num_records(0) // 2
    check_counts(pa, oracle, eng, [f], [(0, w0, w0 + 2048)])
    check_counts(pa, oracle, eng, [f], [(0, w0 + 500, w0 + 1030)], mappings=MAPPINGS[:1])
    eng.close()


def test_filter_round_trip(pa, oracle):
    """Stage, count, exclude one read of a group, count, re-admit it, count -- with update_flags, then with the FLAG
    filter: the compact stream is rebuilt every time the stream words change."""
    reads = [(0, 7000, 30, 0, 5), (0, 7001, 30, 1, 4), (0, 7002, 27, 0, 1), (0, 7003, 30, 0, CAP + 1)]
    f0 = packed(pa, reads)
    flag16 = np.where(f0.flags & 1, 16, 0).astype(np.uint16)
    flag16[2] |= 0x100                          # one read of the first group is a secondary alignment
    f = packed(pa, reads, flag16=flag16, mapq=np.full(f0.n, 30, np.uint8))
    segs = [(0, 6900, 7100)]
    eng = engine_with(pa, [f])
    assert eng.stream_entries(0) == 5
    check_counts(pa, oracle, eng, [f0], segs, mappings=MAPPINGS[:2], what="staged")
    flags = f0.flags.copy()
    flags[f0.n - 1] |= EXCLUDED                 # the 17th read of the last group: its second entry goes
    eng.update_flags(0, flags)
    assert eng.stream_entries(0) == 4
    check_counts(pa, oracle, eng, [with_flags(pa, f0, flags)], segs, mappings=MAPPINGS[:2], what="excluded")
    eng.update_flags(0, f0.flags)
    assert eng.stream_entries(0) == 5
    check_counts(pa, oracle, eng, [f0], segs, mappings=MAPPINGS[:2], what="re-admitted")
    eng.set_flag_filter(exclude=0x100)
    flags = f0.flags.copy()
    flags[2] |= EXCLUDED
    check_counts(pa, oracle, eng, [with_flags(pa, f0, flags)], segs, mappings=MAPPINGS[:2], what="flag filter")
    eng.set_flag_filter(enabled=False)
    assert eng.stream_entries(0) == 5
    check_counts(pa, oracle, eng, [f0], segs, mappings=MAPPINGS[:2], what="flag filter lifted")
    eng.close()


def test_size_filter_drops_one_length_of_a_mixed_group(pa, oracle):
    f = packed(pa, [(0, 8000, 28, 0, 3), (0, 8000, 31, 0, 3), (0, 8000, 31, 1, 2), (0, 8004, 28, 1, 4)])
    eng = engine_with(pa, [f])
    assert eng.stream_entries(0) == 4
    check_counts(pa, oracle, eng, [f], [(0, 7900, 8100)], size_filter=(25, 29))
    check_counts(pa, oracle, eng, [f], [(0, 7900, 8100)])
    eng.close()


def test_two_files_with_duplicates_within_and_between(pa, oracle):
    f1 = packed(pa, [(0, 9000, 30, 0, 6), (0, 9002, 28, 1, 3), (0, 9010, 30, 0, 2)])
    f2 = packed(pa, [(0, 9000, 30, 0, 4), (0, 9002, 28, 1, 20), (0, 9011, 30, 1, 2)])
    eng = engine_with(pa, [f1, f2])
    assert eng.stream_entries(0) == 3 < eng.num_records(0) and eng.stream_entries(1) == 4 < eng.num_records(1)
    check_counts(pa, oracle, eng, [f1, f2], [(0, 8900, 9100)])
    eng.close()


def test_no_duplicates_keeps_no_compact_stream(pa, oracle):
    f = packed(pa, [(0, 11000 + k, 26 + (k % 5), k & 1, 1) for k in range(300)])
    eng = engine_with(pa, [f])
    assert eng.stream_entries(0) == eng.num_records(0) == 300
    check_counts(pa, oracle, eng, [f], [(0, 10900, 11400)])
    eng.close()


def test_compact_and_per_record_counts_are_equal(pa, oracle, monkeypatch):
    """PC_NO_COMPACT stages the same file without a compact stream: `stream_entries` says so, and every count is what
    the compact stream gives (and the oracle)."""
    from plastid_amd import synth
    reads = [(0, 12000 + 3 * (k // 4), 26 + (k % 4), (k >> 1) & 1, 1 + (k * 7) % 40) for k in range(400)]
    f = packed(pa, reads)
    seg = (np.array([0, FAR[0]], np.int32), np.array([11900, FAR[1]], np.int64), np.array([12500, FAR[2]], np.int64))
    lens = seg[2] - seg[1]
    got = {}
    for off in (False, True):
        if off:
            monkeypatch.setenv("PC_NO_COMPACT", "1")
        eng = engine_with(pa, [f])
        assert (eng.stream_entries(0) == eng.num_records(0)) if off else (eng.stream_entries(0) == entries_of_sorted_tiles(f) < eng.num_records(0))
        check_counts(pa, oracle, eng, [f], [(0, 11900, 12500)], what="PC_NO_COMPACT" if off else "compact")
        for mapping in MAPPINGS:
            synth.mapping_factory(mapping)._configure(eng)
            rows = eng.rows
            out_off = np.concatenate([[0], np.cumsum(lens * rows)[:-1]])
            plan = eng.plan(seg[0], seg[1], seg[2], np.full(2, 3, np.uint8), out_off, np.ones(2, np.int8), lens, int((lens * rows).sum()), rows)
            got[(off, mapping[0])] = plan.count(np.int64)
            plan.close()
        eng.close()
    for mapping in MAPPINGS:
        assert np.array_equal(got[(False, mapping[0])], got[(True, mapping[0])]), mapping[0]
