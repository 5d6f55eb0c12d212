"""Sequences of operations on ONE long-lived engine against the model of tests/stateful_cases.py.

Every other randomised GPU test builds a fresh engine per case.  The engine keeps much between counts -- exclusion bits
folded into the staged records by four setters, cached work lists and exact-grid counts per plan, "the compact histogram
is zero where it will be read", center streams, the knob block, ``Engine._state`` -- and a stale piece of any of it gives
wrong counts from correct kernels.  Here the state is exercised on purpose: random sequences (40 seeds, and 24 aimed at the
compact and the canonical stream of a staged file: tests/test_gpu_stream_state.py has their directed cases), the full table
of orders in which filters, files and columns can arrive, the lazy histogram across knob reloads, and the
``BAMGenomeArray`` layer on top.  The expectation always comes from scratch (oracle on the reads the model keeps).
docs/stateful_fuzz.md: the step vocabulary, how to replay a trace, what the tests caught."""
import itertools
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fuzz_cases  # noqa: E402
import stateful_cases as sc  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import plastid_amd as pa
    from oracle import oracle
    return pa, oracle


@pytest.mark.parametrize("seed", sc.SEEDS + sc.STREAM_SEEDS)
def test_operation_sequences_match_the_model(env, seed):
    pa, oracle = env
    sc.run_sequence(pa, oracle, sc.random_sequence(seed, pa))


# ------------------------------------------------------------------------------------------ the filter setters, every order
F1, F2 = (0, 0x100, 10), (0x1, 0x400, 0)
COLUMNS = {"none": (), "sam": ("set_alignment_sam",), "nh": ("set_alignment_nh",),
           "sam, nh": ("set_alignment_sam", "set_alignment_nh"), "nh, sam": ("set_alignment_nh", "set_alignment_sam")}
THEN = {"lift FLAG": (("set_flag_filter", None),), "lift NH": (("set_nh_filter", 0),),
        "lift both": (("set_flag_filter", None), ("set_nh_filter", 0)),
        "change": (("set_flag_filter", F2), ("set_nh_filter", 2))}
TABLE = list(itertools.product(("FLAG before", "FLAG after"), ("NH before", "NH after"), sorted(COLUMNS), sorted(THEN)))


def directed_steps(flag_when, nh_when, columns, then):
    """One cell of the table.  Pool file 1 is staged with both columns (staged file 0), then pool file 0 WITHOUT any
    (staged file 1); the filters are set before or after that; staged file 1's columns arrive (or not) in the order named;
    then the filters are lifted or changed; at last the caller's own exclusions of staged file 1 change (pc_update_flags),
    the filters are lifted, and so are the exclusions.  After every step one of the two plans is counted: the model says
    whether that is a refusal or which counts."""
    steps = [("add_file", 1, True, True), ("open_plan", 0, 0), ("open_plan", 1, 1)]
    if flag_when == "FLAG before":
        steps.append(("set_flag_filter", F1))
    if nh_when == "NH before":
        steps.append(("set_nh_filter", 1))
    steps.append(("add_file", 0, False, False))
    steps += [(kind, 1) for kind in COLUMNS[columns]]
    if flag_when == "FLAG after":
        steps.append(("set_flag_filter", F1))       # (refused while file 0 lacks the columns: the model says so)
    if nh_when == "NH after":
        steps.append(("set_nh_filter", 1))
    steps += list(THEN[then])
    steps += [("update_flags", 1, 77, 30), ("set_flag_filter", None), ("set_nh_filter", 0), ("update_flags", 1, 77, 0)]
    out = []
    for k, s in enumerate(steps):
        out.append(s)
        if k >= 2:
            out.append(("count", k % 2, "int64"))
    return out


def directed_world(pa):
    world = sc.random_world(np.random.default_rng(4242), pa, 4242)
    world["segsets"][1]["layout"] = "mixed"       # (no summed slices: every count of the table is a vector)
    world["segsets"][1]["step"] = np.where(np.arange(len(world["segsets"][1]["tid"])) % 2 == 0, 1, -1).astype(np.int8)
    return world


@pytest.mark.parametrize("flag_when,nh_when,columns,then", TABLE, ids=[" / ".join(c) for c in TABLE])
def test_filters_files_and_columns_in_every_order(env, flag_when, nh_when, columns, then):
    """("FLAG before", "NH before", "nh", "lift FLAG") is the order that left an NH filter silently unapplied: both
    filters set, a file staged with its NH column only, the FLAG filter lifted -- the multi-mappers were counted."""
    pa, oracle = env
    sc.run_sequence(pa, oracle, dict(seed=4242, world=directed_world(pa), steps=directed_steps(flag_when, nh_when, columns, then)))


# ------------------------------------------------------------------------------------------ the lazy histogram
def lazy_world(pa):
    """One contig of 40 000 nt, two files of 20 000 reads with pile-ups.  Segment set 1 has 12 000 positions (its count
    vector: 96 000 bytes), set 2 has 20 000 (its compact histogram: 80 000 bytes, beyond what rides in the plan's table
    block): the pool keeps freed blocks by power-of-two size, so the histogram of a plan of set 2 opened after a plan of
    set 1 was counted and closed is the block that held those counts."""
    rng = np.random.default_rng(99)
    names, lens = ["c0"], [40000]
    pool = []
    for k in range(2):
        f = fuzz_cases.random_file(rng, pa, names, lens, 20000, 44, 0.05, 0.1, True)
        flag16 = rng.integers(0, 1 << 12, f.n).astype(np.uint16)
        mapq = rng.choice(np.array([0, 10, 30, 60], np.uint8), f.n)
        nh = rng.integers(0, 4, f.n).astype(np.uint16)
        pool.append(dict(file=f, flag16=flag16, mapq=mapq, nh=nh, full=sc._with_columns(pa, f, flag16, mapq, nh)))
    def one(name, a, b, strand):
        return dict(name=name, tid=np.zeros(1, np.int32), start=np.array([a], np.int64), end=np.array([b], np.int64),
                    strand=np.array([strand], np.uint8), layout="forward", step=np.ones(1, np.int8))
    hot = int(np.median(pool[0]["file"].pos))
    segsets = [one("single", max(0, hot - 500), max(0, hot - 500) + 1000, 3), one("before", 0, 12000, 3), one("under test", 10000, 30000, 3)]
    return dict(seed=99, names=names, lens=lens, pool=pool, segsets=segsets, strat=(25, 30), big=False, mapping0=("fiveprime", 3))


def test_lazy_histogram_across_knob_reloads(env):
    """A plan counts lazily (PC_HIST_LAZY_BYTES=1: only the slices of merged windows are cleared) on a recycled, non-zero
    block; then the knobs turn lazy off, to PC_HIST_MEMSET=1 and back, each time with other windows merged through the
    histogram (another PC_PILE / PC_WORK_R, other files).  Every count equals the model's.  A count that sets "the histogram
    is clean" after a lazy count gathers what the block held before."""
    pa, oracle = env
    lazy = {"PC_HIST_LAZY_BYTES": "1", "PC_TILE_G": "1024"}
    steps = [
        ("reload_knobs", dict(lazy, PC_PILE="1000000", PC_WORK_R="512")),
        ("add_file", 0, True, True),
        ("open_plan", 0, 1), ("count", 0, "int64"), ("close_plan", 0),            # leaves its count vector to the pool
        ("open_plan", 1, 2), ("count", 1, "int64"),                               # lazy, nothing merged: nothing cleared
        ("reload_knobs", {"PC_TILE_G": "1024", "PC_PILE": "64", "PC_WORK_R": "64"}),   # not lazy; pile-ups now merge
        ("count_twice", 1, "int64"),
        ("reload_knobs", dict(lazy, PC_PILE="1000000", PC_WORK_R="4096")), ("count", 1, "int64"),
        ("reload_knobs", dict(lazy, PC_HIST_MEMSET="1", PC_PILE="2048", PC_WORK_R="64")), ("count", 1, "float64"),
        ("reload_knobs", dict(lazy, PC_PILE="64", PC_WORK_R="512")), ("count", 1, "int64"),
        ("set_alignments", ((1, True, True), (0, True, True))), ("count_twice", 1, "int64"),
        ("reload_knobs", {"PC_TILE_G": "1024", "PC_PILE": "64", "PC_WORK_R": "64"}), ("total", 1, "int64"),
        ("set_mapping", ("center", 2)), ("count", 1, "float64"),
        ("set_mapping", ("threeprime", 0)), ("reload_knobs", dict(lazy, PC_PILE="2048", PC_WORK_R="64")), ("count", 1, "int64"),
        ("update_flags", 0, 5, 60), ("count", 1, "int64"),
        ("reload_knobs", {"PC_TILE_G": "1024", "PC_PILE": "64", "PC_WORK_R": "512"}), ("count", 1, "int64"),
        # the one-window `single` launch under lazy, and through the work lists
        ("set_alignments", ((0, True, True),)), ("reload_knobs", dict(lazy)), ("open_plan", 2, 0), ("count", 2, "int64"),
        ("query_segment", False, "int64"),
        ("reload_knobs", dict(lazy, PC_NO_SINGLE="1", PC_PILE="64", PC_WORK_R="64")), ("count", 2, "int64"), ("count", 1, "int64"),
        ("reload_knobs", {"PC_PILE": "64", "PC_WORK_R": "64"}), ("count", 2, "int64"), ("count_twice", 1, "int64"),
    ]
    sc.run_sequence(pa, oracle, dict(seed=99, world=lazy_world(pa), steps=steps))


# ------------------------------------------------------------------------------------------ BAMGenomeArray
def _ga_model_state(model, world, state, total):
    """Put what the array was asked for into the model: the `flag` slot holds a device filter or a callable on read.flag
    (host-evaluated: it arrives as the caller's exclusion bits), the `size` slot a SizeFilterFactory."""
    model.flag_filter, model.max_nh = None, 0
    for f in model.files:
        p = world["pool"][f["i"]]
        f["mask"] = (p["file"].flags & 0x80) != 0
        if state["flag"] is not None and state["flag"][0] == "callable":
            f["mask"] = f["mask"] | ((p["flag16"] & state["flag"][1]) != 0)
    if state["flag"] is not None and state["flag"][0] == "device":
        model.flag_filter, model.max_nh = tuple(state["flag"][1:4]), state["flag"][4]
    model.size_filter = state["size"]
    model.mapping = state["mapping"]
    model.norm = float(total) if state["normalize"] else None


@pytest.mark.parametrize("order", range(10))
def test_bamgenomearray_kept_alive_over_a_sequence(env, order):
    """One BAMGenomeArray over set_mapping / add_filter / remove_filter / set_normalize and the four ways of asking:
    every vector against the model.  A removed device filter must really be lifted; a callable replaced by a device
    filter of the same name must not leave its exclusion bits behind (``_sync_engine``, ``Engine._state``)."""
    pa, oracle = env
    from plastid_amd import synth
    rng = np.random.default_rng(7000 + order)
    world = sc.random_world(np.random.default_rng(5000 + order), pa, 5000 + 4 * order)     # (never the large world)
    nfiles = 1 + order % 2
    files = [sc.staged_file(pa, world, i, True, True) for i in range(nfiles)]
    model = sc.Model(world)
    for i in range(nfiles):
        model.apply(("add_file", i, True, True))
    state = dict(flag=None, size=None, mapping=world["mapping0"], normalize=False)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ga = pa.BAMGenomeArray(files, mapping=synth.mapping_factory(sc.mapping_of(state["mapping"])))
    total = sum(world["pool"][i]["file"].n for i in range(nfiles))    # every staged record, whatever the filters (the reference's sum())
    assert ga.sum() == total
    names, lens = world["names"], world["lens"]
    trace = []

    def random_segment():
        t = int(rng.integers(0, len(names)))
        a = int(rng.integers(0, lens[t] - 50))
        return t, a, min(lens[t] + 100, a + int(rng.integers(20, 3000))), "+-."[int(rng.integers(0, 3))]

    def expect(segs, strand):
        t = segs[0][0]
        world["segsets"] = [dict(name="q", tid=np.full(len(segs), t, np.int32), start=np.array([s[1] for s in segs], np.int64),
                                 end=np.array([s[2] for s in segs], np.int64), layout="chain", chain_strand=strand,
                                 strand=np.full(len(segs), {"+": 1, "-": 2, ".": 3}[strand], np.uint8))]
        _ga_model_state(model, world, state, total)
        model.plans = {0: dict(set=0, rows=model.rows())}
        return model

    # every order begins with the two transitions this test is for, each followed by a question: a device filter removed
    # (it must really be lifted), and a callable replaced by a device filter of the same name (its exclusion bits must go)
    forced = {0: 0.3, 2: 0.7, 4: 0.5, 6: 0.3}
    seen = []
    for it in range(28):
        u = forced.get(it, rng.random())
        if it % 2 == 0:      # ---- a change of what is asked for
            was = state["flag"]
            if u < 0.25:
                state["mapping"] = sc._random_mapping(rng, world["strat"])
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    ga.set_mapping(synth.mapping_factory(sc.mapping_of(state["mapping"])))
            elif u < 0.45:
                req, exc, mq = sc.FLAG_FILTERS[int(rng.integers(0, len(sc.FLAG_FILTERS)))]
                nh = int(rng.choice([0, 1, 2]))
                state["flag"] = ("device", req, exc, mq, nh)
                ga.add_filter("flag", pa.FlagFilterFactory(req, exc, mq, max_nh=nh))
            elif u < 0.6:
                bit = int(rng.choice([0x1, 0x100, 0x404]))
                state["flag"] = ("callable", bit)
                ga.add_filter("flag", lambda read, bit=bit: (read.flag & bit) == 0)
            elif u < 0.72 and state["flag"] is not None:
                state["flag"] = None
                ga.remove_filter("flag")
            elif u < 0.82:
                lo = int(rng.integers(15, 30))
                state["size"] = (lo, int(rng.choice([-1, lo + 10])))
                ga.add_filter("size", pa.SizeFilterFactory(min=state["size"][0], max=state["size"][1]))
            elif u < 0.88 and state["size"] is not None:
                state["size"] = None
                ga.remove_filter("size")
            else:
                state["normalize"] = not state["normalize"]
                ga.set_normalize(state["normalize"])
            trace.append(dict(state))
            seen.append((None if was is None else was[0], None if state["flag"] is None else state["flag"][0]))
            continue
        # ---- a question
        t, a, b, strand = random_segment()
        seg = pa.GenomicSegment(names[t], a, b, strand)
        rows = sc.rows_of(state["mapping"])
        where = "order %d, step %d, %s:%d-%d(%s); the states so far: %r" % (order, it, names[t], a, b, strand, trace)
        roi_order = True
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            if u < 0.3:
                roi_order = bool(rng.random() < 0.7)
                got = ga.get(seg, roi_order=roi_order)
                kind = "get"
            elif u < 0.5:
                got = ga[seg]
                kind = "getitem"
            elif u < 0.75:
                segs = [(t, a, a + 40), (t, a + 60, a + 61), (t, a + 200, b + 300)]
                chain = pa.SegmentChain(*[pa.GenomicSegment(names[t], s, e, strand) for _, s, e in segs])
                got = ga.get_counts_batch([chain])[0]
                kind = "chain"
            else:
                reads, got = ga.get_reads_and_counts(seg)
                kind = "reads"
        if kind == "chain":
            m = expect(segs, strand)
            exp = m.expected_plan(oracle, 0)[0].astype(np.float64)     # (SegmentChain.get_counts: always float)
        else:
            m = expect([(t, a, b)], strand)
            exp = m.expected_plan(oracle, 0)[0]                        # 5'->3', as roi_order=True gives it
        if rows > 1:
            exp = exp.reshape(rows, -1)
        if strand == "-" and not roi_order:
            exp = np.ascontiguousarray(exp[..., ::-1])                 # genome order
        assert got.dtype == exp.dtype and got.shape == exp.shape and np.array_equal(got, exp), \
            "%s: %s\n%s" % (kind, sc.first_difference(got.reshape(-1), exp.reshape(-1)), where)
        assert ga.sum() == total, where
        if kind == "reads":
            want = []
            for f in range(nfiles):
                want += [(f, int(i)) for i in np.nonzero(m.expected_mapped_reads(oracle, f))[0]]
            assert [(files.index(r.source), r.index) for r in reads] == want, where
    assert ("device", None) in seen and ("callable", "device") in seen, seen
    del ga
