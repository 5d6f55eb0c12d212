"""The generator and the model of the stateful differential test (tests/stateful_cases.py) on their own: no GPU.

The GPU half (tests/test_gpu_stateful.py) runs the same sequences against a real engine; what is asserted here keeps
that run from being vacuous: the sequences are reproducible, the model's composition of caller bits, FLAG / MAPQ and NH
equals the reference's (fixtures made by the reference itself), the 40 committed seeds cover the step vocabulary, the
refusals, the five rules, several files, large plans and both directions of the lazy-histogram knob, and most checks
would SEE a stale engine (the expected vector is not zero and differs from the plan's previous one)."""
import os
import sys
from collections import Counter

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import stateful_cases as sc  # noqa: E402
from oracle import oracle  # noqa: E402
from tests import golden_util as gu  # noqa: E402

SEEDS = sc.SEEDS


@pytest.fixture(scope="module")
def pa():
    import plastid_amd.packing as packing   # (PackedAlignments only: nothing here opens the HIP library)
    return packing


@pytest.fixture(scope="module")
def walked(pa):
    """Every committed sequence, walked by the model alone: per seed ``(seq, [(index, step, refusal, expected)])``."""
    out = []
    for seed in SEEDS:
        seq = sc.random_sequence(seed, pa)
        out.append((seq, list(sc.model_walk(oracle, seq))))
    return out


def _arrays_of(x):
    if isinstance(x, np.ndarray):
        return [x]
    if isinstance(x, dict):
        return [a for k in sorted(x, key=str) for a in _arrays_of(x[k])]
    if isinstance(x, (list, tuple)):
        return [a for v in x for a in _arrays_of(v)]
    if hasattr(x, "tid") and hasattr(x, "blk_len"):
        return [getattr(x, k) for k in ("tid", "pos", "alen", "flags", "nblk", "blk_start", "blk_len")]
    return []


def test_sequences_are_reproducible(pa):
    for seed in SEEDS[:6]:
        a, b = sc.random_sequence(seed, pa), sc.random_sequence(seed, pa)
        assert a["steps"] == b["steps"] and a["outcomes"] == b["outcomes"]
        assert repr(a["steps"]) == repr(eval(repr(a["steps"])))          # a trace can be pasted into a Python prompt
        xa, xb = _arrays_of(a["world"]), _arrays_of(b["world"])
        assert len(xa) == len(xb) > 20
        assert all(p.dtype == q.dtype and np.array_equal(p, q) for p, q in zip(xa, xb))


def test_sequences_follow_the_rules_of_the_issue(walked):
    """30-50 steps, the last one a check; at least every third step is a check; between two mutating steps of one kind
    some check runs; no check asks an engine without alignments, and no plan is opened on one; the generator's recorded
    outcomes are the model's."""
    for seq, walk in walked:
        steps = seq["steps"]
        assert 30 <= len(steps) <= 50
        assert steps[-1][0] in sc.CHECK_KINDS
        run, pending = 0, set()
        m = sc.Model(seq["world"])
        for (at, step, why, exp), recorded in zip(walk, seq["outcomes"]):
            assert why == recorded
            if step[0] in sc.CHECK_KINDS:
                run, pending = 0, set()
                assert exp is not None or why is not None
                assert len(m.files) >= 1, (seq["seed"], at)
            else:
                assert step[0] != "open_plan" or len(m.files) >= 1, (seq["seed"], at)
                if why is None:
                    m.apply(step)
                run += 1
                assert run <= 2, (seq["seed"], at)
                assert step[0] not in pending, (seq["seed"], at, step)
                pending.add(step[0])


def _model_in_state(pa, files, order, filt, mapping, size_filter, norm, segset):
    req, exc, mq, max_nh = filt
    pool = [dict(file=sc._with_columns(pa, f), flag16=f.flag16, mapq=f.mapq, nh=f.nh, full=f) for f in files]
    world = dict(seed=0, pool=pool, segsets=[segset], mapping0=("fiveprime", 0), strat=(25, 35), big=False)
    m = sc.Model(world)
    have_nh = files[0].nh is not None
    if order == "files first":
        for k in range(len(files)):
            assert m.apply(("add_file", k, True, have_nh)) is None
        assert m.apply(("set_flag_filter", (req, exc, mq))) is None
        assert m.apply(("set_nh_filter", max_nh)) is None
        assert m.apply(("set_mapping", mapping)) is None
    else:   # the filters on an engine without files; the columns after the files, NH first; a caller's mask set and lifted
        assert m.apply(("set_mapping", mapping)) is None
        assert m.apply(("set_nh_filter", max_nh)) is None
        assert m.apply(("set_flag_filter", (0, 0x4, 0))) is None
        for k in range(len(files)):
            assert m.apply(("add_file", k, False, False)) is None
        assert m.refusal(("mapped_reads", 0)) == "columns"
        assert m.apply(("set_flag_filter", (req, exc, mq))) == "flag_filter_on"      # refused: the earlier one stays
        assert m.flag_filter == (0, 0x4, 0)
        for k in range(len(files)):
            if have_nh:
                assert m.apply(("set_alignment_nh", k)) is None
            assert m.apply(("update_flags", k, 7, 50)) is None
            assert m.apply(("set_alignment_sam", k)) is None
            assert m.apply(("update_flags", k, 7, 0)) is None
        assert m.apply(("set_flag_filter", (req, exc, mq))) is None
    m.apply(("set_size_filter", size_filter))
    m.apply(("set_normalize", norm))
    m.apply(("open_plan", 0, 0))
    return m


@pytest.mark.parametrize("group", ["flag_filters", "nh_filters"])
def test_model_composes_filters_like_the_reference(pa, group):
    """A model brought into a fixture's state by two different orders of the setters gives the vectors the reference
    returned for plain filter callables (tests/golden/make_flag_golden.py, make_nh_golden.py): segments and chains."""
    from test_gpu_parity import files_of
    g = gu.load(group)
    nq = 0
    for ci, case in enumerate(g.cases):
        files = files_of(pa, g, case)
        s = case["spec"]
        od = gu.offset_dict_of(s)
        if s["kind"] in ("fiveprime", "threeprime", "center"):
            mapping = (s["kind"], s["param"])
        elif s["kind"] == "variable":
            mapping = ("variable", tuple(od.items()))
        else:
            mapping = ("stratified", tuple(od.items()), s["min_len"], s["max_len"])
        filt = tuple(case["filter"]) + (0,) * (4 - len(case["filter"]))
        for q in case["queries"]:
            tid = gu.tid_of(case, q["chrom"])
            if tid < 0:
                continue
            segs = [(q["start"], q["end"])] if q["type"] == "segment" else [tuple(x) for x in q["segments"]]
            segset = dict(name="q", tid=np.full(len(segs), tid, np.int32), start=np.array([a for a, _ in segs], np.int64),
                          end=np.array([b for _, b in segs], np.int64), layout="chain", chain_strand=q["strand"],
                          strand=np.full(len(segs), gu.STRAND_CODE[q["strand"]], np.uint8))
            exp = g[q["expected"]]
            for order in (("files first", "filters first") if (ci + nq) % 4 == 0 else ("files first", "filters first")[nq % 2:][:1]):
                m = _model_in_state(pa, files, order, filt, mapping, tuple(case["size_filter"]) if case["size_filter"] else None,
                                    float(case["sum"]) if case["normalize"] else None, segset)
                assert m.refusal(("count", 0, "float64")) is None
                got, _ = m.expected_plan(oracle, 0)
                if q["type"] == "chain":      # (SegmentChain.get_counts fills a float array, whatever the rule)
                    got = got.astype(np.float64)
                assert got.dtype == exp.dtype and np.array_equal(got.reshape(exp.shape), exp), (case["spec"], case["filter_name"], q, order)
            nq += 1
    assert nq > 600


def test_coverage_of_the_committed_seeds(walked):
    kinds, refusals, rule_checks = Counter(), Counter(), Counter()
    several_files = large = to_lazy = from_lazy = 0
    for seq, walk in walked:
        m = sc.Model(seq["world"])
        two, plan_lazy = False, {}
        for at, step, why, exp in walk:
            kinds[step[0]] += 1
            if why is not None:
                refusals[why] += 1
            if step[0] not in sc.CHECK_KINDS:
                if why is None:
                    m.apply(step)
                continue
            if why is None:
                rule_checks[m.mapping[0]] += 1
                two = two or len(m.files) >= 2
            # a change of the lazy knob counts where it can matter: the SAME plan answered a point-rule count on one side
            # of it and now answers one on the other
            if why is None and step[0] in ("count", "count_twice", "total", "warn_flags") and m.mapping[0] != "center":
                if step[1] in plan_lazy and plan_lazy[step[1]] != m.lazy():
                    to_lazy += m.lazy()
                    from_lazy += not m.lazy()
                plan_lazy[step[1]] = m.lazy()
        several_files += two
        large += any(sc.min_tiles(sg) >= 4096 for sg in seq["world"]["segsets"])
    assert set(kinds) == set(sc.STEP_KINDS) and min(kinds.values()) >= 10, kinds
    assert set(refusals) == set(sc.REFUSAL_KINDS) and min(refusals.values()) >= 3, refusals
    assert set(rule_checks) == {"fiveprime", "threeprime", "center", "variable", "stratified"} and min(rule_checks.values()) >= 20, rule_checks
    assert several_files >= 10 and large >= 10, (several_files, large)
    assert to_lazy >= 10 and from_lazy >= 10, (to_lazy, from_lazy)


def test_checks_would_see_a_stale_engine(walked):
    """At most 10 % of the answered checks expect an all-zero vector, at most 15 % of all steps are refusals, and at least
    80 % of the checks that follow a mutating step -- ANY accepted one, knob reloads and plans opened or closed included,
    although those cannot change an expectation by themselves -- expect another vector than the same plan (or the same
    one-segment query) had at its previous check."""
    nsteps = nrefused = nchecks = nzero = followed = differ = 0
    for seq, walk in walked:
        last, changed = {}, False
        for at, step, why, exp in walk:
            nsteps += 1
            nrefused += why is not None
            if step[0] not in sc.CHECK_KINDS:
                changed = changed or why is None
                continue
            if exp is not None:
                nchecks += 1
                nzero += not exp.any()
                key = (step[0], step[1]) if step[0] in ("mapped_reads", "query_segment") else ("plan", step[1])
                if changed and key in last:
                    followed += 1
                    differ += last[key].shape != exp.shape or not np.array_equal(last[key], exp)
                last[key] = exp
            changed = False
    assert nchecks >= 400 and followed >= 150
    assert nzero <= 0.10 * nchecks, (nzero, nchecks)
    assert nrefused <= 0.15 * nsteps, (nrefused, nsteps)
    assert differ >= 0.80 * followed, (differ, followed)


def test_shrink_drops_what_the_predicate_does_not_need(pa):
    seq = sc.random_sequence(SEEDS[0], pa)
    target = next(s for s in seq["steps"] if s[0] == "set_mapping")
    small = sc.shrink(seq, lambda cand: target in cand["steps"])
    assert small["steps"] == [target]
