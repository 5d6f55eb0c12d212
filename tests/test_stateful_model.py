"""The generator and the model of the stateful differential test (tests/stateful_cases.py) on their own: no GPU.

The GPU half (tests/test_gpu_stateful.py) runs the same sequences against a real engine; what is asserted here keeps
that run from being vacuous: the sequences are reproducible, the model's composition of caller bits, FLAG / MAPQ and NH
equals the reference's (fixtures made by the reference itself), the 40 committed seeds cover the step vocabulary, the
refusals, the five rules, several files, large plans and both directions of the lazy-histogram knob, and most checks
would SEE a stale engine (the expected vector is not zero and differs from the plan's previous one).  The 24 stream seeds
(stateful_cases.STREAM_SEEDS) have conditions of their own: the model has a verdict on the canonical stream at every plan
check, the verdicts fall on both sides, and every transition that can leave a stream stale is walked."""
import hashlib
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
def walked_streams_old(pa):
    """Every committed sequence of the 40 seeds, walked by the model alone: per seed
    ``(seq, [(index, step, refusal, expected, canonical verdict, model)])``."""
    out = []
    for seed in SEEDS:
        seq = sc.random_sequence(seed, pa)
        out.append((seq, list(sc.model_walk(oracle, seq, streams=True))))
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
    assert set(kinds) == set(sc.STEP_KINDS) - set(sc.STREAM_CHECK_KINDS) and min(kinds.values()) >= 10, kinds     # (the two stream kinds: test_stream_seeds_*)
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


def test_the_40_seeds_are_what_they_were(pa):
    """The stream seeds have a world and a generator of their own, so the sequences of seeds 2000-2039 keep every draw:
    sha256 over repr(steps), repr(outcomes) and the bytes of every world array, computed at the commit before the
    stream seeds existed."""
    h = hashlib.sha256()
    for seed in SEEDS:
        seq = sc.random_sequence(seed, pa)
        h.update(repr(seq["steps"]).encode())
        h.update(repr(seq["outcomes"]).encode())
        for a in _arrays_of(seq["world"]):
            h.update(np.ascontiguousarray(a).tobytes())
    assert h.hexdigest() == "d86adb2738a41c5cb40bb1cd3957dd7e4fec968e360898782613e849415fc7b7"


def test_the_40_seeds_still_reach_the_canonical_stream(walked_streams_old):
    """A tripwire, not a target: of the answered plan checks of the 40 seeds, 74 are in a state where the canonical stream
    may be used (one file, a point rule with one row, '+' / '-' windows only, a file with records, PC_NO_CANON unset) --
    all of them through the one-window `single` set, by accident of the draws.  Fewer than 60 means a change of the
    generator has taken that away."""
    eligible = 0
    for seq, walk in walked_streams_old:
        for at, step, why, exp, canon, model in walk:
            if canon is not None:
                pred = canon[0]
                eligible += pred[0] in ("built", "unknown") or (pred[0] == "none" and pred[1] in ("weigh-in", "no valid length", "halo"))
    assert eligible >= 60, eligible


# ------------------------------------------------------------------------------------------ the stream seeds
POINT = ("fiveprime", "threeprime", "variable")
TRANSITIONS = ("rule -> other point rule", "point rule -> center / stratified -> point rule", "size filter set, changed or lifted",
               "update_flags on the counted file", "FLAG or NH filter set or lifted", "columns arriving late under a waiting filter",
               "a second file, then back to one", "set_alignments to a file of another length range", "reload_knobs flips PC_NO_CANON",
               "reload_knobs flips PC_NO_COMPACT / PC_COMPACT_KEEP, then a re-filter", "stranded_dot counted in between",
               "two stranded plans counted alternately")


def _walk_all(pa, seeds):
    """Per seed ``(seq, walk)``: the model alone, with the state behind every step frozen as plain values."""
    out = []
    for seed in seeds:
        seq = sc.random_sequence(seed, pa)
        walk = []
        for at, step, why, exp, canon, m in sc.model_walk(oracle, seq, streams=True):
            f = m.files[0] if m.files else None
            state = dict(mapping=m.mapping, size=m.size_filter, filt=(m.flag_filter, m.max_nh), nfiles=len(m.files), f=f,
                         gen=f["gen"] if f else None, no_canon="PC_NO_CANON" in m.knobs, cknobs=m.compact_knobs(), missing=m.missing_columns(),
                         ranges=sc.sm.stream_ranges(seq["world"]["pool"][f["i"]]["file"]) if f else None, ever_built=m.ever_built,
                         plan_set=m.plans[step[1]]["set"] if step[0] in sc.PLAN_CHECK_KINDS else None,
                         compact=(None if f is None else m.expected_stream_entries(0) < seq["world"]["pool"][f["i"]]["file"].n))
            walk.append((at, step, why, exp, canon, state))
        out.append((seq, walk))
    return out


@pytest.fixture(scope="module")
def walked_streams(pa):
    return _walk_all(pa, sc.STREAM_SEEDS)


@pytest.fixture(scope="module")
def walked(walked_streams_old):
    """... as ``(seq, [(index, step, refusal, expected)])``."""
    return [(seq, [w[:4] for w in walk]) for seq, walk in walked_streams_old]


def transitions_between(walk, a, b):
    """The transitions of TRANSITIONS (by index) between two answered checks of one `stranded` plan, steps a and b."""
    before, after = walk[a][5], walk[b][5]
    mid = walk[a + 1:b]
    found = set()
    point_ends = before["mapping"][0] in POINT and after["mapping"][0] in POINT
    away = any(s[5]["mapping"][0] not in POINT for s in mid)
    if point_ends and not away and before["mapping"] != after["mapping"]:
        found.add(0)
    if point_ends and away:
        found.add(1)
    if before["size"] != after["size"]:
        found.add(2)
    if after["nfiles"] == 1 and any(s[1][0] == "update_flags" and s[2] is None and s[1][1] == 0 and s[5]["f"] is after["f"] for s in mid):
        found.add(3)
    if before["filt"] != after["filt"]:
        found.add(4)
    states = [before] + [s[5] for s in mid]
    for k, s in enumerate(mid):
        if s[1][0] in ("set_alignment_sam", "set_alignment_nh") and s[2] is None and states[k]["missing"] and not s[5]["missing"]:
            found.add(5)
        if s[1][0] == "reload_knobs" and s[5]["cknobs"] != states[k]["cknobs"]:
            if any(later[5]["f"] is s[5]["f"] and later[5]["gen"] > s[5]["gen"] for later in mid[k + 1:]) and after["f"] is s[5]["f"]:
                found.add(9)
    # (the check of the plan while two files are staged -- no canonical stream, file 0's left unserved -- is the "before")
    if after["nfiles"] == 1 and (before["nfiles"] >= 2 or any(s[5]["nfiles"] >= 2 for s in mid)):
        found.add(6)
    if (before["nfiles"] == 1 and after["nfiles"] == 1 and all(s[5]["nfiles"] <= 1 for s in mid) and before["ranges"] != after["ranges"]
            and any(s[1][0] == "set_alignments" for s in mid)):
        found.add(7)
    if before["no_canon"] != after["no_canon"]:
        found.add(8)
    for s in mid:
        if s[4] is not None and s[5]["plan_set"] == sc.SET_DOT:
            found.add(10)
        if s[4] is not None and s[5]["plan_set"] == sc.SET_STRANDED and s[1][1] != walk[b][1][1]:
            found.add(11)
    return found


def stream_statistics(walked_streams):
    """What the conditions below are about, counted once (also printed by ``python tests/test_stateful_model.py``)."""
    st = dict(plan_checks=0, unknown=0, built=0, none=0, stale_none=0, transitions=Counter(), built_with_compact=0, weigh_in=0, kinds=Counter(),
              files=Counter())
    for seq, walk in walked_streams:
        last_check = {}
        with_compact = weigh_in = False
        for k, (at, step, why, exp, canon, state) in enumerate(walk):
            st["kinds"][step[0]] += 1
            if canon is None:
                continue
            pred = canon[0]
            st["plan_checks"] += 1
            st["unknown"] += pred[0] == "unknown" or canon[1] is None
            st["built"] += pred[0] == "built"
            st["none"] += pred[0] == "none"
            st["stale_none"] += pred[0] == "none" and state["ever_built"]
            with_compact = with_compact or (pred[0] == "built" and state["compact"])
            weigh_in = weigh_in or pred == ("none", "weigh-in")
            if state["nfiles"] == 1:
                st["files"][seq["world"]["pool"][state["f"]["i"]]["kind"]] += 1
            if state["plan_set"] == sc.SET_STRANDED:
                if step[1] in last_check:
                    for tr in transitions_between(walk, last_check[step[1]], k):
                        st["transitions"][TRANSITIONS[tr]] += 1
                last_check[step[1]] = k
        st["built_with_compact"] += with_compact
        st["weigh_in"] += weigh_in
    return st


def test_stream_seeds_follow_the_rules(walked_streams):
    """40-50 steps, the last one a check; at most two mutating steps between checks, never two of one kind; no check asks
    an engine without alignments; the recorded outcomes are the model's; the halo of every pool file is certain."""
    for seq, walk in walked_streams:
        assert 40 <= len(seq["steps"]) <= 50 and seq["steps"][-1][0] in sc.CHECK_KINDS, seq["seed"]
        assert all(sc.sm.certain_halo(p["file"]) and p["file"].n in (400, 1500, 4000) for p in seq["world"]["pool"])
        assert all(600 <= n < 9000 for n in seq["world"]["lens"])
        run, pending = 0, set()
        for (at, step, why, exp, canon, state), recorded in zip(walk, seq["outcomes"]):
            assert why == recorded
            if step[0] in sc.CHECK_KINDS:
                run, pending = 0, set()
                assert state["nfiles"] >= 1 and (exp is not None or why is not None), (seq["seed"], at)
            else:
                run += 1
                assert run <= 2 and step[0] not in pending, (seq["seed"], at, step)
                pending.add(step[0])


def test_stream_seeds_decide_the_canonical_stream_on_both_sides(walked_streams):
    """No plan check of a stream world is "unknown"; at least 40 % are predicted "built", at least 15 % "none" on an engine
    that had a stream built earlier in the sequence (the stale-stream case); in 8 sequences or more a "built" check has a
    file that also keeps a compact stream, in 4 or more an eligible check is predicted -1 by the weigh-in alone; both
    stream step kinds and the three knobs occur."""
    st = stream_statistics(walked_streams)
    assert st["plan_checks"] >= 400 and st["unknown"] == 0, st
    assert st["built"] >= 0.40 * st["plan_checks"], st
    assert st["stale_none"] >= 0.15 * st["plan_checks"], st
    assert st["built_with_compact"] >= 8 and st["weigh_in"] >= 4, st
    assert st["kinds"]["stream_entries"] >= 50 and st["kinds"]["canonical_entries"] >= 200, st["kinds"]
    knobs = Counter(k for seq, _ in walked_streams for s in seq["steps"] if s[0] == "reload_knobs" for k in s[1])
    assert all(knobs[k] >= 8 for k in sc.STREAM_KNOBS), knobs
    assert all(not (set(s[1]) & set(sc.STREAM_KNOBS)) for seed in SEEDS[:8] for s in [("reload_knobs", sc.random_knobs(np.random.default_rng(seed)))])


def test_stream_seeds_walk_every_transition(walked_streams):
    """Each transition that can leave a derived stream stale occurs at least 8 times over the 24 seeds, with an answered
    check of the same `stranded` plan on both sides."""
    st = stream_statistics(walked_streams)
    assert all(st["transitions"][name] >= 8 for name in TRANSITIONS), st["transitions"]


def test_stream_checks_would_see_a_stale_engine(walked_streams):
    """The conditions of test_checks_would_see_a_stale_engine for the stream seeds on their own.  They are about the
    count vectors: a stream_entries step reads one number and neither counts as a check here nor ends a change."""
    nsteps = nrefused = nchecks = nzero = followed = differ = 0
    for seq, walk in walked_streams:
        last, changed = {}, False
        for at, step, why, exp, canon, state in walk:
            nsteps += 1
            nrefused += why is not None
            if step[0] == "stream_entries":
                continue
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
    print("checks %d, zeros %d; steps %d, refused %d; followed %d, differ %d" % (nchecks, nzero, nsteps, nrefused, followed, differ))
    assert nchecks >= 400 and followed >= 150, (nchecks, followed)
    assert nzero <= 0.10 * nchecks, (nzero, nchecks)
    assert nrefused <= 0.15 * nsteps, (nrefused, nsteps)
    assert differ >= 0.80 * followed, (differ, followed)


def test_shrink_drops_what_the_predicate_does_not_need(pa):
    seq = sc.random_sequence(SEEDS[0], pa)
    target = next(s for s in seq["steps"] if s[0] == "set_mapping")
    small = sc.shrink(seq, lambda cand: target in cand["steps"])
    assert small["steps"] == [target]


if __name__ == "__main__":     # the measured shares next to the thresholds (docs/stateful_fuzz.md quotes them)
    import plastid_amd.packing as packing
    stats = stream_statistics(_walk_all(packing, sc.STREAM_SEEDS))
    for key in ("plan_checks", "unknown", "built", "none", "stale_none", "built_with_compact", "weigh_in"):
        print(key, stats[key])
    for name in TRANSITIONS:
        print("%4d  %s" % (stats["transitions"][name], name))
    print(dict(stats["files"]), dict(stats["kinds"]))
