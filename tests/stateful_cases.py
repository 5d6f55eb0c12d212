"""Stateful differential cases: SEQUENCES of operations on ONE engine vs the oracle (helper, not collected by pytest;
the sibling of fuzz_cases.py, whose cases are one-shot).

``random_sequence(seed, pa)`` draws a small world (contigs, a pool of alignment files with FLAG / MAPQ / NH columns kept
aside, two or three segment sets) and 30-50 steps; everything comes from ``np.random.default_rng(seed)``.
The seeds of STREAM_SEEDS get a world and steps of their own (``stream_world``, ``stream_sequence``), aimed at the derived
streams of a staged file; tests/stream_models.py holds the numpy models of those streams.

:class:`Model` holds only WHAT WAS ASKED FOR -- the staged files with the columns handed over so far, the caller's
exclusion masks, the filters, the mapping rule, the size filter, the normalisation, the open plans -- and computes every
expectation from scratch with the oracle.  It keeps no cache: the engine is the thing with state.  It also says when the
engine must refuse a step.

``run_sequence(pa, oracle, seq)`` applies every step to a real ``Engine`` and to the model and compares bit for bit at
every check step.  A failing assertion carries the seed, the step index and the op trace so far; to replay one::

    from tests import stateful_cases as sc
    seq = sc.random_sequence(SEED, pa)          # the world of that seed
    seq["steps"] = [...]                        # the trace of the message, pasted
    sc.run_sequence(pa, oracle, seq)

A step is a tuple ``(kind, arguments...)`` of ints, strings, tuples and dicts only (arrays are derived from seeds in the
step), so a trace prints as Python.  The vocabulary is STEP_KINDS below; docs/stateful_fuzz.md describes each kind.
"""
import os
import warnings

import numpy as np

import fuzz_cases
import stream_models as sm
from fuzz_cases import NOFILTER

#: every knob a sequence may set: the runner takes them out of the environment before and after
KNOBS = fuzz_cases.KNOBS + ("PC_HIST_MEMSET", "PC_NO_SINGLE", "PC_NO_CANON", "PC_NO_COMPACT", "PC_COMPACT_KEEP")
#: ... those of them that only the stream seeds draw (reload_knobs)
STREAM_KNOBS = KNOBS[-3:]

#: steps that change the engine (and, but for reload_knobs / open_plan / close_plan, what the model was asked for)
MUTATING_KINDS = ("add_file", "clear_alignments", "set_alignments", "set_alignment_sam", "set_alignment_nh", "update_flags",
                  "set_flag_filter", "set_nh_filter", "set_mapping", "set_size_filter", "set_normalize", "reload_knobs",
                  "open_plan", "close_plan")
#: ... those of them after which the expected vectors are other ones (the model's state changes)
STATE_KINDS = MUTATING_KINDS[:11]
#: the two read-only kinds of the stream seeds: the entry counts of the compact and of the canonical stream
STREAM_CHECK_KINDS = ("stream_entries", "canonical_entries")
CHECK_KINDS = ("count", "count_twice", "total", "warn_flags", "mapped_reads", "query_segment") + STREAM_CHECK_KINDS
#: ... the kinds that count a plan
PLAN_CHECK_KINDS = ("count", "count_twice", "total", "warn_flags", "canonical_entries")
STEP_KINDS = MUTATING_KINDS + CHECK_KINDS
#: why the engine must refuse a step
REFUSAL_KINDS = ("columns", "flag_filter_on", "nh_filter_on", "rows", "sums")

#: the committed seeds of tests/test_gpu_stateful.py (tests/test_stateful_model.py asserts what they cover)
SEEDS = tuple(range(2000, 2040))
#: the seeds of the stream-aimed sequences (a world and a generator of their own: the 40 above keep every draw)
STREAM_SEEDS = tuple(range(2100, 2124))

BIG_NSEG, BIG_STRIDE, BIG_CELL = 4200, 4400, 300   # the large segment set: one segment per 4400 nt, the reads squeezed into 300 of them
MAX_WINDOW = 4096                                  # no counting window is longer (choose_window, host_util.h)


# ---------------------------------------------------------------------------------------------------- the world
def _with_columns(pa, f, flag16=None, mapq=None, nh=None, flags=None):
    return pa.PackedAlignments(f.tid, f.pos, f.alen, f.flags if flags is None else flags, f.nblk, f.blk_start, f.blk_len,
                               references=f.references, lengths=f.lengths, validate=False, flag16=flag16, mapq=mapq, nh=nh)


def _squeeze_into_cells(pa, f):
    """The reads of contig 0 moved into the first BIG_CELL nt of every BIG_STRIDE (a monotonic map of the positions: the
    file stays sorted), so that the large, sparse segment set sees most of them."""
    pos = f.pos.astype(np.int64)
    on0 = f.tid == 0
    new = np.where(on0, pos // BIG_STRIDE * BIG_STRIDE + pos % BIG_STRIDE * BIG_CELL // BIG_STRIDE, pos)
    delta = new - pos
    off = f.block_offsets()
    bs = f.blk_start.astype(np.int64)
    for i in np.nonzero((f.nblk >= 2) & (delta != 0))[0]:
        bs[off[i]:off[i] + int(f.nblk[i])] += delta[i]
    return pa.PackedAlignments(f.tid, new, f.alen, f.flags, f.nblk, bs.astype(np.int32), f.blk_len, references=f.references,
                               lengths=f.lengths, validate=False)


def _layout(segset, rows):
    """Output layout of a segment set for `rows` rows, as fuzz_cases.run_case lays its plans out."""
    lens_ = segset["end"] - segset["start"]
    nseg = len(lens_)
    if segset["layout"] == "chain":      # the segments are one spliced chain, stored 5'->3' (engine.chain_layout)
        from plastid_amd.engine import chain_layout
        _, out_off, step, stride, _, _, out_elems = chain_layout([list(zip(segset["start"].tolist(), segset["end"].tolist()))],
                                                                 [segset["chain_strand"]], rows)
    elif segset["layout"] == "sums":
        step = np.zeros(nseg, np.int8)
        out_off = segset["slot"] * rows
        stride = np.ones(nseg, np.int64)
        out_elems = 7 * rows
    else:
        step = segset["step"]
        base = np.concatenate([[0], np.cumsum(lens_ * rows)[:-1]]).astype(np.int64)
        out_off = np.where(step > 0, base, base + lens_ - 1)
        stride = lens_.astype(np.int64)
        out_elems = int((lens_ * rows).sum())
    return dict(out_off=out_off.astype(np.int64), step=step, stride=stride, out_elems=out_elems)


def _random_mapping(rng, strat):
    kind = str(rng.choice(["fiveprime", "threeprime", "center", "variable", "stratified"]))
    if kind in ("fiveprime", "threeprime"):
        return (kind, int(rng.choice([0, 3, 12, 30])))
    if kind == "center":
        return (kind, int(rng.choice([0, 2, 12])))
    od = {int(L): int(rng.integers(0, L)) for L in rng.integers(10, 60, int(rng.integers(1, 10)))}
    od["default"] = int(rng.integers(0, 14))
    items = tuple(sorted((k for k in od if k != "default"))) + ("default",)
    od = tuple((k, od[k]) for k in items)          # (a tuple of pairs: prints as Python, keeps its order)
    if kind == "variable":
        return (kind, od)
    return (kind, od, strat[0], strat[1])


def mapping_of(m):
    """The step's mapping as fuzz_cases / synth.mapping_factory spell it (offset dictionary as a dict)."""
    if m[0] in ("variable", "stratified"):
        return (m[0], dict(m[1])) + tuple(m[2:])
    return m


def rows_of(m):
    return m[3] - m[2] + 1 if m[0] == "stratified" else 1


def random_world(rng, pa, seed):
    big = seed % 4 == 1
    ntid = int(rng.integers(1, 5))
    names = ["c%d" % i for i in range(ntid)]
    lens = [int(rng.integers(600, 9000)) for _ in range(ntid)]
    if big:
        lens[0] = BIG_NSEG * BIG_STRIDE + 5000
    max_len = int(rng.choice([44, 200, 255, 256, 2500]))
    pool = []
    for k in range(int(rng.integers(3, 5))):
        n = 20000 if big and k < 2 else int(rng.choice([400, 1500, 4000]))
        f = fuzz_cases.random_file(rng, pa, names, lens, n, max_len, float(rng.choice([0.0, 0.05, 0.4])),
                                   float(rng.choice([0.0, 0.1, 0.5])), bool(rng.random() < 0.5))
        if k == 1:
            f = fuzz_cases.lengthen_last_runs(np.random.default_rng(seed + 1000003), pa, f)
        if big:
            f = _squeeze_into_cells(pa, f)
        flag16 = (rng.integers(0, 1 << 12, f.n) & rng.integers(0, 1 << 12, f.n)).astype(np.uint16)
        flag16 = (flag16 & ~np.uint16(0x10)) | ((f.flags & 1).astype(np.uint16) << 4)     # (the strand bit, as a BAM file has it)
        mapq = rng.choice(np.array([0, 1, 3, 10, 30, 42, 60, 255], np.uint8), f.n)
        u = rng.random(f.n)
        nh = np.where(u < 0.15, 0, np.where(u < 0.65, 1, rng.integers(2, 12, f.n))).astype(np.uint16)   # 0: no tag
        pool.append(dict(file=f, flag16=flag16, mapq=mapq, nh=nh, full=_with_columns(pa, f, flag16, mapq, nh)))
    # ---- the segment sets
    t = int(np.argmax([((pool[0]["file"].tid == i).sum()) for i in range(ntid)]))     # where file 0 has most reads
    f0 = pool[0]["file"]
    if big:      # the cell with most reads of file 0
        t = 0
        a = int(np.argmax(np.bincount(f0.pos[f0.tid == 0] // BIG_STRIDE, minlength=BIG_NSEG))) * BIG_STRIDE
        b = a + int(rng.integers(200, 300))
    else:        # around the median read of file 0 on that contig
        ln = int(rng.integers(200, min(lens[t], 3000)))
        mid = int(np.median(f0.pos[f0.tid == t])) if (f0.tid == t).any() else lens[t] // 2
        a = min(max(0, mid - int(rng.integers(0, ln))), lens[t] - ln)
        b = a + ln
    single = dict(name="single", tid=np.array([t], np.int32), start=np.array([a], np.int64), end=np.array([b], np.int64),
                  strand=np.array([int(rng.choice([1, 2, 3, 3]))], np.uint8), layout="forward", step=np.ones(1, np.int8))
    nseg = int(rng.integers(5, 40))
    seg_tid = rng.integers(-1, ntid + 1, nseg).astype(np.int32)
    seg_tid[rng.random(nseg) < 0.5] = int(rng.integers(1 if big and ntid > 1 else 0, ntid))
    seg_start, seg_end = np.zeros(nseg, np.int64), np.zeros(nseg, np.int64)
    for s in range(nseg):
        ln = min(lens[seg_tid[s]], 9000) if 0 <= seg_tid[s] < ntid else 5000
        a = int(rng.integers(0, ln))
        mode = rng.random()
        if mode < 0.08:
            b = a
        elif mode < 0.25:
            b = a + int(rng.integers(1, 40))
        elif mode < 0.4:
            a, b = 0, ln + int(rng.integers(0, 300))
        else:
            b = a + int(rng.integers(1, 5000))
        seg_start[s], seg_end[s] = a, b
    layout = str(rng.choice(["forward", "reversed", "mixed", "sums", "sums"]))
    batch = dict(name="batch", tid=seg_tid, start=seg_start, end=seg_end,
                 strand=rng.choice(np.array([0, 1, 1, 2, 2, 3, 1 | NOFILTER, 2 | NOFILTER], np.uint8), nseg), layout=layout,
                 step={"forward": np.ones(nseg, np.int8), "reversed": -np.ones(nseg, np.int8), "sums": np.zeros(nseg, np.int8),
                       "mixed": rng.choice(np.array([1, -1], np.int8), nseg)}[layout],
                 slot=rng.integers(0, 7, nseg).astype(np.int64))
    segsets = [single, batch]
    if big:
        # one short segment per BIG_STRIDE nt: no two of them fit one counting window (MAX_WINDOW), so the plan has at
        # least BIG_NSEG >= 4096 tiles whatever window size the knobs choose
        st = np.arange(BIG_NSEG, dtype=np.int64) * BIG_STRIDE + rng.integers(0, 40, BIG_NSEG)
        segsets.append(dict(name="big", tid=np.zeros(BIG_NSEG, np.int32), start=st, end=st + rng.integers(30, 250, BIG_NSEG),
                            strand=rng.choice(np.array([1, 2, 3], np.uint8), BIG_NSEG), layout="mixed",
                            step=rng.choice(np.array([1, -1], np.int8), BIG_NSEG)))
    lo = int(rng.integers(15, 35))
    strat = (lo, lo + int(rng.integers(1, 8)))
    return dict(seed=seed, names=names, lens=lens, pool=pool, segsets=segsets, strat=strat, big=big,
                mapping0=("fiveprime", int(rng.choice([0, 3, 12]))))


def min_tiles(segset):
    """A lower bound of the plan's tile count from the segment arithmetic alone: segments on one contig whose starts lie
    further apart than the longest window plus their own length cannot share a tile."""
    order = np.argsort(segset["start"], kind="stable")
    s, e = segset["start"][order], segset["end"][order]
    if len(set(segset["tid"].tolist())) != 1 or not len(s):
        return 1
    apart = np.concatenate([[True], s[1:] - e[:-1] > MAX_WINDOW])
    return int(apart.sum())


# ---------------------------------------------------------------------------------------------------- the model
FILTER_OFF = (None, 0)      # (FLAG / MAPQ filter, NH bound) of an engine without a filter


class Model(object):
    """What the caller asked for, and nothing derived from it."""

    def __init__(self, world):
        self.world = world
        self.files = []          # dict(i=pool index, sam=bool, nh=bool, mask=bool array: the caller's exclusions)
        self.flag_filter = None  # (require, exclude, min_mapq) or None
        self.max_nh = 0
        self.mapping = world["mapping0"]
        self.size_filter = None
        self.norm = None         # the total, or None
        self.plans = {}          # plan id -> dict(set=index, rows=rows it was laid out for)
        self.knobs = {}
        self.ever_built = False  # some count of this sequence had a canonical stream built (stream bookkeeping below)

    # ---- state
    def snapshot(self):
        """The whole state as plain, comparable values."""
        return repr(([(f["i"], f["sam"], f["nh"], f["mask"].tobytes()) for f in self.files], self.flag_filter, self.max_nh,
                     self.mapping, self.size_filter, self.norm, sorted(self.plans.items()), sorted(self.knobs.items())))

    def rows(self):
        return rows_of(self.mapping)

    def natural_dtype(self):
        """The dtype a canonical_entries step counts in: int64 where the counts are integers."""
        return "int64" if self.mapping[0] != "center" and self.norm is None else "float64"

    def lazy(self):
        return self.knobs.get("PC_HIST_LAZY_BYTES") == "1" and "PC_HIST_MEMSET" not in self.knobs

    def _staged(self, i, sam, nh):
        """A file as staging leaves it, then its columns in the order Engine.add_alignment_file hands them over."""
        f = self.world["pool"][i]["file"]
        d = dict(i=i, sam=False, nh=False, mask=(f.flags & 0x80) != 0, applied=FILTER_OFF, valid=True, gen=0, cknobs=None, last=None)
        self._rebuilt(d)
        self.files.append(d)
        if sam:
            self._columns_arrive(d, "sam")
        if nh:
            self._columns_arrive(d, "nh")

    # ---- the engine's bookkeeping of the stream words, restated (pc_update_flags, sync_flag_filter, pc_set_alignment_sam /
    # _nh, build_compact_stream): WHEN a file's words are rewritten -- that is when the compact stream is rebuilt, under the
    # knobs of that moment, and when the canonical stream goes stale -- and WHICH filter's verdicts its exclusion bits hold
    def compact_knobs(self):
        keep = min(1.0, max(0.0, float(self.knobs["PC_COMPACT_KEEP"]))) if "PC_COMPACT_KEEP" in self.knobs else sm.KEEP
        return ("PC_NO_COMPACT" in self.knobs, keep)

    def _rebuilt(self, f):
        f["gen"] += 1
        f["cknobs"] = self.compact_knobs()

    def _columns_present(self, f):
        return (self.flag_filter is None or f["sam"]) and (not self.max_nh or f["nh"])

    def _sync_filter(self):
        want = (self.flag_filter, self.max_nh)
        for f in self.files:
            if self.world["pool"][f["i"]]["file"].n == 0 or not self._columns_present(f):
                continue
            if f["valid"] and f["applied"] == want:
                continue
            if not f["sam"] and not f["nh"] and want == FILTER_OFF:
                continue
            f["applied"], f["valid"] = want, True
            self._rebuilt(f)

    def _columns_arrive(self, f, which):
        f[which] = True
        if which == "sam" and (self.flag_filter is not None or f["applied"][0] is not None):
            f["valid"] = False
        if which == "nh" and (self.max_nh or f["applied"][1]):
            f["valid"] = False
        self._sync_filter()

    def excluded_bits(self, k):
        """The exclusion bits staged file `k` holds right now: the caller's, and the verdicts of the filter last applied
        to it (the engine's own filter wherever a count is answered)."""
        f = self.files[k]
        p = self.world["pool"][f["i"]]
        out = f["mask"].copy()
        ff, max_nh = f["applied"]
        if ff is not None:
            flag = p["flag16"].astype(np.int64)
            out |= ((flag & ff[0]) != ff[0]) | ((flag & ff[1]) != 0) | (p["mapq"] < ff[2])
        if max_nh:
            out |= (p["nh"] == 0) | (p["nh"] > max_nh)
        return out

    def expected_stream_entries(self, k):
        """``Engine.stream_entries(k)``: the compact model under the file's exclusion bits and the knobs of its last build."""
        f = self.files[k]
        pf = self.world["pool"][f["i"]]["file"]
        cn = sm.compact_prediction(pf, self.excluded_bits(k), *f["cknobs"])
        return pf.n if cn is None else cn

    def canonical_check(self, pid):
        """One answered count of plan `pid`, as far as the canonical stream of staged file 0 goes.  Returns
        ``(prediction, entries)``: `prediction` as ``stream_models.canonical_prediction`` gives it -- but where the file's
        stream was built under the very signature before, that verdict stands (PC_COMPACT_KEEP is read at the build and
        is no part of the signature); `entries`: what ``Engine.canonical_entries(0)`` must say afterwards (None: unknown).
        The file's ``last`` -- signature and verdict of the last eligible count -- is all that is kept, and nothing of it
        comes from an engine."""
        plan = self.plans[pid]
        segset = self.world["segsets"][plan["set"]]
        f = self.files[0]
        pf = self.world["pool"][f["i"]]["file"]
        no_canon = "PC_NO_CANON" in self.knobs
        excluded = self.excluded_bits(0)
        flags = ((pf.flags & 1) | np.where(excluded, 0x80, 0)).astype(np.uint8)
        modes = sm.plan_modes_eligible(segset["strand"], segset["tid"], segset["start"], segset["end"], self.world["lens"])
        pred = sm.canonical_prediction(len(self.files), mapping_of(self.mapping), self.size_filter, plan["rows"], modes, pf, flags, no_canon,
                                       sm.compact_prediction(pf, excluded, *f["cknobs"]), self.compact_knobs()[1])
        eligible = pred[0] == "built" or (pred[0] == "none" and pred[1] in ("weigh-in", "no valid length", "halo"))
        if eligible and not segset.get("several_windows"):
            pred = ("unknown",)       # (a plan of one window may be counted by the single launch, which builds no stream)
        if pred[0] == "unknown":
            f["last"] = "unknown"
        elif eligible and f["last"] != "unknown":
            sig = sm.canonical_signature(pf, mapping_of(self.mapping), self.size_filter, f["gen"])
            if f["last"] is None or f["last"][0] != sig:
                f["last"] = (sig, pred[1] if pred[0] == "built" else -1)
            elif f["last"][1] >= 0:
                pred = ("built", f["last"][1])
            elif pred[0] == "built":
                pred = ("none", "weigh-in")
            self.ever_built = self.ever_built or f["last"][1] >= 0
        elif eligible:
            pred = ("unknown",)
        if no_canon or len(self.files) != 1:
            return pred, -1
        if f["last"] == "unknown":
            return pred, None
        return pred, f["last"][1] if f["last"] is not None and f["last"][0][-1] == f["gen"] else -1

    def missing_columns(self, flag_filter="current", max_nh="current"):
        ff = self.flag_filter if flag_filter == "current" else flag_filter
        k = self.max_nh if max_nh == "current" else max_nh
        for f in self.files:
            if self.world["pool"][f["i"]]["file"].n == 0:
                continue
            if (ff is not None and not f["sam"]) or (k and not f["nh"]):
                return True
        return False

    def apply(self, step):
        """Take a mutating step.  Returns None, or the reason why the engine must refuse it -- the state is then unchanged."""
        kind = step[0]
        if kind == "add_file":
            self._staged(*step[1:])
        elif kind == "clear_alignments":
            self.files = []
        elif kind == "set_alignments":
            self.files = []
            for a in step[1]:
                self._staged(*a)
        elif kind == "set_alignment_sam":
            self._columns_arrive(self.files[step[1]], "sam")
        elif kind == "set_alignment_nh":
            self._columns_arrive(self.files[step[1]], "nh")
        elif kind == "update_flags":
            f = self.files[step[1]]
            n = self.world["pool"][f["i"]]["file"].n
            f["mask"] = caller_mask(n, step[2], step[3])
            if n:
                f["applied"], f["valid"] = FILTER_OFF, True
                if (self.flag_filter is not None or self.max_nh) and self._columns_present(f):
                    f["applied"] = (self.flag_filter, self.max_nh)
                self._rebuilt(f)
        elif kind == "set_flag_filter":
            new = None if step[1] is None else tuple(step[1])
            if new != self.flag_filter and new is not None and self.missing_columns(flag_filter=new, max_nh=0):
                return "flag_filter_on"
            if new != self.flag_filter:
                self.flag_filter = new
                self._sync_filter()
        elif kind == "set_nh_filter":
            if step[1] != self.max_nh and step[1] and self.missing_columns(flag_filter=None, max_nh=step[1]):
                return "nh_filter_on"
            if step[1] != self.max_nh:
                self.max_nh = step[1]
                self._sync_filter()
        elif kind == "set_mapping":
            self.mapping = step[1]
        elif kind == "set_size_filter":
            self.size_filter = step[1]
        elif kind == "set_normalize":
            self.norm = step[1]
        elif kind == "reload_knobs":
            self.knobs = dict(step[1])
        elif kind == "open_plan":
            self.plans[step[1]] = dict(set=step[2], rows=self.rows())
        elif kind == "close_plan":
            del self.plans[step[1]]
        else:
            raise ValueError(kind)
        return None

    def refusal(self, step):
        """Why the engine must refuse this check step (None: it must answer), in the order the engine tests."""
        kind = step[0]
        if kind in PLAN_CHECK_KINDS:
            plan = self.plans[step[1]]
            if plan["rows"] != self.rows():
                return "rows"
            if self.missing_columns():
                return "columns"
            if self.world["segsets"][plan["set"]]["layout"] == "sums" and (self.mapping[0] == "center" or self.norm is not None):
                return "sums"
            return None
        if kind == "stream_entries":     # (reads no exclusion bit of a record: never refused)
            return None
        return "columns" if self.missing_columns() else None

    # ---- expectations, from scratch
    def _kept(self, oracle, only_file=None):
        """The records that remain: caller's bits, then FLAG / MAPQ, then NH (tests/test_oracle_golden.py::flag_excluded).
        Returns the oracle's input and, per remaining record, (file, index in the staged file)."""
        from plastid_amd.packing import concat_file_major
        from tests.test_oracle_golden import flag_excluded
        files = self.files if only_file is None else [self.files[only_file]]
        kept, origin = [], []
        for k, f in enumerate(files):
            idx = np.nonzero(~f["mask"])[0]
            kept.append(self.world["pool"][f["i"]]["full"].subset(idx))
            origin.append(idx)
        req, exc, mq = self.flag_filter if self.flag_filter is not None else (0, 0, 0)
        aln, _drop, keep = flag_excluded(concat_file_major(kept), req, exc, mq, self.max_nh)
        return aln, np.concatenate(origin)[keep]

    def spec(self, oracle):
        m = mapping_of(self.mapping)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            if m[0] in ("fiveprime", "threeprime", "center"):
                return oracle.mapping_spec(m[0], m[1], size_filter=self.size_filter)
            if m[0] == "variable":
                return oracle.mapping_spec(m[0], 0, m[1], size_filter=self.size_filter)
            return oracle.mapping_spec(m[0], 0, m[1], m[2], m[3], size_filter=self.size_filter)

    def _segments(self, oracle, aln, segset):
        """Per-segment oracle arrays; the two "no strand filter" codes as in fuzz_cases.oracle_expected."""
        spec = self.spec(oracle)
        st = segset["strand"]
        ostrand = np.where(st == (1 | NOFILTER), 3, st & 3).astype(np.uint8)
        arrays, warn = oracle.count_segments(aln, spec, segset["tid"], segset["start"], segset["end"], ostrand)
        nf = np.nonzero(st == (2 | NOFILTER))[0]
        if len(nf):
            a2, w2 = oracle.count_segments(dict(aln, flags=aln["flags"] | np.uint8(1)), spec, segset["tid"][nf],
                                           segset["start"][nf], segset["end"][nf], ostrand[nf])
            for k, s in enumerate(nf):
                arrays[s] = a2[k]
                warn[s] = w2[k]
        return arrays, warn

    def _normalised(self, exp):
        return exp if self.norm is None else exp.astype(np.float64) / self.norm * 1e6

    def expected_plan(self, oracle, pid):
        """``(vector, warn_flags)`` of plan `pid`: int64 (float64 under the center rule or normalised)."""
        plan = self.plans[pid]
        segset = self.world["segsets"][plan["set"]]
        rows = plan["rows"]
        lay = _layout(segset, rows)
        aln, _ = self._kept(oracle)
        arrays, warn = self._segments(oracle, aln, segset)
        exp = np.zeros(lay["out_elems"], np.float64 if self.mapping[0] == "center" else np.int64)
        for s, arr in enumerate(arrays):
            a2 = arr.reshape(rows, -1)
            for r in range(rows):
                if segset["layout"] == "sums":
                    exp[lay["out_off"][s] + r] += a2[r].sum()
                else:
                    idx = lay["out_off"][s] + int(lay["step"][s]) * np.arange(a2.shape[1]) + r * lay["stride"][s]
                    exp[idx] = a2[r]
        return self._normalised(exp), warn

    def expected_query(self, oracle, reverse):
        aln, _ = self._kept(oracle)
        arrays, _ = self._segments(oracle, aln, self.world["segsets"][0])
        a = arrays[0][::-1] if reverse else arrays[0]
        return self._normalised(np.ascontiguousarray(a))

    def expected_mapped_reads(self, oracle, f):
        """``reads_out`` mask over the records of staged file `f` for the one-window segment."""
        aln, origin = self._kept(oracle, only_file=f)
        sg = self.world["segsets"][0]
        _, _, mapped = oracle.count_segments(aln, self.spec(oracle), sg["tid"], sg["start"], sg["end"], sg["strand"], want_mapped=True)
        mask = np.zeros(self.world["pool"][self.files[f]["i"]]["file"].n, np.uint8)
        mask[origin[np.nonzero(mapped[0])[0]]] = 1
        return mask


def caller_mask(n, seed, share):
    """The caller's exclusions of an update_flags step: `share` percent of the records, drawn from `seed` (0: lifted)."""
    return np.random.default_rng(seed).random(n) < share / 100.0


# ---------------------------------------------------------------------------------------------------- the generator
def random_knobs(rng, was_lazy=False):
    """A new draw of the knobs; the lazy histogram mostly changes sides (PC_HIST_MEMSET=1 is one way of turning it off)."""
    k = {}
    if rng.random() < (0.3 if was_lazy else 0.7):
        k["PC_HIST_LAZY_BYTES"] = "1"
    elif rng.random() < 0.4:
        k["PC_HIST_LAZY_BYTES"] = "1"
        k["PC_HIST_MEMSET"] = "1"
    if rng.random() < 0.7:
        k["PC_TILE_G"] = str(int(rng.choice([256, 512, 768, 1024, 4096])))
        k["PC_WORK_R"] = str(int(rng.choice([64, 512, 4096, 32768])))
        k["PC_PILE"] = str(int(rng.choice([64, 2048, 1000000])))
    if rng.random() < 0.25:
        k["PC_NO_SMALL"] = "1"
    if rng.random() < 0.25:
        k["PC_NO_SINGLE"] = "1"
    if rng.random() < 0.25:
        k["PC_RANGES_CG1"] = "1"
    return k


FLAG_FILTERS = ((0, 0x100, 0), (0, 0x904, 0), (0x1, 0, 0), (0, 0, 10), (0x2, 0x400, 3), (0, 0x10, 0), (0, 0, 30), (0x40, 0x8, 1))


def random_sequence(seed, pa):
    """The world and the steps of sequence `seed`.  Also returns, per step, what the model says must happen
    (``outcomes[i]``: None, or the refusal kind) -- the generator runs the model (never the oracle) to know what is staged."""
    if seed in STREAM_SEEDS:
        return stream_sequence(seed, pa)
    rng = np.random.default_rng(seed)
    world = random_world(rng, pa, seed)
    model = Model(world)
    nsteps = int(rng.integers(30, 51))
    steps, outcomes = [], []
    unchecked = set()        # mutating kinds since the last check
    since_check = 0
    next_plan = 0
    npool = len(world["pool"])
    last_counted = [None]

    def emit(step):
        nonlocal since_check
        if step[0] in CHECK_KINDS:
            out = model.refusal(step)
            if step[0] in ("count", "count_twice", "total", "warn_flags"):
                last_counted[0] = step[1]
            unchecked.clear()
            since_check = 0
        else:
            out = model.apply(step)
            unchecked.add(step[0])
            since_check += 1
        steps.append(step)
        outcomes.append(out)

    def columns():
        u = rng.random()
        return (True, True) if u < 0.55 else (True, False) if u < 0.7 else (False, True) if u < 0.85 else (False, False)

    def draw_check():
        pids = sorted(model.plans)
        fit = [p for p in pids if model.plans[p]["rows"] == model.rows()]
        pid = int(rng.choice(fit)) if fit and rng.random() < 0.9 else int(rng.choice(pids))
        if last_counted[0] in fit and rng.random() < 0.5:      # the same plan again: what it cached is what could be stale
            pid = last_counted[0]
        point = model.mapping[0] != "center" and model.norm is None
        u = rng.random()
        if u < 0.08:
            return ("mapped_reads", int(rng.integers(0, len(model.files))))
        if u < 0.2 and len(model.files) == 1 and model.mapping[0] in ("fiveprime", "threeprime", "variable"):
            return ("query_segment", bool(rng.random() < 0.5), "int64" if point and rng.random() < 0.5 else "float64")
        dtype = "int64" if point and rng.random() < 0.6 else "float64"
        if u < 0.4:
            return ("count_twice", pid, dtype)
        if u < 0.55 and point:
            return ("total", pid, "int64")
        if u < 0.7:
            return ("warn_flags", pid, dtype)
        return ("count", pid, dtype)

    def draw_mutation(state_only=False):
        nf = len(model.files)
        kinds = ["add_file", "clear_alignments", "set_alignments", "set_alignment_sam", "set_alignment_nh", "update_flags",
                 "set_flag_filter", "set_nh_filter", "set_mapping", "set_size_filter", "set_normalize", "reload_knobs",
                 "open_plan", "close_plan"]
        w = np.array([2.0 if nf < 3 else 0.3, 0.5, 1.0, 1.5, 1.5, 2.5, 3.0, 2.5, 3.5, 1.5, 1.2, 3.0,
                      1.5 if len(model.plans) < 4 else 0.0, 1.0 if len(model.plans) > 1 else 0.0])
        if state_only:
            w[11:] = 0.0
        kind = str(rng.choice(kinds, p=w / w.sum()))
        if kind == "add_file":
            return ("add_file", int(rng.integers(0, npool))) + columns()
        if kind == "clear_alignments":
            return ("clear_alignments",)
        if kind == "set_alignments":
            return ("set_alignments", tuple((int(rng.integers(0, npool)),) + columns() for _ in range(int(rng.integers(1, 3)))))
        if kind in ("set_alignment_sam", "set_alignment_nh"):
            lack = [k for k, f in enumerate(model.files) if not f["sam" if kind == "set_alignment_sam" else "nh"]]
            f = int(rng.choice(lack)) if lack else int(rng.integers(0, nf))     # (again for a file that has them: the same columns)
            return (kind, f)
        if kind == "update_flags":
            return ("update_flags", int(rng.integers(0, nf)), int(rng.integers(0, 1 << 30)), int(rng.choice([0, 0, 10, 30, 60])))
        if kind == "set_flag_filter":
            if model.flag_filter is not None and rng.random() < 0.4:
                return ("set_flag_filter", None)
            return ("set_flag_filter", FLAG_FILTERS[int(rng.integers(0, len(FLAG_FILTERS)))])
        if kind == "set_nh_filter":
            if model.max_nh and rng.random() < 0.4:
                return ("set_nh_filter", 0)
            return ("set_nh_filter", int(rng.choice([1, 1, 2, 5])))
        if kind == "set_mapping":
            return ("set_mapping", _random_mapping(rng, world["strat"]))
        if kind == "set_size_filter":
            if model.size_filter is not None and rng.random() < 0.5:
                return ("set_size_filter", None)
            lo = int(rng.integers(10, 35))
            return ("set_size_filter", (lo, int(rng.choice([-1, lo + 3, lo + 10, 400]))))
        if kind == "set_normalize":
            if model.norm is not None and rng.random() < 0.6:
                return ("set_normalize", None)
            return ("set_normalize", float(rng.integers(1, 10 ** 9)))
        if kind == "reload_knobs":
            return ("reload_knobs", random_knobs(rng, model.lazy()))
        if kind == "open_plan":
            return ("open_plan", -1, int(rng.integers(0, len(world["segsets"]))))
        return ("close_plan", int(rng.choice(sorted(model.plans))))

    # the first steps: a file with its columns, a plan of every segment set
    emit(("add_file", 0, True, True))
    for k in range(len(world["segsets"])):
        emit(("open_plan", next_plan, k))
        next_plan += 1
        emit(("count", next_plan - 1, "int64"))
    while len(steps) < nsteps - 3:       # (one turn of the loop emits up to three steps)
        if since_check >= 2 or not model.files:
            if not model.files:
                emit(("add_file", int(rng.integers(0, npool))) + columns())
            emit(draw_check())
            continue
        # a step that changes the engine but not what was asked for (knobs, plans) is mostly followed by one that does,
        # before the next check: the check then expects another vector, and a stale engine shows
        engine_only = bool(steps) and steps[-1][0] in MUTATING_KINDS[11:]
        if rng.random() < (0.1 if engine_only else 0.3):
            emit(draw_check())
            continue
        step = draw_mutation(state_only=engine_only)
        new_rows = step[0] == "set_mapping" and not any(p["rows"] == rows_of(step[1]) for p in model.plans.values()) and len(model.plans) < 6
        if step[0] in unchecked or (step[0] == "clear_alignments" and since_check) or (new_rows and since_check):
            emit(draw_check())
        if step[0] in ("set_alignment_sam", "set_alignment_nh", "update_flags") and not (step[1] < len(model.files)):
            continue
        if step[0] == "open_plan":
            step = ("open_plan", next_plan, step[2])
            next_plan += 1
        emit(step)
        if new_rows:                            # a rule of another row count: a plan laid out for it
            emit(("open_plan", next_plan, int(rng.integers(0, len(world["segsets"])))))
            next_plan += 1
        if step[0] == "clear_alignments":       # (no check step asks an engine without alignments)
            emit(("add_file", int(rng.integers(0, npool))) + columns())
    while steps[-1][0] not in CHECK_KINDS or len(steps) < nsteps:
        emit(draw_check())
    return dict(seed=seed, world=world, steps=steps, outcomes=outcomes)


# ---------------------------------------------------------------------------------------------------- the stream seeds
# A world and a generator of their own (STREAM_SEEDS), aimed at the two derived streams of a staged file: the compact
# stream (rebuilt behind every rewrite of the stream words) and the canonical stream (built at the first count of an
# eligible plan, keyed by a signature).  docs/stateful_fuzz.md lists the transitions; tests/test_stateful_model.py
# counts them.  Every single-run read is at most 44 nt and no span exceeds 64, so the halo of every file is certain
# (stream_models.certain_halo) and the model has a verdict at every plan check.
STREAM_FILE_KINDS = ("dups", "ends", "one_length", "other_range")


def _stream_file(rng, pa, names, lens, n, kind):
    """One pool file of a stream world; the last contig gets no reads.
    dups         two lengths per site and strand, several exact copies of each: a compact stream, and a canonical one
    ends         per site four reads with a common start and four with a common end, all lengths different: no exact
                 duplicate (no compact stream), yet the canonical stream merges them
    one_length   every read 30 nt, several copies per site and strand: the canonical stream has what the compact one
                 has, the weigh-in fails
    other_range  lengths 15 .. 28 at few sites: another entry-table range than the other files'
    The reads of `dups` and `one_length` lie on one contig (see below).  Every kind carries a few two-run reads (the run stream), records without aligned positions and reads of 2 .. 12 nt."""
    nt = len(names) - 1
    rows = []          # (tid, pos, L, reverse)
    # a compaction tile (2 048 consecutive records) over two contigs merges nothing, so the files that are to keep a compact
    # stream have their reads on ONE contig -- but for a fifth of the largest `dups` file: its second tile stays as it is
    home = int(rng.integers(0, nt)) if kind in ("dups", "one_length") else None
    home_share = 0.8 if kind == "dups" and n >= 4000 else 1.0

    def site():
        t = home if home is not None and rng.random() < home_share else int(rng.integers(0, nt))
        return t, int(rng.integers(0, lens[t] - 70))
    nextra = max(3, n // 60)
    nedge = 5 * (nt if home is None or home_share < 1.0 else 1)
    while len(rows) < n - nextra - nedge:
        t, a = site()
        rev = int(rng.integers(0, 2))
        if kind == "dups":
            for L in rng.choice(np.arange(24, 41), 2, replace=False):
                rows += [(t, a, int(L), rev)] * int(rng.integers(3, 10))
        elif kind == "ends":
            for L in rng.choice(np.arange(20, 45), 4, replace=False):
                rows.append((t, a, int(L), rev))
            for L in rng.choice(np.arange(20, 45), 4, replace=False):
                rows.append((t, a + 45 - int(L), int(L), rev))
        elif kind == "one_length":
            rows += [(t, a, 30, rev)] * int(rng.integers(2, 7))
        else:
            for _ in range(int(rng.integers(1, 4))):
                rows += [(t, a + int(rng.integers(0, 3)), int(rng.integers(15, 29)), rev)] * int(rng.integers(1, 5))
    del rows[n - nextra - nedge:]      # (exactly n records in the end)
    for t in (range(nt) if home is None or home_share < 1.0 else [home]):    # the first positions of a contig and its last
        rows += [(t, 0, 30, 0), (t, 0, 30, 1), (t, 1, 27 if kind != "one_length" else 30, 0), (t, lens[t] - 30, 30, 0), (t, lens[t] - 30, 30, 1)]
    extra = []             # (tid, pos, runs or L, reverse)
    for _ in range(nextra):
        t, a = site()
        u = rng.random()
        if u < 0.45:       # two runs, span at most 55 (binned from the run stream, never from the canonical one)
            l1, gap, l2 = int(rng.integers(8, 20)), int(rng.integers(3, 16)), int(rng.integers(8, 20))
            extra.append((t, a, [(a, l1), (a + l1 + gap, l2)], int(rng.integers(0, 2))))
        elif u < 0.6:      # no aligned position at all
            extra.append((t, a, 0, int(rng.integers(0, 2))))
        else:              # shorter than most offsets
            extra.append((t, a, int(rng.integers(2, 13)), int(rng.integers(0, 2))))
    recs = [(t, p, L, r) for (t, p, L, r) in rows] + extra
    order = sorted(range(len(recs)), key=lambda i: (recs[i][0], recs[i][1]))     # (stable)
    tid, pos, alen, nblk, flags, bs, bl = [], [], [], [], [], [], []
    for i in order:
        t, p, L, r = recs[i]
        tid.append(t)
        pos.append(p)
        flags.append(r)
        if isinstance(L, list):
            alen.append(sum(x[1] for x in L))
            nblk.append(len(L))
            bs += [x[0] for x in L]
            bl += [x[1] for x in L]
        else:
            alen.append(L)
            nblk.append(1 if L else 0)
    flags = np.array(flags, np.uint8)
    flags[rng.random(len(flags)) < 0.03] |= 0x80
    return pa.PackedAlignments(np.array(tid, np.int32), np.array(pos, np.int64), np.array(alen, np.int64), flags, np.array(nblk, np.int64),
                               np.array(bs, np.int32), np.array(bl, np.int32), references=names, lengths=lens, validate=False)


def stream_world(rng, pa, seed):
    ntid = int(rng.integers(3, 5))
    names = ["c%d" % i for i in range(ntid)]
    lens = [int(rng.integers(600, 9000)) for _ in range(ntid)]
    pool = []
    for kind in STREAM_FILE_KINDS:
        f = _stream_file(rng, pa, names, lens, int(rng.choice([400, 1500, 4000])), kind)
        flag16 = (rng.integers(0, 1 << 12, f.n) & rng.integers(0, 1 << 12, f.n)).astype(np.uint16)
        flag16 = (flag16 & ~np.uint16(0x10)) | ((f.flags & 1).astype(np.uint16) << 4)
        mapq = rng.choice(np.array([0, 1, 3, 10, 30, 42, 60, 255], np.uint8), f.n)
        u = rng.random(f.n)
        nh = np.where(u < 0.1, 0, np.where(u < 0.7, 1, rng.integers(2, 12, f.n))).astype(np.uint16)
        pool.append(dict(kind=kind, file=f, flag16=flag16, mapq=mapq, nh=nh, full=_with_columns(pa, f, flag16, mapq, nh)))
    # ---- the segment sets: `single` ('.': the canonical stream never serves it), a batch with a '.' segment in front,
    # `stranded` ('+' / '-' only, several windows) and `stranded_dot` (the same and one '.' segment)
    f0 = pool[0]["file"]
    t = int(np.argmax([(f0.tid == i).sum() for i in range(ntid)]))
    ln = int(rng.integers(200, min(lens[t], 3000)))
    mid = int(np.median(f0.pos[f0.tid == t]))
    a = min(max(0, mid - int(rng.integers(0, ln))), lens[t] - ln)
    single = dict(name="single", tid=np.array([t], np.int32), start=np.array([a], np.int64), end=np.array([a + ln], np.int64),
                  strand=np.array([3], np.uint8), layout="forward", step=np.ones(1, np.int8))
    nb = int(rng.integers(5, 20))
    bt = rng.integers(0, ntid, nb).astype(np.int32)
    ba = np.array([int(rng.integers(0, lens[x] - 50)) for x in bt], np.int64)
    be = ba + rng.integers(1, 3000, nb)
    bt[0], ba[0], be[0] = 0, 10, 200
    bstrand = rng.choice(np.array([0, 1, 2, 3, 1 | NOFILTER, 2 | NOFILTER], np.uint8), nb)
    bstrand[0] = 3
    blay = str(rng.choice(["forward", "mixed"]))
    batch = dict(name="batch", tid=bt, start=ba, end=be, strand=bstrand, layout=blay,
                 step=np.ones(nb, np.int8) if blay == "forward" else rng.choice(np.array([1, -1], np.int8), nb))
    segs = []          # (tid, start, end)
    for c in range(ntid - 1):
        segs += [(c, 0, int(rng.integers(3, 40))), (c, lens[c] - int(rng.integers(1, 40)), lens[c])]
        edge = 128 * int(rng.integers(1, lens[c] // 128))
        segs += [(c, edge - int(rng.integers(1, 30)), edge + int(rng.integers(1, 30))), (c, edge, edge + int(rng.integers(1, 60))),
                 (c, max(0, edge - int(rng.integers(1, 60))), edge)]
    segs.append((ntid - 1, 0, min(lens[ntid - 1], int(rng.integers(50, 600)))))      # the contig without reads
    while len(segs) < 5 or (len(segs) < 40 and rng.random() < 0.8):
        c = int(rng.integers(0, ntid - 1))
        s0 = int(rng.integers(0, lens[c] - 1))
        segs.append((c, s0, min(lens[c], s0 + int(rng.integers(1, 2000)))))
    segs = [segs[i] for i in rng.permutation(len(segs))][:40]
    ns = len(segs)
    lay = str(rng.choice(["forward", "reversed", "mixed"]))
    stranded = dict(name="stranded", tid=np.array([s[0] for s in segs], np.int32), start=np.array([s[1] for s in segs], np.int64),
                    end=np.array([s[2] for s in segs], np.int64), strand=rng.choice(np.array([1, 2], np.uint8), ns), layout=lay,
                    step={"forward": np.ones(ns, np.int8), "reversed": -np.ones(ns, np.int8),
                          "mixed": rng.choice(np.array([1, -1], np.int8), ns)}[lay], several_windows=True)
    d = int(rng.integers(0, ntid - 1))
    d0 = int(rng.integers(0, lens[d] - 300))
    dot = dict(stranded, name="stranded_dot", tid=np.append(stranded["tid"], np.int32(d)), start=np.append(stranded["start"], d0),
               end=np.append(stranded["end"], d0 + int(rng.integers(100, 300))), strand=np.append(stranded["strand"], np.uint8(3)),
               step=np.append(stranded["step"], np.int8(1)))
    lo = int(rng.integers(22, 30))
    return dict(seed=seed, names=names, lens=lens, pool=pool, segsets=[single, batch, stranded, dot], strat=(lo, lo + int(rng.integers(1, 6))),
                big=False, stream=True, mapping0=("fiveprime", int(rng.choice([0, 3, 12]))))


SET_STRANDED, SET_DOT = 2, 3      # (indices into a stream world's segment sets)
STREAM_TRANSITIONS = ("rule", "excursion", "size_filter", "update_flags", "filter", "late_columns", "second_file", "other_file",
                      "no_canon", "compact_knobs", "dot_between", "alternate", "normalize")


def _point_mapping(rng):
    kind = str(rng.choice(["fiveprime", "threeprime", "variable"]))
    if kind != "variable":
        return (kind, int(rng.choice([0, 3, 12, 15])))
    od = {int(L): int(rng.integers(0, min(L, 20))) for L in rng.integers(15, 45, int(rng.integers(1, 8)))}
    od["default"] = int(rng.integers(0, 14))
    return (kind, tuple((k, od[k]) for k in tuple(sorted(k for k in od if k != "default")) + ("default",)))


def stream_sequence(seed, pa):
    """The world and the steps of stream sequence `seed`: after three plans are opened on one file (`stranded` twice,
    `stranded_dot`), transitions of STREAM_TRANSITIONS follow one another in an order drawn per seed, each with a check of
    the first `stranded` plan behind it -- the check before it is the one that closed the transition before."""
    rng = np.random.default_rng(seed)
    world = stream_world(rng, pa, seed)
    model = Model(world)
    nsteps = int(rng.integers(40, 51))
    steps, outcomes = [], []
    npool = len(world["pool"])
    A, B, D = 0, 1, 2

    def emit(step):
        out = model.refusal(step) if step[0] in CHECK_KINDS else model.apply(step)
        steps.append(step)
        outcomes.append(out)
        return out

    def check(pid=A):
        fits = model.plans[pid]["rows"] == model.rows()
        u = rng.random()
        if not fits or u < 0.6:
            return emit(("canonical_entries", pid))
        dtype = model.natural_dtype()
        if u < 0.75:
            return emit(("count_twice", pid, dtype))
        if u < 0.85 and dtype == "int64":
            return emit(("total", pid, "int64"))
        return emit(("count", pid, dtype if rng.random() < 0.7 else "float64"))

    def new_mask(shares=(0, 10, 30, 60)):
        """update_flags of file 0 with other exclusions than it has (lifting them only where there are some)."""
        share = int(rng.choice([s for s in shares if s or model.files[0]["mask"].any()]))
        emit(("update_flags", 0, int(rng.integers(0, 1 << 30)), share))

    def new_size_filter():
        lo = int(rng.integers(20, 33))
        sf = (lo, int(rng.choice([-1, lo + 6, lo + 12, 400])))
        emit(("set_size_filter", sf if sf != model.size_filter else None))

    def state_change():
        """One change of what is asked for that keeps the plan eligible: another caller's mask, or another size filter."""
        if rng.random() < 0.6:
            new_mask()
        else:
            new_size_filter()

    def one_file(avoid=None):
        k = int(rng.choice([i for i in range(npool) if i != avoid]))
        return ((k, True, True),)

    emit(("add_file", int(rng.integers(0, npool)), True, True))
    for pid, s in ((A, SET_STRANDED), (D, SET_DOT), (B, SET_STRANDED)):
        emit(("open_plan", pid, s))
        check(pid)
    emit(("stream_entries", 0))
    order = []
    while len(steps) < nsteps - 6:
        if not order:
            order = [STREAM_TRANSITIONS[i] for i in rng.permutation(len(STREAM_TRANSITIONS))]
        what = order.pop()
        if "PC_NO_CANON" in model.knobs and rng.random() < 0.7:
            what = "no_canon"          # (forbidden streams are the exception: mostly allowed again at once)
        if len(model.files) != 1:
            what = "second_file"
        if model.mapping[0] not in ("fiveprime", "threeprime", "variable"):
            what = "excursion"
        if what == "rule":
            m = _point_mapping(rng)
            while m == model.mapping:
                m = _point_mapping(rng)
            emit(("set_mapping", m))
        elif what == "excursion":
            if model.mapping[0] in ("fiveprime", "threeprime", "variable"):
                if rng.random() < 0.6:
                    emit(("set_mapping", ("center", int(rng.choice([0, 2, 12])))))
                    check(A)           # (answered, in float64: the center kernels, no canonical stream)
                else:
                    m = _point_mapping(rng)
                    while m[0] != "variable":
                        m = _point_mapping(rng)
                    emit(("set_mapping", ("stratified", m[1]) + world["strat"]))
                    emit(("stream_entries", 0))
            emit(("set_mapping", _point_mapping(rng)))
        elif what == "size_filter":
            if model.size_filter is not None and rng.random() < 0.5:
                emit(("set_size_filter", None))
            else:
                new_size_filter()
        elif what == "update_flags":
            new_mask()
        elif what == "filter":
            f = model.files[0]
            if not f["sam"]:
                emit(("set_alignment_sam", 0))
            elif not f["nh"]:
                emit(("set_alignment_nh", 0))
            if rng.random() < 0.5:
                new = None if model.flag_filter is not None and rng.random() < 0.5 else FLAG_FILTERS[int(rng.integers(0, len(FLAG_FILTERS)))]
                emit(("set_flag_filter", new if new != model.flag_filter else None))
            else:
                new = 0 if model.max_nh and rng.random() < 0.5 else int(rng.choice([1, 2, 5]))
                emit(("set_nh_filter", new if new != model.max_nh else 0))
            if model.missing_columns():    # (the other filter was waiting for the column that is still missing)
                emit(("set_alignment_nh" if not model.files[0]["nh"] else "set_alignment_sam", 0))
        elif what == "late_columns":
            which = "sam" if rng.random() < 0.5 else "nh"
            if which == "sam" and model.flag_filter is None:
                emit(("set_flag_filter", FLAG_FILTERS[int(rng.integers(0, len(FLAG_FILTERS)))]))
                check(A)
            if which == "nh" and not model.max_nh:
                emit(("set_nh_filter", int(rng.choice([1, 2, 5]))))
                check(A)
            emit(("set_alignments", ((model.files[0]["i"] if rng.random() < 0.2 else one_file(avoid=model.files[0]["i"])[0][0], which != "sam", which != "nh"),)))
            check(A)                   # refused: the filter waits for the column
            emit(("set_alignment_" + which, 0))
        elif what == "second_file":
            if len(model.files) == 1:
                f = model.files[0]
                emit(("add_file", int(rng.integers(0, npool)), f["sam"] or model.flag_filter is not None, f["nh"] or bool(model.max_nh)))
                check(A)               # two files: no canonical stream, and the one file 0 had is not served
                if rng.random() < 0.3:
                    check(B)
            if rng.random() < 0.5:
                emit(("set_alignments", one_file()))
            else:
                emit(("clear_alignments",))
                emit(("add_file",) + one_file()[0])
        elif what == "other_file":
            emit(("set_alignments", one_file(avoid=model.files[0]["i"])))
        elif what == "no_canon":
            k = {x: v for x, v in model.knobs.items() if x not in STREAM_KNOBS[:1]}
            if "PC_NO_CANON" not in model.knobs:
                k["PC_NO_CANON"] = "1"
            if rng.random() < 0.3:     # (the other knobs move along now and then)
                k = dict(random_knobs(rng, model.lazy()), **{x: v for x, v in k.items() if x in STREAM_KNOBS})
            emit(("reload_knobs", k))
            if rng.random() < 0.7:
                state_change()
        elif what == "compact_knobs":
            k = {x: v for x, v in model.knobs.items() if x not in STREAM_KNOBS[1:]}
            was = model.compact_knobs()
            while True:
                c = {}
                if rng.random() < 0.4:
                    c["PC_NO_COMPACT"] = "1"
                if rng.random() < 0.6:
                    c["PC_COMPACT_KEEP"] = str(rng.choice(["0.5", "1.0"]))
                if ("PC_NO_COMPACT" in c, float(c.get("PC_COMPACT_KEEP", sm.KEEP))) != was:
                    break
            emit(("reload_knobs", dict(k, **c)))
            if rng.random() < 0.85:    # a re-filter of the file: its compact stream is rebuilt under the new knobs
                new_mask((0, 10, 30))
            else:                      # ... or the file staged again
                emit(("set_alignments", ((model.files[0]["i"], True, True),)))
        elif what == "dot_between":
            check(D)
        elif what == "alternate":
            check(B)
        elif what == "normalize":
            emit(("set_normalize", None if model.norm is not None else float(rng.integers(1, 10 ** 9))))
        check(A)
        if rng.random() < 0.25:
            emit(("stream_entries", int(rng.integers(0, len(model.files)))))
        elif rng.random() < 0.1:
            emit(("mapped_reads", 0) if rng.random() < 0.5 else ("count", D, model.natural_dtype()))
    while steps[-1][0] not in CHECK_KINDS or len(steps) < 40:
        check(A if rng.random() < 0.6 else (B if rng.random() < 0.5 else D))
    return dict(seed=seed, world=world, steps=steps, outcomes=outcomes)


# ---------------------------------------------------------------------------------------------------- the runner
def format_trace(seed, steps, upto):
    lines = ["seed %d, step %d; the op trace so far (seq['steps'] = [...] replays it):" % (seed, upto), "["]
    lines += ["    %r," % (s,) for s in steps[:upto + 1]]
    return "\n".join(lines + ["]"])


def first_difference(got, exp):
    got, exp = np.asarray(got), np.asarray(exp)
    if got.shape != exp.shape or got.dtype != exp.dtype:
        return "got %s%s, expected %s%s" % (got.dtype, got.shape, exp.dtype, exp.shape)
    bad = np.nonzero(got != exp)[0]
    if not len(bad):
        return "equal"
    return "%d of %d positions differ, the first at %d: got %r, expected %r" % (len(bad), exp.size, bad[0], got[bad[0]], exp[bad[0]])


def staged_file(pa, world, i, sam, nh, flags=None):
    p = world["pool"][i]
    return _with_columns(pa, p["file"], p["flag16"] if sam else None, p["mapq"] if sam else None, p["nh"] if nh else None, flags)


def run_sequence(pa, oracle, seq, on_check=None):
    """Apply `seq` to a real engine and to the model; AssertionError on the first disagreement.  Nothing is tried twice."""
    from plastid_amd import synth
    from plastid_amd.engine import Engine
    from plastid_amd.exceptions import EngineError
    raises = {"columns": EngineError, "flag_filter_on": EngineError, "nh_filter_on": EngineError, "rows": ValueError, "sums": ValueError}
    world, steps = seq["world"], seq["steps"]
    model = Model(world)
    saved = {k: os.environ.pop(k, None) for k in KNOBS}
    eng = Engine(0)
    plans = {}
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            synth.mapping_factory(mapping_of(model.mapping))._configure(eng)
        for at, step in enumerate(steps):
            kind = step[0]
            where = lambda what: "%s\n%s" % (what, format_trace(seq["seed"], steps, at))    # noqa: E731

            def same(got, exp, what):
                assert got.dtype == exp.dtype and np.array_equal(got, exp), where("%s: %s" % (what, first_difference(got, exp)))

            if kind in CHECK_KINDS:
                why = model.refusal(step)
                dtype = (None if kind in ("mapped_reads", "stream_entries") else
                         np.dtype(model.natural_dtype() if kind == "canonical_entries" else step[-1]))
                sg = world["segsets"][0]
                seg = (int(sg["tid"][0]), int(sg["start"][0]), int(sg["end"][0]), int(sg["strand"][0]))

                if kind == "mapped_reads":
                    lo, hi = np.searchsorted(world["pool"][model.files[step[1]]["i"]]["file"].tid, [seg[0], seg[0] + 1])

                def ask():
                    if kind == "mapped_reads":     # over the file's records on the segment's contig (the caller's fetch range)
                        return eng.mapped_reads(step[1], lo, hi, *seg)
                    if kind == "query_segment":
                        return eng.query_segment(seg[0], seg[1], seg[2], seg[3], step[1], dtype.type)
                    if kind == "stream_entries":
                        return eng.stream_entries(step[1])
                    return plans[step[1]].count(dtype)
                if why is not None:
                    try:
                        ask()
                    except raises[why]:
                        pass
                    else:
                        raise AssertionError(where("the engine answered where it must refuse (%s)" % why))
                    if on_check:
                        on_check(at, step, None)
                    continue
                got = ask()
                if kind == "mapped_reads":
                    exp = model.expected_mapped_reads(oracle, step[1])
                    assert not exp[:lo].any() and not exp[hi:].any()
                    same(got, exp[lo:hi], "mapped_reads")
                elif kind == "query_segment":
                    exp = model.expected_query(oracle, step[1]).astype(dtype)
                    same(got, exp, "query_segment")
                elif kind == "stream_entries":
                    exp = model.expected_stream_entries(step[1])
                    assert got == exp, where("stream_entries(%d): got %d, the compact model says %d (of %d records)"
                                             % (step[1], got, exp, eng.num_records(step[1])))
                else:
                    exp, warn = model.expected_plan(oracle, step[1])
                    exp = exp.astype(dtype)
                    plan = plans[step[1]]
                    if world["segsets"][model.plans[step[1]]["set"]]["name"] == "big":
                        assert plan.tiles >= 4096, where("the large plan has %d tiles" % plan.tiles)
                    same(got, exp, "count")
                    if kind == "count_twice":
                        eng.sync()
                        same(plan.count(dtype), exp, "second count (exact grids)")
                    elif kind == "total":
                        got_total = plan.total()
                        assert got_total.dtype == exp.dtype and got_total == exp.sum(), where("total: got %r, expected %r" % (got_total, exp.sum()))
                    elif kind == "warn_flags":
                        same(plan.warn_flags(), warn, "warn_flags")
                    # the canonical stream of file 0 behind this count (the model follows every answered count; the entry
                    # number is read where the step asks for it, and after every plan check of a stream world)
                    pred, entries = model.canonical_check(step[1])
                    if kind == "canonical_entries" or world.get("stream"):
                        assert not (world.get("stream") and entries is None), where("the model has no verdict in a stream world: %r" % (pred,))
                        if entries is not None:
                            got_entries = eng.canonical_entries(0)
                            assert got_entries == entries, where("canonical_entries(0): got %d, the model says %d (%r)" % (got_entries, entries, pred))
                if on_check:
                    on_check(at, step, exp)
                continue
            # ---- a mutating step: the engine first (it may refuse), the model decides whether it had to
            before = model.snapshot()
            why = model.apply(step)

            def do():
                if kind == "add_file":
                    eng.add_alignment_file(staged_file(pa, world, *step[1:]))
                elif kind == "clear_alignments":
                    eng.clear_alignments()
                elif kind == "set_alignments":
                    eng.set_alignments([staged_file(pa, world, *a) for a in step[1]])
                elif kind == "set_alignment_sam":
                    p = world["pool"][model.files[step[1]]["i"]]
                    eng.set_alignment_sam(step[1], p["flag16"], p["mapq"])
                elif kind == "set_alignment_nh":
                    eng.set_alignment_nh(step[1], world["pool"][model.files[step[1]]["i"]]["nh"])
                elif kind == "update_flags":
                    f = world["pool"][model.files[step[1]]["i"]]["file"]
                    eng.update_flags(step[1], (f.flags & 1) | np.where(caller_mask(f.n, step[2], step[3]), 0x80, 0).astype(np.uint8))
                elif kind == "set_flag_filter":
                    if step[1] is None:
                        eng.set_flag_filter(enabled=False)
                    else:
                        eng.set_flag_filter(*step[1])
                elif kind == "set_nh_filter":
                    eng.set_nh_filter(step[1])
                elif kind == "set_mapping":
                    with warnings.catch_warnings():
                        warnings.simplefilter("ignore")
                        synth.mapping_factory(mapping_of(step[1]))._configure(eng)
                elif kind == "set_size_filter":
                    if step[1] is None:
                        eng.set_size_filter(None)
                    else:
                        eng.set_size_filter(*step[1])
                elif kind == "set_normalize":
                    eng.set_normalize(step[1] is not None, 1.0 if step[1] is None else step[1])
                elif kind == "reload_knobs":
                    for k in KNOBS:
                        os.environ.pop(k, None)
                    os.environ.update(step[1])
                    eng.reload_knobs()
                elif kind == "open_plan":
                    sgs = world["segsets"][step[2]]
                    lay = _layout(sgs, model.rows())
                    plans[step[1]] = eng.plan(sgs["tid"], sgs["start"], sgs["end"], sgs["strand"], lay["out_off"], lay["step"],
                                              lay["stride"], lay["out_elems"], model.rows())
                elif kind == "close_plan":
                    plans.pop(step[1]).close()
            if why is not None:
                try:
                    do()
                except raises[why]:
                    pass
                else:
                    raise AssertionError(where("the engine accepted what it must refuse (%s)" % why))
                assert model.snapshot() == before, where("the model changed at a refused step")
            else:
                do()
    finally:
        for p in plans.values():
            p.close()
        eng.close()
        for k in KNOBS:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]


def model_walk(oracle, seq, streams=False):
    """The model alone over a sequence (no engine): yields ``(index, step, refusal kind or None, expected or None)`` for
    every step; `expected` is the vector of a check step that must be answered (the entry count, as a vector of one, for
    a stream_entries step).  `streams`: a fifth value -- None, or for an answered plan check ``(prediction, entries)`` of
    ``Model.canonical_check`` -- and the model itself as a sixth, in the state BEHIND the step (to look at, not to change)."""
    model = Model(seq["world"])
    for at, step in enumerate(seq["steps"]):
        if step[0] not in CHECK_KINDS:
            why = model.apply(step)
            yield (at, step, why, None, None, model) if streams else (at, step, why, None)
            continue
        why = model.refusal(step)
        exp = canon = None
        if why is None:
            if step[0] == "mapped_reads":
                exp = model.expected_mapped_reads(oracle, step[1])
            elif step[0] == "query_segment":
                exp = model.expected_query(oracle, step[1])
            elif step[0] == "stream_entries":
                exp = np.array([model.expected_stream_entries(step[1])], np.int64)
            else:
                exp = model.expected_plan(oracle, step[1])[0]
                canon = model.canonical_check(step[1])
        yield (at, step, why, exp, canon, model) if streams else (at, step, why, exp)


# ---------------------------------------------------------------------------------------------------- the shrinker
def shrink(seq, still_fails):
    """Drop steps while ``still_fails(candidate_seq)`` holds -- first from the front, then one at a time.  For the CPU
    side of debugging a recorded mismatch, with a predicate the developer supplies (for instance: the model, fed the
    candidate, still reaches the state of the mismatch).  Candidates that the model cannot follow (a step naming a file
    or a plan that is no longer there) are skipped.  No test calls this, and the predicate must not run on a GPU in a loop."""
    def valid(steps):
        m = Model(seq["world"])
        try:
            for s in steps:
                if s[0] in CHECK_KINDS:
                    if s[0] in PLAN_CHECK_KINDS:
                        m.plans[s[1]]
                    elif s[0] in ("mapped_reads", "stream_entries"):
                        m.files[s[1]]
                    elif not m.files:
                        return False
                else:
                    m.apply(s)
        except (KeyError, IndexError):
            return False
        return True

    def attempt(steps):
        return valid(steps) and still_fails(dict(seq, steps=steps))
    steps = list(seq["steps"])
    while len(steps) > 1 and attempt(steps[1:]):
        steps = steps[1:]
    changed = True
    while changed:            # from the back, so that a check goes before the plan or the file it names
        changed = False
        for k in range(len(steps) - 1, -1, -1):
            cand = steps[:k] + steps[k + 1:]
            if cand and attempt(cand):
                steps, changed = cand, True
    return dict(seq, steps=steps)
