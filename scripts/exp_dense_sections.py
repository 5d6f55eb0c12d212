"""Experiment: time of the steady C2 count -- one launch of k_dense_gather -- with the library named by PLASTID_AMD_LIB:
a build variant with -DPC_DENSE_SKIP=<mask> (sections of the kernel left out: results are then wrong, only the time
counts), -DPC_DENSE_BATCH=<B> or -DPC_DENSE_NT=1 (dense_kernels.hip.h).  2 000 launches per repeat, REPEATS repeats, one
process.  PLAN=uniform replaces the annotation by segments of exactly 2 048 positions laid end to end over both strands
of every contig, as many positions as the annotation has: the only plan a PC_DENSE_SKIP=4 build (descriptors made from
the block index) can be compared on.  Three more plans over the same cells say what a plan's shape costs
(profiles/dense_chunks/NOTES.md): PLAN=shifted, the uniform plan behind a leading one-element segment (every item 8
bytes off its line); PLAN=short, line-aligned segments of 1 280 positions (lane fill 0.625 of an item);
PLAN=reverse, the uniform plan with step -1.
usage: PLASTID_AMD_LIB=build_variants/dskip1.so python scripts/exp_dense_sections.py"""
import os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from plastid_amd import synth
from plastid_amd.engine import Engine
ITEM = 2048
genome, tx, reads, mapping = synth.make_config("C2", scale=float(os.environ.get("SCALE", "1.0")))
annotation = tx.plan_arrays(rows=1)


def make_plan(kind):
    p = annotation
    if kind == "annotation":
        return p
    assert kind in ("uniform", "shifted", "short", "reverse"), kind
    # segments of `seg` positions laid end to end in the output (1 280 elements are 80 lines: still line aligned, no gap),
    # each reading the first `seg` cells of a slot of ITEM cells
    seg = 1280 if kind == "short" else ITEM
    want = int(p["out_elems"]) // seg
    tid, start, strand = [], [], []
    for t, ln in enumerate(genome[1]):
        for st in (1, 2):
            s0 = np.arange(0, int(ln) - ITEM + 1, ITEM, dtype=np.int64)
            tid.append(np.full(len(s0), t, np.int32)); start.append(s0); strand.append(np.full(len(s0), st, np.uint8))
    tid, start, strand = (np.concatenate(x) for x in (tid, start, strand))
    rep = -(-want // len(tid))
    tid, start, strand = (np.tile(x, rep)[:want] for x in (tid, start, strand))
    n = len(tid)
    out_off = np.arange(n, dtype=np.int64) * seg
    step = np.ones(n, np.int8)
    if kind == "reverse":          # position i of a segment goes to out_off - i
        out_off = out_off + seg - 1
        step = -step
    p = dict(tid=tid, start=start, end=start + seg, strand=strand, out_off=out_off, out_step=step,
             row_stride=np.full(n, seg, np.int64), out_elems=n * seg)
    if kind == "shifted":          # a leading one-element segment: every item starts 8 bytes behind a line
        p = dict(tid=np.concatenate([tid[:1], tid]), start=np.concatenate([start[:1], start]), end=np.concatenate([start[:1] + 1, start + seg]),
                 strand=np.concatenate([strand[:1], strand]), out_off=np.concatenate([[0], out_off + 1]).astype(np.int64),
                 out_step=np.ones(n + 1, np.int8), row_stride=np.concatenate([[1], np.full(n, seg, np.int64)]), out_elems=n * seg + 1)
    return p


eng = Engine(0)
eng.set_alignments([reads])
synth.mapping_factory(mapping)._configure(eng)
n = int(os.environ.get("STEPS", "2000"))
for kind in os.environ.get("PLAN", "annotation").split(","):   # (a list: one staging of the reads serves every plan)
    p = make_plan(kind)
    plan = eng.plan(p["tid"], p["start"], p["end"], p["strand"], p["out_off"], p["out_step"], p["row_stride"], p["out_elems"], 1)
    for _ in range(50):
        plan.launch(np.int64)
    eng.sync()
    assert eng.dense_cells(0) > 0, "the plan is not served from the dense vector"
    res, host = [], []
    for _ in range(int(os.environ.get("REPEATS", "3"))):
        t0 = time.perf_counter()
        for _ in range(n):
            plan.launch(np.int64)
        host.append((time.perf_counter() - t0) / n * 1e3)     # the host's share: n launches queued, none waited for
        eng.sync()
        res.append((time.perf_counter() - t0) / n * 1e3)
    t0 = time.perf_counter()
    for _ in range(n):
        plan.launch(np.int64)
        eng.sync()
    each = (time.perf_counter() - t0) / n * 1e3
    path = eng.dense_path() if hasattr(eng, "dense_path") else "items"
    print("C2 %-10s %-24s %s ms per count (%d positions; by %s; host alone %s, with a sync per count %.4f)"
          % (kind, os.path.basename(os.environ.get("PLASTID_AMD_LIB", "product")) + (" PC_DENSE_ITEMS" if os.environ.get("PC_DENSE_ITEMS") else ""),
             " ".join("%.4f" % x for x in res), int(p["out_elems"]), path, " ".join("%.4f" % x for x in host), each), flush=True)
    plan.close()
