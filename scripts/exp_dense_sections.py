"""Experiment: time of the steady C2 count -- one launch of k_dense_gather -- with the library named by PLASTID_AMD_LIB:
a build variant with -DPC_DENSE_SKIP=<mask> (sections of the kernel left out: results are then wrong, only the time
counts), -DPC_DENSE_BATCH=<B> or -DPC_DENSE_NT=1 (dense_kernels.hip.h).  2 000 launches per repeat, REPEATS repeats, one
process.  PLAN=uniform replaces the annotation by segments of exactly 2 048 positions laid end to end over both strands
of every contig, as many positions as the annotation has: the only plan a PC_DENSE_SKIP=4 build (descriptors made from
the block index) can be compared on.
usage: PLASTID_AMD_LIB=build_variants/dskip1.so python scripts/exp_dense_sections.py"""
import os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from plastid_amd import synth
from plastid_amd.engine import Engine
ITEM = 2048
genome, tx, reads, mapping = synth.make_config("C2", scale=float(os.environ.get("SCALE", "1.0")))
p = tx.plan_arrays(rows=1)
kind = os.environ.get("PLAN", "annotation")
if kind == "uniform":
    want = int(p["out_elems"]) // ITEM
    tid, start, strand = [], [], []
    for t, ln in enumerate(genome[1]):
        for st in (1, 2):
            s0 = np.arange(0, int(ln) - ITEM + 1, ITEM, dtype=np.int64)
            tid.append(np.full(len(s0), t, np.int32)); start.append(s0); strand.append(np.full(len(s0), st, np.uint8))
    tid, start, strand = (np.concatenate(x) for x in (tid, start, strand))
    rep = -(-want // len(tid))
    tid, start, strand = (np.tile(x, rep)[:want] for x in (tid, start, strand))
    n = len(tid)
    p = dict(tid=tid, start=start, end=start + ITEM, strand=strand, out_off=np.arange(n, dtype=np.int64) * ITEM, out_step=np.ones(n, np.int8),
             row_stride=np.full(n, ITEM, np.int64), out_elems=n * ITEM)
eng = Engine(0)
eng.set_alignments([reads])
synth.mapping_factory(mapping)._configure(eng)
plan = eng.plan(p["tid"], p["start"], p["end"], p["strand"], p["out_off"], p["out_step"], p["row_stride"], p["out_elems"], 1)
for _ in range(50):
    plan.launch(np.int64)
eng.sync()
assert eng.dense_cells(0) > 0, "the plan is not served from the dense vector"
n = int(os.environ.get("STEPS", "2000"))
res = []
for _ in range(int(os.environ.get("REPEATS", "3"))):
    t0 = time.perf_counter()
    for _ in range(n):
        plan.launch(np.int64)
    eng.sync()
    res.append((time.perf_counter() - t0) / n * 1e3)
print("C2 %-10s %-24s %s ms per count (%d positions)" % (kind, os.path.basename(os.environ.get("PLASTID_AMD_LIB", "product")),
                                                         " ".join("%.4f" % x for x in res), int(p["out_elems"])), flush=True)
