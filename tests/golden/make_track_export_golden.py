#!/usr/bin/env python
"""Golden data for the mutable GenomeArray (writes, arithmetic, nonzero, export), from the REFERENCE ITSELF.

Run only in the build container (needs the scratch reference of build_scratch_reference.sh):

    bash tests/golden/build_scratch_reference.sh /tmp/oracle
    PYTHONPATH=/tmp/oracle:/tmp/oracle/stubs:. python tests/golden/make_track_export_golden.py

Drives the reference's ``GenomeArray`` (plastid/genomics/genome_array.py:1323-2104): ``__setitem__`` over segments and
chains, ``add_from_wiggle``, ``apply_operation`` / ``+`` / ``-`` / ``*``, ``nonzero``, ``to_bedgraph`` and
``to_variable_step``.  Writes DATA ONLY to ``tests/golden/track_export_fixture.npz``: per case the construction steps, the
resulting arrays, ``chroms()``, ``lengths()``, ``nonzero()`` (as differences) and both texts for '+' and '-'; where the reference raises
(``all`` over differing contig sets) the manifest records that it raised.
"""
import io
import json
import operator
import os
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

from plastid.genomics.genome_array import GenomeArray
from plastid.genomics.roitools import GenomicSegment, SegmentChain

MIN_CHR = 2000
FUNCS = {"add": operator.add, "sub": operator.sub, "mul": operator.mul}
NAN, INF = float("nan"), float("inf")

#: the values whose text is not digits and ".0" (ISSUE: the formatter's cases), and the plain ones around them
ODD = [0.1, 1.0 / 3.0, 1e15, 1e16, float(2 ** 53 - 1), float(2 ** 53), 1e-4, 1e-5, 5e-324, -7.0, 999999999999999.9, 3.0, 2.5, 1e22, 123456.789]


def seg_set(target, chrom, strand, start, end, value):
    return {"op": "set", "target": target, "chrom": chrom, "strand": strand, "segments": [[start, end]], "chain": False, "value": value}


def chain_set(target, chrom, strand, segments, value):
    return {"op": "set", "target": target, "chrom": chrom, "strand": strand, "segments": [list(s) for s in segments], "chain": True, "value": value}


def new(target, chr_lengths):
    return {"op": "new", "target": target, "chr_lengths": chr_lengths}


def arith(target, left, right, func, mode=None, how="apply"):
    return {"op": "arith", "target": target, "left": left, "right": right, "func": func, "mode": mode, "how": how}


def base_a():
    """Array `a`: chr2 / chr10 / chrA declared, writes on both strands, growth past the length, an undeclared contig."""
    return [
        new("a", {"chr2": 300, "chr10": 500, "chrA": 40}),
        seg_set("a", "chr2", "+", 0, 4, 3.0),                                   # first non-zero at position 0
        seg_set("a", "chr2", "+", 10, 16, [1.0, 2.0, 2.0, 0.0, 2.0, 5.0]),
        seg_set("a", "chr2", "-", 20, 26, [1.0, 2.0, 3.0, 4.0, 5.0, 6.0]),      # '-' segment, vector: reversed
        chain_set("a", "chr10", "-", [(5, 8), (20, 24), (100, 103)], [float(x) for x in range(1, 11)]),   # '-' chain: reversed as a whole
        chain_set("a", "chr10", "+", [(30, 33), (40, 42)], [7.0, 7.0, 8.0, 9.0, 9.0]),
        chain_set("a", "chr10", "+", [(200, 210), (220, 230)], 4.0),
        seg_set("a", "chr2", "+", 440, 450, 6.0),                               # growth: 450 >= 300 -> 10450
        seg_set("a", "chrU", "+", 10, 20, 2.0),                                 # undeclared: born at min_chr_size
        seg_set("a", "chrU", "-", 1990, 1999, [float(x) for x in range(9)]),
    ]


def cases():
    c = []
    c.append({"name": "writes", "steps": base_a(), "result": "a"})
    c.append({"name": "overwrite_and_wiggle", "result": "a", "steps": base_a() + [
        seg_set("a", "chr2", "+", 2, 12, 0.0),
        {"op": "wiggle", "target": "a", "strand": "+", "text": "chr2 1 5 2\nchr10 31 41 1.5\nvariableStep chrom=chrW span=2\n7 0.25\n"},
        seg_set("a", "chr10", "-", 21, 23, [0.5, 1e-5])]})
    c.append({"name": "values", "result": "v", "steps": [
        new("v", {"chr2": 100, "chr10": 100, "chrA": 100, "chrNeg": 50, "chrZero": 50, "chrNaN": 50, "chrInf": 50, "chrBig": 50}),
        seg_set("v", "chr2", "+", 0, len(ODD), ODD),                            # first non-zero at 0
        seg_set("v", "chr2", "-", 50, 50 + len(ODD), ODD),
        # -0.0 inside a zero run, at the head of a zero run, and heading a run of its own behind a value
        seg_set("v", "chr10", "+", 5, 17, [3.0, 0.0, -0.0, 0.0, 3.0, -0.0, 0.0, 5.0, 5.0, -0.0, -0.0, 1.0]),
        seg_set("v", "chrA", "+", 99, 100, 1.0),                                # nothing on '-', last cell of the contig
        seg_set("v", "chrNeg", "+", 3, 6, [1.0, -7.0, 2.0]),                    # sum < 0: no bedGraph
        seg_set("v", "chrNeg", "-", 3, 6, [1.0, -7.0, 20.0]),
        seg_set("v", "chrZero", "+", 3, 6, [5.0, -5.0, 0.0]),                   # sum == 0: no bedGraph
        seg_set("v", "chrZero", "-", 0, 2, [-0.0, -0.0]),                       # no non-zero cell at all
        seg_set("v", "chrNaN", "+", 3, 8, [1.0, NAN, NAN, 2.0, NAN]),           # NaN next to NaN (sum NaN: no bedGraph)
        seg_set("v", "chrInf", "+", 3, 7, [INF, INF, 2.0, 2.0]),
        seg_set("v", "chrInf", "-", 3, 6, [-INF, 2.0, 2.0]),                    # sum -inf
        seg_set("v", "chrBig", "+", 1, 4, [1.7976931348623157e308, 5e-324, 5e-324]),
    ]})
    b_steps = [new("b", {"chr2": 10450, "chr10": 500, "chrA": 40, "chrU": 2000}),
               seg_set("b", "chr2", "+", 1, 14, 0.5), seg_set("b", "chr2", "-", 22, 30, [float(x) for x in range(8)]),
               seg_set("b", "chr10", "-", 0, 25, 2.0), seg_set("b", "chr10", "+", 205, 480, 1.0), seg_set("b", "chrU", "+", 15, 18, -2.0)]
    d_steps = [new("d", {"chr2": 400, "chr10": 9000, "chrA": 40, "chrU": 100}),
               seg_set("d", "chr2", "+", 1, 14, 0.5), seg_set("d", "chr2", "-", 350, 399, 3.0),
               seg_set("d", "chr10", "-", 0, 25, 2.0), seg_set("d", "chr10", "+", 205, 560, 1.0), seg_set("d", "chrU", "+", 15, 18, -2.0)]
    # (a scalar acts on every cell up to the length: a short array keeps the texts short)
    s_steps = [new("s", {"chr2": 130, "chr10": 70}), seg_set("s", "chr2", "+", 0, 4, 3.0), seg_set("s", "chr2", "-", 20, 26, [1.0, 2.0, 3.0, 4.0, 5.0, -1.0]),
               chain_set("s", "chr10", "-", [(5, 8), (20, 24)], [0.5, 1.0, 1.0, 2.0, 2.0, 2.0, 0.25])]
    c.append({"name": "scalar_add", "result": "r", "steps": s_steps + [arith("r", "s", 1, "add", how="operator")]})
    c.append({"name": "scalar_mul", "result": "r", "steps": s_steps + [arith("r", "s", 2.5, "mul", how="operator")]})
    c.append({"name": "scalar_sub_apply", "result": "r", "steps": s_steps + [arith("r", "s", 0.75, "sub", "same")]})
    for f in ("add", "sub", "mul"):
        c.append({"name": "same_%s" % f, "result": "r", "steps": base_a() + b_steps + [arith("r", "a", "b", f, "same")]})
        c.append({"name": "all_%s" % f, "result": "r", "steps": base_a() + d_steps + [arith("r", "a", "d", f, "all")]})
        c.append({"name": "truncate_%s" % f, "result": "r", "steps": base_a() + d_steps + [arith("r", "a", "d", f, "truncate")]})
        c.append({"name": "operator_%s" % f, "result": "r", "steps": base_a() + d_steps + [arith("r", "a", "d", f, how="operator")]})
    e_steps = [new("e", {"chr2": 400, "chrE": 60}), seg_set("e", "chr2", "+", 1, 14, 0.5), seg_set("e", "chrE", "-", 3, 9, 2.0)]
    c.append({"name": "all_differing_contigs", "result": "r", "steps": base_a() + e_steps + [arith("r", "a", "e", "add", "all")]})
    return c


def run_steps(steps):
    arrays, raised = {}, None
    for st in steps:
        if st["op"] == "new":
            arrays[st["target"]] = GenomeArray(chr_lengths=st["chr_lengths"], min_chr_size=MIN_CHR)
        elif st["op"] == "set":
            segs = [GenomicSegment(st["chrom"], a, b, st["strand"]) for a, b in st["segments"]]
            roi = SegmentChain(*segs) if st["chain"] else segs[0]
            val = st["value"]
            arrays[st["target"]][roi] = np.array(val, float) if isinstance(val, list) else val
        elif st["op"] == "wiggle":
            arrays[st["target"]].add_from_wiggle(io.StringIO(st["text"]), st["strand"])
        elif st["op"] == "arith":
            left = arrays[st["left"]]
            right = arrays[st["right"]] if isinstance(st["right"], str) else st["right"]
            try:
                if st["how"] == "operator":
                    r = {"add": lambda: left + right, "sub": lambda: left - right, "mul": lambda: left * right}[st["func"]]()
                else:
                    r = left.apply_operation(right, FUNCS[st["func"]], mode=st["mode"])
                arrays[st["target"]] = r
            except Exception as e:  # noqa: BLE001 -- whatever the reference raises is recorded
                raised = type(e).__name__
                break
    return arrays, raised


def text_of(ga, what, strand):
    fh = io.StringIO()
    getattr(ga, what)(fh, "golden", strand, color="0,0,255", altColor="255,0,0")
    return fh.getvalue()


def main():
    warnings.simplefilter("ignore")
    manifest = {"min_chr_size": MIN_CHR, "cases": []}
    out = {}
    for case in cases():
        arrays, raised = run_steps(case["steps"])
        m = {"name": case["name"], "steps": case["steps"], "result": case["result"], "reference_raises": raised}
        if raised is None:
            ga = arrays[case["result"]]
            m["chroms"] = list(ga.chroms())
            m["strands"] = list(ga.strands())
            m["lengths"] = {k: int(v) for k, v in ga.lengths().items()}
            nz = ga.nonzero()
            for ch in m["chroms"]:
                for st in m["strands"]:
                    out["%s|%s|%s" % (case["name"], ch, st)] = np.array(ga._chroms[ch][st], np.float64)
                    # (the indices as differences: a scalar sum makes every position non-zero)
                    out["%s|%s|%s|nz_diff" % (case["name"], ch, st)] = np.diff(np.array(nz[ch][st], np.int64), prepend=0)
            m["bedgraph"] = {st: text_of(ga, "to_bedgraph", st) for st in "+-"}
            m["variable_step"] = {st: text_of(ga, "to_variable_step", st) for st in "+-"}
        manifest["cases"].append(m)
        print("%-28s %s" % (case["name"], "raises %s" % raised if raised else "%d contigs, bedGraph %d + %d bytes" % (
            len(m["chroms"]), len(m["bedgraph"]["+"]), len(m["bedgraph"]["-"]))))
    path = os.path.join(HERE, "track_export_fixture.npz")
    np.savez_compressed(path, manifest=np.array(json.dumps(manifest)), odd=np.array(ODD, np.float64), **out)
    print("wrote %s: %d cases; %.0f kB" % (path, len(manifest["cases"]), os.path.getsize(path) / 1e3))


if __name__ == "__main__":
    main()
