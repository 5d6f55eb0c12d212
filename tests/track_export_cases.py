"""tests/golden/track_export_fixture.npz (the reference's mutable GenomeArray: writes, arithmetic, nonzero, both exports)
for the host and the GPU tests: the cases, their arrays as a host ``DenseGenomeArray``, and the recorded construction steps
replayed on any array class with the reference's interface."""
import json
import operator
import os

import numpy as np

_Z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "track_export_fixture.npz"))
MANIFEST = json.loads(str(_Z["manifest"]))
MIN_CHR = MANIFEST["min_chr_size"]
ODD = _Z["odd"]
KWARGS = {"color": "0,0,255", "altColor": "255,0,0"}
TRACKNAME = "golden"
FUNCS = {"add": operator.add, "sub": operator.sub, "mul": operator.mul}
_CASES = {c["name"]: c for c in MANIFEST["cases"]}


def case_names(raised=False):
    return [c["name"] for c in MANIFEST["cases"] if (c["reference_raises"] is not None) == raised]


def case(name):
    return _CASES[name]


def cells(name, chrom, strand):
    return _Z["%s|%s|%s" % (name, chrom, strand)]


def nonzero(name, chrom, strand):
    return np.cumsum(_Z["%s|%s|%s|nz_diff" % (name, chrom, strand)])


def host_array(name):
    """The case's resulting array as a DenseGenomeArray (the reference's cells)."""
    from plastid_amd.genome_array import DenseGenomeArray
    c = case(name)
    ga = DenseGenomeArray({ch: c["lengths"][ch] for ch in c["chroms"]}, tuple(c["strands"]))
    for ch in c["chroms"]:
        for st in c["strands"]:
            ga._chroms[ch][st][:] = cells(name, ch, st)
    return ga


def replay(steps, make_array):
    """Run the recorded steps; `make_array(chr_lengths)` makes an empty array.  Returns ``{target: array}``."""
    from plastid_amd.roitools import GenomicSegment, SegmentChain
    import io
    arrays = {}
    for st in steps:
        if st["op"] == "new":
            arrays[st["target"]] = make_array(st["chr_lengths"])
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
            if st["how"] == "operator":
                arrays[st["target"]] = {"add": lambda: left + right, "sub": lambda: left - right, "mul": lambda: left * right}[st["func"]]()
            else:
                arrays[st["target"]] = left.apply_operation(right, FUNCS[st["func"]], mode=st["mode"])
    return arrays


def combine_model(a, b, func, mode):
    """numpy model of ``apply_operation`` between two host arrays as its docstring describes it (ISSUE section 2): ``all`` is
    the union at the longer length with zero for what one side lacks, `a`'s contigs and strands first; ``truncate`` the
    common ones at the shorter length; ``same`` is ``all`` with the reference's growth of its result, 10000 per strand (it
    writes whole contigs through ``__setitem__``, and a write that ends at the length grows the contig).  Returns ``(chroms, strands, {chrom: {strand: cells}})``."""
    ca, cb = list(a.chroms()), list(b.chroms())
    sa, sb = list(a.strands()), list(b.strands())
    if mode == "truncate":
        chroms, strands = [c for c in ca if c in cb], [s for s in sa if s in sb]
    else:
        chroms, strands = ca + [c for c in cb if c not in ca], sa + [s for s in sb if s not in sa]
    out = {}
    for c in chroms:
        la = a.lengths()[c] if c in ca else None
        lb = b.lengths()[c] if c in cb else None
        n = min(la, lb) if mode == "truncate" else max(x for x in (la, lb) if x is not None)
        if mode == "same":
            n += 10000 * len(strands)
        out[c] = {}
        for s in strands:
            x, y = np.zeros(n), np.zeros(n)
            if c in ca and s in sa:
                v = a._chroms[c][s][:n]
                x[:len(v)] = v
            if c in cb and s in sb:
                v = b._chroms[c][s][:n]
                y[:len(v)] = v
            out[c][s] = func(x, y)
    return chroms, strands, out
