"""What the tests of the count export share (tests/test_count_export_host.py, tests/test_gpu_count_export.py): the 36
texts the reference wrote (tests/golden/export_regions.npz) with the oracle's vectors for them, the reference's window loop
restated, and designed reads -- `c` single-end '+' reads that start at `p` give count `c` at `p` under
``FivePrimeMapFactory(0)``, so run counts and digit widths are exact."""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
_golden = None


def golden():
    """``(manifest, packed arrays)`` of tests/golden/export_regions.npz."""
    global _golden
    if _golden is None:
        z = np.load(os.path.join(HERE, "golden", "export_regions.npz"))
        _golden = json.loads(str(z["manifest"])), {k[4:]: z[k] for k in z.files if k.startswith("aln_")}
    return _golden


def golden_packed(pa):
    man, aln = golden()
    return pa.PackedAlignments(aln["tid"], aln["pos"], aln["alen"], aln["flags"], aln["nblk"], aln["blk_start"], aln["blk_len"],
                               references=man["references"], lengths=man["lengths"], mapped=man["mapped"])


def export_id(ex):
    return "%s-%s%s-%s-%d" % (ex["what"], ex["spec"]["kind"], "-norm" if ex["normalize"] else "", {"+": "fw", "-": "rc", ".": "both"}[ex["strand"]], ex["window"])


def factory(pa, spec):
    from tests import golden_util as gu
    k = spec["kind"]
    if k == "fiveprime":
        return pa.FivePrimeMapFactory(spec["param"])
    if k == "threeprime":
        return pa.ThreePrimeMapFactory(spec["param"])
    if k == "center":
        return pa.CenterMapFactory(spec["param"])
    return pa.VariableFivePrimeMapFactory(gu.offset_dict_of(spec))


_vectors = {}


def oracle_vectors(ex):
    """``{contig: vector}`` of a golden export from the oracle: ``get(whole contig, roi_order=False)`` under its rule,
    strand and normalisation.  Computed once per (rule, normalisation, strand)."""
    from oracle import oracle
    from tests import golden_util as gu
    man, aln = golden()
    key = (json.dumps(ex["spec"], sort_keys=True), ex["normalize"], ex["strand"])
    if key not in _vectors:
        s = ex["spec"]
        spec = oracle.mapping_spec(s["kind"], s.get("param", 0), gu.offset_dict_of(s))
        _vectors[key] = {c: oracle.get_segment(aln, spec, t, 0, n, ex["strand"], roi_order=False, normalize_sum=man["mapped"] if ex["normalize"] else None)
                         for t, (c, n) in enumerate(zip(man["references"], man["lengths"]))}
    return _vectors[key]


def reference_bedgraph(vectors, window):
    """The reference's window loop (genome_array.py:1079-1111) over ``{contig: vector}``, without the track line."""
    out = []
    for chrom in sorted(vectors):
        v = vectors[chrom]
        for w0 in range(0, len(v), window):
            c = v[w0:min(w0 + window, len(v))]
            if c.sum() > 0:
                start, last = w0, c[0]
                for x, val in enumerate(c[1:]):
                    if val != last:
                        if last > 0:
                            out.append("%s\t%s\t%s\t%s\n" % (chrom, start, 1 + x + w0, last))
                        start, last = 1 + x + w0, val
                if last > 0:
                    out.append("%s\t%s\t%s\t%s\n" % (chrom, start, w0 + len(c), last))
    return "".join(out)


def reference_variable_step(vectors, window):
    """The reference's loop (genome_array.py:1025-1039) over ``{contig: vector}``, without the track line."""
    out = []
    for chrom in sorted(vectors):
        v = vectors[chrom]
        out.append("variableStep chrom=%s span=1\n" % chrom)
        for w0 in range(0, len(v), window):
            c = v[w0:min(w0 + window, len(v))]
            if c.sum() > 0:
                for i in c.nonzero()[0]:
                    out.append("%s\t%s\n" % (w0 + i + 1, c[i]))
    return "".join(out)


def designed_packed(pa, lengths, counts, reverse=(), alen=1):
    """Reads for ``{contig: length}`` (in this order) that give ``counts[contig][position] = c`` under
    ``FivePrimeMapFactory(0)``: `c` one-block reads of `alen` nt starting at `position`, on '+' (on '-' for the contigs in
    `reverse`: with 1-nt reads the count is the same)."""
    names = list(lengths)
    tid, pos, flags = [], [], []
    for t, c in enumerate(names):
        for p in sorted(counts.get(c, {})):
            n = int(counts[c][p])
            tid += [t] * n
            pos += [p] * n
            flags += [1 if c in reverse else 0] * n
    n = len(tid)
    return pa.PackedAlignments(np.array(tid, np.int32), np.array(pos, np.int32), np.full(n, alen, np.uint16), np.array(flags, np.uint8), np.ones(n, np.uint8),
                               references=names, lengths=[int(lengths[c]) for c in names])
