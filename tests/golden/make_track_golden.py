#!/usr/bin/env python
"""Golden data for count tracks read back in (bedGraph / wiggle -> GenomeArray), from the REFERENCE ITSELF.

Run only in the build container (needs the scratch reference of build_scratch_reference.sh):

    bash tests/golden/build_scratch_reference.sh /tmp/oracle
    PYTHONPATH=/tmp/oracle:/tmp/oracle/stubs:. python tests/golden/make_track_golden.py

Drives the reference's own ``WiggleReader`` (plastid/readers/wiggle.py:43-174) and ``GenomeArray.add_from_wiggle`` /
``get`` / ``sum`` (plastid/genomics/genome_array.py:1323-1533, 1978-1994) with ``SegmentChain.get_counts`` /
``get_masked_counts`` over small texts.  Writes DATA ONLY to ``tests/golden/track_fixture.npz``: the input texts, the
reader's tuples, ``chroms()``, ``lengths()``, ``sum()``, the arrays after import, segment and chain values on '+' and '-'
(masked chains and normalised gets included) and, for every refused text, the 1-based line that is at fault.
"""
import io
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

from plastid.genomics.genome_array import GenomeArray
from plastid.genomics.roitools import GenomicSegment, SegmentChain
from plastid.readers.wiggle import WiggleReader

MIN_CHR = 2000


def export_texts():
    """A bedGraph as BAMGenomeArray.to_bedgraph writes it: the fiveprime export of export_regions.npz, '+' and '-'."""
    m = json.loads(str(np.load(os.path.join(HERE, "export_regions.npz"))["manifest"]))
    out = {}
    for e in m["exports"]:
        if e["what"] == "bedgraph" and e["spec"]["kind"] == "fiveprime" and not e["normalize"] and e["window"] == 777 and e["strand"] in "+-":
            out[e["strand"]] = e["text"]
    return out, dict(zip(m["references"], m["lengths"]))


def cases():
    exp, exp_lengths = export_texts()
    c = []
    c.append({"name": "bedgraph_export", "chr_lengths": exp_lengths, "integer": True, "adds": [(exp["+"], "+"), (exp["-"], "-")]})
    c.append({"name": "variable_step", "integer": True, "adds": [(
        "variableStep chrom=chrA\n11 3\n12 5\n40 2\nvariableStep chrom=chrA span=3\n100 7\n200 1\nvariableStep chrom=chrB span=3\n5 4\n", "+")]})
    c.append({"name": "fixed_step", "integer": True, "adds": [(
        "fixedStep chrom=chrA start=11 step=5 span=2\n1\n2\n3\n4\nfixedStep chrom=chrB start=3\n9\n8\n7\nfixedStep chrom=chrA step=10 start=500\n6\n6\n", "-")]})
    c.append({"name": "mixed_formats", "integer": True, "adds": [(
        "track type=bedGraph name=a\nchrA\t10\t20\t3\nchrA\t20\t25\t1\ntrack type=wiggle_0 name=b description=\"x y\"\n"
        "variableStep chrom=chrB span=2\n7 5\n30 6\ntrack type=wiggle_0\nfixedStep chrom=chrC start=1 step=3\n1\n2\n3\nchrA 100 110 4\n", "+")]})
    c.append({"name": "four_tokens_in_variable", "integer": True, "adds": [(
        "variableStep chrom=chrA span=2\n10 1\n20 2\n30 40 50 60\n70 3\nchrA 5 8 2\n80 4\n", "+")]})
    c.append({"name": "data_after_bedgraph", "integer": True, "adds": [("chrA 10 20 3\n15 2\n7\n1 2 3\nchrA 30 31 1\n5 5 5 5 5\n", "+")]})
    c.append({"name": "data_before_any_header", "integer": True, "adds": [("15 2\n7\nvariableStep chrom=chrA\n3 1\n", "+")]})
    c.append({"name": "comments_blank", "integer": True, "adds": [(
        "# a comment\n\n   \t \nchrA 1 3 2\n#chrA 1 3 2\n \nvariableStep chrom=chrB\n# in a block\n4 4\n\n5 5\n", "+")]})
    c.append({"name": "crlf", "integer": True, "adds": [(
        "track type=bedGraph\r\nchrA\t1\t4\t2\r\nvariableStep chrom=chrB span=2\r\n4 4\r\n\r\nfixedStep chrom=chrB start=20\r\n5\r\n6\r\n", "+")]})
    c.append({"name": "no_final_newline", "integer": True, "adds": [("chrA 1 4 2\nchrA 9 12 5", "+"), ("fixedStep chrom=chrA start=2\n1\n7", "-")]})
    c.append({"name": "empty", "integer": True, "adds": [("", "+")]})
    c.append({"name": "growth", "chr_lengths": {"chrA": 500, "chrB": 300}, "integer": True, "adds": [(
        "chrA 10 20 1\nchrA 490 499 2\nchrA 495 500 3\nchrA 10400 10600 1\nchrZ 5 9 4\nchrZ 1990 2000 1\nchrY 1 2 1\nchrA 10499 10500 9\n", "+")]})
    c.append({"name": "two_calls", "integer": True, "adds": [
        ("chrA 10 20 1\nchrA 30 40 2\n", "+"), ("variableStep chrom=chrA span=4\n15 5\nvariableStep chrom=chrB\n1 1\n", "+"), ("chrA 0 50 1\n", "-")]})
    c.append({"name": "overlap_order", "integer": False, "adds": [(
        "chrA 10 20 0.1\nchrA 15 25 0.2\nchrA 18 30 0.3\nchrA 100 140 1e16\nchrA 110 120 0.1\nchrA 105 130 -1e16\nchrA 112 118 0.2\n"
        "chrA 300 310 0.3\nchrB 5 9 0.1\nchrB 7 8 0.2\nchrA 12 19 1e16\nchrA 12 19 -1e16\n", "+"),
        ("chrA 16 19 0.7\n", "+")]})
    c.append({"name": "specials", "integer": False, "adds": [(
        "chrA 1 3 -0.0\nchrA 5 6 nan\nchrA 8 9 inf\nchrA 10 11 -Infinity\nchrA 12 13 NaN\nchrA 14 15 -0\nchrA 16 17 1.\nchrA 18 19 .5\n", "+")]})
    c.append({"name": "python_ints", "integer": True, "adds": [(
        "chrA 1_0 +20 007\nchrA +5 0_0_8 1_0\nvariableStep chrom=chrA span=0_2\n1_00 3\n+50 2\n007 1\nfixedStep chrom=chrB start=+1_0 step=0_3\n1_1\n+2\n", "+")]})
    c.append({"name": "digits17", "integer": False, "adds": [(
        "chrA 1 2 0.12345678901234567\nchrA 3 4 12345678901234567\nchrA 5 6 9007199254740993\nchrA 7 8 0.1\nchrA 9 10 123456.789e3\nchrA 11 12 9007199254740992\n"
        "chrA 13 14 1.7976931348623157e308\nchrA 15 16 5e-324\nchrA 17 18 0.000001\n", "+")]})
    c.append({"name": "exponent_edges", "integer": False, "adds": [(
        "chrA 1 2 1e23\nchrA 3 4 1e22\nchrA 5 6 1e-22\nchrA 7 8 1e-23\nchrA 9 10 9007199254740992e22\nchrA 11 12 3e-22\nchrA 13 14 8.5e-5\n", "+")]})
    for x in c:
        x.setdefault("chr_lengths", None)
    return c


#: refused texts: (name, text, 1-based line at fault, does the reference raise too?)
REFUSED = [
    ("negative_start", "chrA 5 10 1\nchrA -5 10 1\n", 2, False),
    ("negative_variable", "variableStep chrom=chrA\n5 1\n0 1\n", 3, False),
    ("no_chrom", "# c\nvariableStep span=2\n\n5 1\n", 4, False),   # (the reference files the values under the contig None)
    ("header_token_without_key", "chrA 1 2 3\nfixedStep oops chrom=chrA\n1\n", 2, True),
    ("fixed_two_tokens", "fixedStep chrom=chrA start=1\n1\n2 3\n", 3, True),
    ("fixed_three_tokens", "fixedStep chrom=chrA start=1\n1 2 3\n", 2, True),
    ("variable_one_token", "variableStep chrom=chrA\n5 1\n6\n", 3, True),
    ("bad_int", "chrA 1 2 3\nchrA 1.5 10 2\n", 2, True),
    ("bad_value", "chrA 1 2 3\n\nchrA 1 10 abc\n", 3, True),
    ("hex_int", "chrA 0x1 5 1\n", 1, True),
    ("hex_value", "chrA 1 5 0x1p3\n", 1, True),
    ("double_underscore", "chrA 1__0 50 1\n", 1, True),
    ("trailing_underscore", "chrA 1 50 1_\n", 1, True),
    ("header_bad_span", "variableStep chrom=chrA span=two\n5 1\n", 1, True),
    ("header_two_equals", "variableStep chrom=chrA span=2=3\n5 1\n", 1, True),
    ("lowest_line_first", "chrA 1 2 3\nchrA 1 2 x\nchrA -1 2 3\nchrA 1 y 3\n", 2, True),
    ("no_newline_at_fault", "chrA 1 2 3\nchrA 1 2 3e", 2, True),
]

SEGMENTS = [("chrA", 0, 60, "+"), ("chrA", 0, 60, "-"), ("chrA", 5, 35, "-"), ("chrA", 95, 145, "+"), ("chrB", 0, 40, "+"), ("chrB", 0, 40, "-"),
            ("chrA", 480, 499, "+")]
CHAINS = [
    {"chrom": "chrA", "strand": "+", "segments": [(0, 30), (100, 150)], "masks": []},
    {"chrom": "chrA", "strand": "-", "segments": [(5, 25), (28, 45), (100, 130)], "masks": [(10, 30)]},
    {"chrom": "chrB", "strand": "+", "segments": [(0, 12), (20, 25)], "masks": [(3, 5)]},
    {"chrom": "chrB", "strand": "-", "segments": [(2, 30)], "masks": []},
]


def run_case(case):
    ga = GenomeArray(chr_lengths=case["chr_lengths"], min_chr_size=MIN_CHR)
    tuples = []
    for text, strand in case["adds"]:
        tuples.append([[t[0], int(t[1]), int(t[2]), float(t[3])] for t in WiggleReader(io.StringIO(text))])
        ga.add_from_wiggle(io.StringIO(text), strand)
    chroms = list(ga.chroms())
    lengths = {k: int(v) for k, v in ga.lengths().items()}
    total = float(ga.sum())
    arrays = {}
    for ch in chroms:
        for st in ("+", "-"):
            arrays["%s|%s|%s" % (case["name"], ch, st)] = np.array(ga._chroms[ch][st], np.float64)
    # queries stay inside the arrays of the contigs the case holds: the reference's get grows what it is asked beyond
    segs, chains = [], []
    for ch, a, b, st in SEGMENTS:
        if ch in lengths and b < lengths[ch]:
            segs.append({"seg": [ch, a, b, st], "key": "%s|seg%d" % (case["name"], len(segs))})
            arrays[segs[-1]["key"]] = np.array(ga[GenomicSegment(ch, a, b, st)], np.float64)
    for c in CHAINS:
        if c["chrom"] not in lengths:
            continue
        ivc = SegmentChain(*[GenomicSegment(c["chrom"], s, e, c["strand"]) for s, e in c["segments"]])
        if c["masks"]:
            ivc.add_masks(*[GenomicSegment(c["chrom"], s, e, c["strand"]) for s, e in c["masks"]])
        key = "%s|chain%d" % (case["name"], len(chains))
        arrays[key] = np.array(ivc.get_counts(ga), np.float64)
        masked = ivc.get_masked_counts(ga)
        arrays[key + "|masked"] = np.array(masked.data, np.float64)
        arrays[key + "|mask"] = np.array(np.ma.getmaskarray(masked), np.uint8)
        chains.append(dict(c, key=key))
    norm = []
    if case["integer"] and total > 0:
        ga.set_normalize(True)
        for s in segs:
            ch, a, b, st = s["seg"]
            key = s["key"] + "|norm"
            arrays[key] = np.array(ga[GenomicSegment(ch, a, b, st)], np.float64)
            norm.append(key)
        ga.set_normalize(False)
    assert {k: int(v) for k, v in ga.lengths().items()} == lengths and list(ga.chroms()) == chroms, "a query changed the reference array"
    return {"name": case["name"], "chr_lengths": case["chr_lengths"], "integer": case["integer"], "adds": [list(a) for a in case["adds"]],
            "tuples": tuples, "chroms": chroms, "lengths": lengths, "sum": repr(total), "segments": segs, "chains": chains, "normalised": norm}, arrays


def main():
    manifest = {"min_chr_size": MIN_CHR, "cases": [], "refused": []}
    arrays = {}
    for case in cases():
        m, a = run_case(case)
        manifest["cases"].append(m)
        arrays.update(a)
    for name, text, line, raises in REFUSED:
        raised = None
        try:
            GenomeArray(min_chr_size=MIN_CHR).add_from_wiggle(io.StringIO(text), "+")
        except Exception as e:  # noqa: BLE001 -- whatever the reference raises is recorded
            raised = type(e).__name__
        if (raised is not None) != raises:
            print("note: %s: the reference %s (the table says otherwise)" % (name, "raises %s" % raised if raised else "does not raise"))
        manifest["refused"].append({"name": name, "text": text, "line": line, "reference_raises": raised})
    out = os.path.join(HERE, "track_fixture.npz")
    np.savez_compressed(out, manifest=np.array(json.dumps(manifest)), **arrays)
    print("wrote %s: %d cases, %d refused texts; %.0f kB" % (out, len(manifest["cases"]), len(manifest["refused"]), os.path.getsize(out) / 1e3))


if __name__ == "__main__":
    main()
