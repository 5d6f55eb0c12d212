"""Shared by tests/test_sam_text.py and tests/test_gpu_sam.py: BAM / SAM twins of the same records (tests/bam_writer.py and
tests/sam_writer.py), the htslib-written SAM fixture, and the malformed files with the message each must raise.  Nothing
here looks at what the code under test returns."""
import os

import numpy as np

from tests import bam_sort_cases, bam_writer, sam_writer
from tests import golden_util as gu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REFS, LENS = ["chrA", "chrB", "chrEnd"], [5000000, 3000000, 2147483647]
COLS = bam_sort_cases.COLS
same_columns = bam_sort_cases.same_columns


def same_with_order(a, b, what=""):
    same_columns(a, b, what)
    if a.file_order is None or b.file_order is None:
        assert a.file_order is None and b.file_order is None, what
    else:
        assert np.array_equal(a.file_order, b.file_order), what


def hts_sam(tmp):
    """(path of the SAM text htslib wrote for the records of hts_fixture.npz, that fixture, alignment lines in the text)."""
    fix = np.load(os.path.join(GOLDEN, "sam_fixture.npz"))
    path = os.path.join(str(tmp), "htslib.sam")
    with open(path, "wb") as fh:
        fh.write(fix["sam"].tobytes())
    return path, np.load(os.path.join(GOLDEN, "hts_fixture.npz")), int(fix["n_lines"])


def wide_packed():
    """The first file of the first genome-array case of wide_reads.npz (reads beyond the 16-bit / 8-bit columns)."""
    import plastid_amd as pa
    g = gu.load("wide_reads")
    case = [c for c in g.cases if c["kind"] == "ga"][0]
    aln = g.aln(case)
    nb = aln["nblk"].astype(np.int64)
    nb[aln["wide_idx"]] = aln["wide_nblk"]
    off = np.concatenate([[0], np.cumsum(np.where(nb >= 2, nb, 0))])
    idx = np.nonzero(aln["file_id"] == 0)[0]
    lo, hi = idx[0], idx[-1] + 1
    w = (aln["wide_idx"] >= lo) & (aln["wide_idx"] < hi)
    return pa.PackedAlignments(aln["tid"][lo:hi], aln["pos"][lo:hi], aln["alen"][lo:hi], aln["flags"][lo:hi], aln["nblk"][lo:hi],
                               aln["blk_start"][off[lo]:off[hi]], aln["blk_len"][off[lo]:off[hi]], references=case["aln"]["references"],
                               lengths=case["aln"]["lengths"], wide_idx=aln["wide_idx"][w] - lo, wide_alen=aln["wide_alen"][w],
                               wide_nblk=aln["wide_nblk"][w])


def synthetic_twins(tmp):
    """[(name, BAM path, SAM path)]: an unspliced C2 sample and a spliced C4 sample written like an aligner's output (names,
    sequences, qualities, NH and MD tags), the C4 sample in the bare packed form too, and the wide reads."""
    from plastid_amd import synth
    tmp = str(tmp)
    out = []
    for name, scale in (("C2", 0.0005), ("C4", 0.0003)):
        reads = synth.make_config(name, scale=scale)[2]
        bam, sam = os.path.join(tmp, name + ".bam"), os.path.join(tmp, name + ".sam")
        bam_writer.write_bam_realistic(bam, reads, threads=2)
        sam_writer.write_sam_realistic(sam, reads, nh_at="last" if name == "C4" else "first")
        out.append((name, bam, sam))
        if name == "C4":
            bam, sam = os.path.join(tmp, "C4p.bam"), os.path.join(tmp, "C4p.sam")
            bam_writer.write_bam_packed(bam, reads, threads=2)
            sam_writer.write_sam_packed(sam, reads)
            out.append(("C4-packed", bam, sam))
    wide = wide_packed()
    recs = bam_writer.packed_to_records(wide)
    bam, sam = os.path.join(tmp, "wide.bam"), os.path.join(tmp, "wide.sam")
    bam_writer.write_bam(bam, wide.references, wide.lengths, recs)
    sam_writer.write_sam(sam, wide.references, wide.lengths, recs)
    out.append(("wide", bam, sam))
    return out


# ---------------------------------------------------------------- malformed files
HEAD = ["@HD\tVN:1.6\tSO:coordinate", "@SQ\tSN:chrA\tLN:5000000", "@SQ\tLN:3000000\tSN:chrB", "@CO\tany other header line is ignored",
        "@SQ\tSN:chrEnd\tLN:2147483647"]
NHEAD = len(HEAD)


def good_line(i, tid=0, pos=None, cigar="30M", flag=0, mapq=30, tags="NH:i:1"):
    pos = 100 + 10 * i if pos is None else pos
    return "\t".join(["r%d" % i, str(flag), REFS[tid] if tid >= 0 else "*", str(pos + 1), str(mapq), cigar, "*", "0", "0", "A" * 30, "*"] + ([tags] if tags else []))


def with_field(i, k, value):
    """good line i with mandatory field k (0-based) replaced"""
    f = good_line(i).split("\t")
    f[k] = value
    return "\t".join(f)


def sam_msg(path, line, what):
    return "%s: SAM line %d: %s" % (path, line, what)


FLAG_TEXT = "FLAG is not a decimal number in 0 .. 65535"
POS_TEXT = "POS is not a decimal number in 0 .. 2^31 - 1"
MAPQ_TEXT = "MAPQ is not a decimal number in 0 .. 255"
CIGLEN_TEXT = "CIGAR operation without a length, or with one above 2^28 - 1"
REF_TEXT = "RNAME is not the SN of any @SQ header line"
FEW_TEXT = "fewer than 11 tab-separated fields"


def malformed_files():
    """[(name, header lines, body lines, expected)]: `expected` is ("sam", 1-based line, text) for a defect of SAM's own, or
    ("plain", text with {path}) for one worded as the BAM decoders word it.  Every file has a SECOND defect of another kind
    on a later line: the lowest line wins.  The long files put the defects into later tiles / pieces than the first."""
    n0 = NHEAD
    later_flag = with_field(9, 1, "0x10")
    later_ref = with_field(9, 2, "chrZ")

    def body(bad_at, bad, later, n=10):
        lines = [good_line(i) for i in range(n)]
        lines[bad_at] = bad
        lines[n - 1] = later
        return lines
    out = [
        ("empty-line", HEAD, body(3, "", later_flag), ("sam", n0 + 4, "empty line")),
        ("header-in-body", HEAD, body(2, "@CO\tlate", later_ref), ("sam", n0 + 3, "header line ('@') behind the first alignment line")),
        ("ten-fields", HEAD, body(5, "\t".join(good_line(5).split("\t")[:10]), later_flag), ("sam", n0 + 6, FEW_TEXT)),
        ("one-field", HEAD, body(0, "justaname", later_ref), ("sam", n0 + 1, FEW_TEXT)),
        ("flag-hex", HEAD, body(4, with_field(4, 1, "0x10"), later_ref), ("sam", n0 + 5, FLAG_TEXT)),
        ("flag-plus", HEAD, body(4, with_field(4, 1, "+5"), later_ref), ("sam", n0 + 5, FLAG_TEXT)),
        ("flag-big", HEAD, body(4, with_field(4, 1, "65536"), later_ref), ("sam", n0 + 5, FLAG_TEXT)),
        ("flag-empty", HEAD, body(4, with_field(4, 1, ""), later_ref), ("sam", n0 + 5, FLAG_TEXT)),
        ("rname-unknown", HEAD, body(6, with_field(6, 2, "chrZ"), later_flag), ("sam", n0 + 7, REF_TEXT)),
        ("rname-prefix", HEAD, body(6, with_field(6, 2, "chr"), later_flag), ("sam", n0 + 7, REF_TEXT)),
        ("pos-negative", HEAD, body(1, with_field(1, 3, "-1"), later_flag), ("sam", n0 + 2, POS_TEXT)),
        ("pos-big", HEAD, body(1, with_field(1, 3, "2147483648"), later_flag), ("sam", n0 + 2, POS_TEXT)),
        ("pos-zero-placed", HEAD, body(0, with_field(0, 3, "0"), later_flag), ("sam", n0 + 1, "alignment with a reference name and POS 0")),
        ("mapq-big", HEAD, body(7, with_field(7, 4, "256"), later_ref), ("sam", n0 + 8, MAPQ_TEXT)),
        ("cigar-no-length", HEAD, body(2, with_field(2, 5, "10MM5M"), later_flag), ("sam", n0 + 3, CIGLEN_TEXT)),
        ("cigar-length-big", HEAD, body(2, with_field(2, 5, "268435456M"), later_flag), ("sam", n0 + 3, CIGLEN_TEXT)),
        ("cigar-empty", HEAD, body(2, with_field(2, 5, ""), later_flag), ("sam", n0 + 3, "empty mandatory field")),
        ("cigar-unknown-op", HEAD, body(2, with_field(2, 5, "10M3Q5M"), later_flag), ("plain", "unknown CIGAR operation in {path}")),
        ("cigar-digits-only", HEAD, body(2, with_field(2, 5, "30"), later_flag), ("plain", "unknown CIGAR operation in {path}")),
        ("end-beyond", HEAD, [good_line(0), good_line(1, tid=2, pos=2147483600, cigar="30M10N30M"), later_flag],
         ("plain", "alignment ends beyond 2^31 - 1")),
        ("unsorted", HEAD, [good_line(0, pos=500), good_line(1, pos=400), later_flag], ("plain", "BAM file is not coordinate sorted: {path}")),
        ("placed-behind-unplaced", HEAD, [good_line(0), good_line(1, tid=-1, pos=-1, flag=4), good_line(2), later_flag],
         ("plain", "BAM file is not coordinate sorted: {path}")),
        ("deletion-first", HEAD, [good_line(0, pos=100, cigar="50D20M"), good_line(1, pos=120), later_flag],
         ("plain", "alignment starting with a deletion breaks coordinate order; not supported")),
        ("sq-no-sn", HEAD[:2] + ["@SQ\tLN:5"] + HEAD[2:], [good_line(0), later_flag], ("sam", 3, "@SQ line without an SN field")),
        ("sq-no-ln", HEAD[:2] + ["@SQ\tSN:x\tM5:abc"] + HEAD[2:], [good_line(0), later_flag], ("sam", 3, "@SQ line without an LN field")),
        ("sq-ln-zero", HEAD + ["@SQ\tSN:x\tLN:0"], [good_line(0), later_flag], ("sam", n0 + 1, "@SQ LN is not a decimal number in 1 .. 2^31 - 1")),
        ("sq-ln-big", HEAD + ["@SQ\tSN:x\tLN:2147483648"], [good_line(0), later_flag], ("sam", n0 + 1, "@SQ LN is not a decimal number in 1 .. 2^31 - 1")),
        ("sq-duplicate", HEAD + ["@SQ\tSN:chrA\tLN:7"], [good_line(0), later_flag], ("sam", n0 + 1, "@SQ line repeats the SN of an earlier one")),
        ("no-sq", ["@HD\tVN:1.6", "@PG\tID:x"], [good_line(0, tid=-1, pos=-1, flag=4)], ("sam", 3, "alignment lines in a file without any @SQ header line")),
    ]
    # long files: the first defect 2 500 lines in (another tile of the line-start kernels, another workgroup of the fields
    # kernel, another piece of the host reader), a defect of another kind 400 lines later
    n = 3000
    lines = [good_line(i) for i in range(n)]
    lines[2500] = with_field(2500, 4, "300")
    lines[2900] = with_field(2900, 1, "x")
    out.append(("long-mapq-then-flag", HEAD, lines, ("sam", n0 + 2501, MAPQ_TEXT)))
    lines = [good_line(i) for i in range(n)]
    lines[2600] = with_field(2600, 5, "10M3Q")
    lines[2601] = with_field(2601, 2, "nope")
    out.append(("long-op-then-ref", HEAD, lines, ("plain", "unknown CIGAR operation in {path}")))
    return out


def write_lines(path, head, body, eol="\n", final_newline=True):
    with open(path, "wb") as fh:
        fh.write(sam_writer.join_lines(list(head) + list(body), eol, final_newline))


def expected_message(expected, path):
    return sam_msg(path, expected[1], expected[2]) if expected[0] == "sam" else expected[1].format(path=path)
