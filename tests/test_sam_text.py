"""``read_sam`` (csrc/bam_stager.cpp ``pb_open_sam``, the line parser of csrc/sam_host.h): SAM text -- an aligner's output
as it is written -- gives the arrays ``read_bam`` gives for the same records in a BAM file.  Pinned against the text the
reference-held htslib wrote for the records of ``hts_fixture.npz`` (tests/golden/sam_fixture.npz), against BAM / SAM twins
of synthetic samples (tests/sam_writer.py), against the shuffled cases of tests/bam_sort_cases.py with ``sort=True``, and
on malformed files, each of which must raise the message of its lowest bad line.  CPU only."""
import gzip
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from plastid_amd import packing  # noqa: E402
from plastid_amd.bam import build_index, read_bam, read_sam, sam_header  # noqa: E402
from tests import bam_sort_cases, sam_cases, sam_writer  # noqa: E402
from tests.test_hts_golden import _expected_nh, _htslib_runs, _placed  # noqa: E402

REFS3, LENS3 = ["chrA", "chrB", "chrC"], [5000000, 3000000, 100000]


@pytest.fixture(scope="module")
def twins(tmp_path_factory):
    return sam_cases.synthetic_twins(tmp_path_factory.mktemp("sam_twins"))


def check_against_htslib(got, hts, n_lines):
    """`got` (a reader's arrays for the htslib-written text) against the columns htslib reported for the same records."""
    keep = _placed(hts)
    keep = keep[keep < n_lines]
    assert got.n == len(keep)
    assert list(got.references) == [str(x) for x in hts["references"]] and list(got.lengths) == [int(x) for x in hts["lengths"]]
    assert np.array_equal(got.tid, hts["tid"][keep])
    assert np.array_equal(got.flag16, hts["flag"][keep].astype(np.uint16))
    assert np.array_equal(got.flags & 1, (hts["flag"][keep] >> 4) & 1)
    assert np.array_equal(got.mapq, hts["mapq"][keep].astype(np.uint8))
    assert np.array_equal(got.qlen, hts["l_qseq"][keep].astype(np.int32))
    assert np.array_equal(got.nh, _expected_nh(hts)[keep])
    assert got.mapped == int(((hts["flag"][:n_lines] & 0x4) == 0).sum())
    for k, i in enumerate(keep):                                # positions from the runs
        runs, L = _htslib_runs(hts, i)
        assert got.runs_of(k) == runs and int(got.true_alen()[k]) == L, i
        assert int(got.pos[k]) == (runs[0][0] if runs else int(hts["pos"][i])), i


def test_htslib_written_text_column_for_column(tmp_path):
    path, hts, n_lines = sam_cases.hts_sam(tmp_path)
    assert n_lines == len(hts["tid"])
    for threads in (1, 4):
        check_against_htslib(read_sam(path, threads=threads), hts, n_lines)
    assert sam_header(path) == ([str(x) for x in hts["references"]], [int(x) for x in hts["lengths"]])


def test_htslib_text_equals_the_htslib_bam(tmp_path, monkeypatch):
    """... and both of htslib's files give the same arrays, also when the text is dealt out in pieces of a few lines."""
    path, hts, _ = sam_cases.hts_sam(tmp_path)
    bam = str(tmp_path / "htslib.bam")
    open(bam, "wb").write(hts["bam"].tobytes())
    want = read_bam(bam)
    sam_cases.same_columns(read_sam(path), want)
    monkeypatch.setenv("PB_SAM_PIECE", "700")
    sam_cases.same_columns(read_sam(path, threads=3), want)


def test_twins_equal_as_arrays(twins, monkeypatch):
    for name, bam, sam in twins:
        want = read_bam(bam)
        assert want.n > 0
        sam_cases.same_columns(read_sam(sam), want, name)
    monkeypatch.setenv("PB_SAM_PIECE", "5000")                  # many pieces: the stitching
    for name, bam, sam in twins:
        sam_cases.same_columns(read_sam(sam, threads=4), read_bam(bam), name)
    assert len(read_bam(twins[-1][1]).wide_idx) >= 2            # (the wide reads are wide)


def test_nh_wherever_it_stands_and_odd_tags(tmp_path):
    recs, want_nh = sam_cases.bam_writer.odd_aux_records()
    for nh_at in ("as_is", "first", "last"):
        path = str(tmp_path / ("odd_%s.sam" % nh_at))
        sam_writer.write_sam(path, REFS3, LENS3, recs, nh_at=nh_at)
        assert list(read_sam(path).nh) == want_nh, nh_at
    bam = str(tmp_path / "odd.bam")
    sam_cases.bam_writer.write_bam(bam, REFS3, LENS3, recs)
    sam_cases.same_columns(read_sam(str(tmp_path / "odd_as_is.sam")), read_bam(bam))
    # look-alikes: a tag VALUE that holds NH:i:, a string-typed NH, zero, beyond the column, negative
    lines = [sam_cases.good_line(i, tags=t) for i, t in enumerate(["XX:Z:aNH:i:5", "NH:Z:3", "NH:i:0", "NH:i:70000", "NH:i:-1", "XS:A:+\tNH:i:7\tNH:i:9", ""])]
    path = str(tmp_path / "alike.sam")
    sam_cases.write_lines(path, sam_cases.HEAD, lines)
    assert list(read_sam(path).nh) == [0, 0, 0, 65535, 0, 7, 0]


@pytest.mark.parametrize("name", ["0", "1", "2", "257", "4097", "wide", "pile"])
def test_sort_equals_the_bam_result(tmp_path, name, monkeypatch):
    """The shuffled cases of tests/bam_sort_cases.py written as SAM: ``sort=True`` gives the BAM reader's result, ``file_order``
    included; without ``sort`` a file out of order raises the unsorted error."""
    if name == "wide":
        recs = bam_sort_cases.wide_records()
    elif name == "pile":
        recs = bam_sort_cases.tie_pile(600)
    else:
        recs = bam_sort_cases.random_records(int(name), 3, seed=int(name) + 7)
    bam, sam = str(tmp_path / "s.bam"), str(tmp_path / "s.sam")
    bam_sort_cases.write_fast(bam, REFS3, LENS3, recs)
    sam_writer.write_sam(sam, REFS3, LENS3, recs)
    if name == "4097":
        monkeypatch.setenv("PB_SAM_PIECE", "20000")
    timing = {}
    got, want = read_sam(sam, sort=True, timing=timing), read_bam(bam, sort=True)
    sam_cases.same_with_order(got, want, name)
    bam_sort_cases.same_file_order(got, recs, name)
    assert timing["records_moved"] == bam_sort_cases.model_order(recs)[1] and timing["sorted_input"] == bam_sort_cases.in_order(recs)
    if not bam_sort_cases.in_order(recs):
        with pytest.raises(ValueError) as e:
            read_sam(sam)
        assert str(e.value) == "%s: %s" % (bam_sort_cases.UNSORTED, sam)


def test_line_ends_and_small_files(tmp_path):
    recs = bam_sort_cases.twin_of(bam_sort_cases.random_records(300, 3, seed=11))
    base = str(tmp_path / "lf.sam")
    sam_writer.write_sam(base, REFS3, LENS3, recs)
    want = read_sam(base)
    assert want.n > 200
    for k, (eol, final) in enumerate((("\r\n", True), ("\n", False), ("\r\n", False))):
        path = str(tmp_path / ("v%d.sam" % k))
        sam_writer.write_sam(path, REFS3, LENS3, recs, eol=eol, final_newline=final)
        sam_cases.same_columns(read_sam(path), want, (eol, final))
    # a header and no record; nothing at all; an '@' header without @SQ and without records
    for k, text in enumerate((sam_writer.join_lines(sam_writer.header_lines(REFS3, LENS3)), b"", b"@HD\tVN:1.6\n@CO\tnothing\n")):
        path = str(tmp_path / ("e%d.sam" % k))
        open(path, "wb").write(text)
        got = read_sam(path)
        assert got.n == 0 and got.mapped == 0 and list(got.references) == (REFS3 if k == 0 else [])
        assert read_sam(path, sort=True).n == 0
    assert sam_header(str(tmp_path / "e0.sam")) == (REFS3, LENS3)
    # @SQ fields in any order, other fields around them
    path = str(tmp_path / "order.sam")
    open(path, "wb").write(b"@SQ\tM5:0123\tLN:77\tAS:x\tSN:one\n@HD\tVN:1.0\n@SQ\tSN:two\tLN:2147483647\n")
    assert sam_header(path) == (["one", "two"], [77, 2147483647])


@pytest.mark.parametrize("case", sam_cases.malformed_files(), ids=lambda c: c[0])
def test_malformed_files_raise_the_lowest_line(tmp_path, case, monkeypatch):
    name, head, body, expected = case
    path = str(tmp_path / (name + ".sam"))
    sam_cases.write_lines(path, head, body)
    want = sam_cases.expected_message(expected, path)
    for piece in (None, "400"):
        if piece:
            monkeypatch.setenv("PB_SAM_PIECE", piece)
        with pytest.raises(ValueError) as e:
            read_sam(path, threads=3)
        assert str(e.value) == want, piece
    # with sort=True a file out of order is no defect, and a line's own defect comes before a pair that breaks the order
    # of the first aligned positions (include/plastid_counts.h, PC_BAM_SORT): those three files raise their LATER defect
    if name in ("unsorted", "placed-behind-unplaced", "deletion-first"):
        want = sam_cases.sam_msg(path, len(head) + len(body), sam_cases.FLAG_TEXT)
    with pytest.raises(ValueError) as e:
        read_sam(path, sort=True)
    assert str(e.value) == want


def test_refusals(tmp_path):
    from plastid_amd.genome_array import _open_alignment_source
    recs = [(0, 5, [(0, 30)], 0), (1, 9, [(0, 30)], 16)]
    path = str(tmp_path / "r.SAM")                              # (the suffix in any letter case)
    sam_writer.write_sam(path, REFS3, LENS3, recs)
    aln = _open_alignment_source(path, decode="host")
    assert aln.n == 2 and aln.decoder == "host"
    with pytest.raises(ValueError) as e:
        _open_alignment_source(path, regions=[("chrA", 0, 100)], decode="host")
    assert "SAM text has no index" in str(e.value)
    with pytest.raises(ValueError) as e:
        build_index(path)
    assert "SAM text" in str(e.value)
    gz = str(tmp_path / "z.sam")
    with gzip.open(gz, "wb") as fh:
        fh.write(open(path, "rb").read())
    for call in (lambda: read_sam(gz), lambda: sam_header(gz), lambda: _open_alignment_source(gz, decode="host")):
        with pytest.raises(ValueError) as e:
            call()
        assert "compressed SAM" in str(e.value)
    with pytest.raises(IOError):
        read_sam(str(tmp_path / "absent.sam"))
    assert packing.PackedAlignments is type(aln)
