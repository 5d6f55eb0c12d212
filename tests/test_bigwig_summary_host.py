"""Binned summaries of a bigWig file, the host model (plastid_amd.summarize_bigwig / summary_elements_bigwig;
csrc/bigwig_summary_host.h), on the CPU: Kent's ``bigWigSummaryArray`` bit for bit over the recorded queries of
tests/golden/bigwig_summary_fixture.npz -- files with Kent's zoom levels and with ours, bins that cut records -- and over the
``unaligned_*`` and ``sum_*`` keys of bigwig_zoom_fixture.npz; a restatement of the rules in Python floats on seeded queries
beyond the fixture; the coordinate-order refusal; the argument errors; the model under the sanitizers.  No GPU needed."""
import os
import shutil
import subprocess
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import plastid_amd as pa  # noqa: E402
from tests import bigwig_summary_cases as sc  # noqa: E402
from tests import bigwig_write_cases as wc  # noqa: E402
from tests import bigwig_zoom_cases as zc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORDER = "bigWig: summarize needs records in coordinate order"


def quiet(call, *args, **kwargs):
    """`call` without the DataWarning of a contig the file lacks."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", pa.DataWarning)
        return call(*args, **kwargs)


@pytest.mark.parametrize("tag", sc.tags())
def test_the_model_gives_what_kents_reader_recorded(tag):
    """Every recorded query and kind of one file: np.array_equal with NaN as the fill."""
    image, seen = sc.image_of(tag), 0
    for n_bins, rows, want in sc.batches(tag):
        got = quiet(pa.summarize_bigwig, image, rows, n_bins, kind=sc.KINDS)
        for k, kind in enumerate(sc.KINDS):
            assert sc.same(got[kind], want[k]), (tag, n_bins, kind)
        one = quiet(pa.summarize_bigwig, image, rows[:1], n_bins, kind="coverage", fill=-7.0)      # (a coverage is never NaN)
        assert sc.same(one, np.where(np.isnan(want[3][:1]), -7.0, want[3][:1]))
        seen += len(rows)
    assert seen == len(sc.fixture()["q_" + tag])


def test_the_recorded_queries_reach_every_table():
    """Rule 1 restated over the fixture: every level of every file, and the items, are selected; the edge cases are there."""
    fx = sc.fixture()
    for tag in sc.tags():
        reductions, q = [int(r) for r in fx["reductions_" + tag]], fx["q_" + tag]
        assert {sc.level_of(reductions, int(s), int(e), int(nb)) for c, s, e, nb in q if c >= 0} == set(range(-1, len(reductions))), tag
        sizes = fx["sizes_" + tag]
        assert (q[:, 3] == 1).any() and (q[:, 3] > q[:, 2] - q[:, 1]).any() and (q[:, 3] > 64).any()
        assert any(c >= 0 and e > sizes[c] for c, s, e, nb in q)
    assert [int(r) for r in fx["reductions_kent_mixed"]] == [140, 560, 2240, 8960] and len(fx["reductions_py_mixed"]) == 0


@pytest.mark.parametrize("name", zc.integer_cases())
def test_the_zoom_fixtures_unaligned_and_aligned_queries(name):
    """bigwig_zoom_fixture.npz: the ``unaligned_*`` keys (one query whose bins cut windows; recorded, never asserted until
    now) and the ``sum_*`` keys (bins of two whole windows) of the compressed and the stored file."""
    fx = np.load(os.path.join(ROOT, "tests", "golden", "bigwig_zoom_fixture.npz"))
    case = zc.cases()[name]
    levels = zc.expected_zoom(case)
    for comp in (1, 0):
        tag = "%s_%d" % (name, comp)
        image, seen = sc.image_of(tag), 0
        for k, lv in enumerate(levels):
            for ci, c in enumerate(sorted(case.contigs)):
                nb = wc.contig_size(case.contigs[c]) // (2 * lv.reduction)
                if nb < 1:
                    continue
                got = pa.summarize_bigwig(image, [(c, 0, 2 * lv.reduction * nb)], nb, kind=sc.KINDS)
                for kind in sc.KINDS:
                    assert sc.same(got[kind][0], fx["sum_%s_%d_%d_%s" % (tag, k, ci, kind)]), (tag, k, c, kind)
                seen += 1
        assert seen or name in ("grid8_a_short", "first_max")
        c = max(case.contigs, key=lambda x: wc.contig_size(case.contigs[x]))
        if "unaligned_%s_mean" % name in fx.files:
            got = pa.summarize_bigwig(image, [(c, 3, wc.contig_size(case.contigs[c]) - 2)], 3, kind=sc.KINDS)
            for kind in sc.KINDS:
                assert sc.same(got[kind][0], fx["unaligned_%s_%s" % (name, kind)]), (tag, kind)
    assert sum(1 for k in fx.files if k.startswith("unaligned_")) == 25


@pytest.mark.parametrize("tag", ["kent_mixed", "kent_two_per_block", "py_mixed", "grid8_1", "auto_0", "wide64_1"])
def test_a_restatement_of_the_rules_agrees_beyond_the_fixture(tag):
    """Rules 1 to 5 in Python floats over the host readers' tables, Kent's list walked as a list: seeded queries at every
    scale, on every contig and on a name the file lacks."""
    image = sc.image_of(tag)
    queries = sc.seeded_queries(tag, 60, 977)
    for n_bins in sorted(set(q[3] for q in queries)):
        rows = [q[:3] for q in queries if q[3] == n_bins]
        got = quiet(pa.summarize_bigwig, image, rows, n_bins, kind=sc.KINDS)
        el = quiet(pa.summary_elements_bigwig, image, rows, n_bins)
        for i, (chrom, start, end) in enumerate(rows):
            want = sc.restate(tag, chrom, start, end, n_bins)
            for k, kind in enumerate(sc.KINDS):
                assert sc.same(got[kind][i], want[k]), (tag, chrom, start, end, n_bins, kind)
            assert np.array_equal(el["valid"][i] == 0, np.isnan(want[0]))
            live = el["valid"][i] > 0
            assert np.array_equal(el["sum"][i][live] / el["valid"][i][live], want[0][live], equal_nan=True)
            assert np.array_equal(el["min"][i][live], want[1][live], equal_nan=True) and np.array_equal(el["max"][i][live], want[2][live], equal_nan=True)
            assert not el["sum"][i][~live].any() and not el["sumsq"][i][~live].any() and not el["min"][i][~live].any()


def test_one_kind_is_an_array_a_tuple_a_dict_and_segments_are_queries():
    image = sc.image_of("kent_mixed")
    name = str(sc.fixture()["names_kent_mixed"][0])
    rows = [(name, 5, 905), (name, 100, 130)]
    both = pa.summarize_bigwig(image, rows, 4, kind=("max", "mean"))
    assert sorted(both) == ["max", "mean"] and both["max"].shape == (2, 4) and both["max"].dtype == np.float64
    assert sc.same(pa.summarize_bigwig(image, rows, 4, kind="max"), both["max"])
    assert sc.same(pa.summarize_bigwig(image, rows, 4), both["mean"])
    segs = [pa.GenomicSegment(name, 5, 905, "-"), pa.GenomicSegment(name, 100, 130, "+")]
    assert sc.same(pa.summarize_bigwig(image, segs, 4, kind="max"), both["max"])      # (the host function knows no strands)
    assert pa.summarize_bigwig(image, [], 4).shape == (0, 4)
    el = pa.summary_elements_bigwig(image, rows, 4)
    assert sorted(el) == ["max", "min", "sum", "sumsq", "valid"] and all(v.shape == (2, 4) for v in el.values())
    with pytest.warns(pa.DataWarning, match="No data for chromosome 'chrNone'"):
        assert np.isnan(pa.summarize_bigwig(image, [("chrNone", 0, 10)], 2)).all()


def test_a_path_reads_as_its_bytes(tmp_path):
    image = sc.image_of("kent_stored")
    p = tmp_path / "k.bw"
    p.write_bytes(image)
    n_bins, rows, want = sc.batches("kent_stored")[0]
    assert sc.same(quiet(pa.summarize_bigwig, str(p), rows, n_bins, kind="coverage"), want[3])
    with pytest.raises(IOError):
        pa.summarize_bigwig(str(tmp_path / "missing.bw"), rows, n_bins)


def test_records_out_of_coordinate_order_are_refused_and_read_bigwig_is_not_touched():
    """``py_overlaps`` (items that overlap and go backwards; no levels): every summary needs its items, which are not in
    coordinate order; read_bigwig reads the file as before."""
    image = sc.image_of("py_overlaps")
    fx = sc.read_fixture()
    before = pa.read_bigwig(image).tuples()
    name = str(fx["py_overlaps_chroms"][0])
    with pytest.raises(ValueError, match="^<memory>: " + ORDER + "$"):
        pa.summarize_bigwig(image, [(name, 0, 50)], 5)
    with pytest.raises(ValueError, match=ORDER):
        pa.summary_elements_bigwig(image, [(name, 0, 5000)], 1)
    after = pa.read_bigwig(image)
    assert after.tuples() == before and len(before) > 0
    assert after.stats["blocks"] == len(fx["py_overlaps_blocks"])
    # a query on a contig the file lacks needs no table
    assert np.isnan(quiet(pa.summarize_bigwig, image, [("chrNone", 0, 50)], 5)).all()


def test_the_argument_errors():
    image = sc.image_of("kent_one")
    name = str(sc.fixture()["names_kent_one"][0])
    for n_bins in (0, -3):
        with pytest.raises(ValueError, match="n_bins"):
            pa.summarize_bigwig(image, [(name, 0, 10)], n_bins)
    for start, end in ((10, 10), (11, 10)):
        with pytest.raises(ValueError, match="start >= end"):
            pa.summarize_bigwig(image, [(name, 0, 5), (name, start, end)], 2)
    for start, end in ((0, 2 ** 31), (2 ** 31, 2 ** 31 + 5), (-1, 5)):
        with pytest.raises(ValueError, match="2\\^31"):
            pa.summarize_bigwig(image, [(name, start, end)], 2)
    with pytest.raises(ValueError, match="kind 'median'"):
        pa.summarize_bigwig(image, [(name, 0, 10)], 2, kind="median")
    with pytest.raises(ValueError, match="kind"):
        pa.summarize_bigwig(image, [(name, 0, 10)], 2, kind=("mean", "sum"))
    with pytest.raises(ValueError, match="bigWig: shorter than the 64-byte header"):
        pa.summarize_bigwig(image[:40], [(name, 0, 10)], 2)
    assert pa.summarize_bigwig(image, [(name, 0, 2 ** 31 - 1)], 1).shape == (1, 1)      # the largest end there is


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_the_model_under_the_sanitizers(tmp_path):
    """tests/bigwig_summary_host_test.cpp: the model over hand-built images -- an empty level, a truncated level block, a
    record that spans the whole query -- as a stand-alone program under ASan and UBSan."""
    exe = str(tmp_path / "bigwig_summary_host_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                    "-I", os.path.join(ROOT, "plastid_amd", "csrc"), os.path.join(ROOT, "tests", "bigwig_summary_host_test.cpp"), "-o", exe, "-lz"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout
