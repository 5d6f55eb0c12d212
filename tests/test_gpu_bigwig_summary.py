"""BigWigReader.summarize / summarize_batch / summary_elements_batch -- the tables and kernels of
csrc/bigwig_summary.hip.h and csrc/bigwig_summary_kernels.hip.h (k_bbi_zoom_records, k_bbi_items, k_bbi_index,
k_bbi_summarize) -- against the serial host model (plastid_amd.summarize_bigwig / summary_elements_bigwig, tested on the
CPU by test_bigwig_summary_host.py) bit for bit, and against what Kent's reader recorded
(tests/golden/bigwig_summary_fixture.npz), over every fixture file and query: contigs of 1200 to 3000 positions for
Kent's files, our integer zoom cases compressed and stored.  One batch mixes every table of a file; lanes cross a wave
and a workgroup; an empty batch; the second call loads nothing; '-' segments; an unknown contig; records out of
coordinate order; damaged zoom levels and data blocks refused with the host readers' words, the table left unloaded;
a to_bigwig(zoom=True) file against its cells; compress="dynamic"."""
import collections
import ctypes
import io
import os
import struct
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import plastid_amd as pa  # noqa: E402
from plastid_amd import _lib  # noqa: E402
from plastid_amd.engine import Engine  # noqa: E402
from tests import bigwig_summary_cases as sc  # noqa: E402
from tests import bigwig_writer as bw  # noqa: E402
from tests import bigwig_zoom_cases as zc  # noqa: E402
from tests import test_bigwig_host as host  # noqa: E402

pytestmark = pytest.mark.gpu
ELEMENTS = ("valid", "min", "max", "sum", "sumsq")


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def readers(eng, tmp_path_factory):
    """tag -> a BigWigReader over the file of the tag, on one engine, opened once."""
    made, root = {}, tmp_path_factory.mktemp("bws")

    def get(tag, image=None):
        if tag not in made:
            p = root / (tag + ".bw")
            p.write_bytes(sc.image_of(tag) if image is None else image)
            made[tag] = pa.BigWigReader(str(p), engine=eng)
        return made[tag]
    yield get
    for r in made.values():
        r.close()


def quiet(call, *args, **kwargs):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", pa.DataWarning)
        return call(*args, **kwargs)


def same_bits(a, b):
    """Equal as bit patterns but for the sign and payload of a NaN (the elements of a NaN item)."""
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a) & ~np.isnan(a), np.signbit(b) & ~np.isnan(b))


@pytest.mark.parametrize("tag", sc.tags())
def test_every_fixture_query_is_the_host_models_and_kents(readers, tag):
    r, image = readers(tag), sc.image_of(tag)
    for n_bins, rows, want in sc.batches(tag):
        got = quiet(r.summarize_batch, rows, n_bins, kind=sc.KINDS)
        host = quiet(pa.summarize_bigwig, image, rows, n_bins, kind=sc.KINDS)
        for k, kind in enumerate(sc.KINDS):
            assert same_bits(got[kind], host[kind]), (tag, n_bins, kind)
            assert sc.same(got[kind], want[k]), (tag, n_bins, kind)
        el, host_el = quiet(r.summary_elements_batch, rows, n_bins), quiet(pa.summary_elements_bigwig, image, rows, n_bins)
        for k in ELEMENTS:
            assert same_bits(el[k], host_el[k]), (tag, n_bins, k)
    st = r.summary_stats()
    assert st["tables"] == st["tables_loaded"] == len(sc.fixture()["reductions_" + tag]) + 1
    assert all(t["records"] is not None and t["queries"] > 0 for t in st["per_table"].values())


def test_one_batch_mixes_every_table_of_a_file(readers):
    """kent_mixed, one bin per query: spans that select the items and each of the four levels, in one call and one
    launch per table; the answer is the host model's, row by row, in the caller's order."""
    tag = "kent_mixed"
    fx = sc.fixture()
    names, reductions = [str(x) for x in fx["names_" + tag]], [int(x) for x in fx["reductions_" + tag]]
    rows = []
    for k, span in enumerate([3] + [2 * x + 7 for x in reductions]):
        for c in range(len(names)):
            rows.append((names[c], 11 * k + c, 11 * k + c + span))
    rows = rows[::2] + rows[1::2]                                # (the tables interleaved)
    picked = [sc.level_of(reductions, s, e, 1) for _, s, e in rows]
    assert set(picked) == set(range(-1, len(reductions)))
    r = readers(tag)
    before = r.summary_stats()["per_table"]
    got = r.summarize_batch(rows, 1, kind=sc.KINDS)
    host = pa.summarize_bigwig(sc.image_of(tag), rows, 1, kind=sc.KINDS)
    for kind in sc.KINDS:
        assert same_bits(got[kind], host[kind]), kind
        assert sc.same(got[kind][:, 0], np.array([sc.restate(tag, c, s, e, 1)[sc.KINDS.index(kind), 0] for c, s, e in rows])), kind
    after = r.summary_stats()["per_table"]
    for key, level in zip(after, range(-1, len(reductions))):
        assert after[key]["queries"] - before[key]["queries"] == picked.count(level)


def test_lanes_cross_a_wave_and_a_workgroup(readers):
    """Seven queries of 97 bins (679 lanes: three workgroups; a query's bins span two waves) from the items and from a
    level, and 300 queries of 3 bins."""
    for tag in ("kent_two_per_block", "wide64_1"):
        r, image = readers(tag), sc.image_of(tag)
        fx = sc.fixture()
        names, sizes = [str(x) for x in fx["names_" + tag]], fx["sizes_" + tag]
        c = int(np.argmax(sizes))
        rng = np.random.default_rng(5)
        for n_bins, nq, spans in ((97, 7, (150, 97 * 2 * 140 + 9)), (3, 300, (7, 900))):
            rows = []
            for i in range(nq):
                span = spans[i % 2]
                start = int(rng.integers(0, sizes[c]))
                rows.append((names[c], start, start + span))
            got, host = r.summarize_batch(rows, n_bins, kind=sc.KINDS), pa.summarize_bigwig(image, rows, n_bins, kind=sc.KINDS)
            for kind in sc.KINDS:
                assert same_bits(got[kind], host[kind]), (tag, n_bins, kind)
            assert np.isfinite(got["mean"]).sum() > n_bins


def test_an_empty_batch_and_one_segment(readers):
    r = readers("kent_one")
    assert r.summarize_batch([], 4).shape == (0, 4)
    assert sorted(r.summary_elements_batch([], 2)) == sorted(ELEMENTS)
    name = str(sc.fixture()["names_kent_one"][0])
    seg = pa.GenomicSegment(name, 10, 1510, "+")
    one = r.summarize(seg, 5)
    assert one.shape == (5,) and same_bits(one, pa.summarize_bigwig(sc.image_of("kent_one"), [seg], 5)[0])
    assert r.summarize(seg).shape == (1,)
    both = r.summarize(seg, 5, kind=("min", "std"))
    assert sorted(both) == ["min", "std"] and both["min"].shape == (5,)
    assert same_bits(r.summarize(seg, 5, fill=0.5), np.where(np.isnan(one), 0.5, one))


def test_the_second_call_loads_nothing(eng, tmp_path):
    p = tmp_path / "k.bw"
    p.write_bytes(sc.image_of("kent_stored"))
    r = pa.BigWigReader(str(p), engine=eng)
    try:
        n_bins, rows, _ = sc.batches("kent_stored")[0]
        st0 = r.summary_stats()
        assert st0["tables_loaded"] == 0 and st0["bytes_uploaded"] == 0 and all(t["records"] is None for t in st0["per_table"].values())
        first = quiet(r.summarize_batch, rows, n_bins)
        st1, t1 = r.summary_stats(), r.summary_timing()
        assert st1["tables_loaded"] >= 1 and st1["bytes_uploaded"] > 0
        second = quiet(r.summarize_batch, rows, n_bins)
        st2, t2 = r.summary_stats(), r.summary_timing()
        assert same_bits(first, second)
        assert (st2["tables_loaded"], st2["bytes_uploaded"], st2["bytes_inflated"]) == (st1["tables_loaded"], st1["bytes_uploaded"], st1["bytes_inflated"])
        assert [t["records"] for t in st2["per_table"].values()] == [t["records"] for t in st1["per_table"].values()]
        assert sum(t["queries"] for t in st2["per_table"].values()) == 2 * sum(t["queries"] for t in st1["per_table"].values())
        assert t2["upload"] == t2["inflate_adler"] == t2["records_order_check"] == 0.0 and t2["kernel"] > 0.0
        assert sorted(t1) == ["inflate_adler", "kernel", "read_back", "records_order_check", "upload"]
    finally:
        r.close()


def test_minus_segments_come_reversed(readers):
    r = readers("kent_mixed")
    name = str(sc.fixture()["names_kent_mixed"][0])
    plus, minus = pa.GenomicSegment(name, 20, 1400, "+"), pa.GenomicSegment(name, 20, 1400, "-")
    fwd = r.summarize_batch([plus, minus], 6, kind=("mean", "max"))
    for k in fwd:
        assert same_bits(fwd[k][1], fwd[k][0][::-1]) and not same_bits(fwd[k][0], fwd[k][0][::-1])
    assert same_bits(r.summarize_batch([minus], 6, roi_order=False), fwd["mean"][:1])
    assert same_bits(r.summarize(minus, 6), fwd["mean"][0][::-1])


def test_an_unknown_contig_warns_and_gives_the_fill(readers):
    r = readers("kent_mixed")
    name = str(sc.fixture()["names_kent_mixed"][0])
    with pytest.warns(pa.DataWarning, match="No data for chromosome 'chrNone'"):
        got = r.summarize_batch([("chrNone", 0, 100), (name, 0, 900)], 3, fill=-1.0)
    assert (got[0] == -1.0).all() and same_bits(got[1], pa.summarize_bigwig(sc.image_of("kent_mixed"), [(name, 0, 900)], 3, fill=-1.0)[0])
    for bad in (dict(n_bins=0), dict(n_bins=2, rows=[(name, 5, 5)]), dict(n_bins=2, rows=[(name, 0, 2 ** 31)])):
        with pytest.raises(ValueError):
            r.summarize_batch(bad.get("rows", [(name, 0, 10)]), bad["n_bins"])
    with pytest.raises(ValueError, match="kind"):
        r.summarize_batch([(name, 0, 10)], 2, kind="median")


def test_records_out_of_order_raise_and_get_still_answers(readers):
    r = readers("py_overlaps")
    fx = sc.read_fixture()
    name = str(fx["py_overlaps_chroms"][0])
    seg = pa.GenomicSegment(name, 0, 40, "+")
    before = r.get(seg)
    with pytest.raises(ValueError, match="py_overlaps.bw: bigWig: summarize needs records in coordinate order$"):
        r.summarize(seg, 4)
    with pytest.raises(ValueError, match="coordinate order"):
        r.summary_elements_batch([seg], 1)
    assert np.array_equal(r.get(seg), before) and before.shape == (40,)
    assert r.summary_stats()["per_table"]["items"]["queries"] == 0


# ---------------------------------------------------------------------------------------------------------------------
# refusals of the device summary: error returns, not faults.  The words are the host readers' for the same file and path.

def zoomed_image(compress):
    fh = io.BytesIO()
    pa.write_bigwig(zc.host_array(zc.cases()["grid8_d_plus1"]), fh, "+", compress=compress, zoom=8)
    return fh.getvalue()


def damaged(image, at, fmt, value):
    b = bytearray(image)
    b[at:at + struct.calcsize(fmt)] = struct.pack(fmt, value)
    return bytes(b)


def host_words(read, *args):
    with pytest.raises(ValueError) as e:
        read(*args)
    return str(e.value)


def test_a_damaged_compressed_zoom_level_is_refused_twice_and_the_items_still_answer(eng, tmp_path):
    image = zoomed_image(True)
    headers = zc.zoom_headers(image)
    reductions = [z[0] for z in pa.bigwig_zoom_info(image)]
    p = tmp_path / "damaged_zoom.bw"
    p.write_bytes(damaged(image, headers[0][2] + 4 + 12, "<I", 0x5a5a5a5a))
    want = host_words(pa.read_bigwig_zoom, str(p), 0)
    assert want in ("%s: bigWig: zoom level 0: block 0: %s" % (p, w) for w in ("DEFLATE error", "Adler-32 mismatch"))
    r = pa.BigWigReader(str(p), engine=eng)                     # (the import does not read zoom blocks)
    try:
        coarse, fine = pa.GenomicSegment("d_plus1", 0, 25, "+"), pa.GenomicSegment("d_plus1", 0, 24, "+")
        assert sc.level_of(reductions, 0, 25, 1) == 0 and sc.level_of(reductions, 0, 24, 4) == -1
        for _ in range(2):                                      # (the table stays unloaded and is tried again)
            with pytest.raises(ValueError) as e:
                r.summarize(coarse, 1)
            assert str(e.value) == want
        assert r.summary_stats()["per_table"][reductions[0]]["records"] is None
        assert same_bits(r.summarize(fine, 4), pa.summarize_bigwig(p.read_bytes(), [fine], 4)[0])
        assert np.array_equal(r.get(coarse), zc.cases()["grid8_d_plus1"].contigs["d_plus1"].cells)
    finally:
        r.close()


@pytest.mark.parametrize("what", ["leaf_size_33", "count_5"])
def test_a_zoom_level_of_a_wrong_shape_is_refused(eng, tmp_path, what):
    if what == "leaf_size_33":
        image = zoomed_image(False)
        h = zc.zoom_headers(image)[0]
        image = damaged(image, h[3] + 48 + 4 + 24, "<Q", 33)
        words = "zoom level 0: block 0: not a whole number of 32-byte records"
    else:
        image = zoomed_image(True)
        image = damaged(image, zc.zoom_headers(image)[0][2], "<I", 5)
        words = "zoom level 0: the blocks hold 4 records, the level's count says 5"
    p = tmp_path / (what + ".bw")
    p.write_bytes(image)
    assert host_words(pa.read_bigwig_zoom, str(p), 0) == "%s: bigWig: %s" % (p, words)
    r = pa.BigWigReader(str(p), engine=eng)
    try:
        with pytest.raises(ValueError) as e:
            r.summarize(pa.GenomicSegment("d_plus1", 0, 25, "+"), 1)
        assert str(e.value) == "%s: bigWig: %s" % (p, words)
    finally:
        r.close()


@pytest.mark.parametrize("name,words", [("deflate", "block 0: DEFLATE error"), ("adler", "block 1: Adler-32 mismatch")])
def test_damaged_data_blocks_are_refused_by_the_summary_handle(eng, tmp_path, name, words):
    L = _lib.load()
    p = tmp_path / "refused.bw"
    p.write_bytes(host.refused_image(name))
    want = host_words(pa.read_bigwig, str(p))
    assert want == "%s: bigWig: %s" % (p, words)
    h = ctypes.c_void_p()
    _lib.check(L.pc_bigwig_summary_open_path(eng._h, os.fsencode(str(p)), ctypes.byref(h)))      # (the container is whole)
    try:
        contig, start, end, out = np.zeros(1, np.int32), np.zeros(1, np.int64), np.full(1, 9, np.int64), np.zeros(5, np.float64)
        with pytest.raises(ValueError) as e:
            _lib.check(L.pc_bigwig_summary_query(h, 1, contig.ctypes.data, start.ctypes.data, end.ctypes.data, 1, out.ctypes.data))
        assert str(e.value) == want
    finally:
        _lib.check(L.pc_bigwig_summary_close(h))
    # and the engine goes on working
    ga = pa.GenomeArray({"chrA": 1000}, strands=("+",), engine=eng)
    try:
        good = tmp_path / "good.bw"
        good.write_bytes(bw.write_bigwig(host.CHROMS, host.GOOD))
        _lib.check(L.pc_track_add_bigwig_path(ga._h, os.fsencode(str(good)), 0))
        assert ga.to_host()._chroms["chrB"]["+"][100:108].tolist() == [1.0, 1.0, 0.0, 2.0, 2.0, 0.0, 3.0, 3.0]
    finally:
        ga.close()


@pytest.mark.parametrize("compress", [True, "dynamic", False])
def test_a_file_of_to_bigwig_against_its_cells(eng, tmp_path, compress):
    """GenomeArray.to_bigwig(zoom=True) read back through BigWigReader.summarize: for bins of two whole windows of the
    level they select, mean, min, max and coverage are what the cells give (small integers: exact); the three compress
    modes read the same."""
    case = zc.cases()["auto"].contigs
    ga = pa.GenomeArray(collections.OrderedDict((k, v.length) for k, v in case.items()), strands=("+",), engine=eng)
    r = None
    try:
        for k, v in case.items():
            ga[pa.GenomicSegment(k, 0, len(v.cells), "+")] = v.cells
        p = tmp_path / "auto.bw"
        ga.to_bigwig(str(p), "+", compress=compress, zoom=True)
        image = p.read_bytes()
        r = pa.BigWigReader(str(p), engine=eng)
        levels = [z[0] for z in pa.bigwig_zoom_info(image)]
        assert len(levels) >= 2
        cells = np.asarray(case["wide"].cells, np.float64)
        for red in levels[:3]:
            nb = len(cells) // (2 * red)
            seg = pa.GenomicSegment("wide", 0, 2 * red * nb, "+")
            got = r.summarize(seg, nb, kind=("mean", "min", "max", "coverage"))
            x = cells[:2 * red * nb].reshape(nb, 2 * red)
            n = (x != 0).sum(axis=1)
            with np.errstate(invalid="ignore", divide="ignore"):
                mean = np.where(n > 0, x.sum(axis=1) / n, np.nan)
            assert same_bits(got["mean"], mean)
            assert same_bits(got["max"], np.where(n > 0, x.max(axis=1), np.nan))
            assert same_bits(got["min"], np.where(n > 0, np.where(x == 0, np.inf, x).min(axis=1), np.nan))
            assert same_bits(got["coverage"], np.where(n > 0, (float(nb) / float(2 * red * nb)) * n, np.nan))
            assert same_bits(r.get(seg), cells[:2 * red * nb])
        rows = [("wide", 7, 50007), ("single", 3, 2900), ("wide", 100, 133)]
        for kind in sc.KINDS:
            assert same_bits(r.summarize_batch(rows, 9, kind=kind), pa.summarize_bigwig(image, rows, 9, kind=kind))
    finally:
        if r is not None:
            r.close()
        ga.close()
