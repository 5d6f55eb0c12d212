"""The zoom levels of plastid_amd.write_bigwig(zoom=...) -- the serial model of csrc/bigwig_write_host.h ("zoom levels") --
and the host readers bigwig_zoom_info / read_bigwig_zoom, on the CPU, over the cases of tests/bigwig_zoom_cases.py with
items_per_slot in {1, 2, 1024}, block_size in {2, 256} and the three compress modes: every level read back equals the
numpy restatement of the cases module bit for bit (records, level list, reductions, counts); the container is laid out as
the header states and every zoom block inflates with Python's zlib to whole records within uncompressBufSize;
zoom=False gives the recorded bytes of the existing fixture; read_bigwig reads a zoomed file as its twin; what is
refused; the stand-alone program tests/bigwig_zoom_host_test.cpp under the sanitizers; and what Kent's
bigWigSummaryArray returned for our files when tests/golden/bigwig_zoom_fixture.npz was made.  No GPU needed."""
import io
import os
import shutil
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import plastid_amd as pa  # noqa: E402
from tests import bigwig_write_cases as wc  # noqa: E402
from tests import bigwig_zoom_cases as zc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = zc.cases()
_expected = {}


def expected(name):
    if name not in _expected:
        _expected[name] = zc.expected_zoom(CASES[name])
    return _expected[name]


def write(name, ips=1024, bs=256, comp=True, **kw):
    case = CASES[name]
    fh = io.BytesIO()
    stats = pa.write_bigwig(zc.host_array(case), fh, "+", items_per_slot=ips, block_size=bs, compress=comp, zoom_stats=True, **dict(dict(zoom=case.zoom), **kw))
    return fh.getvalue(), stats


@pytest.mark.parametrize("name", list(CASES))
def test_levels_are_the_restatement(name):
    want = expected(name)
    for ips, bs, comp in zc.GRID:
        image, stats = write(name, ips, bs, comp)
        info = pa.bigwig_zoom_info(image)
        assert [(r, n) for r, _, _, n in info] == [(lv.reduction, len(lv.chrom_id)) for lv in want], (ips, bs, comp)
        for k, lv in enumerate(want):
            got = zc.table_bits(pa.read_bigwig_zoom(image, k))
            for a, b, col in zip(got, lv[1:], zc.Level._fields[1:]):
                assert a.dtype == np.uint32 and np.array_equal(a, b), (ips, bs, comp, k, col)
            blocks = zc.expected_blocks(lv, ips)
            assert (stats["zoom"][k]["reduction"], stats["zoom"][k]["records"], stats["zoom"][k]["blocks"], stats["zoom"][k]["raw_bytes"]) == \
                (lv.reduction, len(lv.chrom_id), len(blocks), 32 * len(lv.chrom_id))
        assert len(stats["zoom"]) == len(want)


def test_the_cases_reach_what_they_were_made_for():
    lv = expected("grid8")
    assert len(lv) >= 3 and lv[0].reduction == 8 and [x.reduction for x in lv] == [8 * 4 ** k for k in range(len(lv))]
    per_contig = np.bincount(lv[0].chrom_id, minlength=7)
    assert list(per_contig[:6]) == [1, 3, 0, 4, 768, 769] and len(lv[0].chrom_id) > 256
    assert expected("grid8_a_short")[0].end[0] == 5 and len(expected("grid8_a_short")) == 1          # level 1 would repeat level 0
    assert expected("grid8_d_plus1")[0].valid[-1] == 1 and list(expected("grid8_d_plus1")[0].start) == [0, 8, 16, 24]
    assert [x.reduction for x in expected("auto_single")][0] == 40 and expected("auto")[0].reduction > 40
    assert len(expected("wide64")) >= 6 and len(expected("wide64")[0].chrom_id) > 8000
    assert expected("no_items") == [] and expected("first_max")[0].reduction == 2 ** 24 and len(expected("first_max")) == 1
    sp = expected("special8")[0]
    rows = {int(s): k for k, (c, s) in enumerate(zip(sp.chrom_id, sp.start)) if c == 2}               # (sorted: big, fractions, special)
    assert sp.min[rows[8]] == zc.NAN_BITS and sp.max[rows[8]] == zc.NAN_BITS and sp.sum[rows[8]] == zc.NAN_BITS and sp.valid[rows[8]] == 8
    assert sp.sum[rows[48]] == zc.NAN_BITS and sp.sumsq[rows[56]] == 0x7f800000                       # inf - inf; 1e60 as float32
    assert sp.min[rows[64]] == 0x80000000 and sp.max[rows[64]] == 0 and sp.min[rows[0]] == struct.unpack("<I", struct.pack("<f", -1.5))[0]
    assert sp.sum[rows[40]] == zc.f32_bits(8.0 * (2.0 ** 24 + 2))


@pytest.mark.parametrize("name", list(CASES))
def test_the_container(name):
    want = expected(name)
    for ips, bs, comp in zc.GRID:
        image, stats = write(name, ips, bs, comp)
        plain, _ = write(name, ips, bs, comp, zoom=False)
        magic, version, zooms, ct, data, index, fc, dfc, aso, tso, buf, ext = struct.unpack("<IHHQQQHHQQIQ", image[:64])
        assert (magic, version, zooms, fc, dfc, aso, ext) == (0x888FFC26, 4, len(want), 0, 0, 0, 0) and image[-4:] == image[:4]
        L = len(want)
        if not L:
            assert image == plain
            continue
        # everything through the unzoomed R-tree is the plain file, moved behind the zoom headers
        p = struct.unpack("<IHHQQQHHQQIQ", plain[:64])
        assert (tso, ct, data, index) == (64 + 24 * L, p[3] + 24 * L, p[4] + 24 * L, p[5] + 24 * L)
        assert image[tso:tso + 40] == plain[64:104] and image[data:index] == plain[p[4]:p[5]]
        _, _, leaves, end = zc.rtree_leaves(image, index)
        _, _, pleaves, pend = zc.rtree_leaves(plain, p[5])
        assert [(x[:4], x[4] - 24 * L, x[5]) for x in leaves] == [(x[:4], x[4], x[5]) for x in pleaves] and pend + 4 == len(plain)
        headers = zc.zoom_headers(image)
        assert pa.bigwig_zoom_info(image) == [(h[0], h[2], h[3], len(lv.chrom_id)) for h, lv in zip(headers, want)]
        largest, at = 0, end
        for k, (h, lv) in enumerate(zip(headers, want)):
            assert h[0] == lv.reduction and h[1] == 0 and h[2] == at
            count, blocks, leaves, end = zc.read_level(image, h)
            cut = zc.expected_blocks(lv, ips)
            assert count == len(lv.chrom_id) and len(blocks) == len(cut) == stats["zoom"][k]["blocks"]
            assert zc.rtree_leaves(image, h[3])[0] == bs
            off = h[2] + 4
            for raw, leaf, (c, first, n) in zip(blocks, leaves, cut):
                assert len(raw) == 32 * n and leaf[4] == off and (not buf or len(raw) <= buf)
                assert leaf[:4] == (c, lv.start[first], c, lv.end[first + n - 1])
                rec = np.frombuffer(raw, "<u4").reshape(n, 8)
                assert np.array_equal(rec[:, 0], lv.chrom_id[first:first + n]) and np.array_equal(rec[:, 1], lv.start[first:first + n])
                assert np.array_equal(rec[:, 7], lv.sumsq[first:first + n])
                off += leaf[5]
                largest = max(largest, len(raw))
            assert off == h[3] and stats["zoom"][k]["file_bytes"] == off - h[2] - 4
            at = end
        assert at + 4 == len(image)
        sections = [zlib.decompress(image[o:o + n]) if buf else image[o:o + n] for _, _, _, _, o, n in zc.rtree_leaves(image, index)[2]]
        assert buf == (max([largest] + [len(s) for s in sections]) if comp else 0)


@pytest.mark.parametrize("name,ips,bs,comp", wc.RECORDED)
def test_zoom_false_writes_the_recorded_bytes(name, ips, bs, comp):
    case = wc.array_cases()[name]
    fh = io.BytesIO()
    pa.write_bigwig(wc.host_array(case), fh, "+", items_per_slot=ips, block_size=bs, compress=comp, zoom=False)
    assert fh.getvalue() == wc.load_fixture()["ours_" + wc.key(name, ips, bs, comp)].tobytes()
    assert pa.bigwig_zoom_info(fh.getvalue()) == []


@pytest.mark.parametrize("name", ["grid8", "special8", "auto", "no_items"])
def test_read_bigwig_reads_a_zoomed_file_as_its_twin(name, tmp_path):
    for ips, bs, comp in ((1024, 256, True), (2, 2, "dynamic"), (1, 256, False)):
        image, _ = write(name, ips, bs, comp)
        plain, _ = write(name, ips, bs, comp, zoom=False)
        a, b = pa.read_bigwig(image), pa.read_bigwig(plain)
        assert a.names == b.names and a.lengths == b.lengths and len(a) == len(b)
        for col in ("chrom", "start", "stop", "block"):
            assert np.array_equal(getattr(a, col), getattr(b, col))
        assert np.array_equal(a.value, b.value, equal_nan=True)
        assert list(pa.bigwig_info(image)["chroms"].items()) == list(pa.bigwig_info(plain)["chroms"].items())
        assert len(pa.bigwig_info(image)["blocks"]) == len(pa.bigwig_info(plain)["blocks"])
    p = tmp_path / "z.bw"
    p.write_bytes(image)
    assert pa.bigwig_zoom_info(str(p)) == pa.bigwig_zoom_info(image)
    if pa.bigwig_zoom_info(image):
        assert all(np.array_equal(x, y) for x, y in zip(zc.table_bits(pa.read_bigwig_zoom(str(p), 0)), zc.table_bits(pa.read_bigwig_zoom(image, 0))))


def test_refusals(tmp_path):
    ga = zc.host_array(CASES["grid8_d_plus1"])
    for bad in (7, 2 ** 24 + 1, 0, -1, 1.5, 8.0, "auto", None, np.float64(16)):
        fh = io.BytesIO()
        with pytest.raises(ValueError, match="zoom"):
            pa.write_bigwig(ga, fh, "+", zoom=bad)
        assert fh.getvalue() == b""
    for ok in (8, 2 ** 24, np.int64(16), True, np.bool_(True)):
        fh = io.BytesIO()
        pa.write_bigwig(ga, fh, "+", zoom=ok)
        assert len(pa.bigwig_zoom_info(fh.getvalue())) >= 1
    image, _ = write("grid8_d_plus1")
    assert len(pa.bigwig_zoom_info(image)) == 2
    p = tmp_path / "file.bw"
    p.write_bytes(image)
    for level in (2, -1, 99):
        with pytest.raises(ValueError, match=r"file\.bw: bigWig: zoom level %d of 2" % level):
            pa.read_bigwig_zoom(str(p), level)
    with pytest.raises(ValueError, match="<memory>: bigWig: zoom level 0 of 0"):
        pa.read_bigwig_zoom(write("no_items")[0], 0)
    headers = zc.zoom_headers(image)

    def damaged(at, fmt, value):
        b = bytearray(image)
        b[at:at + struct.calcsize(fmt)] = struct.pack(fmt, value)
        return bytes(b)
    for what, bad in (("zoom level 1: the index lies outside the file", damaged(64 + 24 + 16, "<Q", len(image) - 40)),
                      ("zoom level 0: the record count lies outside the file", damaged(64 + 8, "<Q", len(image) - 3)),
                      ("zoom level 0: the index has a wrong magic", damaged(headers[0][3], "<I", 0x12345678)),
                      ("zoom level 1: a reduction of 0", damaged(64 + 24, "<I", 0)),
                      ("the zoom headers lie outside the file", damaged(6, "<H", 60000))):
        with pytest.raises(ValueError, match="<memory>: bigWig: " + what):
            pa.bigwig_zoom_info(bad)
        with pytest.raises(ValueError, match="<memory>: bigWig: " + what):
            pa.read_bigwig_zoom(bad, 0)
    first_leaf = headers[0][3] + 48 + 4
    for what, bad in (("zoom level 0: the blocks hold 4 records, the level's count says 5", damaged(headers[0][2], "<I", 5)),
                      ("zoom level 0: a node of the index lies outside the file", damaged(headers[0][3] + 48 + 2, "<H", 60000)),
                      ("zoom level 0: block 0: the block lies outside the file", damaged(first_leaf + 16, "<Q", len(image) - 8)),
                      ("zoom level 0: block 0: not a zlib stream", damaged(headers[0][2] + 4, "<H", 0xFFFF)),
                      ("zoom level 0: block 0: (DEFLATE error|Adler-32 mismatch)", damaged(headers[0][2] + 4 + 12, "<I", 0x5a5a5a5a))):
        assert pa.bigwig_zoom_info(bad)[0][0] == 8                          # the headers stand
        with pytest.raises(ValueError, match="<memory>: bigWig: " + what):
            pa.read_bigwig_zoom(bad, 0)
    stored, _ = write("grid8_d_plus1", comp=False)
    h = zc.zoom_headers(stored)[0]
    leaf = h[3] + 48 + 4
    b = bytearray(stored)
    b[leaf + 24:leaf + 32] = struct.pack("<Q", 33)
    with pytest.raises(ValueError, match="zoom level 0: block 0: not a whole number of 32-byte records"):
        pa.read_bigwig_zoom(bytes(b), 0)
    with pytest.raises(ValueError, match="bigWig: shorter than the 64-byte header"):
        pa.bigwig_zoom_info(image[:40])
    with pytest.raises(IOError):
        pa.bigwig_zoom_info(str(tmp_path / "missing.bw"))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_the_model_parser_and_container_under_the_sanitizers(tmp_path):
    """tests/bigwig_zoom_host_test.cpp: the serial model against a restatement of its own, the zoom parser over whole,
    truncated and corrupted files, the container's offsets -- a stand-alone program under ASan and UBSan."""
    exe = str(tmp_path / "bigwig_zoom_host_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                    "-I", os.path.join(ROOT, "plastid_amd", "csrc"), os.path.join(ROOT, "tests", "bigwig_zoom_host_test.cpp"), "-o", exe, "-lz"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout


# ------------------------------------------------------------------ Kent's reader (tests/golden/bigwig_zoom_fixture.npz)
@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(ROOT, "tests", "golden", "bigwig_zoom_fixture.npz"))


def cells_f32(contig):
    v = np.zeros(wc.contig_size(contig), np.float64)
    v[:len(contig.cells)] = contig.cells.astype(np.float32)
    return v


def expected_summary(v, r, nb, kind):
    """What the cells give for nb bins of 2 r positions from 0 (NaN: a bin without data), exact for the integer cases: mean
    = sum / valid; min and max over the written cells; coverage = valid / bin size, the quotient taken as Kent takes it,
    (bins / span) x valid -- the same number, and the same double whenever the bin size is a power of two; std by
    calcStdFromSums restated in float64."""
    out = np.full(nb, np.nan)
    for b in range(nb):
        x = v[2 * r * b:2 * r * (b + 1)]
        x = x[x != 0.0]
        n = len(x)
        if not n:
            continue
        s, ss = float(x.sum()), float((x * x).sum())
        if kind == "mean":
            out[b] = s / n
        elif kind == "min":
            out[b] = x.min()
        elif kind == "max":
            out[b] = x.max()
        elif kind == "coverage":
            out[b] = (nb / float(2 * r * nb)) * n
        else:
            var = ss - s * s / n
            if n > 1:
                var /= n - 1
            out[b] = np.sqrt(var)
    return out


@pytest.mark.parametrize("comp", [True, False])
@pytest.mark.parametrize("name", zc.integer_cases())
def test_kents_summaries_of_our_files_are_what_the_cells_give(fx, name, comp):
    """bigWigSummaryArray over write_bigwig(zoom=...)'s file when the fixture was made: every query [0, 2 r_k nb) with nb =
    size // (2 r_k) bins picks level k (bbiBestZoom) and every bin is two whole windows; the file is still the one written."""
    case = CASES[name]
    image, _ = write(name, comp=comp)
    tag = "%s_%d" % (name, 1 if comp else 0)
    assert zlib.crc32(image) == int(fx["crc_" + tag])
    seen = 0
    for k, lv in enumerate(expected(name)):
        for ci, c in enumerate(sorted(case.contigs)):
            nb = wc.contig_size(case.contigs[c]) // (2 * lv.reduction)
            if nb < 1:
                continue
            v = cells_f32(case.contigs[c])
            for kind in ("mean", "min", "max", "coverage", "std"):
                got = fx["sum_%s_%d_%d_%s" % (tag, k, ci, kind)]
                want = expected_summary(v, lv.reduction, nb, kind)
                assert len(got) == nb and np.array_equal(got, want, equal_nan=True), (k, c, kind)
                seen += 1
    # (grid8_a_short and first_max hold no contig of two windows: Kent is asked nothing of them but to read the data)
    assert (seen >= 5) == any(wc.contig_size(v) >= 2 * expected(name)[0].reduction for v in case.contigs.values())
    assert seen >= 5 or name in ("grid8_a_short", "first_max")


@pytest.mark.parametrize("name", zc.integer_cases())
def test_kent_reads_a_zoomed_file_as_its_twin(fx, name):
    """Kent's bbiChromList and bigWigValsOnChromFetchData over the zoomed file: the cast arrays, and (``twins``) the very
    arrays they gave for the zoomed and the zoom=False file, compressed and stored, when the fixture was made."""
    assert fx["twins_" + name].tolist() == [True] * 4
    case = CASES[name]
    chroms = [str(c) for c in fx["read_%s_zoom_chroms" % name]]
    assert list(zip(chroms, fx["read_%s_zoom_ids" % name], fx["read_%s_zoom_sizes" % name])) == \
        [(c, i, wc.contig_size(case.contigs[c])) for i, c in enumerate(sorted(case.contigs))]
    arrays = {c: np.zeros(wc.contig_size(case.contigs[c])) for c in case.contigs}
    for (ci, a, b), v in zip(fx["read_%s_zoom_runs" % name], fx["read_%s_zoom_run_values" % name]):
        arrays[chroms[ci]][a:b] = v
    for c in case.contigs:
        assert np.array_equal(arrays[c], cells_f32(case.contigs[c]))
