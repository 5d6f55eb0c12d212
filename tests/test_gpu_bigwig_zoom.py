"""GenomeArray.to_bigwig(zoom=...) and BAMGenomeArray.to_bigwig(zoom=...) -- the kernels of csrc/bigwig_zoom_kernels.hip.h
(level 0 from the item columns, the levels above, records, block table), k_zlib_deflate over the zoom blocks and the host
layout of csrc/bigwig_writer.hip.h -- against the serial host model (plastid_amd.write_bigwig(zoom=...), tested on the CPU
by test_bigwig_zoom_host.py): for every case of tests/bigwig_zoom_cases.py, items_per_slot in {1, 2, 1024}, block_size
in {2, 256} and the three compress modes the device's file is the host writer's over ``to_host()``, byte for byte -- but
for the 16 bytes of the TOTAL summary's two sums where the values are not integers, which the export adds in a fixed
tree and the host serially (the bound of test_gpu_bigwig_write.py; the zoom levels themselves, every byte behind the
unzoomed R-tree included, are compared exactly in every case); the zoom statistics are bigwig_zoom_info's; zoom=False
is the call without the keyword; a BAMGenomeArray's counts; BigWigReader reads a zoomed file as its twin; two exports
in a row give equal bytes; what is refused."""
import collections
import io
import math
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import plastid_amd as pa  # noqa: E402
from plastid_amd import track  # noqa: E402
from plastid_amd.engine import Engine  # noqa: E402
from plastid_amd.genome_array import DenseGenomeArray  # noqa: E402
from tests import bigwig_zoom_cases as zc  # noqa: E402
from tests import count_export_cases as cc  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = zc.cases()


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def arrays(eng):
    """name -> (device array with the case on '+', and a decoy on '-'; its host copy), made once."""
    made = {}

    def get(name):
        if name not in made:
            case = CASES[name].contigs
            ga = pa.GenomeArray(collections.OrderedDict((k, v.length) for k, v in case.items()), engine=eng)
            for k, v in case.items():
                if len(v.cells):
                    ga[pa.GenomicSegment(k, 0, len(v.cells), "+")] = v.cells
                    ga[pa.GenomicSegment(k, 0, min(3, len(v.cells)), "-")] = 5.0
            made[name] = (ga, ga.to_host())
        return made[name]
    yield get
    for ga, _ in made.values():
        ga.close()


def device_file(ga, strand="+", **kw):
    fh = io.BytesIO()
    ga.to_bigwig(fh, strand, **kw)
    return fh.getvalue()


def host_file(host, strand="+", **kw):
    fh = io.BytesIO()
    stats = pa.write_bigwig(host, fh, strand, zoom_stats=True, **kw)
    return fh.getvalue(), stats


def assert_same_file(got, want, integers):
    """Byte for byte; where the values are not integers the total summary's two sums by the reordering bound."""
    assert len(got) == len(want)
    if integers or not struct.unpack("<Q", want[44:52])[0]:
        assert got == want
        return
    at = struct.unpack("<Q", want[44:52])[0] + 24
    assert got[:at] == want[:at] and got[at + 16:] == want[at + 16:]
    items = pa.read_bigwig(want)
    w = (items.stop - items.start).astype(np.float64)
    for off, terms in ((at, items.value * w), (at + 8, items.value * items.value * w)):
        a, b = struct.unpack("<d", got[off:off + 8])[0], struct.unpack("<d", want[off:off + 8])[0]
        if b != b or math.isinf(b):
            assert (a != a and b != b) or a == b
        else:
            assert abs(a - b) <= 2 * len(items) * 2.0 ** -53 * float(np.abs(terms).sum())


@pytest.mark.parametrize("name", list(CASES))
def test_device_file_is_the_host_models(arrays, name):
    ga, host = arrays(name)
    case = CASES[name]
    for ips, bs, comp in zc.GRID:
        kw = dict(items_per_slot=ips, block_size=bs, compress=comp, zoom=case.zoom)
        want, stats = host_file(host, **kw)
        got = device_file(ga, **kw)
        assert_same_file(got, want, case.integer)
        levels = ga.bigwig_export_zoom_stats()
        assert levels == stats["zoom"], (ips, bs, comp)
        assert [(x["reduction"], x["records"]) for x in levels] == [(r, n) for r, _, _, n in pa.bigwig_zoom_info(got)]
        assert {k: v for k, v in stats.items() if k != "zoom"} == ga.bigwig_export_stats()
        assert set(ga.bigwig_export_zoom_timing()) == {"level0", "upper_levels", "records", "deflate_compaction"}
    if name == "no_items":
        assert levels == []
    else:
        assert len(levels) >= 1 and levels[0]["records"] > 0


def test_zoom_false_is_the_call_without_the_keyword(arrays):
    ga, host = arrays("grid8")
    for kw in (dict(), dict(items_per_slot=2, block_size=2, compress="dynamic"), dict(compress=False)):
        plain = device_file(ga, **kw)
        assert device_file(ga, zoom=False, **kw) == plain == host_file(host, **kw)[0]
        assert ga.bigwig_export_zoom_stats() == [] and pa.bigwig_zoom_info(plain) == []
        assert all(v == 0.0 for v in ga.bigwig_export_zoom_timing().values())
    # the C seam: zoom 0 through the new entry point
    n = track.ctypes.c_int64(0)
    assert ga._lib.pc_track_export_bigwig_zoom(ga._h, 0, 1024, 256, 1, 0, track.ctypes.byref(n)) == 0
    image = np.empty(n.value, np.uint8)
    assert ga._lib.pc_track_export_bigwig_read(ga._h, image.ctypes.data, n.value) == 0
    assert image.tobytes() == device_file(ga)


def test_two_exports_in_a_row_give_equal_bytes(arrays):
    ga, _ = arrays("wide64")
    first = device_file(ga, zoom=64, compress="dynamic")
    assert device_file(ga, zoom=64, compress="dynamic") == first
    other = device_file(ga, zoom=True)
    assert other != first and device_file(ga, zoom=64, compress="dynamic") == first


@pytest.mark.parametrize("name", ["grid8", "special8"])
def test_bigwig_reader_reads_a_zoomed_file_as_its_twin(arrays, eng, tmp_path, name):
    ga, host = arrays(name)
    zoomed, plain = tmp_path / "zoomed.bw", tmp_path / "plain.bw"
    ga.to_bigwig(str(zoomed), "+", items_per_slot=2, block_size=2, zoom=CASES[name].zoom)
    ga.to_bigwig(str(plain), "+", items_per_slot=2, block_size=2)
    a, b = pa.BigWigReader(str(zoomed), engine=eng), pa.BigWigReader(str(plain), engine=eng)
    try:
        assert a.chroms == b.chroms
        for k in host.lengths():
            with np.errstate(over="ignore"):
                want = host._chroms[k]["+"].astype(np.float32).astype(np.float64)
            got = a.get_chromosome_counts(k)
            assert np.array_equal(got, b.get_chromosome_counts(k), equal_nan=True) and np.array_equal(got[:len(want)], want, equal_nan=True)
        # imported and written again with the levels: the same file
        if CASES[name].integer:
            assert device_file(a._ga, ".", items_per_slot=2, block_size=2, zoom=CASES[name].zoom) == zoomed.read_bytes()
    finally:
        a.close()
        b.close()


def test_bam_counts_with_zoom_levels():
    lengths = {"c0001": 1, "c2047": 2047, "c2049": 2049, "c4097": 4097, "quiet": 300}
    counts = {"c0001": {0: 3}, "c2047": {0: 1, 1: 1, 2: 10, 1000: 99, 1001: 100, 2045: 7, 2046: 7}, "c2049": {**{p: 4 for p in range(2046, 2049)}, 3: 1000, 510: 1, 511: 1},
              "c4097": {**{p: 6 for p in range(2040, 2060)}, **{p: 2 for p in range(4090, 4097)}, 0: 12, 4095: 8, 4096: 8}}
    reads = cc.designed_packed(pa, lengths, counts, reverse=("c2049",))
    bga = pa.BAMGenomeArray(reads, mapping=pa.FivePrimeMapFactory(0))
    for strand in ("+", "-"):
        vectors = {c: bga.get(pa.GenomicSegment(c, 0, int(n), strand), roi_order=False) for c, n in bga.lengths().items()}
        host = DenseGenomeArray(bga.lengths(), (strand,))
        for c, v in vectors.items():
            host._chroms[c][strand] = np.asarray(v, np.float64)
        for kw in (dict(zoom=True), dict(zoom=8, items_per_slot=2, block_size=2, compress="dynamic"), dict(zoom=True, compress=False, _batch_elems=3000)):
            hkw = {k: v for k, v in kw.items() if k != "_batch_elems"}
            want, stats = host_file(host, strand, **hkw)
            fh = io.BytesIO()
            bga.to_bigwig(fh, strand, **kw)
            assert fh.getvalue() == want
            assert bga.bigwig_export_zoom_stats() == stats["zoom"] and len(stats["zoom"]) >= 1
            assert bga.bigwig_export_stats() == {k: v for k, v in stats.items() if k != "zoom"}
    fh = io.BytesIO()
    bga.to_bigwig(fh, "+")
    assert bga.bigwig_export_zoom_stats() == [] and pa.bigwig_zoom_info(fh.getvalue()) == []
    # to_genome_array stops one position short of every contig's end, as the reference does: with no count on a last
    # position its host copy gives the same file
    inner = {c: {p: v for p, v in per.items() if p < lengths[c] - 1} for c, per in counts.items() if c != "c0001"}
    bga = pa.BAMGenomeArray(cc.designed_packed(pa, lengths, inner, reverse=("c2049",)), mapping=pa.FivePrimeMapFactory(0))
    dev = bga.to_genome_array(pa.GenomeArray)
    try:
        host = dev.to_host()
    finally:
        dev.close()
    for strand in ("+", "-"):
        want, stats = host_file(host, strand, zoom=True)
        fh = io.BytesIO()
        bga.to_bigwig(fh, strand, zoom=True)
        assert fh.getvalue() == want and bga.bigwig_export_zoom_stats() == stats["zoom"] and stats["items"] > 0


def test_refusals_write_nothing(arrays):
    ga, _ = arrays("grid8_d_plus1")
    for bad in (7, 2 ** 24 + 1, 0, -1, 1.5, "auto", None):
        fh = io.BytesIO()
        with pytest.raises(ValueError, match="zoom"):
            ga.to_bigwig(fh, "+", zoom=bad)
        assert fh.getvalue() == b""
    # the library's own refusal, under the Python check
    n = track.ctypes.c_int64(0)
    for bad in (7, -2, 2 ** 24 + 1, 1):
        assert ga._lib.pc_track_export_bigwig_zoom(ga._h, 0, 1024, 256, 1, bad, track.ctypes.byref(n)) == -1
    assert ga._lib.pc_track_export_bigwig_read(ga._h, None, 0) == -1            # nothing waits
    assert len(pa.bigwig_zoom_info(device_file(ga, zoom=2 ** 24))) == 1
