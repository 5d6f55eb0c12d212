"""GenomeArray.to_bigwig and BAMGenomeArray.to_bigwig -- the kernels of csrc/bigwig_write_kernels.hip.h (item heads, items,
section headers, total summary), k_zlib_deflate over the sections and the host layout of csrc/bigwig_writer.hip.h --
against the serial host writer (plastid_amd.write_bigwig, tested on the CPU by test_bigwig_write_host.py): for every
array of tests/bigwig_write_cases.py, items_per_slot in {1, 2, 1024}, block_size in {2, 256} and both compress settings the
device's file is the host writer's over ``to_host()``, byte for byte (the summary's two sums within the reordering bound
where the values are not integers); a written file read back by BigWigReader gives the cast array; a file imported and
written again gives the same bytes; the statistics are the model's; the counts of a BAMGenomeArray, both strands, raw and
normalised, in several batches; a stratified rule and bad parameters are refused and nothing is written; and one export
with PC_STAGE_SLICE small, so that the blocks come back through the transfer ring in pieces."""
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
from plastid_amd import synth, track  # noqa: E402
from plastid_amd.engine import Engine  # noqa: E402
from plastid_amd.genome_array import DenseGenomeArray  # noqa: E402
from tests import bigwig_write_cases as wc  # noqa: E402
from tests import count_export_cases as cc  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = wc.array_cases()
GRID = [(ips, bs, comp) for ips in (1, 2, 1024) for bs in (2, 256) for comp in (True, False)]


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
            case = CASES[name]
            ga = pa.GenomeArray(collections.OrderedDict((k, v.length + 1) for k, v in case.items()), engine=eng)
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
    stats = pa.write_bigwig(host, fh, strand, **kw)
    return fh.getvalue(), stats


def assert_same_file(got, want, integers, nitems):
    """Byte for byte; where the values are not integers the summary's two sums (bytes 88 .. 104) by the reordering bound."""
    assert len(got) == len(want)
    if integers or not nitems:
        assert got == want
        return
    assert got[:88] == want[:88] and got[104:] == want[104:]
    items = pa.read_bigwig(want)
    w = (items.stop - items.start).astype(np.float64)
    for at, terms in ((88, items.value * w), (96, items.value * items.value * w)):
        a, b = struct.unpack("<d", got[at:at + 8])[0], struct.unpack("<d", want[at:at + 8])[0]
        if b != b or math.isinf(b):
            assert (a != a and b != b) or a == b
        else:
            assert abs(a - b) <= 2 * nitems * 2.0 ** -53 * float(np.abs(terms).sum())


def test_the_geometry_the_cases_were_cut_for():
    assert track._export_geometry()[0] == wc.EXPORT_TILE


@pytest.mark.parametrize("name", list(CASES))
def test_device_file_is_the_host_writers(arrays, name):
    ga, host = arrays(name)
    case = CASES[name]
    exp = wc.expected_file_items(case)
    for ips, bs, comp in GRID:
        kw = dict(items_per_slot=ips, block_size=bs, compress=comp)
        want, stats = host_file(host, **kw)
        got = device_file(ga, **kw)
        assert_same_file(got, want, wc.is_integer_case(case), len(exp))
        assert ga.bigwig_export_stats() == stats, (ips, bs, comp)
        assert set(ga.bigwig_export_timing()) == {"runs_items", "sections_summary", "deflate_adler", "sizes_compaction", "read_back", "host_layout"}
    # the file holds the case: the items as the cases module computes them
    t = pa.read_bigwig(got)
    assert [(a, b, c) for a, b, c, _ in t.tuples()] == [(k, a, b) for k, a, b, _ in exp]
    assert all((g != g and e != e) or g == float(e) for g, e in zip(t.value, (f for _, _, _, f in exp)))
    # the other strand is another file
    assert len(pa.read_bigwig(device_file(ga, "-"))) == sum(1 for v in case.values() if len(v.cells))


@pytest.mark.parametrize("name", ["integers", "mixed"])
def test_round_trips(arrays, eng, tmp_path, name):
    ga, host = arrays(name)
    p = tmp_path / "written.bw"
    ga.to_bigwig(str(p), "+", items_per_slot=2, block_size=2)
    reader = pa.BigWigReader(str(p), engine=eng)
    try:
        for k, n in host.lengths().items():
            with np.errstate(over="ignore"):
                want = host._chroms[k]["+"].astype(np.float32).astype(np.float64)
            assert reader.chroms[k] == n and np.array_equal(reader.get_chromosome_counts(k), want, equal_nan=True)
        if name == "integers":
            # imported and written again: the same bytes (float32 values survive the trip; the sizes are the file's)
            again = device_file(reader._ga, ".", items_per_slot=2, block_size=2)
            assert again == p.read_bytes()
            again = device_file(reader._ga, ".")
            assert again == device_file(ga)
    finally:
        reader.close()


def test_file_sizes_and_cells_beyond_the_length(eng, tmp_path):
    """A file the host writer wrote -- a contig whose last cell is set, one stored beyond its reported length -- imported
    (contigs at the file's sizes, no growth) and written by the device: the same bytes."""
    case = CASES["integers"]
    want, _ = host_file(wc.host_array(case), items_per_slot=1024)
    p = tmp_path / "host.bw"
    p.write_bytes(want)
    reader = pa.BigWigReader(str(p), engine=eng)
    try:
        assert reader.chroms["beyond"] == 150 and reader.chroms["chrM_long_name"] == 1000
        assert device_file(reader._ga, ".") == want
    finally:
        reader.close()


def test_blocks_through_the_transfer_ring(arrays, monkeypatch):
    ga, host = arrays("integers")
    want, _ = host_file(host, items_per_slot=64)
    monkeypatch.setenv("PC_STAGE_SLICE", "1")            # pieces of one 4 KiB page
    assert len(want) > 5 * 4096 and device_file(ga, items_per_slot=64) == want
    stored, _ = host_file(host, items_per_slot=64, compress=False)
    assert device_file(ga, items_per_slot=64, compress=False) == stored


def test_stored_sections_are_counted(eng):
    """Sections of random values do not shrink: they fall back to the stored block, and the statistics say so."""
    rng = np.random.default_rng(5)
    at = np.cumsum(rng.integers(2, 40, 3000))                   # single cells, random gaps, random values: literals only
    cells = np.zeros(int(at[-1]) + 1)
    cells[at] = rng.random(3000) * 1e6 + 1.0
    ga = pa.GenomeArray({"r": 200000, "z": 3000}, engine=eng)
    ga[pa.GenomicSegment("r", 0, len(cells), "+")] = cells
    ga[pa.GenomicSegment("z", 0, 2000, "+")] = np.tile([1.0, 2.0], 1000)
    want, stats = host_file(ga.to_host())
    got = device_file(ga)
    assert_same_file(got, want, False, 5000)
    assert ga.bigwig_export_stats() == stats and 1 <= stats["stored_sections"] < stats["sections"]
    ga.close()


def test_refusals_write_nothing(arrays, tmp_path):
    ga, _ = arrays("singles")
    with open(tmp_path / "text.bw", "w") as fh:
        with pytest.raises(TypeError, match="binary"):
            ga.to_bigwig(fh, "+")
    assert os.path.getsize(tmp_path / "text.bw") == 0
    for bad in (dict(items_per_slot=0), dict(items_per_slot=2049), dict(block_size=1), dict(block_size=65536)):
        fh = io.BytesIO()
        with pytest.raises(ValueError, match="outside"):
            ga.to_bigwig(fh, "+", **bad)
        assert fh.getvalue() == b""
    # the library's own refusal, under the Python check
    n = track.ctypes.c_int64(0)
    assert ga._lib.pc_track_export_bigwig(ga._h, 0, 0, 256, 1, track.ctypes.byref(n)) == -1
    assert ga._lib.pc_track_export_bigwig(ga._h, 0, 1024, 1, 1, track.ctypes.byref(n)) == -1
    assert ga._lib.pc_track_export_bigwig(ga._h, 2, 1024, 256, 1, track.ctypes.byref(n)) == -1
    assert ga._lib.pc_track_export_bigwig_read(ga._h, None, 0) == -1            # nothing waits
    assert len(pa.read_bigwig(device_file(ga))) == 3000


# ------------------------------------------------------------------ BAMGenomeArray
SEAM_LENGTHS = {"c0001": 1, "c2047": 2047, "c2048": 2048, "c2049": 2049, "c4097": 4097, "quiet": 300}


def _seam_counts():
    """The small case of tests/test_gpu_count_export.py: runs over the borders of 2048 export elements, at position 0 and
    at the last position of a contig."""
    counts = {"c0001": {0: 3}}
    counts["c2047"] = {0: 1, 1: 1, 2: 10, 1000: 99, 1001: 100, 2045: 7, 2046: 7}
    counts["c2048"] = {**{p: 5 for p in range(2040, 2048)}, 0: 9, 254: 2, 255: 2, 256: 2, 257: 3}
    counts["c2049"] = {**{p: 4 for p in range(2046, 2049)}, 3: 1000, 510: 1, 511: 1}
    counts["c4097"] = {**{p: 6 for p in range(2040, 2060)}, **{p: 2 for p in range(4090, 4097)}}
    counts["c4097"].update({0: 12, 2047: 6, 2048: 6, 4095: 8, 4096: 8})
    return counts


@pytest.mark.parametrize("rule", ["fiveprime", "threeprime-norm"])
def test_bam_counts_as_bigwig(rule):
    reads = cc.designed_packed(pa, SEAM_LENGTHS, _seam_counts(), reverse=("c2049",))
    mapping = {"fiveprime": pa.FivePrimeMapFactory(0), "threeprime-norm": pa.ThreePrimeMapFactory(0)}[rule]
    bga = pa.BAMGenomeArray(reads, mapping=mapping)
    bga.set_normalize(rule == "threeprime-norm")
    for strand in ("+", "-"):
        vectors = {c: bga.get(pa.GenomicSegment(c, 0, int(n), strand), roi_order=False) for c, n in bga.lengths().items()}
        host = DenseGenomeArray(bga.lengths(), (strand,))
        for c, v in vectors.items():
            host._chroms[c][strand] = np.asarray(v, np.float64)
        for kw in (dict(), dict(items_per_slot=2, block_size=2), dict(compress=False, _batch_elems=3000)):
            hkw = {k: v for k, v in kw.items() if k != "_batch_elems"}
            want, stats = host_file(host, strand, **hkw)
            fh = io.BytesIO()
            bga.to_bigwig(fh, strand, **kw)
            assert_same_file(fh.getvalue(), want, rule == "fiveprime", stats["items"])
            assert bga.bigwig_export_stats() == stats and stats["items"] > 0
        if rule == "fiveprime" and strand == "+":
            items = pa.read_bigwig(want).tuples()
            assert ("c4097", 2040, 2060, 6.0) in items and ("c2048", 2040, 2048, 5.0) in items      # no window cuts a run
            assert ("c0001", 0, 1, 3.0) in items and ("c4097", 4095, 4097, 8.0) in items
    # a stratified rule: TypeError, nothing written
    bga.set_mapping(pa.StratifiedVariableFivePrimeMapFactory(synth.VARIABLE_OFFSETS, 25, 35))
    fh = io.BytesIO()
    with pytest.raises(TypeError):
        bga.to_bigwig(fh, "+")
    assert fh.getvalue() == b""
