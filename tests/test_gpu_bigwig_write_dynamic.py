"""GenomeArray.to_bigwig and BAMGenomeArray.to_bigwig with compress="dynamic" -- the sections through the dynamic
instantiation of k_zlib_deflate -- against the serial host writer (plastid_amd.write_bigwig(compress="dynamic"), tested on
the CPU by test_bigwig_write_dynamic_host.py): for the arrays of tests/bigwig_write_cases.py and items_per_slot in
{1, 1024, 2048} the device's file is the host writer's, byte for byte (the summary's two sums within the reordering bound
where the values are not integers); the file read back by BigWigReader on the GPU gives the array cast to float32; the
block types of the statistics add up to the sections and are the model's; compress=True and "fixed" stay the same bytes;
the counts of a BAMGenomeArray; a bad compress value is refused and nothing is written."""
import collections
import io
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import plastid_amd as pa  # noqa: E402
from plastid_amd import track  # noqa: E402
from plastid_amd.engine import Engine  # noqa: E402
from plastid_amd.genome_array import DenseGenomeArray  # noqa: E402
from tests import bigwig_write_cases as wc  # noqa: E402
from tests import count_export_cases as cc  # noqa: E402
from tests.test_gpu_bigwig_write import SEAM_LENGTHS, _seam_counts, assert_same_file, device_file, host_file  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = wc.array_cases()


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def device_array(eng, case):
    ga = pa.GenomeArray(collections.OrderedDict((k, v.length + 1) for k, v in case.items()), engine=eng)
    for k, v in case.items():
        if len(v.cells):
            ga[pa.GenomicSegment(k, 0, len(v.cells), "+")] = v.cells
            ga[pa.GenomicSegment(k, 0, min(3, len(v.cells)), "-")] = 5.0
    return ga


@pytest.mark.parametrize("name", ["mixed", "integers", "singles", "runs1025", "long", "fractions", "empty"])
def test_device_file_is_the_host_writers(eng, name):
    case = CASES[name]
    ga = device_array(eng, case)
    try:
        host = ga.to_host()
        nitems = len(wc.expected_file_items(case))
        for ips in (1, 1024, 2048):
            kw = dict(items_per_slot=ips, compress="dynamic")
            want, stats = host_file(host, block_types=True, **kw)
            got = device_file(ga, **kw)
            assert_same_file(got, want, wc.is_integer_case(case), nitems)
            have = ga.bigwig_export_stats(block_types=True)
            assert have == stats, ips
            assert have["stored_sections"] + have["fixed_sections"] + have["dynamic_sections"] == have["sections"]
            assert ga.bigwig_export_stats() == {k: stats[k] for k in track.BIGWIG_WRITE_STATS}
            fixed = device_file(ga, items_per_slot=ips)
            assert len(got) <= len(fixed) and fixed == device_file(ga, items_per_slot=ips, compress="fixed")
            if name in ("singles", "long") and ips >= 1024:
                assert have["dynamic_sections"] == have["sections"] and len(got) < 0.85 * len(fixed)
    finally:
        ga.close()


@pytest.mark.parametrize("name", ["integers", "mixed"])
def test_the_file_read_back_on_the_gpu(eng, tmp_path, name):
    case = CASES[name]
    ga = device_array(eng, case)
    p = tmp_path / "dynamic.bw"
    try:
        ga.to_bigwig(str(p), "+", compress="dynamic")
        assert ga.bigwig_export_stats(block_types=True)["dynamic_sections"] > 0
        host = ga.to_host()
    finally:
        ga.close()
    reader = pa.BigWigReader(str(p), engine=eng)
    try:
        for k, n in host.lengths().items():
            with np.errstate(over="ignore"):
                want = host._chroms[k]["+"].astype(np.float32).astype(np.float64)
            assert reader.chroms[k] == n and np.array_equal(reader.get_chromosome_counts(k), want, equal_nan=True)
    finally:
        reader.close()


def test_bam_counts_as_bigwig(eng):
    """The smallest BAM case of tests/test_gpu_bigwig_write.py, five-prime counts."""
    reads = cc.designed_packed(pa, SEAM_LENGTHS, _seam_counts(), reverse=("c2049",))
    bga = pa.BAMGenomeArray(reads, mapping=pa.FivePrimeMapFactory(0))
    for strand in ("+", "-"):
        host = DenseGenomeArray(bga.lengths(), (strand,))
        for c, n in bga.lengths().items():
            host._chroms[c][strand] = np.asarray(bga.get(pa.GenomicSegment(c, 0, int(n), strand), roi_order=False), np.float64)
        for kw in (dict(), dict(items_per_slot=2, block_size=2)):
            want, stats = host_file(host, strand, compress="dynamic", block_types=True, **kw)
            fh = io.BytesIO()
            bga.to_bigwig(fh, strand, compress="dynamic", **kw)
            assert_same_file(fh.getvalue(), want, True, stats["items"])
            assert bga.bigwig_export_stats(block_types=True) == stats and stats["items"] > 0
            assert stats["stored_sections"] + stats["fixed_sections"] + stats["dynamic_sections"] == stats["sections"]
            assert set(bga.bigwig_export_stats()) == set(track.BIGWIG_WRITE_STATS)
    fh = io.BytesIO()
    with pytest.raises(ValueError, match="compress"):
        bga.to_bigwig(fh, "+", compress="best")
    assert fh.getvalue() == b""


def test_a_bad_compress_value_is_refused(eng):
    ga = device_array(eng, CASES["chr10"])
    try:
        for bad in ("gzip", 2, 3, -1):
            fh = io.BytesIO()
            with pytest.raises(ValueError, match="compress"):
                ga.to_bigwig(fh, "+", compress=bad)
            assert fh.getvalue() == b""
        n = track.ctypes.c_int64(0)
        assert ga._lib.pc_track_export_bigwig(ga._h, 0, 1024, 256, 3, track.ctypes.byref(n)) == -1
        assert ga._lib.pc_track_export_bigwig(ga._h, 0, 1024, 256, -1, track.ctypes.byref(n)) == -1
        assert len(pa.read_bigwig(device_file(ga, compress="dynamic"))) == 1
    finally:
        ga.close()
