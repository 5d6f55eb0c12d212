"""plastid_amd.write_bigwig -- the serial bigWig WRITER of csrc/bigwig_write_host.h (the item walk, the model encoder of
csrc/deflate_host.h, the container code the device export shares) -- on the CPU, over the arrays of
tests/bigwig_write_cases.py, with items_per_slot in {1, 2, 1024}, block_size in {2, 256} (R-trees of one level and of many)
and both compress settings: read_bigwig gives exactly the expected items, chromosome_counts the array cast to float32,
bigwig_info the contigs and sizes; a reader of the tests' own (tests/bigwig_writer.py: struct + zlib) reads the same;
every block inflates with zlib to the block of the uncompressed file; the total summary (validCount, min, max exact; the
two sums exact for integer arrays, within the reordering bound otherwise); what is refused.  No GPU needed."""
import io
import math
import os
import struct
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import plastid_amd as pa  # noqa: E402
from plastid_amd import track  # noqa: E402
from tests import bigwig_write_cases as wc  # noqa: E402
from tests import bigwig_writer as bw  # noqa: E402

CASES = wc.array_cases()
GRID = [(ips, bs, comp) for ips in (1, 2, 1024) for bs in (2, 256) for comp in (True, False)]


def write(case, ips, bs, comp, strand="+"):
    fh = io.BytesIO()
    stats = pa.write_bigwig(wc.host_array(case, strand), fh, strand, items_per_slot=ips, block_size=bs, compress=comp)
    return fh.getvalue(), stats


def same_value(a, b):
    return (a != a and b != b) or (a == b and math.copysign(1.0, a) == math.copysign(1.0, b))


def check_summary(image, case):
    """validCount, min and max exact; the sums exact for integers, else within 2 n 2^-53 sum|term|."""
    exp = wc.expected_summary(case)
    got = wc.file_summary(image)
    if exp["n"] == 0:
        assert got == (0,)
        return
    off, valid, mn, mx, s, ss = got
    assert off == 64 and valid == exp["valid"]
    if exp["min"] is None:
        assert mn != mn and mx != mx
    else:
        assert (mn, mx) == (exp["min"], exp["max"])
    for have, terms in ((s, exp["sum_terms"]), (ss, exp["sq_terms"])):
        if any(t != t for t in terms):
            assert have != have
        elif any(math.isinf(t) for t in terms):
            want = sum(terms)                                     # (+-inf or, with both signs, NaN)
            assert (have != have and want != want) or have == want
        elif wc.is_integer_case(case):
            assert have == math.fsum(terms)
        else:
            assert abs(have - math.fsum(terms)) <= 2 * exp["n"] * 2.0 ** -53 * math.fsum(abs(t) for t in terms)


@pytest.mark.parametrize("ips,bs,comp", GRID)
@pytest.mark.parametrize("name", list(CASES))
def test_the_file_holds_the_array(name, ips, bs, comp):
    case = CASES[name]
    image, stats = write(case, ips, bs, comp)
    exp = wc.expected_file_items(case)
    # the project's reader
    t = pa.read_bigwig(image)
    got = t.tuples()
    assert len(got) == len(exp)
    assert all(g[:3] == e[:3] and same_value(g[3], float(e[3])) for g, e in zip(got, exp))
    sizes = [(k, wc.contig_size(case[k])) for k in sorted(case)]
    assert list(zip(t.names, t.lengths)) == sizes and list(track.bigwig_info(image)["chroms"].items()) == sizes
    for k in sorted(case):
        with np.errstate(over="ignore"):
            want = np.zeros(wc.contig_size(case[k]), np.float64)
            want[:len(case[k].cells)] = case[k].cells.astype(np.float32)
        assert np.array_equal(t.chromosome_counts(k), want, equal_nan=True)
    # the tests' own reader, and the shape of the file
    chroms, blocks, items = bw.read_model(image)
    assert [(n, i, s) for n, i, s in chroms] == [(k, i, s) for i, (k, s) in enumerate(sizes)]
    assert len(items) == len(exp) and all(i[1:3] == e[1:3] and chroms[i[0]][0] == e[0] for i, e in zip(items, exp))
    per_contig = [len(wc.expected_items(case[k].cells)) for k in sorted(case)]
    nsec = sum((n + ips - 1) // ips for n in per_contig)
    assert len(blocks) == nsec and stats == {"contigs": len(case), "items": len(exp), "sections": nsec, "raw_bytes": 24 * nsec + 12 * len(exp),
                                             "block_bytes": sum(b[1] for b in blocks), "stored_sections": stats["stored_sections"]}
    magic, version, zooms, ct, data, index, fc, dfc, aso, tso, buf, ext = struct.unpack("<IHHQQQHHQQIQ", image[:64])
    assert (magic, version, zooms, fc, dfc, aso, ext) == (0x888FFC26, 4, 0, 0, 0, 0, 0) and image[-4:] == image[:4]
    assert ct == (104 if exp else 64) and tso == (64 if exp else 0)
    assert struct.unpack("<Q", image[data:data + 8])[0] == nsec and [b[0] for b in blocks][:1] == ([data + 8] if nsec else [])
    assert all(a[0] + a[1] == b[0] for a, b in zip(blocks, blocks[1:])) and (not blocks or blocks[-1][0] + blocks[-1][1] == index)
    assert buf == (max([24 + 12 * min(ips, n) for n in per_contig if n] or [0]) if comp else 0)
    assert struct.unpack("<I", image[ct + 4:ct + 8])[0] == min(bs, len(case))       # the chromosome tree's fan-out
    check_summary(image, case)


@pytest.mark.parametrize("ips,bs", [(1, 2), (2, 256), (1024, 256)])
@pytest.mark.parametrize("name", ["mixed", "singles", "runs1025"])
def test_blocks_inflate_to_the_stored_file(name, ips, bs):
    packed, st = write(CASES[name], ips, bs, True)
    stored, _ = write(CASES[name], ips, bs, False)
    a, b = bw.read_model(packed)[1], bw.read_model(stored)[1]
    assert len(a) == len(b)
    for (ao, an), (bo, bn) in zip(a, b):
        assert zlib.decompress(packed[ao:ao + an]) == stored[bo:bo + bn] and an <= bn + 11
    assert st["block_bytes"] == sum(n for _, n in a)
    if ips == 1024:
        assert st["block_bytes"] < 0.8 * st["raw_bytes"]
    # the R-tree: one level for block_size 256 over few sections, four or more for block_size 2
    index = struct.unpack("<Q", packed[24:32])[0]
    depth, at = 1, index + 48
    while packed[at] == 0:
        at = struct.unpack("<Q", packed[at + 4 + 16:at + 4 + 24])[0]
        depth += 1
    assert depth >= 4 if bs == 2 and len(a) >= 9 else depth == 1 or len(a) > bs


def test_the_strand_is_the_one_asked_for_and_a_path_is_written(tmp_path):
    case = CASES["integers"]
    ga = wc.host_array(case, "-")
    p = tmp_path / "minus.bw"
    pa.write_bigwig(ga, str(p), "-")
    assert p.read_bytes() == write(case, 1024, 256, True, strand="-")[0]
    pa.write_bigwig(ga, p, "+")
    decoy = pa.read_bigwig(p.read_bytes())
    assert all(v == 5.0 for v in decoy.value) and len(decoy) == len(case)


def test_refusals(tmp_path):
    ga = wc.host_array(CASES["singles"])
    with open(tmp_path / "text.bw", "w") as fh:
        with pytest.raises(TypeError, match="binary"):
            pa.write_bigwig(ga, fh, "+")
    with pytest.raises(TypeError, match="binary"):
        pa.write_bigwig(ga, io.StringIO(), "+")
    assert os.path.getsize(tmp_path / "text.bw") == 0
    for bad in (dict(items_per_slot=0), dict(items_per_slot=2049), dict(block_size=1), dict(block_size=65536)):
        fh = io.BytesIO()
        with pytest.raises(ValueError, match="outside"):
            pa.write_bigwig(ga, fh, "+", **bad)
        assert fh.getvalue() == b""
    for ok in (dict(items_per_slot=2048), dict(block_size=65535)):
        fh = io.BytesIO()
        pa.write_bigwig(ga, fh, "+", **ok)
        assert len(pa.read_bigwig(fh.getvalue())) == 3000


# ------------------------------------------------------------------ Kent's library (tests/golden/bigwig_write_fixture.npz)
@pytest.fixture(scope="module")
def fx():
    return wc.load_fixture()


@pytest.mark.parametrize("name,ips,bs,comp", wc.KENT_READS)
def test_kent_reads_our_files_as_the_cast_arrays(fx, name, ips, bs, comp):
    """What bbiChromList and bigWigValsOnChromFetchData gave for the file write_bigwig wrote when the fixture was made:
    the contigs with their ids and sizes, and, run by run, the arrays cast to float32."""
    case, k = CASES[name], "read_" + wc.key(name, ips, bs, comp)
    chroms = [str(c) for c in fx[k + "_chroms"]]
    assert list(zip(chroms, fx[k + "_ids"], fx[k + "_sizes"])) == [(c, i, wc.contig_size(case[c])) for i, c in enumerate(sorted(case))]
    arrays = {c: np.zeros(wc.contig_size(case[c])) for c in case}
    for (ci, a, b), v in zip(fx[k + "_runs"], fx[k + "_run_values"]):
        arrays[chroms[ci]][a:b] = v
    for c in case:
        want = np.zeros(wc.contig_size(case[c]))
        want[:len(case[c].cells)] = case[c].cells.astype(np.float32)
        assert np.array_equal(arrays[c], want)


@pytest.mark.parametrize("name,ips", wc.KENT_WRITES)
def test_our_data_region_is_kents(fx, name, ips):
    """Kent's bigWigFileCreate over OUR items as bedGraph text, uncompressed, the same items per slot: the section count and
    the sections, byte for byte."""
    assert wc.data_region(write(CASES[name], ips, 256, False)[0]) == fx["kent_" + wc.key(name, ips) + "_data"].tobytes()


@pytest.mark.parametrize("name,ips,bs,comp", wc.RECORDED)
def test_write_bigwig_still_writes_the_recorded_bytes(fx, name, ips, bs, comp):
    assert write(CASES[name], ips, bs, comp)[0] == fx["ours_" + wc.key(name, ips, bs, comp)].tobytes()
