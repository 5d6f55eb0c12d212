"""plastid_amd.write_bigwig with compress="dynamic" -- the serial writer of csrc/bigwig_write_host.h over the model encoder's
dynamic codes (csrc/deflate_host.h) -- on the CPU, over the arrays of tests/bigwig_write_cases.py with items_per_slot in
{1, 1024, 2048}: read_bigwig gives the array cast to float32; the block table and uncompressBufSize say what the fixed file
says, block for block never larger; every block inflates to the stored file's; compress=True and compress="fixed" are the
same bytes; the block types add up; a bad compress value is refused.  No GPU needed."""
import io
import os
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import plastid_amd as pa  # noqa: E402
from plastid_amd import track  # noqa: E402
from tests import bigwig_write_cases as wc  # noqa: E402
from tests import deflate_dynamic_cases as dc  # noqa: E402

CASES = wc.array_cases()


def write(case, ips, comp, bs=256, strand="+", **kw):
    fh = io.BytesIO()
    stats = pa.write_bigwig(wc.host_array(case, strand), fh, strand, items_per_slot=ips, block_size=bs, compress=comp, **kw)
    return fh.getvalue(), stats


@pytest.mark.parametrize("ips", [1, 1024, 2048])
@pytest.mark.parametrize("name", list(CASES))
def test_the_dynamic_file_holds_the_array(name, ips):
    case = CASES[name]
    image, stats = write(case, ips, "dynamic", block_types=True)
    fixed, fixed_stats = write(case, ips, "fixed", block_types=True)
    stored, _ = write(case, ips, False)
    # the array, cast to float32
    t = pa.read_bigwig(image)
    for k in sorted(case):
        with np.errstate(over="ignore"):
            want = np.zeros(wc.contig_size(case[k]), np.float64)
            want[:len(case[k].cells)] = case[k].cells.astype(np.float32)
        assert np.array_equal(t.chromosome_counts(k), want, equal_nan=True)
    f = pa.read_bigwig(fixed)
    assert [x[:3] for x in t.tuples()] == [x[:3] for x in f.tuples()] and np.array_equal(t.value, f.value, equal_nan=True)
    # the shape of the file: as the fixed file, block for block never larger
    info, finfo, sinfo = track.bigwig_info(image), track.bigwig_info(fixed), track.bigwig_info(stored)
    assert info["chroms"] == finfo["chroms"] and info["uncompress_buf_size"] == finfo["uncompress_buf_size"] and info["version"] == finfo["version"]
    assert len(info["blocks"]) == len(finfo["blocks"]) == stats["sections"]
    assert all(n <= fn for (_, n), (_, fn) in zip(info["blocks"], finfo["blocks"]))
    assert len(image) <= len(fixed) and len(image) - len(fixed) == stats["block_bytes"] - fixed_stats["block_bytes"]
    assert wc.file_summary(image)[0] == wc.file_summary(fixed)[0] and image[64:104] == fixed[64:104]      # the total summary, bit for bit
    # every block: the stored file's section; a dynamic block where it is smaller, else the fixed file's block
    types = [0, 0, 0]
    for (a, n), (fa, fn), (sa, sn) in zip(info["blocks"], finfo["blocks"], sinfo["blocks"]):
        block = image[a:a + n]
        assert zlib.decompress(block) == stored[sa:sa + sn]
        btype = (block[2] >> 1) & 3
        types[btype] += 1
        assert n < fn if btype == 2 else block == fixed[fa:fa + fn]
    assert types == [stats["stored_sections"], stats["fixed_sections"], stats["dynamic_sections"]] and sum(types) == stats["sections"]
    assert fixed_stats["dynamic_sections"] == 0 and fixed_stats["stored_sections"] + fixed_stats["fixed_sections"] == stats["sections"]
    assert {k: v for k, v in stats.items() if k not in ("block_bytes", "stored_sections", "fixed_sections", "dynamic_sections")} == \
        {k: v for k, v in fixed_stats.items() if k not in ("block_bytes", "stored_sections", "fixed_sections", "dynamic_sections")}


def test_sections_of_counts_take_the_dynamic_block():
    """Sections of 1 024 and 2 048 items of small counts: the dynamic block wins, its tokens read back to the section."""
    case = CASES["singles"]                                    # 3 000 items
    for ips in (1024, 2048):
        image, stats = write(case, ips, "dynamic", block_types=True)
        fixed, fixed_stats = write(case, ips, True)
        stored, _ = write(case, ips, False)
        assert stats["dynamic_sections"] == stats["sections"] == (3000 + ips - 1) // ips
        assert stats["block_bytes"] < 0.80 * fixed_stats["block_bytes"]
        for (a, n), (sa, sn) in zip(track.bigwig_info(image)["blocks"], track.bigwig_info(stored)["blocks"]):
            btype, tokens, tables = dc.block_tokens(image[a:a + n])
            assert btype == 2 and wc.replay(tokens) == stored[sa:sa + sn]


@pytest.mark.parametrize("ips", [1, 1024])
def test_true_and_fixed_are_the_same_bytes(ips):
    case = CASES["mixed"]
    a, sa = write(case, ips, True)
    b, sb = write(case, ips, "fixed")
    c, sc = write(case, ips, 1)
    assert a == b == c and sa == sb == sc and set(sa) == set(track.BIGWIG_WRITE_STATS)
    off, _ = write(case, ips, False, block_types=True)
    assert off == write(case, ips, 0)[0] and write(case, ips, False, block_types=True)[1]["fixed_sections"] == 0


def test_a_bad_compress_value_is_refused():
    case = CASES["chr10"]
    for bad in ("gzip", "Dynamic", 2, 3, -1, 1.5, b"fixed"):
        fh = io.BytesIO()
        with pytest.raises(ValueError, match="compress"):
            pa.write_bigwig(wc.host_array(case), fh, "+", compress=bad)
        assert fh.getvalue() == b""
    # the library's own refusal, under the Python check
    from plastid_amd.bam import _load
    L = _load()
    for bad in (3, -1):
        assert not L.pb_bigwig_write_open(1024, 256, bad) and b"compress" in L.pb_last_error()
    h = L.pb_bigwig_write_open(1024, 256, 2)
    assert h
    L.pb_bigwig_write_close(h)
