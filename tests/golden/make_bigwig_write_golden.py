#!/usr/bin/env python
"""Generate ``tests/golden/bigwig_write_fixture.npz``: what Kent's bigWig library -- the one the reference links -- makes of
the files ``plastid_amd.write_bigwig`` writes, and what its own writer writes from our items.

    python tests/golden/make_bigwig_write_golden.py

needs the reference checkout (``KENT_SRC``); it reuses ``build_harness`` and ``read_back`` of ``make_bigwig_golden.py`` and the
harness ``oracle/_ref/bw_golden`` unchanged.  Only DATA is committed.

READ (``KENT_READS`` of tests/bigwig_write_cases.py: the cases with finite values): the file of ``write_bigwig`` goes through
``bbiChromList`` and ``bigWigValsOnChromFetchData``: ``read_<key>_chroms`` / ``_ids`` / ``_sizes`` / ``_runs`` (contig index,
start, end) / ``_run_values``.  WRITE (``KENT_WRITES``: cases where every contig holds an item, since Kent's writer drops the
others and numbers the rest): OUR item list as bedGraph text through ``bigWigFileCreate``, uncompressed, the same items per
slot: ``kent_<key>_data``, the bytes from unzoomedDataOffset to unzoomedIndexOffset.  RECORDED: ``ours_<key>``, the bytes
``write_bigwig`` wrote when the fixture was made.  The script asserts what the tests assert."""
import io
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, HERE]
from make_bigwig_golden import build_harness, contig_arrays, read_back  # noqa: E402


def ours(pa, wc, case, ips, bs, comp):
    fh = io.BytesIO()
    pa.write_bigwig(wc.host_array(case), fh, "+", items_per_slot=ips, block_size=bs, compress=comp)
    return fh.getvalue()


def main():
    import plastid_amd as pa
    from tests import bigwig_write_cases as wc
    exe = build_harness()
    cases = wc.array_cases()
    tmp = tempfile.mkdtemp(prefix="bww_golden_")
    out = dict(kent=np.array("kent/src/lib as vendored by the reference"))
    for name, ips, bs, comp in wc.KENT_READS:
        case, k = cases[name], wc.key(name, ips, bs, comp)
        path = os.path.join(tmp, k + ".bw")
        open(path, "wb").write(ours(pa, wc, case, ips, bs, comp))
        rb = read_back(exe, path)
        assert list(zip(rb["chroms"], rb["ids"], rb["sizes"])) == [(c, i, wc.contig_size(case[c])) for i, c in enumerate(sorted(case))], k
        arrays = contig_arrays(rb)
        for c in case:
            want = np.zeros(wc.contig_size(case[c]))
            want[:len(case[c].cells)] = case[c].cells.astype(np.float32)
            assert np.array_equal(arrays[c], want), (k, c)
        out["read_" + k + "_chroms"] = np.array(rb["chroms"])
        out["read_" + k + "_ids"] = np.array(rb["ids"], np.int32)
        out["read_" + k + "_sizes"] = np.array(rb["sizes"], np.int64)
        out["read_" + k + "_runs"] = np.array(rb["runs"], np.int32).reshape(-1, 3)
        out["read_" + k + "_run_values"] = np.array(rb["run_values"], np.float64)
    for name, ips in wc.KENT_WRITES:
        case, k = cases[name], wc.key(name, ips)
        bg, sizes, path = (os.path.join(tmp, k + e) for e in (".bedGraph", ".sizes", ".kent.bw"))
        open(bg, "w").write(wc.bedgraph_text(case))
        open(sizes, "w").write("".join("%s\t%d\n" % (c, wc.contig_size(case[c])) for c in sorted(case)))
        subprocess.check_call([exe, "write", bg, sizes, "256", str(ips), "0", path])
        kent = wc.data_region(open(path, "rb").read())
        assert kent == wc.data_region(ours(pa, wc, case, ips, 256, False)), k
        out["kent_" + k + "_data"] = np.frombuffer(kent, np.uint8)
    for name, ips, bs, comp in wc.RECORDED:
        out["ours_" + wc.key(name, ips, bs, comp)] = np.frombuffer(ours(pa, wc, cases[name], ips, bs, comp), np.uint8)
    dst = os.path.join(HERE, "bigwig_write_fixture.npz")
    np.savez_compressed(dst, **out)
    print("%s: %d keys, %d bytes" % (dst, len(out), os.path.getsize(dst)))
    assert os.path.getsize(dst) <= 512 * 1024


if __name__ == "__main__":
    main()
