#!/usr/bin/env python
"""Generate ``tests/golden/bigwig_zoom_fixture.npz``: what the SUMMARY reader of Kent's bigWig library -- the one the
reference links -- returns for the files ``plastid_amd.write_bigwig(zoom=...)`` writes.

    python tests/golden/make_bigwig_zoom_golden.py

needs the reference checkout (``KENT_SRC``); it reuses ``build_harness`` (the library ``oracle/_ref/libkent_bw.a`` and the
harness ``oracle/_ref/bw_golden``) and ``read_back`` of ``make_bigwig_golden.py`` and compiles ``bw_zoom_golden.c`` beside
them into ``oracle/_ref/bw_zoom_golden``.  Only DATA is committed.

For the integer cases of tests/bigwig_zoom_cases.py, compressed and stored (``<tag>`` = ``<case>_<1|0>``):
``crc_<tag>``: the CRC-32 of the file the summaries were taken from.  ``sum_<tag>_<level>_<contig>_<type>``:
``bigWigSummaryArray`` over ``[0, 2 r_k nb)`` in ``nb = size // (2 r_k) >= 1`` bins for mean, min, max, coverage and std:
``bbiBestZoom`` picks level k for that query and every bin is two whole windows, so every value is exactly what the
cells give -- asserted here and again by tests/test_bigwig_zoom_host.py.  ``read_<case>_zoom_*``: ``read_back`` over the
zoomed, compressed file; ``twins_<case>``: whether ``read_back`` gave those very arrays for the zoomed and the
``zoom=False`` file, compressed and stored (asserted: all four).  ``unaligned_*``: one query whose bins cut windows,
recorded and not asserted (Kent scales a cut window's sums by the overlap)."""
import io
import os
import subprocess
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, HERE]
import make_bigwig_golden as mg  # noqa: E402

KINDS = ("mean", "min", "max", "coverage", "std")


def build_zoom_harness():
    mg.build_harness()
    ref = os.path.join(ROOT, "oracle", "_ref")
    flags = ["-O1", "-w", "-std=gnu99", "-D_FILE_OFFSET_BITS=64", "-D_LARGEFILE_SOURCE", "-D_GNU_SOURCE", "-DMACHTYPE_x86_64",
             "-I", os.path.join(mg.KENT, "inc"), "-I", os.path.join(mg.KENT, "htslib")]
    exe = os.path.join(ref, "bw_zoom_golden")
    subprocess.check_call(["gcc"] + flags + [os.path.join(HERE, "bw_zoom_golden.c"), os.path.join(ref, "libkent_bw.a"), os.path.join(ref, "libhts_ref.a"),
                                             "-lssl", "-lcrypto", "-lz", "-lm", "-lpthread", "-o", exe])
    return exe, os.path.join(ref, "bw_golden")


def summaries(exe, path, chrom, start, end, bins):
    """``(reductions of the file's levels, {type: values})`` of one query."""
    out, levels = {}, None
    for line in subprocess.check_output([exe, path, chrom, str(start), str(end), str(bins)]).decode().splitlines():
        f = line.split()
        if f[0] == "LEVELS":
            levels = [int(x) for x in f[2:]]
        else:
            out[f[0]] = np.array([float(x) for x in f[1:]], np.float64)
    return levels, out


def main():
    import tempfile
    import plastid_amd as pa
    from tests import bigwig_zoom_cases as zc
    from tests import test_bigwig_zoom_host as th
    exe, reader = build_zoom_harness()
    cases = zc.cases()
    tmp = tempfile.mkdtemp(prefix="bwz_golden_")
    out = dict(kent=np.array("kent/src/lib as vendored by the reference"))
    asserted = 0
    for name in zc.integer_cases():
        case = cases[name]
        want = zc.expected_zoom(case)
        first, same = None, []
        for comp in (True, False):
            tag = "%s_%d" % (name, 1 if comp else 0)
            paths = {}
            for kind, zoom in (("zoom", case.zoom), ("plain", False)):
                fh = io.BytesIO()
                pa.write_bigwig(zc.host_array(case), fh, "+", compress=comp, zoom=zoom)
                paths[kind] = os.path.join(tmp, "%s_%s.bw" % (tag, kind))
                open(paths[kind], "wb").write(fh.getvalue())
                if kind == "zoom":
                    out["crc_" + tag] = np.array(zlib.crc32(fh.getvalue()), np.int64)
                rb = mg.read_back(reader, paths[kind])
                rb = dict(chroms=np.array(rb["chroms"]), ids=np.array(rb["ids"], np.int32), sizes=np.array(rb["sizes"], np.int64),
                          runs=np.array(rb["runs"], np.int32).reshape(-1, 3), run_values=np.array(rb["run_values"], np.float64))
                if first is None:
                    first = rb
                    for part, v in rb.items():
                        out["read_%s_zoom_%s" % (name, part)] = v
                same.append(all(np.array_equal(first[part], v) for part, v in rb.items()))
            for k, lv in enumerate(want):
                for ci, c in enumerate(sorted(case.contigs)):
                    size = zc.wc.contig_size(case.contigs[c])
                    nb = size // (2 * lv.reduction)
                    if nb < 1:
                        continue
                    levels, got = summaries(exe, paths["zoom"], c, 0, 2 * lv.reduction * nb, nb)
                    assert levels == [x.reduction for x in want], (tag, levels)
                    v = th.cells_f32(case.contigs[c])
                    for kind in KINDS:
                        exp = th.expected_summary(v, lv.reduction, nb, kind)
                        assert np.array_equal(got[kind], exp, equal_nan=True), (tag, k, c, kind, got[kind], exp)
                        out["sum_%s_%d_%d_%s" % (tag, k, ci, kind)] = got[kind]
                        asserted += 1
        assert all(same) and len(same) == 4, (name, same)
        out["twins_" + name] = np.array(same)
        # one query whose bins cut windows: recorded, not asserted
        c = max(case.contigs, key=lambda x: zc.wc.contig_size(case.contigs[x]))
        size = zc.wc.contig_size(case.contigs[c])
        if size >= 7 * want[0].reduction:
            _, got = summaries(exe, paths["zoom"], c, 3, size - 2, 3)
            for kind in KINDS:
                out["unaligned_%s_%s" % (name, kind)] = got[kind]
    dst = os.path.join(HERE, "bigwig_zoom_fixture.npz")
    np.savez_compressed(dst, **out)
    print("%s: %d keys, %d summaries asserted, %d bytes" % (dst, len(out), asserted, os.path.getsize(dst)))
    assert os.path.getsize(dst) <= 512 * 1024


if __name__ == "__main__":
    main()
