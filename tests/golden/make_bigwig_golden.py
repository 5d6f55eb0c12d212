#!/usr/bin/env python
"""Generate ``tests/golden/bigwig_fixture.npz`` by running Kent's bigWig library -- the one the reference links -- and the
reference's own ``BigWigGenomeArray`` class in the build container.

    bash tests/golden/build_scratch_reference.sh /tmp/oracle
    python tests/golden/make_bigwig_golden.py

The Kent sources the reference's ``setup.py`` lists (:157-207), plus ``bwgCreate.c``, are compiled from where they lie into
``oracle/_ref/libkent_bw.a`` (beside the htslib of ``oracle/build_ref.sh``, which ``linefile.c`` calls) and the harness ``tests/golden/bw_golden.c`` against it into ``oracle/_ref/bw_golden`` (both
git-ignored).  Only DATA is committed.

WRITE: the texts of ``tests/bigwig_cases.py`` go through ``bigWigFileCreate`` (1024 items per block; 2 items per block and
an R-tree of fan-out 4; uncompressed).  READ BACK, for those files and for the files ``tests/bigwig_writer.py`` writes
(overlapping items): ``bbiChromList``'s order, the blocks per contig, ``bigWigValsOnChromFetchData`` per contig and
``bigWigIntervalQuery`` over seeded regions.  The script asserts that assigning a query's intervals in their order gives the
slice of the whole-contig values, then runs the reference's ``BigWigGenomeArray`` (the scratch reference) with a numpy
stand-in for the Cython ``BigWigReader``, built on those read-backs, with ``sum()`` restated from bigwig.pyx:265-302 (the
position counter that is never reset) -- the pattern of the duck-typed alignment source of the BAM fixtures.

Keys: ``files``; per file ``file_<f>`` (bytes), ``<f>_chroms`` / ``_ids`` / ``_sizes`` (bbiChromList order), ``<f>_blocks``
(contig index, offset, size), ``<f>_runs`` (contig index, start, end) + ``<f>_run_values``, ``<f>_regions`` (contig index,
start, end), ``<f>_region_off``, ``<f>_ivs`` (start, end) + ``<f>_iv_values``, ``<f>_sum``; ``arrays``; per array ``<a>_chroms``
(sorted), ``<a>_length_names`` / ``_lengths`` (the order of ``lengths()``), ``<a>_strands``, ``<a>_sum``, ``<a>_get_off`` +
``<a>_get`` / ``<a>_get_norm`` (every segment of ``query_segments`` on '+', '-', '.'; then every chain on the three), and
``<a>_ga_names`` / ``_ga_lengths`` / ``_ga_sum`` / ``_ga_<chrom>_<strand index>`` of ``to_genome_array()``.
"""
import collections
import math
import os
import subprocess
import sys
import tempfile
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
KENT = os.environ.get("KENT_SRC", "/root/reference/kent/src")
ORACLE = os.environ.get("PLASTID_SCRATCH_REFERENCE", "/tmp/oracle")
NREG, SEED = 40, 20261020
KENT_LIB = """aliType asParse base64 basicBed bbiAlias bbiRead bbiWrite bigBed binRange bits bPlusTree bwgQuery bwgValsOnChrom cirTree
colHash common dlist dnautil dystring errAbort ffAli freeType gemfont hash hex hmmstats htmlColor internet intExp kxTok linefile localmem
mgCircle mgPolygon memalloc memgfx obscure osunix pipeline psl rangeTree rbTree sqlNum sqlList tokenizer udc verbose wildcmp zlibFace
bwgCreate""".split()


def build_harness():
    subprocess.check_call(["bash", os.path.join(ROOT, "oracle", "build_ref.sh")])    # (linefile.c reads tabix files through htslib)
    ref = os.path.join(ROOT, "oracle", "_ref")
    hts = os.path.join(ref, "libhts_ref.a")
    if not os.path.exists(hts):
        raise SystemExit("oracle/_ref/libhts_ref.a was not built (is the reference present?)")
    objs = os.path.join(ref, "kent_bw_obj")
    os.makedirs(objs, exist_ok=True)
    flags = ["-O1", "-w", "-std=gnu99", "-D_FILE_OFFSET_BITS=64", "-D_LARGEFILE_SOURCE", "-D_GNU_SOURCE", "-DMACHTYPE_x86_64",
             "-I", os.path.join(KENT, "inc"), "-I", os.path.join(KENT, "htslib")]
    out = []
    for f in KENT_LIB:
        o = os.path.join(objs, f + ".o")
        if not os.path.exists(o):
            subprocess.check_call(["gcc"] + flags + ["-c", os.path.join(KENT, "lib", f + ".c"), "-o", o])
        out.append(o)
    lib = os.path.join(ref, "libkent_bw.a")
    if os.path.exists(lib):
        os.remove(lib)
    subprocess.check_call(["ar", "rcs", lib] + out)
    exe = os.path.join(ref, "bw_golden")
    subprocess.check_call(["gcc"] + flags + [os.path.join(HERE, "bw_golden.c"), lib, hts, "-lssl", "-lcrypto", "-lz", "-lm", "-lpthread", "-o", exe])
    return exe


def read_back(exe, path):
    text = subprocess.check_output([exe, "read", path, str(NREG), str(SEED)]).decode()
    chroms, ids, sizes, blocks, runs, run_values, regions, reg_off, ivs, iv_values = [], [], [], [], [], [], [], [0], [], []
    for line in text.splitlines():
        f = line.split()
        if f[0] == "CHROM":
            chroms.append(f[1]); ids.append(int(f[2])); sizes.append(int(f[3]))
        elif f[0] == "BLOCK":
            blocks.append((chroms.index(f[1]), int(f[2]), int(f[3])))
        elif f[0] == "RUN":
            runs.append((chroms.index(f[1]), int(f[2]), int(f[3]))); run_values.append(float(f[4]))
        elif f[0] == "REG":
            if regions:
                reg_off.append(len(ivs))
            regions.append((chroms.index(f[1]), int(f[2]), int(f[3])))
        elif f[0] == "IV":
            ivs.append((int(f[1]), int(f[2]))); iv_values.append(float(f[3]))
    reg_off.append(len(ivs))
    return dict(chroms=chroms, ids=ids, sizes=sizes, blocks=blocks, runs=runs, run_values=run_values, regions=regions, region_off=reg_off, ivs=ivs,
                iv_values=iv_values)


def contig_arrays(rb):
    arrays = collections.OrderedDict((c, np.zeros(n, np.float64)) for c, n in zip(rb["chroms"], rb["sizes"]))
    for (ci, a, b), v in zip(rb["runs"], rb["run_values"]):
        arrays[rb["chroms"][ci]][a:b] = v
    return arrays


class KentReader(object):
    """The reference's BigWigReader over Kent's read-backs: what its Cython methods compute, restated (bigwig.pyx:178-412)."""

    def __init__(self, filename, rb):
        from plastid.genomics.roitools import SegmentChain
        self._chain = SegmentChain
        self.filename, self.fill, self._sum = filename, 0.0, None
        self.chroms = collections.OrderedDict(zip(rb["chroms"], rb["sizes"]))
        self._arrays = contig_arrays(rb)

    def get(self, roi, roi_order=True, fill=np.nan):
        from plastid.util.services.exceptions import DataWarning
        if isinstance(roi, self._chain):
            return roi.get_counts(self)
        counts = np.full(len(roi), self.fill, dtype=float)
        if roi.chrom not in self.chroms:
            warnings.warn("No data for chromosome '%s' in file '%s'." % (roi.chrom, self.filename), DataWarning)
            return counts
        whole = self._arrays[roi.chrom]
        a, b = max(roi.start, 0), min(roi.end, len(whole))
        if b > a:
            counts[a - roi.start:b - roi.start] = whole[a:b]
        if roi.strand == "-" and roi_order is True:
            counts = counts[::-1]
        return counts

    def __getitem__(self, roi):
        return self.get(roi)

    def get_chromosome_counts(self, chrom):
        return self._arrays[chrom].copy() if chrom in self.chroms else np.array(0, dtype=float)

    def sum(self):
        if self._sum is None:
            mysum, i = 0.0, 0                       # `i` is set once, in front of the loop over the contigs (bigwig.pyx:278)
            for chrom in self.chroms:
                vbuf = self._arrays[chrom]
                while i < len(vbuf):
                    mysum += vbuf[i]
                    i += 1
            self._sum = mysum
        return self._sum


def main():
    from tests import bigwig_cases as bc
    sys.path[:0] = [ORACLE, os.path.join(ORACLE, "stubs")]
    exe = build_harness()
    tmp = tempfile.mkdtemp(prefix="bw_golden_")
    sizes_path = os.path.join(tmp, "chrom.sizes")
    open(sizes_path, "w").write(bc.chrom_sizes_text())
    files = collections.OrderedDict()
    for name, (text, per_slot, block_size, compress) in bc.kent_texts().items():
        wig, out = os.path.join(tmp, name + ".wig"), os.path.join(tmp, name + ".bw")
        open(wig, "w").write(text)
        subprocess.check_call([exe, "write", wig, sizes_path, str(block_size), str(per_slot), str(compress), out])
        files[name] = open(out, "rb").read()
    for name, image in bc.python_files().items():
        open(os.path.join(tmp, name + ".bw"), "wb").write(image)
        files[name] = image
    out = dict(files=np.array(list(files)), kent=np.array("kent/src/lib as vendored by the reference"))
    readers = {}
    for name, image in files.items():
        rb = read_back(exe, os.path.join(tmp, name + ".bw"))
        arrays = contig_arrays(rb)
        # a query's intervals, assigned in their order, are the slice of the whole-contig values (both Kent readers agree)
        for r, (ci, a, b) in enumerate(rb["regions"]):
            got = np.zeros(b - a)
            for k in range(rb["region_off"][r], rb["region_off"][r + 1]):
                s, e = rb["ivs"][k]
                got[s - a:e - a] = rb["iv_values"][k]
            assert np.array_equal(got, arrays[rb["chroms"][ci]][a:b]), (name, r)
        readers[name] = KentReader(name + ".bw", rb)
        total = readers[name].sum()
        quirk = [x for (lo, hi), arr in zip(sum_ranges(rb["sizes"]), arrays.values()) for x in arr[lo:hi]]
        assert total == math.fsum(quirk), name     # (multiples of 2^-10 below 2^40: every order gives these bits)
        out["file_" + name] = np.frombuffer(image, np.uint8)
        out[name + "_chroms"], out[name + "_ids"], out[name + "_sizes"] = np.array(rb["chroms"]), np.array(rb["ids"], np.int64), np.array(rb["sizes"], np.int64)
        out[name + "_blocks"] = np.array(rb["blocks"], np.int64).reshape(-1, 3)
        out[name + "_runs"], out[name + "_run_values"] = np.array(rb["runs"], np.int64).reshape(-1, 3), np.array(rb["run_values"], np.float64)
        out[name + "_regions"], out[name + "_region_off"] = np.array(rb["regions"], np.int64).reshape(-1, 3), np.array(rb["region_off"], np.int64)
        out[name + "_ivs"], out[name + "_iv_values"] = np.array(rb["ivs"], np.int64).reshape(-1, 2), np.array(rb["iv_values"], np.float64)
        out[name + "_sum"] = np.array(total)
        print("%s: %d bytes, %d contigs, %d blocks, %d runs, sum %r (all positions: %r)" % (
            name, len(image), len(rb["chroms"]), len(rb["blocks"]), len(rb["runs"]), total, math.fsum(x for arr in arrays.values() for x in arr)))

    import plastid.genomics.genome_array as ga_mod
    from plastid.genomics.roitools import GenomicSegment, SegmentChain
    ga_mod.BigWigReader = lambda filename, **kw: readers[filename]
    # genome_array.py calls warnings.warn on a strand the array lacks (:1206) without importing warnings: as shipped that
    # get() ends in a NameError.  The fixture records what the line is written to do -- the warning, then zeros.
    ga_mod.warnings = warnings
    segs, chains = bc.query_segments(SEED)
    out["arrays"] = np.array(list(bc.ARRAYS))
    warnings.simplefilter("ignore")
    for aname, adds in bc.ARRAYS.items():
        arr = ga_mod.BigWigGenomeArray()
        for strand, fname in adds:
            arr.add_from_bigwig(fname, strand)
        out[aname + "_chroms"] = np.array(sorted(arr.chroms()))
        out[aname + "_length_names"], out[aname + "_lengths"] = np.array(list(arr.lengths())), np.array(list(arr.lengths().values()), np.int64)
        out[aname + "_strands"] = np.array(list(arr.strands()))
        out[aname + "_sum"] = np.array(float(arr.sum()))
        for norm in (False, True):
            arr.set_normalize(norm)
            vecs = []
            for strand in "+-.":
                for c, a, b in segs:
                    vecs.append(arr.get(GenomicSegment(c, a, b, strand)))
                    assert np.array_equal(vecs[-1], arr[GenomicSegment(c, a, b, strand)])
            for strand in "+-.":
                for ch in chains:
                    vecs.append(SegmentChain(*[GenomicSegment(c, a, b, strand) for c, a, b in ch]).get_counts(arr))
            if not norm:
                out[aname + "_get_off"] = np.concatenate([[0], np.cumsum([len(v) for v in vecs])]).astype(np.int64)
            out[aname + ("_get_norm" if norm else "_get")] = np.concatenate(vecs)
        arr.set_normalize(False)
        ga = arr.to_genome_array()
        out[aname + "_ga_names"] = np.array(list(ga.lengths()))
        out[aname + "_ga_lengths"] = np.array(list(ga.lengths().values()), np.int64)
        out[aname + "_ga_sum"] = np.array(float(ga.sum()))
        for c in ga.chroms():
            for si, st in enumerate(ga.strands()):
                out["%s_ga_%s_%d" % (aname, c, si)] = np.asarray(ga._chroms[c][st], np.float64)
        print("%s: strands %s, sum %r, to_genome_array lengths %s sum %r" % (aname, list(arr.strands()), float(arr.sum()), dict(ga.lengths()), float(ga.sum())))
    dest = os.path.join(HERE, "bigwig_fixture.npz")
    np.savez_compressed(dest, **out)
    size = os.path.getsize(dest)
    print("wrote %s: %.0f KB" % (dest, size / 1e3))
    assert size <= 512 * 1024


def sum_ranges(lengths):
    out, i = [], 0
    for n in lengths:
        out.append((min(i, n), n))
        i = max(i, n)
    return out


if __name__ == "__main__":
    sys.exit(main())
