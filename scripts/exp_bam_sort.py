"""Experiment: what the coordinate sort at decode (PC_BAM_SORT) costs.  N records as an aligner writes them
(bam_writer.write_bam_realistic over the C2 reads, as bench.py writes its e2e file) in coordinate order, and the same
records fully shuffled; file -> staged (pc_add_alignment_bam_path[_flags] + pc_clear_alignments, wall clock) for
  the sorted file without the flag, the sorted file with it (one key kernel and one 8-byte read-back more), and the
  shuffled file with it (the radix sort and the rank kernels);
and the sort phase alone (pc_bam_sort_stats' GPU time).  One warm-up and five passes each; one JSON line with the medians
and, after each group of passes, the device memory in use (hipMemGetInfo: the engine's pool keeps the decoder's scratch
blocks between opens, so the growth from one group to the next is what the sort's buffers took).

usage: python scripts/exp_bam_sort.py write DIR [N]            writes DIR/sorted.bam and DIR/shuffled.bam (default N 2e7)
       python scripts/exp_bam_sort.py measure DIR [--lib SO]   --lib: another build of the library (an earlier commit's, for
                                                               its file -> staged time of the same sorted file on the same
                                                               box); a library without the _flags entry points measures
                                                               the sorted file without the flag only
Run each step under its own time limit:
    timeout -k 10 900 python scripts/exp_bam_sort.py write /tmp/x && timeout -k 10 300 python scripts/exp_bam_sort.py measure /tmp/x"""
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PASSES = 5


def write(folder, n):
    import numpy as np
    from plastid_amd import synth
    from tests import bam_writer
    os.makedirs(folder, exist_ok=True)
    genome, tx, reads, mapping = synth.make_config("C2", scale=n / float(synth.CONFIGS["C2"][4]))
    threads = min(16, os.cpu_count() or 1)
    for name, aln in (("sorted", reads), ("shuffled", reads.subset(np.random.default_rng(7).permutation(reads.n), validate=False))):
        t0 = time.perf_counter()
        path = os.path.join(folder, name + ".bam")
        bam_writer.write_bam_realistic(path, aln, threads=threads)
        sys.stderr.write("%s: %d records, %.1f MB, written in %.0f s\n" % (path, aln.n, os.path.getsize(path) / 1e6, time.perf_counter() - t0))


def measure(folder, lib_path):
    from plastid_amd import _lib
    L = ctypes.CDLL(lib_path or _lib.LIB_PATH)
    vp, i64p = ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64)
    L.pc_create.argtypes = [ctypes.c_int, ctypes.POINTER(vp)]
    L.pc_destroy.argtypes = [vp]
    L.pc_clear_alignments.argtypes = [vp]
    L.pc_add_alignment_bam_path.argtypes = [vp, ctypes.c_char_p, i64p]
    L.pc_last_error.restype = ctypes.c_char_p
    has_flags = hasattr(L, "pc_add_alignment_bam_path_flags")
    if has_flags:
        L.pc_add_alignment_bam_path_flags.argtypes = [vp, ctypes.c_char_p, ctypes.c_uint32, i64p]
        L.pc_bam_open_path_flags.argtypes = [vp, ctypes.c_char_p, ctypes.c_uint32, ctypes.POINTER(vp)]
        L.pc_bam_sort_stats.argtypes = [vp, vp, ctypes.POINTER(ctypes.c_double)]
        L.pc_bam_close.argtypes = [vp]
    eng = vp()

    def ok(rc):
        if rc != 0:
            raise RuntimeError(L.pc_last_error().decode())

    ok(L.pc_create(0, ctypes.byref(eng)))
    hip = ctypes.CDLL("libamdhip64.so")

    def in_use_mb():
        free, total = ctypes.c_size_t(0), ctypes.c_size_t(0)
        return (total.value - free.value) / 1e6 if hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0 else -1.0

    def staged(path, sort):
        mapped = ctypes.c_int64(0)
        t = time.perf_counter()
        if sort:
            ok(L.pc_add_alignment_bam_path_flags(eng, os.fsencode(path), 1, ctypes.byref(mapped)))
        else:
            ok(L.pc_add_alignment_bam_path(eng, os.fsencode(path), ctypes.byref(mapped)))
        ms = (time.perf_counter() - t) * 1e3
        ok(L.pc_clear_alignments(eng))
        return ms

    def sort_phase(path):
        h = vp()
        ok(L.pc_bam_open_path_flags(eng, os.fsencode(path), 1, ctypes.byref(h)))
        st, ms = (ctypes.c_int64 * 4)(), ctypes.c_double(0.0)
        ok(L.pc_bam_sort_stats(h, st, ctypes.byref(ms)))
        L.pc_bam_close(h)
        return ms.value, list(st)

    def passes(fn, *args):
        fn(*args)                                   # page cache, library and pool warm-up
        return [fn(*args) for _ in range(PASSES)]

    s, u = os.path.join(folder, "sorted.bam"), os.path.join(folder, "shuffled.bam")
    out = dict(library=lib_path or "this tree", file_bytes=os.path.getsize(s))
    try:
        ms = passes(staged, s, False)
        out.update(sorted_plain_ms=ms, sorted_plain_median_ms=statistics.median(ms), in_use_after_plain_mb=in_use_mb())
        if has_flags:
            ms = passes(staged, s, True)
            out.update(sorted_sort_ms=ms, sorted_sort_median_ms=statistics.median(ms), in_use_after_sorted_sort_mb=in_use_mb())
            ms = passes(staged, u, True)
            out.update(shuffled_sort_ms=ms, shuffled_sort_median_ms=statistics.median(ms), shuffled_file_bytes=os.path.getsize(u),
                       in_use_after_shuffled_sort_mb=in_use_mb())
            ph = passes(sort_phase, s)
            out.update(sorted_sort_phase_median_ms=statistics.median(p[0] for p in ph), sorted_stats=ph[0][1])
            ph = passes(sort_phase, u)
            out.update(shuffled_sort_phase_median_ms=statistics.median(p[0] for p in ph), shuffled_stats=ph[0][1])
    finally:
        L.pc_destroy(eng)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    if len(sys.argv) < 3 or sys.argv[1] not in ("write", "measure"):
        sys.exit(__doc__)
    if sys.argv[1] == "write":
        write(sys.argv[2], int(float(sys.argv[3])) if len(sys.argv) > 3 else 20000000)
    else:
        measure(sys.argv[2], sys.argv[sys.argv.index("--lib") + 1] if "--lib" in sys.argv else None)
