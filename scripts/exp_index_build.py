"""Experiment: the BAI index of a BAM file built on the GPU (bam.build_index) beside the whole-file open of the same file
(pc_bam_open_path + pc_bam_close), N records written as bench.py writes its two e2e files: the 42-byte skeleton records
(`skeleton`) or records as an aligner writes them (`realistic`).  One process; three passes of each after a warm-up pass;
prints one JSON line with the medians, the laps of pc_bam_index_timing and the index's counts.
usage: python scripts/exp_index_build.py skeleton 1e8 [--index-only]      (--index-only: one warm-up and one index pass,
for a kernel trace)
Run each file as a step of its own, under its own time limit:
    timeout -k 10 900 python scripts/exp_index_build.py skeleton 1e8 && timeout -k 10 1100 python scripts/exp_index_build.py realistic 1e8"""
import ctypes
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from plastid_amd import _lib, synth  # noqa: E402
from plastid_amd.bam import build_index  # noqa: E402
from plastid_amd.engine import Engine  # noqa: E402
from tests import bam_writer  # noqa: E402

kind = sys.argv[1] if len(sys.argv) > 1 else "skeleton"
n = int(float(sys.argv[2])) if len(sys.argv) > 2 else 20000000
index_only = "--index-only" in sys.argv
genome, tx, reads, mapping = synth.make_config("C2", scale=n / float(synth.CONFIGS["C2"][4]))
tmp = tempfile.mkdtemp(prefix="pc_index_")
path = os.path.join(tmp, "s.bam")
t0 = time.perf_counter()
writer = bam_writer.write_bam_realistic if kind == "realistic" else bam_writer.write_bam_packed
nbytes = writer(path, reads, threads=min(16, os.cpu_count() or 1))
sys.stderr.write("file: %d records, %.1f MB compressed, %.1f MB inflated, written in %.0f s\n"
                 % (reads.n, os.path.getsize(path) / 1e6, nbytes / 1e6, time.perf_counter() - t0))
eng = Engine(0)
L = _lib.load()


def open_pass():
    h = ctypes.c_void_p()
    t = time.perf_counter()
    _lib.check(L.pc_bam_open_path(eng._h, os.fsencode(path), ctypes.byref(h)))
    ms = (ctypes.c_double * 4)()
    L.pc_bam_timing(h, ms)            # upload, inflate, chain, fields + columns (the engine's stream)
    L.pc_bam_close(h)
    return (time.perf_counter() - t) * 1e3, list(ms)


def index_pass():
    timing = {}
    t = time.perf_counter()
    build_index(path, engine=eng, overwrite=True, timing=timing)
    timing["wall_ms"] = (time.perf_counter() - t) * 1e3
    return timing


try:
    index_pass()                      # page cache, library and pool warm-up
    if index_only:
        out = dict(kind=kind, records=reads.n, index=index_pass())
    else:
        open_pass()
        passes = [open_pass() for _ in range(3)]
        opens, open_laps = [w for w, _ in passes], [statistics.median(l[k] for _, l in passes) for k in range(4)]
        idx = [index_pass() for _ in range(3)]
        laps = ("upload_ms", "inflate_ms", "chain_ms", "fields_ms", "index_ms", "readback_ms", "finish_ms", "total_ms", "wall_ms")
        out = dict(kind=kind, records=reads.n, file_bytes=os.path.getsize(path), open_ms=opens, open_median_ms=statistics.median(opens),
                   open_laps_median_ms=dict(zip(("upload_ms", "inflate_ms", "chain_ms", "decode_ms"), open_laps)),
                   index_ms=[t["wall_ms"] for t in idx], index_median_ms=statistics.median(t["wall_ms"] for t in idx),
                   laps_median_ms={k: statistics.median(t[k] for t in idx) for k in laps},
                   **{k: idx[0][k] for k in ("placed", "runs", "chunks", "bins", "linear", "n_no_coor", "mapped", "index_bytes")})
    print(json.dumps(out), flush=True)
finally:
    eng.close()
    for f in (path, path + ".bai"):
        if os.path.exists(f):
            os.remove(f)
    os.rmdir(tmp)
