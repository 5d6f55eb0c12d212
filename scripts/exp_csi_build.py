"""Experiment: the BAI and the CSI index of one BAM file built on the GPU (bam.build_index, fmt="bai" / fmt="csi"), N
records written as bench.py writes its skeleton e2e file.  One process; a warm-up of each, then three passes of each,
alternating; prints one JSON line with the medians of every lap of pc_bam_index_timing and the indexes' counts.
usage: python scripts/exp_csi_build.py [records=2e7] [min_shift=14]
    timeout -k 10 600 python scripts/exp_csi_build.py 2e7"""
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from plastid_amd import synth  # noqa: E402
from plastid_amd.bam import build_index  # noqa: E402
from plastid_amd.engine import Engine  # noqa: E402
from tests import bam_writer  # noqa: E402

n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 20000000
min_shift = int(sys.argv[2]) if len(sys.argv) > 2 else 14
genome, tx, reads, mapping = synth.make_config("C2", scale=n / float(synth.CONFIGS["C2"][4]))
tmp = tempfile.mkdtemp(prefix="pc_csi_")
path = os.path.join(tmp, "s.bam")
t0 = time.perf_counter()
nbytes = bam_writer.write_bam_packed(path, reads, threads=min(16, os.cpu_count() or 1))
sys.stderr.write("file: %d records, %.1f MB compressed, %.1f MB inflated, written in %.0f s\n"
                 % (reads.n, os.path.getsize(path) / 1e6, nbytes / 1e6, time.perf_counter() - t0))
eng = Engine(0)


def one(fmt):
    timing = {}
    t = time.perf_counter()
    build_index(path, engine=eng, overwrite=True, timing=timing, fmt=fmt, min_shift=min_shift if fmt == "csi" else 14)
    timing["wall_ms"] = (time.perf_counter() - t) * 1e3
    return timing


try:
    for fmt in ("bai", "csi"):
        one(fmt)                      # page cache, library and pool warm-up
    passes = {"bai": [], "csi": []}
    for _ in range(3):
        for fmt in ("bai", "csi"):
            passes[fmt].append(one(fmt))
    out = dict(records=reads.n, min_shift=min_shift)
    for fmt, ps in passes.items():
        med = {k: statistics.median(p[k] for p in ps) for k in ps[0] if k.endswith("_ms")}
        med["index_plus_readback_ms"] = statistics.median(p["index_ms"] + p["readback_ms"] for p in ps)
        out[fmt] = dict(median=med, index_plus_readback_passes=[p["index_ms"] + p["readback_ms"] for p in ps],
                        counts={k: ps[0][k] for k in ("runs", "chunks", "bins", "linear", "index_bytes", "depth")})
    print(json.dumps(out))
finally:
    eng.close()
    for f in os.listdir(tmp):
        os.remove(os.path.join(tmp, f))
    os.rmdir(tmp)
