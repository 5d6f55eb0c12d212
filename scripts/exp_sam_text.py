"""Experiment: SAM text against its BAM twin, host against GPU.  Writes a realistic file of N records (default 2e7: a C2
sample with names, sequences, qualities, NH and MD tags; tests/sam_writer.py) and its BAM twin, untimed, then reports the
median of five passes, in alternating order, of

    read_sam (16 threads) | read_sam_gpu | Engine.add_sam | read_bam_gpu | Engine.add_bam

with the GPU laps of read_sam_gpu (upload, line starts, fields, placement + columns), the ratio of the parse laps to the
upload lap (the PCIe rate is the yardstick of the GPU path), and -- for the ``decode="auto"`` threshold -- host against GPU
on leading pieces of the file from 1 MB up.  The result goes to stdout and, as JSON, to the file named by the second argument.

usage: python scripts/exp_sam_text.py [N] [out.json]"""
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from plastid_amd import synth  # noqa: E402
from plastid_amd.bam import read_bam_gpu, read_sam, read_sam_gpu  # noqa: E402
from plastid_amd.engine import Engine  # noqa: E402
from tests import bam_writer, sam_writer  # noqa: E402

n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 20000000
out_json = sys.argv[2] if len(sys.argv) > 2 else None
PASSES = 5
THREADS = 16


def say(*a):
    print(*a, flush=True)


tmp = tempfile.gettempdir()
sam, bam = os.path.join(tmp, "pc_samtext_%d.sam" % n), os.path.join(tmp, "pc_samtext_%d.bam" % n)
if not (os.path.exists(sam) and os.path.exists(bam)):
    t0 = time.perf_counter()
    reads = synth.make_config("C2", scale=n / 1e8)[2]
    say("sample: %d records (%.0f s)" % (reads.n, time.perf_counter() - t0))
    bam_writer.write_bam_realistic(bam, reads, threads=THREADS)
    say("BAM twin written (%.0f s)" % (time.perf_counter() - t0))
    sam_writer.write_sam_realistic(sam + ".tmp", reads, chunk=1 << 19)
    os.replace(sam + ".tmp", sam)
    say("SAM text written (%.0f s)" % (time.perf_counter() - t0))
    del reads
sam_bytes, bam_bytes = os.path.getsize(sam), os.path.getsize(bam)
say("== %s: %.0f MB of text; BAM twin %.0f MB" % (os.path.basename(sam), sam_bytes / 1e6, bam_bytes / 1e6))

eng = Engine(0)
laps = []


def t_read_sam():
    return read_sam(sam, threads=THREADS).n


def t_read_sam_gpu():
    timing = {}
    k = read_sam_gpu(sam, eng, timing=timing).n
    laps.append(timing)
    return k


def t_add_sam():
    eng.clear_alignments()
    return eng.add_sam(sam)


def t_read_bam_gpu():
    return read_bam_gpu(bam, eng).n


def t_add_bam():
    eng.clear_alignments()
    return eng.add_bam(bam)


def median_of(jobs, passes):
    """ms per job: the median of `passes` passes, the jobs in alternating order (forward, backward, ...)"""
    times = {name: [] for name, _ in jobs}
    for p in range(passes):
        for name, fn in (jobs if p % 2 == 0 else jobs[::-1]):
            t0 = time.perf_counter()
            fn()
            times[name].append((time.perf_counter() - t0) * 1e3)
    return {k: statistics.median(v) for k, v in times.items()}, times


jobs = [("read_sam", t_read_sam), ("read_sam_gpu", t_read_sam_gpu), ("add_sam", t_add_sam), ("read_bam_gpu", t_read_bam_gpu), ("add_bam", t_add_bam)]
for name, fn in jobs:          # one warm pass each: page cache, the engine's pool, the page-locked ring
    fn()
laps.clear()
med, every = median_of(jobs, PASSES)
eng.clear_alignments()
result = dict(records=n, sam_bytes=sam_bytes, bam_bytes=bam_bytes, passes=PASSES, threads=THREADS, median_ms=med, all_ms=every)
say("median of %d passes, ms:" % PASSES)
for k, v in med.items():
    say("  %-14s %9.1f   (%s)" % (k, v, " ".join("%.0f" % x for x in every[k])))
lap_med = {k: statistics.median(t[k] for t in laps) for k in ("upload_ms", "lines_ms", "fields_ms", "place_ms", "open_wall_ms", "read_wall_ms")}
up = lap_med["upload_ms"]
parse = lap_med["lines_ms"] + lap_med["fields_ms"] + lap_med["place_ms"]
result.update(gpu_laps_ms=lap_med, upload_gb_s=laps[0]["uploaded_bytes"] / up / 1e6 if up > 0 else 0.0, parse_over_upload=parse / up if up > 0 else 0.0,
              fields_over_upload=lap_med["fields_ms"] / up if up > 0 else 0.0)
say("read_sam_gpu laps (median, ms): upload %.1f | line starts %.1f | fields %.1f | placement + columns %.1f | open %.1f | columns to host %.1f" % (
    up, lap_med["lines_ms"], lap_med["fields_ms"], lap_med["place_ms"], lap_med["open_wall_ms"], lap_med["read_wall_ms"]))
say("upload %.1f GB/s; parse / upload %.2f; fields / upload %.2f" % (result["upload_gb_s"], result["parse_over_upload"], result["fields_over_upload"]))

# the crossover of the two SAM readers: leading pieces of the file, cut at a line end
cross = []
data = open(sam, "rb")
for mb in (1, 2, 4, 8, 16, 32, 64, 128):
    want = mb << 20
    if want >= sam_bytes:
        break
    data.seek(0)
    blob = data.read(want + (1 << 16))
    blob = blob[:blob.index(b"\n", want) + 1]
    piece = os.path.join(tmp, "pc_samtext_piece.sam")
    with open(piece, "wb") as fh:
        fh.write(blob)
    pj = [("host", lambda: read_sam(piece, threads=THREADS).n), ("gpu", lambda: read_sam_gpu(piece, eng).n)]
    for _, fn in pj:
        fn()
    m, _ = median_of(pj, PASSES)
    cross.append(dict(mb=mb, host_ms=m["host"], gpu_ms=m["gpu"]))
    say("  %4d MB: host %.1f ms, gpu %.1f ms" % (mb, m["host"], m["gpu"]))
    os.remove(piece)
result["crossover"] = cross
eng.close()
if out_json:
    with open(out_json, "w") as fh:
        json.dump(result, fh, indent=1)
