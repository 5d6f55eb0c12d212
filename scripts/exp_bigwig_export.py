#!/usr/bin/env python
"""Laps of a bigWig export beside the bedGraph export of the same array (profiles/track_text/NOTES.md).

    python scripts/exp_bigwig_export.py [--lines 10000000] [--repeat 5] [--codes fixed|dynamic] [--out result.json]

The track of scripts/exp_track_text.py and scripts/exp_bigwig_import.py (`--lines` items of integer counts over runs of
1 .. 8 positions on 16 contigs) is written as a bigWig by tests/bigwig_writer.py and imported once (``BigWigReader``): its
one-strand array in HBM is the source.  Timed in ONE process on one engine, `--repeat` times each after one untimed call:
1. ``GenomeArray.to_bigwig`` into memory: wall clock and the laps of ``bigwig_export_timing()``;
2. ``GenomeArray.to_bedgraph`` of the same array into memory, the parent's way out: wall clock and ``export_timing()``;
3. ``write_bigwig`` of ``to_host()`` on one host thread, once (wall clock, without ``to_host``).
Sizes: the file, its block bytes, the raw bytes of the sections, and the same sections through ``zlib.compress(., 6)``,
which is what Kent's writer would store.  The device's file is compared with the host writer's once.  `--codes`: the
Huffman codes of the encoder (``compress="fixed"``, the default of ``to_bigwig``, or ``"dynamic"``)."""
import argparse
import io
import json
import os
import statistics
import sys
import tempfile
import time
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import plastid_amd as pa  # noqa: E402
from plastid_amd.engine import Engine  # noqa: E402
from tests import bigwig_writer as bw  # noqa: E402


def track(n_lines, seed=1):
    """Per contig (name, start, width, value) of scripts/exp_track_text.py's bedGraph."""
    rng = np.random.default_rng(seed)
    per = n_lines // 16
    out = []
    for c in range(16):
        width = rng.integers(1, 9, per)
        gap = rng.integers(0, 4, per)
        start = np.cumsum(width + gap) - width
        val = rng.integers(1, 400, per)
        out.append(("chr%d" % (c + 1), start, width, val))
    return out


def spread(runs, key):
    v = [r[key] for r in runs]
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=10_000_000)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--codes", choices=("fixed", "dynamic"), default="fixed")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"lines": a.lines, "repeat": a.repeat, "codes": a.codes}
    eng = Engine(0)
    with tempfile.TemporaryDirectory() as tmp:
        chroms, sections = [], []
        for k, (name, start, width, val) in enumerate(track(a.lines)):
            items = np.zeros(len(start), bw.ITEM_DTYPES[1])
            items["start"], items["end"], items["value"] = start, start + width, val
            chroms.append((name, int((start + width).max()) + 1000))
            sections.append(bw.Section(k, "bedgraph", items))
        path = os.path.join(tmp, "exp.bw")
        with open(path, "wb") as fh:
            fh.write(bw.write_bigwig(chroms, sections, items_per_block=1024, level=1))
        del sections
        reader = pa.BigWigReader(path, engine=eng)
    ga = reader._ga
    # 1. to_bigwig
    runs, image = [], None
    for k in range(a.repeat + 1):
        fh = io.BytesIO()
        t0 = time.perf_counter()
        ga.to_bigwig(fh, ".", compress=a.codes)
        wall = (time.perf_counter() - t0) * 1e3
        if k:
            runs.append(dict(ga.bigwig_export_timing(), wall=wall))
        image = fh.getvalue()
    res["to_bigwig_ms"] = {key: spread(runs, key) for key in runs[0]}
    res["to_bigwig_stats"] = ga.bigwig_export_stats(block_types=True)
    res["file_bytes"] = len(image)
    # 2. to_bedgraph of the same array
    runs = []
    for k in range(a.repeat + 1):
        fh = io.BytesIO()
        t0 = time.perf_counter()
        ga.to_bedgraph(fh, "exp", ".")
        wall = (time.perf_counter() - t0) * 1e3
        if k:
            runs.append(dict(ga.export_timing(), wall=wall))
        res["bedgraph_bytes"] = len(fh.getvalue())
    res["to_bedgraph_ms"] = {key: spread(runs, key) for key in runs[0]}
    # 3. the host writer, one thread
    host = ga.to_host()
    fh = io.BytesIO()
    t0 = time.perf_counter()
    res["write_bigwig_stats"] = pa.write_bigwig(host, fh, ".", compress=a.codes)
    res["write_bigwig_ms"] = (time.perf_counter() - t0) * 1e3
    res["same_file"] = fh.getvalue() == image
    # the sections through zlib level 6
    fh = io.BytesIO()
    ga.to_bigwig(fh, ".", compress=False)
    stored = fh.getvalue()
    blocks = pa.bigwig_info(stored)["blocks"]
    t0 = time.perf_counter()
    res["zlib6_block_bytes"] = sum(len(zlib.compress(stored[o:o + n], 6)) for o, n in blocks)
    res["zlib6_ms"] = (time.perf_counter() - t0) * 1e3
    reader.close()
    eng.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
