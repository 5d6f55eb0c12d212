#!/usr/bin/env python
"""Laps of a bigWig import beside the text import of the same track (profiles/track_text/NOTES.md).

    python scripts/exp_bigwig_import.py [--lines 10000000] [--repeat 3] [--out result.json]

The bedGraph of scripts/exp_track_text.py (`--lines` lines of integer counts over runs of 1 .. 8 positions on 16 contigs)
is written as text and, by tests/bigwig_writer.py, as a bigWig of 1024 items per block (zlib level 6, bedGraph sections, no
zoom levels).  Timed, `--repeat` times each after one untimed call, on one engine:
1. ``BigWigGenomeArray.add_from_bigwig(path, '+')``: wall clock and the laps of ``BigWigReader.import_timing()`` -- upload,
   inflate + Adler-32, sections + items, sort + apply;
2. ``GenomeArray.add_from_wiggle(text path, '+')`` of the same track on the same commit: wall clock and its laps;
3. ``read_bigwig(path)`` on one host thread (zlib), wall clock.
The two arrays are compared cell for cell once (``to_genome_array() == GenomeArray``)."""
import argparse
import json
import os
import sys
import tempfile
import time

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=10_000_000)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"lines": a.lines, "repeat": a.repeat}
    eng = Engine(0)
    with tempfile.TemporaryDirectory() as tmp:
        t0 = time.perf_counter()
        contigs = track(a.lines)
        text_path, bw_path = os.path.join(tmp, "exp.bedgraph"), os.path.join(tmp, "exp.bw")
        with open(text_path, "w") as fh:
            fh.write("track type=bedGraph name=exp\n")
            for name, start, width, val in contigs:
                fh.write("".join("%s\t%d\t%d\t%d\n" % (name, s, s + w, v) for s, w, v in zip(start.tolist(), width.tolist(), val.tolist())))
        res["text_bytes"] = os.path.getsize(text_path)
        chroms, sections = [], []
        for k, (name, start, width, val) in enumerate(contigs):
            items = np.zeros(len(start), bw.ITEM_DTYPES[1])
            items["start"], items["end"], items["value"] = start, start + width, val
            chroms.append((name, int((start + width).max()) + 1000))
            sections.append(bw.Section(k, "bedgraph", items))
        image = bw.write_bigwig(chroms, sections, items_per_block=1024, fanout=256, level=6)
        with open(bw_path, "wb") as fh:
            fh.write(image)
        res["bigwig_bytes"] = len(image)
        del image, sections
        res["generate_s"] = time.perf_counter() - t0
        # 1. the bigWig import
        runs = []
        for k in range(a.repeat + 1):
            arr = pa.BigWigGenomeArray(engine=eng)
            t0 = time.perf_counter()
            arr.add_from_bigwig(bw_path, "+")
            wall = (time.perf_counter() - t0) * 1e3
            reader = arr._strand_dict["+"][0]
            if k == 0:
                res["bigwig_stats"] = reader.import_stats()
            else:
                runs.append(dict(reader.import_timing(), wall=wall))
            if k < a.repeat:
                arr.close()
        res["bigwig_import_ms"] = runs
        # 2. the text import of the same track
        runs = []
        for k in range(a.repeat + 1):
            ga = pa.GenomeArray(engine=eng)
            t0 = time.perf_counter()
            ga.add_from_wiggle(text_path, "+")
            wall = (time.perf_counter() - t0) * 1e3
            if k:
                runs.append(dict(ga.import_timing(), wall=wall))
            if k < a.repeat:
                ga.close()
        res["text_import_ms"] = runs
        mine = arr.to_genome_array()
        res["equal_cells"] = bool(mine == ga) and mine.sum() == ga.sum()
        mine.close(); ga.close(); arr.close()
        # 3. the host reader
        t0 = time.perf_counter()
        table = pa.read_bigwig(bw_path)
        res["read_bigwig_ms"] = (time.perf_counter() - t0) * 1e3
        res["read_bigwig_rows"] = len(table)
    eng.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
