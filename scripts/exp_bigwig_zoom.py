#!/usr/bin/env python
"""The zoom levels of a bigWig export beside the export without them (profiles/track_text/NOTES.md).

    python scripts/exp_bigwig_zoom.py [--lines 10000000] [--repeat 5] [--out result.json]

The track of scripts/exp_bigwig_export.py (`--lines` items of integer counts over runs of 1 .. 8 positions on 16 contigs,
imported once through ``BigWigReader``) is the source.  Timed in ONE process on one engine, for ``compress=True`` and
``compress="dynamic"``, `--repeat` times each after one untimed call, the two calls taking turns:
1. ``GenomeArray.to_bigwig()`` into memory: wall clock and ``bigwig_export_timing()`` -- the call of the parent commit;
2. ``GenomeArray.to_bigwig(zoom=True)`` into memory: wall clock, ``bigwig_export_timing()`` and the zoom lap split by
   ``bigwig_export_zoom_timing()`` into level 0, the levels above, records + block table, deflate + compaction;
3. ``write_bigwig(zoom=True)`` and ``write_bigwig()`` of ``to_host()`` on one host thread, once each (wall clock, without
   ``to_host``), and whether the first wrote the device's file.
Reported per mode: the medians (with min and max), the records, blocks and bytes of every level, both file sizes."""
import argparse
import io
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import plastid_amd as pa  # noqa: E402
from plastid_amd.engine import Engine  # noqa: E402
from scripts.exp_bigwig_export import spread, track  # noqa: E402
from tests import bigwig_writer as bw  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=10_000_000)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"lines": a.lines, "repeat": a.repeat}
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
    host = ga.to_host()
    for codes in ("fixed", "dynamic"):
        plain_runs, zoom_runs, images, levels = [], [], {}, []
        for k in range(a.repeat + 1):
            for zoom, runs in ((False, plain_runs), (True, zoom_runs)):
                fh = io.BytesIO()
                t0 = time.perf_counter()
                ga.to_bigwig(fh, ".", compress=codes, zoom=zoom)
                wall = (time.perf_counter() - t0) * 1e3
                if k:
                    lap = dict(ga.bigwig_export_timing(), wall=wall)
                    if zoom:
                        parts = ga.bigwig_export_zoom_timing()
                        lap.update(("zoom_" + key, v) for key, v in parts.items())
                        lap["zoom_all"] = sum(parts.values())
                    runs.append(lap)
                images[zoom] = fh.getvalue()
                if zoom:
                    levels = ga.bigwig_export_zoom_stats()
        out = {"to_bigwig_ms": {key: spread(plain_runs, key) for key in plain_runs[0]},
               "to_bigwig_zoom_ms": {key: spread(zoom_runs, key) for key in zoom_runs[0]},
               "file_bytes": len(images[False]), "zoom_file_bytes": len(images[True]), "levels": levels,
               "file_growth": (len(images[True]) - len(images[False])) / float(len(images[False]))}
        out["wall_ratio"] = out["to_bigwig_zoom_ms"]["wall"]["median"] / out["to_bigwig_ms"]["wall"]["median"]
        fh = io.BytesIO()
        t0 = time.perf_counter()
        pa.write_bigwig(host, fh, ".", compress=codes, zoom=True)
        out["write_bigwig_zoom_ms"] = (time.perf_counter() - t0) * 1e3
        out["same_file"] = fh.getvalue() == images[True]
        fh = io.BytesIO()
        t0 = time.perf_counter()
        pa.write_bigwig(host, fh, ".", compress=codes)
        out["write_bigwig_ms"] = (time.perf_counter() - t0) * 1e3
        res[codes] = out
    reader.close()
    eng.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
