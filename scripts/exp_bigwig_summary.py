#!/usr/bin/env python
"""Binned summaries from the zoom levels beside the gather over the cells and the host model (profiles/track_text/NOTES.md).

    python scripts/exp_bigwig_summary.py [--lines 10000000] [--regions 20000] [--bins 100] [--repeat 5] [--out result.json]

The track of scripts/exp_bigwig_zoom.py (`--lines` items of integer counts over runs of 1 .. 8 positions on 16 contigs) is
imported once and written back with ``to_bigwig(zoom=True)``; that file is the subject.  `--regions` regions -- a seeded
contig and start, spans log-uniform between 2 000 and 2 000 000 positions, so that the bins select the items and every
zoom level -- of `--bins` bins each, in ONE process on one engine:
1. ``BigWigReader.summarize_batch`` (mean): the FIRST call, which loads every table it selects (wall clock, the
   ``summary_timing()`` laps, ``summary_stats()``), then `--repeat` steady calls (medians of the wall clock and the laps);
2. the same means from the cells: ``get_counts_batch`` plus a numpy reduction (sum over the written cells / their number
   per bin), over the first regions that fit `--gather-positions` positions per call -- the cells of all 20 000 regions
   would be tens of GB -- reported per region beside the summaries' time per region, with the largest relative
   difference of the two means (the levels scale a cut record by its overlap; the cells do not);
3. ``summarize_bigwig`` of the same file and regions on one host thread (wall clock), and whether it gave the device's
   answer bit for bit."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import plastid_amd as pa  # noqa: E402
from plastid_amd.engine import Engine  # noqa: E402
from scripts.exp_bigwig_export import track  # noqa: E402
from tests import bigwig_writer as bw  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=10_000_000)
    ap.add_argument("--regions", type=int, default=20000)
    ap.add_argument("--bins", type=int, default=100)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--gather-positions", type=int, default=200_000_000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"lines": a.lines, "regions": a.regions, "bins": a.bins, "repeat": a.repeat}
    eng = Engine(0)
    with tempfile.TemporaryDirectory() as tmp:
        chroms, sections = [], []
        for k, (name, start, width, val) in enumerate(track(a.lines)):
            items = np.zeros(len(start), bw.ITEM_DTYPES[1])
            items["start"], items["end"], items["value"] = start, start + width, val
            chroms.append((name, int((start + width).max()) + 1000))
            sections.append(bw.Section(k, "bedgraph", items))
        plain = os.path.join(tmp, "plain.bw")
        with open(plain, "wb") as fh:
            fh.write(bw.write_bigwig(chroms, sections, items_per_block=1024, level=1))
        del sections
        source = pa.BigWigReader(plain, engine=eng)
        path = os.path.join(tmp, "zoomed.bw")
        source._ga.to_bigwig(path, ".", zoom=True)
        source.close()
        res["file_bytes"] = os.path.getsize(path)
        res["levels"] = [z[0] for z in pa.bigwig_zoom_info(path)]
        reader = pa.BigWigReader(path, engine=eng)

        rng = np.random.default_rng(7)
        names, sizes = [c for c, _ in chroms], [s for _, s in chroms]
        regions = []
        for _ in range(a.regions):
            c = int(rng.integers(0, len(names)))
            span = int(min(np.exp(rng.uniform(np.log(2e3), np.log(2e6))), sizes[c] - 1))
            start = int(rng.integers(0, sizes[c] - span))
            regions.append(pa.GenomicSegment(names[c], start, start + span, "."))       # (a reader's track has the one strand '.')

        # 1. the summaries: the first call loads the tables
        t0 = time.perf_counter()
        first = reader.summarize_batch(regions, a.bins)
        res["first_call_ms"] = dict(reader.summary_timing(), wall=(time.perf_counter() - t0) * 1e3)
        res["stats"] = reader.summary_stats()
        res["stats"]["per_table"] = {str(k): v for k, v in res["stats"]["per_table"].items()}
        runs = []
        for _ in range(a.repeat):
            t0 = time.perf_counter()
            again = reader.summarize_batch(regions, a.bins)
            runs.append(dict(reader.summary_timing(), wall=(time.perf_counter() - t0) * 1e3))
        res["steady_call_ms"] = {k: statistics.median(r[k] for r in runs) for k in runs[0]}
        res["steady_equals_first"] = bool(np.array_equal(first, again, equal_nan=True))
        res["bins_with_data"] = int(np.isfinite(first).sum())

        # 2. the same means from the cells, over the regions that fit one call
        take, positions = 0, 0
        while take < len(regions) and positions + len(regions[take]) <= a.gather_positions:
            positions += len(regions[take])
            take += 1
        chains = [pa.SegmentChain(r) for r in regions[:take]]
        laps, worst = [], 0.0
        for k in range(min(a.repeat, 3) + 1):
            t0 = time.perf_counter()
            cells = reader._ga.get_counts_batch(chains)
            t1 = time.perf_counter()
            means = np.full((take, a.bins), np.nan)
            for i, v in enumerate(cells):
                edges = (len(v) * np.arange(a.bins + 1, dtype=np.int64)) // a.bins
                s = np.add.reduceat(v, edges[:-1])
                n = np.add.reduceat((v != 0).astype(np.int64), edges[:-1])
                with np.errstate(invalid="ignore", divide="ignore"):
                    means[i] = np.where(n > 0, s / n, np.nan)
            t2 = time.perf_counter()
            if k:
                laps.append({"gather": (t1 - t0) * 1e3, "numpy": (t2 - t1) * 1e3, "wall": (t2 - t0) * 1e3})
            del cells
        both = np.isfinite(means) & np.isfinite(first[:take])
        if both.any():
            worst = float(np.max(np.abs(means[both] - first[:take][both]) / np.abs(means[both])))
        res["gather_path"] = {"regions": take, "positions": positions, "ms": {k: statistics.median(r[k] for r in laps) for k in laps[0]},
                              "bins_where_only_one_has_data": int((np.isfinite(means) != np.isfinite(first[:take])).sum()), "largest_relative_difference_of_the_means": worst}
        res["ms_per_region"] = {"summarize_batch_steady": res["steady_call_ms"]["wall"] / len(regions), "gather_and_numpy": res["gather_path"]["ms"]["wall"] / max(take, 1)}

        # 3. the host model, one thread
        t0 = time.perf_counter()
        host = pa.summarize_bigwig(path, regions, a.bins)
        res["summarize_bigwig_ms"] = (time.perf_counter() - t0) * 1e3
        res["host_equals_device"] = bool(np.array_equal(host, first, equal_nan=True))
        reader.close()
    eng.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
