#!/usr/bin/env python
"""Laps of a count-track import and the rate of the track gather (profiles/track_text/NOTES.md).

    python scripts/exp_track_text.py [--lines 10000000] [--repeat 3] [--out result.json]

1. A bedGraph of `--lines` lines (integer counts over runs of 1 .. 8 positions on 16 contigs, as ``to_bedgraph`` writes
   them) is generated here and written to a temporary file.  ``GenomeArray.add_from_wiggle(path, '+')`` is timed
   `--repeat` times on a fresh array each (after one untimed import): the laps of ``import_timing()`` on the engine's
   stream -- upload, line starts, classify + state records, fields, growth + sort + apply -- and the wall clock.
2. ``read_wiggle(path)`` on the host (one thread: the host reader is the model, not a product path), wall clock.
3. ``get_counts_batch`` of 20 000 transcript chains (config C2 of bench.py) on the track, beside the same call on the
   ``BAMGenomeArray`` the track was exported from, which the dense vector serves; wall clock, best of `--repeat`.
4. The escaped share of a normalised float track: the same counts as ``repr(1e6 * v / total)``.
"""
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
from plastid_amd import synth  # noqa: E402
from plastid_amd.engine import Engine  # noqa: E402


def bedgraph_text(n_lines, values=None, seed=1):
    rng = np.random.default_rng(seed)
    per = n_lines // 16
    parts = []
    for c in range(16):
        width = rng.integers(1, 9, per)
        gap = rng.integers(0, 4, per)
        start = np.cumsum(width + gap) - width
        val = rng.integers(1, 400, per) if values is None else values(rng, per)
        name = "chr%d" % (c + 1)
        parts.append("".join("%s\t%d\t%d\t%s\n" % (name, a, a + w, v) for a, w, v in zip(start.tolist(), width.tolist(), val.tolist())))
    return "track type=bedGraph name=exp\n" + "".join(parts)


def best(f, repeat):
    t = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        f()
        t.append((time.perf_counter() - t0) * 1e3)
    return min(t), t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=10_000_000)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"lines": a.lines, "repeat": a.repeat}
    eng = Engine(0)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "exp.bedgraph")
        t0 = time.perf_counter()
        text = bedgraph_text(a.lines)
        with open(path, "w") as fh:
            fh.write(text)
        res["text_bytes"] = len(text)
        res["generate_s"] = time.perf_counter() - t0
        # 1. the import
        ga = pa.GenomeArray(engine=eng)
        ga.add_from_wiggle(path, "+")
        res["import_stats"] = ga.import_stats()
        ga.close()
        runs = []
        for _ in range(a.repeat):
            ga = pa.GenomeArray(engine=eng)
            t0 = time.perf_counter()
            ga.add_from_wiggle(path, "+")
            wall = (time.perf_counter() - t0) * 1e3
            runs.append(dict(ga.import_timing(), wall=wall))
            ga.close()
        res["import_ms"] = runs
        # 2. the host reader
        t0 = time.perf_counter()
        table = pa.read_wiggle(path)
        res["read_wiggle_ms"] = (time.perf_counter() - t0) * 1e3
        res["read_wiggle_rows"] = len(table)
        del table, text
        # 4. a normalised float track
        def shortest(rng, n):
            v = rng.integers(1, 400, n)
            return np.array([repr(1e6 * int(x) / 123456789.0) for x in v], object)
        ftext = bedgraph_text(min(a.lines, 1_000_000), values=shortest, seed=2)
        ga = pa.GenomeArray(engine=eng)
        ga.add_from_wiggle(io.StringIO(ftext), "+")
        st = ga.import_stats()
        res["float_track"] = {"lines": st["lines"], "yielded": st["yielded"], "escaped": st["escaped"],
                              "escaped_share": st["escaped"] / max(st["yielded"], 1), "import_ms": ga.import_timing()}
        ga.close()
        # 3. the gather beside the dense vector's
        from tests import bam_writer
        genome, tx, reads, _ = synth.make_config("C2", scale=0.002, tx_scale=1.0)
        bam = os.path.join(tmp, "reads.bam")
        bam_writer.write_bam(bam, list(reads.references), list(reads.lengths), bam_writer.packed_to_records(reads))
        bga = pa.BAMGenomeArray(bam, mapping=pa.FivePrimeMapFactory(12))
        ga = pa.GenomeArray(dict(zip(reads.references, (int(x) for x in reads.lengths))), engine=eng)
        for strand in "+-":
            buf = io.StringIO()
            bga.to_bedgraph(buf, "t", strand)
            ga.add_from_wiggle(io.StringIO(buf.getvalue()), strand)
        chains = tx.chains()
        positions = int(sum(c.length for c in chains))
        same = all(np.array_equal(x, y) for x, y in zip(ga.get_counts_batch(chains), bga.get_counts_batch(chains)))
        t_track, _ = best(lambda: ga.get_counts_batch(chains), a.repeat)
        t_dense, _ = best(lambda: bga.get_counts_batch(chains), a.repeat)
        res["gather"] = {"chains": len(chains), "positions": positions, "equal": bool(same), "track_ms": t_track, "bam_dense_ms": t_dense,
                         "dense_cells": bga._engine.dense_cells(0) if hasattr(bga._engine, "dense_cells") else None}
        ga.close()
    eng.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
