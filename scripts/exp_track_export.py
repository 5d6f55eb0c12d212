#!/usr/bin/env python
"""Laps of a count-track export beside the host writer, and two array operations (profiles/track_text/NOTES.md).

    python scripts/exp_track_export.py [--lines 10000000] [--repeat 3] [--out result.json]

The bedGraph of scripts/exp_track_text.py (`--lines` lines, integer counts on 16 contigs) is imported onto '+';
``to_bedgraph`` into a binary file object is timed `--repeat` times after one untimed call: the laps of
``export_timing()`` -- slot sums, run heads + select, listed values, line lengths + offsets, format on the engine's stream,
the read-back on the host clock -- the bytes, and the wall clock of the call.  Beside it the thing it replaces:
``write_bedgraph(ga.to_host(), ...)`` on one host thread (the ``to_host()`` is timed apart).  Then ``ga * 2.5`` and
``ga + ga`` (wall clock, best of `--repeat`), and the same export of ``ga * 1.1``, nearly all of whose values are listed.
"""
import argparse
import io
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import plastid_amd as pa  # noqa: E402
from plastid_amd import track  # noqa: E402
from plastid_amd.engine import Engine  # noqa: E402
from scripts.exp_track_text import bedgraph_text, best  # noqa: E402


class Sink(io.RawIOBase):
    """A binary file that counts what it is given."""
    n = 0

    def writable(self):
        return True

    def write(self, b):
        self.n += len(b)
        return len(b)


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
        text = bedgraph_text(a.lines)
        with open(path, "w") as fh:
            fh.write(text)
        res["text_bytes"] = len(text)
        del text
        ga = pa.GenomeArray(engine=eng)
        ga.add_from_wiggle(path, "+")
        res["cells"] = int(sum(e["+"] for e in ga.extents().values()))
        ga.to_bedgraph(Sink(), "exp", "+")
        res["export_stats"] = ga.export_stats()
        runs = []
        for _ in range(a.repeat):
            sink = Sink()
            t0 = time.perf_counter()
            ga.to_bedgraph(sink, "exp", "+")
            wall = (time.perf_counter() - t0) * 1e3
            runs.append(dict(ga.export_timing(), wall=wall, bytes=sink.n))
        res["export_ms"] = runs
        t0 = time.perf_counter()
        host = ga.to_host()
        res["to_host_ms"] = (time.perf_counter() - t0) * 1e3
        sink = Sink()
        t0 = time.perf_counter()
        res["host_writer_stats"] = track.write_bedgraph(host, sink, "exp", "+")
        res["host_writer_ms"] = (time.perf_counter() - t0) * 1e3
        res["host_writer_bytes"] = sink.n
        del host

        def scaled():
            (ga * 2.5).close()

        def doubled():
            (ga + ga).close()
        res["scalar_multiply_ms"] = best(scaled, a.repeat)[0]
        res["array_add_ms"] = best(doubled, a.repeat)[0]
        r = ga * 2.5
        res["scalar_multiply_cells"] = int(sum(sum(e.values()) for e in r.extents().values()))
        r.close()
        # nearly every value listed: k * 1.1
        odd = ga * 1.1
        odd.to_bedgraph(Sink(), "exp", "+")
        sink = Sink()
        t0 = time.perf_counter()
        odd.to_bedgraph(sink, "exp", "+")
        res["listed_track"] = dict(odd.export_timing(), wall=(time.perf_counter() - t0) * 1e3, written=sink.n, **odd.export_stats())
        odd.close()
        ga.close()
    eng.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
