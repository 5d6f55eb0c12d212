#!/usr/bin/env python
"""``BAMGenomeArray.to_bedgraph`` and ``to_genome_array`` on the device beside the paths they replace
(profiles/track_text/NOTES.md).

    python scripts/exp_bam_export.py [--scale 0.1] [--repeat 3] [--out result.json]

A seeded sample of config C2 (``--scale 0.1``: 10^7 reads on the yeast-scale genome, 5' rule with offset 12) is staged
once.  The '+' bedGraph goes into a sink that counts what it is given: in one process the device export
(``pc_counts_export``) alternates with the loop it replaced -- one count per chromosome, ``Plan.rle``, the run table to
the host, one ``"%s\\t%s\\t%s\\t%s\\n" %`` and one ``fh.write`` per line, restated here -- `--repeat` timed calls each
after one untimed call; both texts are compared once.  Then ``to_genome_array(array_type=GenomeArray)`` (one
``pc_track_set_counts`` per contig and strand) beside the round trip through the host and ``__setitem__``.  Prints one
JSON line: medians, the spread (min, max), ``export_timing()`` of every device call."""
import argparse
import io
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import plastid_amd as pa  # noqa: E402
from plastid_amd import synth  # noqa: E402
from plastid_amd.engine import STRAND_CODE  # noqa: E402


class Sink(io.RawIOBase):
    """A binary file that counts what it is given."""
    n = 0

    def writable(self):
        return True

    def write(self, b):
        self.n += len(b)
        return len(b)


class TextSink(object):
    """A text file that counts what it is given."""
    n = 0

    def write(self, s):
        self.n += len(s)


def loop_to_bedgraph(ga, fh, trackname, strand, window_size=100000):
    """The export this change replaced: per chromosome one count, the GPU run-length encoder, the run table to the host,
    a Python loop over the lines."""
    fh.write("track type=bedGraph name=%s\n" % trackname)
    for chrom in sorted(ga.chroms()):
        size = ga.lengths()[chrom]
        if size <= 0:
            continue
        ga._sync_engine([(chrom, 0, size, strand)])
        plan = ga._engine.plan([ga._chrom_index[chrom]], [0], [size], [STRAND_CODE[strand]], [0], np.ones(1, np.int8), [size], size, 1)
        plan.launch(ga._out_dtype())
        starts, values = plan.rle(window_size)
        plan.close()
        ends = np.append(starts[1:], size)
        keep = values > 0
        for a, b, v in zip(starts[keep], ends[keep], values[keep]):
            fh.write("%s\t%s\t%s\t%s\n" % (chrom, a, b, v))


def host_to_genome_array(bga):
    """``to_genome_array`` through the host: every vector read back and uploaded again by ``__setitem__``."""
    ga = pa.GenomeArray(chr_lengths=bga.lengths(), strands=bga.strands())
    for chrom in bga.chroms():
        for strand in bga.strands():
            seg = pa.GenomicSegment(chrom, 0, bga.lengths()[chrom] - 1, strand)
            ga[seg] = bga[seg]
    return ga


def note(what):
    print("[exp_bam_export] %s" % what, file=sys.stderr, flush=True)


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def summary(ms):
    return {"median": statistics.median(ms), "min": min(ms), "max": max(ms), "all": ms}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=0.1)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    genome, tx, reads, _ = synth.make_config("C2", scale=a.scale, tx_scale=0.001)
    res = {"reads": int(reads.n), "positions": int(sum(reads.lengths)), "repeat": a.repeat}
    note("%d reads made" % reads.n)
    bga = pa.BAMGenomeArray(reads, mapping=pa.FivePrimeMapFactory(12))
    note("staged")

    # ---- the same text, once
    new, old = io.StringIO(), io.StringIO()
    bga.to_bedgraph(new, "exp", "+")
    loop_to_bedgraph(bga, old, "exp", "+")
    res["texts_equal"] = new.getvalue() == old.getvalue()
    res["text_bytes"] = len(new.getvalue())
    res["export_stats"] = bga.export_stats()
    del new, old

    note("texts compared: %s, %d bytes" % (res["texts_equal"], res["text_bytes"]))
    # ---- alternating timed calls (the comparison above was the untimed call of both)
    dev, loop, laps = [], [], []
    for _ in range(a.repeat):
        sink = Sink()
        dev.append(timed(lambda: bga.to_bedgraph(sink, "exp", "+"))[0])
        laps.append(bga.export_timing())
        text = TextSink()
        loop.append(timed(lambda: loop_to_bedgraph(bga, text, "exp", "+"))[0])
        res["sink_bytes"] = [sink.n, text.n]
    res["device_export_ms"] = summary(dev)
    res["device_export_laps_ms"] = laps
    res["loop_export_ms"] = summary(loop)

    note("exports timed")
    # ---- to_genome_array
    ga_dev = bga.to_genome_array(array_type=pa.GenomeArray)
    ga_host = host_to_genome_array(bga)
    a_txt, b_txt = io.StringIO(), io.StringIO()
    ga_dev.to_bedgraph(a_txt, "exp", "+")
    ga_host.to_bedgraph(b_txt, "exp", "+")
    res["arrays_equal"] = a_txt.getvalue() == b_txt.getvalue() and ga_dev.sum() == ga_host.sum() and dict(ga_dev.lengths()) == dict(ga_host.lengths())
    res["array_sum"] = ga_dev.sum()
    del a_txt, b_txt
    ga_dev.close()
    ga_host.close()
    d2d, via_host = [], []
    for _ in range(a.repeat):
        ms, g = timed(lambda: bga.to_genome_array(array_type=pa.GenomeArray))
        d2d.append(ms)
        g.close()
        ms, g = timed(lambda: host_to_genome_array(bga))
        via_host.append(ms)
        g.close()
    res["device_to_genome_array_ms"] = summary(d2d)
    res["host_to_genome_array_ms"] = summary(via_host)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
