"""The bigWig cases of tests/golden/bigwig_fixture.npz, shared by its generator (tests/golden/make_bigwig_golden.py) and by
tests/test_bigwig_host.py / tests/test_gpu_bigwig.py: the texts Kent's writer turns into files, the files
tests/bigwig_writer.py writes (overlaps inside a block and across blocks: Kent's writer refuses those), the
BigWigGenomeArray configurations, and the kernel-seam files of the GPU test.

Every value is a multiple of 2^-10 below 2^5 and every file holds fewer than 2^20 covered positions, so every total is a
multiple of 2^-10 below 2^40: any summation order gives the same bits (the generator asserts sequential == math.fsum)."""
import collections
import os
import random

import numpy as np

from tests import bigwig_writer as bw

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "bigwig_fixture.npz")
SIZES = collections.OrderedDict([("chrA", 3000), ("chrB", 1200), ("chrC", 2500)])     # chrB is shorter than chrA: the sum() quirk shows
S = bw.Section


def val(rng):
    return rng.randrange(1, 1 << 15) / 1024.0


def bedgraph_text(rng, chrom, size, n, first=0):
    """n bedGraph lines on `chrom`, ascending, without overlap."""
    out, at = [], first
    for _ in range(n):
        at += rng.randrange(0, 4)
        ln = rng.choice([1, 1, 2, 3, 32, 33, 40])
        if at + ln > size:
            break
        out.append("%s\t%d\t%d\t%r" % (chrom, at, at + ln, val(rng)))
        at += ln
    return "\n".join(out) + "\n"


def variable_text(rng, chrom, size, n, span, first=1):
    out, at = ["variableStep chrom=%s span=%d" % (chrom, span)], first
    for _ in range(n):
        at += rng.randrange(0, 3) * span
        if at - 1 + span > size:
            break
        out.append("%d\t%r" % (at, val(rng)))
        at += span
    return "\n".join(out) + "\n"


def fixed_text(rng, chrom, size, n, start, step, span):
    n = min(n, (size - (start - 1) - span) // step + 1)
    return "fixedStep chrom=%s start=%d step=%d span=%d\n" % (chrom, start, step, span) + "".join("%r\n" % val(rng) for _ in range(n))


def kent_texts():
    """name -> (wiggle text, itemsPerSlot, blockSize, compress) for Kent's bigWigFileCreate."""
    rng = random.Random(20261020)
    one = bedgraph_text(rng, "chrA", SIZES["chrA"], 300)
    mixed = (bedgraph_text(rng, "chrA", 1500, 120) + fixed_text(rng, "chrA", SIZES["chrA"], 150, 1601, 7, 3) +
             variable_text(rng, "chrB", SIZES["chrB"], 130, 5) + fixed_text(rng, "chrC", 1000, 200, 11, 1, 1) +
             variable_text(rng, "chrC", SIZES["chrC"], 100, 1, first=1200) + bedgraph_text(rng, "chrC", SIZES["chrC"], 60, first=2000))
    return collections.OrderedDict([
        ("kent_one", (one, 1024, 256, 1)),
        ("kent_mixed", (mixed, 1024, 256, 1)),
        ("kent_two_per_block", (mixed, 2, 4, 1)),          # a few hundred items, two per block: an R-tree of several levels
        ("kent_stored", (mixed, 64, 256, 0)),
    ])


def chrom_sizes_text():
    return "".join("%s\t%d\n" % kv for kv in SIZES.items())


def python_files():
    """name -> image, written by tests/bigwig_writer.py: what Kent's writer refuses to write."""
    rng = random.Random(7)
    chroms = list(SIZES.items())
    # overlaps inside a block (items 0-2: the middle one the longest) and across blocks (the second block rewrites part of
    # the first; a later section of another type lands on both)
    over = [S(0, "bedgraph", [(100, 140, 1.5), (90, 400, 2.25), (120, 130, 3.0), (500, 501, 4.0)]),
            S(0, "bedgraph", [(395, 410, 5.5), (2990, 3000, 0.5)]),
            S(0, "fixed", [val(rng) for _ in range(40)], span=4, step=3, start=380),
            S(1, "variable", [(10, 1.0), (12, 2.0), (11, 3.0), (700, 4.0)], span=5),
            S(2, "bedgraph", [(0, 2500, 0.25)]),
            S(2, "variable", [(a, val(rng)) for a in range(5, 2400, 97)], span=33)]
    mixed = [S(0, "bedgraph", [(a, a + 2, val(rng)) for a in range(0, 600, 5)]),
             S(1, "fixed", [val(rng) for _ in range(100)], span=2, step=11, start=3),
             S(2, "variable", [(a, val(rng)) for a in range(1, 2400, 13)], span=7)]
    return collections.OrderedDict([
        ("py_overlaps", bw.write_bigwig(chroms, over, items_per_block=3, fanout=2, level=6)),
        ("py_mixed", bw.write_bigwig(chroms, mixed, items_per_block=50, fanout=4, chrom_fanout=2, level=[0, 1, 9])),
    ])


#: BigWigGenomeArray configurations: name -> [(strand, file)] in add_from_bigwig order
ARRAYS = collections.OrderedDict([
    ("one", [("+", "kent_one")]),
    ("stranded", [("+", "kent_mixed"), ("-", "py_overlaps")]),
    ("two_readers", [("+", "kent_two_per_block"), ("+", "py_overlaps"), ("-", "kent_one"), ("+", "py_mixed")]),
    ("stored", [("-", "kent_stored"), ("-", "py_mixed")]),
])


def query_segments(seed):
    """(chrom, start, end) of the segments every array is asked for, on each of '+', '-' and '.'; and chains as lists of such."""
    rng = random.Random(seed)
    segs = [("chrA", 0, 3000), ("chrB", 0, 1200), ("chrC", 2400, 2500), ("chrA", 85, 505), ("chrZ", 5, 25), ("chrB", 1190, 1260)]
    for _ in range(10):
        c = rng.choice(list(SIZES))
        a = rng.randrange(0, SIZES[c] - 1)
        segs.append((c, a, min(a + rng.randrange(1, 300), SIZES[c])))
    chains = [[("chrA", 10, 60), ("chrA", 100, 140), ("chrA", 390, 520)], [("chrC", 0, 40), ("chrC", 2000, 2100)], [("chrB", 5, 15)],
              [("chrZ", 0, 10), ("chrZ", 20, 30)]]
    return segs, chains


def load_fixture():
    return np.load(FIXTURE, allow_pickle=False)


def fixture_files(fx=None):
    """name -> image of every file of the fixture (Kent's and the writer's: the bytes Kent's readers were given)."""
    fx = load_fixture() if fx is None else fx
    return collections.OrderedDict((str(n), fx["file_" + str(n)].tobytes()) for n in fx["files"])
