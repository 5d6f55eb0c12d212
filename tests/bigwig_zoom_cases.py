"""The cases of the bigWig ZOOM LEVELS (``zoom=`` of write_bigwig / GenomeArray.to_bigwig), shared by the CPU tests
(test_bigwig_zoom_host.py), the GPU tests (test_gpu_bigwig_zoom.py) and the fixture of Kent's reader
(golden/make_bigwig_zoom_golden.py), and ``expected_zoom``: an independent restatement of what a level is, computed from
the cells with numpy and Python floats.  Nothing here calls the library.

What a level is (csrc/bigwig_write_host.h, "zoom levels"): reductions ``r_k = r0 * 4**k`` (at most 10, ``r_k <= 2**30``);
window ``w`` of level ``k`` on a contig covers ``[w r_k, min((w + 1) r_k, size))``; level 0 takes every window's overlap
with the ITEMS in order (float64 sums over the float32 values), level k + 1 adds level k's float64 accumulators, four
children in order, the empty ones skipped; a window with ``valid > 0`` is a 32-byte record, cast to float32 there alone;
level 0 is written when the file has items, level k while it has fewer records than level k - 1; every
``min(items_per_slot, 768)`` records of a contig make one block.

Integer cases hold values in {1, 2, 3, 5} on contigs of at most 600 000 positions: every window's sum and sum of squares
stays below 2^24 (25 x 600 000 = 1.5 x 10^7) and is exact in float32, so Kent's reader must return exactly what the cells give."""
import collections
import math
import struct
import zlib

import numpy as np

from tests import bigwig_write_cases as wc

Contig = wc.Contig
MAX_LEVELS, MAX_REDUCTION, AUTO_CAP, RECORD, MAX_BLOCK_RECORDS = 10, 2 ** 30, 2 ** 20, 32, 768
NAN_BITS = 0x7fc00000
GRID = [(ips, bs, comp) for ips in (1, 2, 1024) for bs in (2, 256) for comp in (True, "dynamic", False)]
ZoomCase = collections.namedtuple("ZoomCase", "contigs zoom integer")


def _every_window(n_windows, r, rng, values=(1.0, 2.0, 3.0, 5.0)):
    """Cells of n_windows x r positions with at least one written cell in every window of r."""
    cells = np.zeros(n_windows * r, np.float64)
    at = np.arange(n_windows) * r + rng.integers(0, r, n_windows)
    cells[at] = rng.choice(values, n_windows)
    extra = rng.integers(0, len(cells), n_windows // 2)
    cells[extra] = rng.choice(values, len(extra))
    return cells


def _wide_items(size, rng, lo, hi, values=(1.0, 2.0, 3.0, 5.0)):
    """Items of lo .. hi - 1 cells, a gap behind some, neighbours of different value."""
    cells = np.zeros(size, np.float64)
    at, last = int(rng.integers(0, hi)), None
    while at < size:
        n = int(rng.integers(lo, hi))
        v = values[int(rng.integers(0, len(values)))]
        if v == last:
            v = values[(values.index(v) + 1) % len(values)]
        cells[at:at + n] = v
        last = v
        at += n
        if rng.random() < 0.3:
            at += int(rng.integers(1, 3 * hi))
            last = None
    return cells


def cases():
    rng = np.random.default_rng(4242)
    out = collections.OrderedDict()

    # r0 = 8: the edges of the grid
    g = collections.OrderedDict()
    short = np.array([0.0, 2.0, 2.0, 0.0, 1.0])
    g["a_short"] = Contig(5, short, True)                                   # a contig shorter than r0
    exact = np.zeros(24, np.float64)
    exact[4:8] = 3.0                                                        # an item that ends on a window edge
    exact[9:24] = 2.0                                                       # windows 1 and 2, up to the contig's end
    g["b_exact"] = Contig(24, exact, True)                                  # size = 3 r0
    g["c_empty"] = Contig(40, np.zeros(40, np.float64), True)               # an empty contig between two with data
    plus1 = np.zeros(25, np.float64)
    plus1[7:24] = 5.0                                                       # an item over three windows: 0, 1, 2
    plus1[24] = 1.0                                                         # the last window holds one position
    g["d_plus1"] = Contig(25, plus1, True)                                  # size = 3 r0 + 1
    g["e_768"] = Contig(768 * 8, _every_window(768, 8, rng), True)          # 768 records at level 0: one block of 768
    g["f_769"] = Contig(769 * 8 + 3, _every_window(769, 8, rng), True)      # 769: a block of 768 and one of 1; cells end before the size
    g["g_beyond"] = Contig(10, np.concatenate([np.zeros(12), [2.0, 2.0, 3.0]]), True)     # cells beyond the reported length
    out["grid8"] = ZoomCase(g, 8, True)
    for k in ("a_short", "d_plus1", "f_769"):
        out["grid8_" + k] = ZoomCase(collections.OrderedDict([(k, g[k])]), 8, True)        # a_short: level 1 has level 0's one record

    # the automatic first reduction: items of 30 .. 59 cells on one contig, single cells on the other
    a = collections.OrderedDict()
    a["wide"] = Contig(60000, _wide_items(60000, rng, 30, 60), True)
    a["single"] = Contig(3001, np.concatenate([np.tile([0.0, 1.0, 0.0, 2.0], 750), [3.0]]), True)
    out["auto"] = ZoomCase(a, True, True)
    out["auto_single"] = ZoomCase(collections.OrderedDict([("single", a["single"])]), True, True)     # valid // items = 1: r0 = 40

    # a larger grid: 9 375 windows at level 0, many workgroups and six levels
    w = collections.OrderedDict()
    w["chrL"] = Contig(600000, _wide_items(600000, rng, 1, 40), True)
    w["chrS"] = Contig(2 * 64 * 4 + 1, _wide_items(2 * 64 * 4 + 1, rng, 1, 9), True)
    out["wide64"] = ZoomCase(w, 64, True)

    # values that are not small integers
    s = collections.OrderedDict()
    sp = np.zeros(96, np.float64)
    sp[0:3] = [-1.5, -1.5, 0.25]                                            # negative values
    sp[8:16] = np.nan                                                       # an all-NaN window (eight items)
    sp[16:19] = [np.nan, 4.0, -0.0]                                         # a NaN item beside a number
    sp[24:32] = 0.1                                                         # a fraction: the order of the sums shows
    sp[32:40] = [0.1, 0.2, 0.3, 0.1, 0.7, 1e-3, 0.9, 0.1]
    sp[40:48] = 2.0 ** 24 + 2                                               # a sum above 2^24: the cast rounds
    sp[48:50] = [np.inf, -np.inf]                                           # the sum is NaN
    sp[56:58] = [1e30, 1e-30]                                               # the sum of squares overflows float32
    sp[64:66] = [-1e-50, 1e-50]                                             # cast to -0.0 and +0.0
    sp[72:80] = 16777217.0                                                  # 2^24 + 1 as a double, 2^24 as float32
    s["special"] = Contig(96, sp, False)
    frac = np.round(rng.random(5000) * 40) / 30.0 * (rng.random(5000) < 0.7)
    s["fractions"] = Contig(5000, frac, False)
    big = _every_window(300, 8, rng, values=(3.0e7, 16777217.0, 0.1, -5.0e6))
    s["big"] = Contig(2400, big, False)
    out["special8"] = ZoomCase(s, 8, False)

    # the largest first reduction: four candidate levels, one window each
    out["first_max"] = ZoomCase(collections.OrderedDict([("m", Contig(1000, _wide_items(1000, rng, 1, 9), True))]), 2 ** 24, True)
    # a file without items: no levels, the bytes of zoom=False
    out["no_items"] = ZoomCase(collections.OrderedDict([("e", Contig(50, np.zeros(50, np.float64), True)), ("a", Contig(7, np.zeros(0, np.float64), True))]), True, True)
    return out


def integer_cases():
    return [k for k, v in cases().items() if v.integer and k != "no_items"]


# ---------------------------------------------------------------------------------------------------------------------
# the restatement

def _order_key(x):
    """The order min and max are taken in: by value, -0.0 below +0.0."""
    return (x, 0 if math.copysign(1.0, x) < 0 else 1)


class Acc(object):
    __slots__ = ("valid", "lo", "hi", "sum", "sumsq")

    def __init__(self):
        self.valid, self.lo, self.hi, self.sum, self.sumsq = 0, None, None, 0.0, 0.0

    def copy(self):
        c = Acc()
        c.valid, c.lo, c.hi, c.sum, c.sumsq = self.valid, self.lo, self.hi, self.sum, self.sumsq
        return c


def first_reduction(zoom, items, valid):
    if zoom is True:
        return min(4 * max(10, valid // items), AUTO_CAP)
    return int(zoom)


def _level0(cells, size, r):
    """{window: Acc} of one contig from its items in order."""
    acc = {}
    for a, b, f in wc.expected_items(cells):
        v = float(f)
        for w in range(a // r, (b - 1) // r + 1):
            o = min(b, (w + 1) * r, size) - max(a, w * r)
            x = acc.setdefault(w, Acc())
            x.valid += o
            if v == v:
                if x.lo is None or _order_key(v) < _order_key(x.lo):
                    x.lo = v
                if x.hi is None or _order_key(v) > _order_key(x.hi):
                    x.hi = v
            with np.errstate(all="ignore"):
                x.sum = float(np.float64(x.sum) + np.float64(v) * np.float64(o))
                x.sumsq = float(np.float64(x.sumsq) + np.float64(v) * np.float64(v) * np.float64(o))
    return acc


def _level_up(below):
    acc = {}
    for w in sorted(below):
        c = below[w]
        if w // 4 not in acc:
            acc[w // 4] = c.copy()
            continue
        x = acc[w // 4]
        x.valid += c.valid
        if c.lo is not None and (x.lo is None or _order_key(c.lo) < _order_key(x.lo)):
            x.lo = c.lo
        if c.hi is not None and (x.hi is None or _order_key(c.hi) > _order_key(x.hi)):
            x.hi = c.hi
        with np.errstate(all="ignore"):
            x.sum = float(np.float64(x.sum) + np.float64(c.sum))
            x.sumsq = float(np.float64(x.sumsq) + np.float64(c.sumsq))
    return acc


def f32_bits(x):
    """The float32 nearest to the double x (ties to even) as its bits; NaN, and None (no number), as 0x7fc00000."""
    if x is None or x != x:
        return NAN_BITS
    with np.errstate(over="ignore", under="ignore"):
        return int(np.array([x], np.float64).astype(np.float32).view(np.uint32)[0])


Level = collections.namedtuple("Level", "reduction chrom_id start end valid min max sum sumsq")     # min .. sumsq: float32 bits


def expected_zoom(case):
    """The levels the file of `case` must hold: ``[Level]``, records in (chrom_id, start) order."""
    contigs, zoom = case.contigs, case.zoom
    names = sorted(contigs)
    items = [wc.expected_items(contigs[k].cells) for k in names]
    n = sum(len(x) for x in items)
    if not n or zoom is False:
        return []
    r0 = first_reduction(zoom, n, sum(b - a for x in items for a, b, _ in x))
    levels, accs, r = [], None, r0
    while len(levels) < MAX_LEVELS and r <= MAX_REDUCTION:
        sizes = [wc.contig_size(contigs[k]) for k in names]
        accs = [_level0(contigs[k].cells, s, r) for k, s in zip(names, sizes)] if accs is None else [_level_up(a) for a in accs]
        rows = [(c, w * r, min((w + 1) * r, sizes[c]), a[w]) for c, a in enumerate(accs) for w in sorted(a)]
        assert all(x.valid > 0 for _, _, _, x in rows)
        if levels and len(rows) >= len(levels[-1].chrom_id):
            break
        levels.append(Level(r, np.array([x[0] for x in rows], np.uint32), np.array([x[1] for x in rows], np.uint32), np.array([x[2] for x in rows], np.uint32),
                            np.array([x[3].valid for x in rows], np.uint32), np.array([f32_bits(x[3].lo) for x in rows], np.uint32),
                            np.array([f32_bits(x[3].hi) for x in rows], np.uint32), np.array([f32_bits(x[3].sum) for x in rows], np.uint32),
                            np.array([f32_bits(x[3].sumsq) for x in rows], np.uint32)))
        r *= 4
    return levels


def expected_blocks(level, ips):
    """``[(chrom_id, first record, records)]`` of a level: min(ips, 768) records of a contig each."""
    per, out = min(ips, MAX_BLOCK_RECORDS), []
    for c in np.unique(level.chrom_id):
        at = np.flatnonzero(level.chrom_id == c)
        out += [(int(c), int(at[0]) + a, min(per, len(at) - a)) for a in range(0, len(at), per)]
    return out


def table_bits(t):
    """A BigWigZoomTable as the tuple of uint32 arrays a Level holds behind its reduction."""
    return (t.chrom_id, t.start, t.end, t.valid) + tuple(np.asarray(x, np.float32).view(np.uint32) for x in (t.min, t.max, t.sum, t.sumsq))


def host_array(case, strand="+"):
    return wc.host_array(case.contigs, strand)


# ---------------------------------------------------------------------------------------------------------------------
# the container, read with struct + zlib

def zoom_headers(image):
    """``[(reduction, reserved, dataOffset, indexOffset)]`` of the zoom headers at offset 64."""
    n = struct.unpack("<H", image[6:8])[0]
    return [struct.unpack("<IIQQ", image[64 + 24 * k:88 + 24 * k]) for k in range(n)]


def rtree_leaves(image, index):
    """``(fan-out, item count, [(startChrom, startBase, endChrom, endBase, offset, size)] in walk order, end of the tree)``."""
    magic, fan, count, _, _, _, _, end_off, per_slot, _ = struct.unpack("<IIQIIIIQII", image[index:index + 48])
    assert magic == 0x2468ACE0 and end_off == index and per_slot == 1
    leaves, top = [], [index + 48]

    def walk(off):
        leaf, _, n = struct.unpack("<BBH", image[off:off + 4])
        assert 1 <= n <= fan
        top[0] = max(top[0], off + 4 + n * (32 if leaf else 24))
        for k in range(n):
            if leaf:
                leaves.append(struct.unpack("<IIIIQQ", image[off + 4 + 32 * k:off + 36 + 32 * k]))
            else:
                walk(struct.unpack("<Q", image[off + 4 + 24 * k + 16:off + 4 + 24 * k + 24])[0])
    if count:
        walk(index + 48)
    return fan, count, leaves, top[0]


def read_level(image, header):
    """``(record count, [raw block bytes], leaves, end of the level)`` of one zoom level."""
    buf = struct.unpack("<I", image[52:56])[0]
    _, _, data, index = header
    count = struct.unpack("<I", image[data:data + 4])[0]
    _, _, leaves, end = rtree_leaves(image, index)
    blocks = []
    for leaf in leaves:
        raw = image[leaf[4]:leaf[4] + leaf[5]]
        blocks.append(zlib.decompress(raw) if buf else raw)
    return count, blocks, leaves, end
