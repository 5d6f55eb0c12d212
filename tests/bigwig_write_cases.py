"""The cases of the bigWig WRITER and of the zlib encoder under it, seeded and shared by the CPU tests (test_deflate_host.py,
test_bigwig_write_host.py) and the GPU tests (test_gpu_deflate.py, test_gpu_bigwig_write.py).

1. ``deflate_inputs()``: inputs of the encoder, each at most 24 600 bytes (``MAX_INPUT``), and ``many_inputs()``: 200 of
   mixed kinds for ONE call.  ``fixed_tokens`` reads a fixed-Huffman stream back into its tokens, so that a test can say
   which length and distance codes the inputs really reach.
2. ``array_contigs()``: the contigs of the `mixed` array, each also an array on its own; ``expected_items`` is the item
   list the writers must produce, computed here with numpy alone."""
import collections
import struct
import zlib

import numpy as np

MAX_INPUT = 24600
LENGTH_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LENGTH_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]


def hash4(data):
    """The encoder's hash (csrc/deflate_host.h: hash4) of every position p with p + 4 <= len(data), as an array."""
    b = np.frombuffer(bytes(data), np.uint8).astype(np.uint64)
    if len(b) < 4:
        return np.zeros(0, np.uint32)
    w = b[:-3] | (b[1:-2] << np.uint64(8)) | (b[2:-1] << np.uint64(16)) | (b[3:] << np.uint64(24))
    return (((w * np.uint64(2654435761)) & np.uint64(0xffffffff)) >> np.uint64(20)).astype(np.uint32)


def bedgraph_section(rng, n, dense=True, chrom=3):
    """A bedGraph section of n items with small integer counts, as the writer cuts them."""
    lens = rng.integers(1, 6, n) if dense else rng.integers(1, 3, n)
    gaps = np.where(rng.random(n) < (0.2 if dense else 0.8), rng.integers(1, 400, n), 0)
    starts = np.cumsum(lens + gaps) - lens + 100000
    items = np.zeros(n, np.dtype([("s", "<u4"), ("e", "<u4"), ("v", "<f4")]))
    items["s"], items["e"], items["v"] = starts, starts + lens, rng.poisson(3, n).astype(np.float32) + 1
    return struct.pack("<IIIIIBBH", chrom, int(starts[0]), int(starts[-1] + lens[-1]), 0, 0, 1, 0, n) + items.tobytes()


def run_text(lo, hi):
    """One run of every length lo .. hi of one byte, between separators of three bytes that occur once."""
    out = bytearray()
    for k, n in enumerate(range(lo, hi + 1)):
        out += bytes([0xF0 | (k >> 7), 0x80 | (k & 0x7F), 0xEF]) + bytes([k + 33]) * n
    return bytes(out)


def marker_text(rng):
    """A 4-byte marker of its own for every distance-code base, twice, that far apart, in a filler of zeros (random filler
    would send the whole input to the stored block) no position of which, between the two, hashes as the marker does: the
    second marker's candidate is the first."""
    n = MAX_INPUT
    data = np.zeros(n, np.uint8)
    fixed = np.zeros(n, bool)
    pairs = []
    for k, gap in enumerate(DIST_BASE):
        a = 1300 + 20 * k if gap < 4 else (0 if gap == DIST_BASE[-1] else 40 * (k + 1))
        if gap >= 4:
            marker = np.array([0xA0 + k, 0x5A, k, 0xC3], np.uint8)
            spots = (a, a + gap)
        else:                                      # (the two markers would overlap: a run of the gap's period instead)
            marker = None
            spots = ()
            unit = np.array([0x11 * (k + 1), 0x77, 0x99][:gap], np.uint8)
            data[a:a + 12] = np.resize(unit, 12)
            fixed[a:a + 12] = True
        for p in spots:
            assert not fixed[p:p + 4].any()
            data[p:p + 4] = marker
            fixed[p:p + 4] = True
        if marker is not None:
            pairs.append((a, gap))
    for _ in range(200):
        h = hash4(data)
        bad = np.zeros(n, bool)
        for a, gap in pairs:
            between = np.flatnonzero(h[a + 1:a + gap] == h[a]) + a + 1
            bad[between] = True
        todo = np.flatnonzero(bad)
        if not len(todo):
            break
        for p in todo:
            q = [x for x in range(p, min(p + 4, n)) if not fixed[x]]
            assert q
            data[q[0]] = rng.integers(1, 256)
    else:
        raise AssertionError("the filler keeps colliding")
    return data.tobytes()


def deflate_inputs():
    rng = np.random.default_rng(20240719)
    out = collections.OrderedDict()
    for n in range(6):
        out["len%d" % n] = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    for n in (257, 258, 259, 260, MAX_INPUT):
        out["repeat%d" % n] = bytes([0x41 + n % 7]) * n
    out["all_bytes_twice"] = bytes(range(256)) * 2
    out["runs_3_180"] = run_text(3, 180)
    out["runs_181_259"] = run_text(181, 259)
    out["markers"] = marker_text(rng)
    out["random12312"] = rng.integers(0, 256, 12312, dtype=np.uint8).tobytes()
    out["random24600"] = rng.integers(0, 256, MAX_INPUT, dtype=np.uint8).tobytes()
    for n in (1, 2, 1023, 1024, 2048):
        out["section%d" % n] = bedgraph_section(rng, n, dense=n % 2 == 0)
    assert all(len(v) <= MAX_INPUT for v in out.values())
    return out


def many_inputs(count=200):
    """`count` inputs of mixed kinds, lengths spread over 0 .. 24 600, for one call."""
    rng = np.random.default_rng(77)
    lens = np.concatenate([[0, 1, MAX_INPUT, 4, 5], rng.integers(0, MAX_INPUT + 1, count - 5)])
    out = []
    for k, n in enumerate(int(x) for x in lens):
        kind = k % 4
        if kind == 0:
            raw = (bedgraph_section(rng, max((n - 24) // 12, 1), dense=k % 8 == 0) + bytes(12))[:n]
        elif kind == 1:
            raw = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        elif kind == 2:
            raw = rng.integers(0, 4, n, dtype=np.uint8).tobytes()
        else:
            raw = (b"chr%d\t%d\t" % (k, k * 7) * (n // 8 + 1))[:n]
        assert len(raw) == n
        out.append(raw)
    return out


def fixed_tokens(stream):
    """The tokens of a zlib stream whose body is one fixed-Huffman block: ``[("lit", byte) | ("match", length, distance)]``;
    None for a stored block."""
    body = stream[2:-4]
    bits = np.unpackbits(np.frombuffer(body, np.uint8), bitorder="little")
    assert bits[0] == 1
    if bits[1] == 0 and bits[2] == 0:
        return None
    assert bits[1] == 1 and bits[2] == 0
    at = 3

    def take(n):          # n bits, first bit lowest
        nonlocal at
        v = int(sum(int(b) << i for i, b in enumerate(bits[at:at + n])))
        at += n
        return v

    def code(n):          # n bits, first bit highest
        nonlocal at
        v = 0
        for b in bits[at:at + n]:
            v = (v << 1) | int(b)
        at += n
        return v

    out = []
    while True:
        v = code(7)
        if v <= 0x17:
            sym = 256 + v
        else:
            v = (v << 1) | code(1)
            if 0x30 <= v <= 0xBF:
                sym = v - 0x30
            elif 0xC0 <= v <= 0xC7:
                sym = 280 + v - 0xC0
            else:
                sym = 144 + ((v << 1) | code(1)) - 0x190
        if sym == 256:
            break
        if sym < 256:
            out.append(("lit", sym))
            continue
        k = sym - 257
        length = LENGTH_BASE[k] + take(LENGTH_EXTRA[k])
        d = code(5)
        out.append(("match", length, DIST_BASE[d] + take(DIST_EXTRA[d])))
    assert (at + 7) // 8 == len(body)
    return out


def replay(tokens):
    out = bytearray()
    for t in tokens:
        if t[0] == "lit":
            out.append(t[1])
        else:
            for _ in range(t[1]):
                out.append(out[-t[2]])
    return bytes(out)


def check_stream(stream, raw):
    """What every stream must satisfy, whoever made it."""
    assert stream[:2] == b"\x78\x01" and len(stream) <= len(raw) + 11
    assert zlib.decompress(stream) == raw
    assert struct.unpack(">I", stream[-4:])[0] == zlib.adler32(raw)


# ---------------------------------------------------------------------------------------------------------------------
# arrays

EXPORT_TILE = 2048        # pc_track_export_geometry()[0]: the tests assert that it still is

Contig = collections.namedtuple("Contig", "length cells integer")


def _runs(n, rng, values=(1.0, 2.0, 3.0, 5.0)):
    """Cells of exactly n runs: runs of 1 .. 4 cells, neighbours of different value, a gap of zeros now and then."""
    out, last = [], None
    for k in range(n):
        v = values[int(rng.integers(0, len(values)))]
        gap = int(rng.integers(0, 3)) if k else 0
        if v == last and not gap:
            v = values[(values.index(v) + 1) % len(values)]
        out += [0.0] * gap + [v] * int(rng.integers(1, 5))
        last = v
    return np.array(out, np.float64)


def array_contigs():
    rng = np.random.default_rng(1234)
    c = collections.OrderedDict()
    special = np.zeros(64, np.float64)
    special[2:13] = [1.0, 2.0 ** 24 + 1, 0.1, -3.5, np.nan, np.nan, np.inf, -np.inf, 1e-50, 1e39, -0.0]
    special[20:22] = [1.0000000001, 1.0000000002]            # differ as doubles, cast to the same float32
    special[30:34] = [7.0, 7.0, -0.0, 7.0]                     # -0.0 is not written: it cuts the run
    special[40:42] = [-1e-50, 1e-50]                           # cast to -0.0 and +0.0: written, as cast
    special[44] = 1e-40                                        # a float32 denormal
    c["chr2"] = Contig(64, special, False)
    only0 = np.zeros(10, np.float64)
    only0[0] = 4.0
    c["chr10"] = Contig(10, only0, True)
    last = np.zeros(1000, np.float64)
    last[999] = 9.0
    c["chrM_long_name"] = Contig(1000, last, True)
    c["e"] = Contig(50, np.zeros(50, np.float64), True)
    beyond = np.zeros(150, np.float64)
    beyond[90:141] = 3.0
    c["beyond"] = Contig(100, beyond, True)
    c["runs1024"] = Contig(6000, _runs(1024, rng), True)
    c["runs1025"] = Contig(6000, _runs(1025, rng), True)
    n = 3 * EXPORT_TILE + 517
    long = np.zeros(n, np.float64)
    long[:] = np.repeat(rng.integers(0, 3, n // 7 + 1), 7)[:n]               # runs of 7 cells: they cross every border
    long[EXPORT_TILE - 300:EXPORT_TILE + 300] = 6.0                          # one run over a workgroup border
    long[2 * EXPORT_TILE - 1:2 * EXPORT_TILE + 1] = [8.0, 9.0]               # a run ends with a workgroup's last cell
    long[256 * 3 - 1:256 * 3 + 1] = 11.0
    c["long"] = Contig(n, long, True)
    singles = np.zeros(6100, np.float64)
    singles[np.arange(3000) * 2 + 1] = rng.integers(1, 9, 3000)
    c["singles"] = Contig(6100, singles, True)
    frac = np.round(rng.random(500) * 4) / 3.0
    c["fractions"] = Contig(500, frac, False)
    return c


def array_cases():
    """name -> OrderedDict(contig -> Contig): `mixed`, every contig on its own, `integers` (exact sums), `all_hold_items`
    (what Kent's writer, which drops a contig without items, numbers as we do) and `empty` (contigs without any item)."""
    contigs = array_contigs()
    out = collections.OrderedDict(mixed=contigs)
    for k, v in contigs.items():
        out[k] = collections.OrderedDict([(k, v)])
    out["integers"] = collections.OrderedDict((k, v) for k, v in contigs.items() if v.integer)
    out["all_hold_items"] = collections.OrderedDict((k, v) for k, v in contigs.items() if v.integer and k != "e")
    out["empty"] = collections.OrderedDict([("e", contigs["e"]), ("a", Contig(7, np.zeros(0, np.float64), True))])
    return out


def is_integer_case(case):
    return all(v.integer for v in case.values())


def host_array(case, strand="+", strands=("+", "-")):
    """The case as a host DenseGenomeArray: `strand` holds the cells, the other strands a decoy."""
    from plastid_amd.genome_array import DenseGenomeArray
    ga = DenseGenomeArray(collections.OrderedDict((k, v.length) for k, v in case.items()), strands)
    for k, v in case.items():
        for st in strands:
            ga._chroms[k][st] = v.cells.copy() if st == strand else np.full(max(v.length, 1), 5.0)
    return ga


def contig_size(v):
    return max(v.length, len(v.cells))


def expected_items(cells):
    """``[(start, end, float32 value)]`` of one contig's cells."""
    v = np.asarray(cells, np.float64)
    w = v != 0.0
    if not len(v):
        return []
    with np.errstate(invalid="ignore", over="ignore"):
        same = np.concatenate([[False], (v[1:] == v[:-1]) & w[1:] & w[:-1]])
        heads = np.flatnonzero(w & ~same)
        nxt = np.concatenate([same[1:], [False]])
        tails = np.flatnonzero(w & ~nxt)
        vals = v[heads].astype(np.float32)
    return [(int(a), int(b) + 1, f) for a, b, f in zip(heads, tails, vals)]


def expected_file_items(case):
    """``[(contig name, start, end, float32 value)]`` in file order: contigs sorted, items ascending."""
    return [(k, a, b, f) for k in sorted(case) for a, b, f in expected_items(case[k].cells)]


def expected_summary(case):
    """validCount, min, max (None without a number), and the terms of sumData and sumSquares."""
    items = expected_file_items(case)
    widths = [b - a for _, a, b, _ in items]
    vals = [float(f) for _, _, _, f in items]
    nums = [x for x in vals if x == x]
    return {"valid": sum(widths), "min": min(nums) if nums else None, "max": max(nums) if nums else None,
            "sum_terms": [x * w for x, w in zip(vals, widths)], "sq_terms": [x * x * w for x, w in zip(vals, widths)], "n": len(items)}


def file_summary(image):
    """(totalSummaryOffset, validCount, min, max, sumData, sumSquares) of a bigWig image."""
    off = struct.unpack("<Q", image[44:52])[0]
    if not off:
        return (0,)
    return (off,) + struct.unpack("<Qdddd", image[off:off + 40])


# ---------------------------------------------------------------------------------------------------------------------
# the fixture of Kent's library (tests/golden/make_bigwig_write_golden.py -> tests/golden/bigwig_write_fixture.npz)

# (not `e` and `empty`: a file without sections has the form tests/bigwig_writer.py gives it, an R-tree header without a
# root node, and Kent's block query reads a root node whatever the count says; Kent's own writer refuses to write such a file)
KENT_READS = [(name, 1024, 256, True) for name in ("chr10", "chrM_long_name", "beyond", "runs1024", "runs1025", "long", "singles", "fractions",
                                                    "integers", "all_hold_items")] + [("integers", 2, 2, True), ("integers", 1, 256, False),
                                                                                               ("fractions", 2, 2, False)]
KENT_WRITES = [(name, ips) for name in ("chr10", "chrM_long_name", "beyond", "runs1024", "runs1025", "long", "singles", "fractions", "all_hold_items")
               for ips in ((1, 2, 1024) if name in ("runs1025", "all_hold_items", "fractions") else (1024,))]
RECORDED = [("integers", 1024, 256, True), ("fractions", 2, 2, True), ("mixed", 1024, 256, True), ("empty", 1024, 256, True), ("singles", 1, 2, False)]


def key(name, ips, bs=None, comp=None):
    return "%s_%d" % (name, ips) if bs is None else "%s_%d_%d_%d" % (name, ips, bs, 1 if comp else 0)


def bedgraph_text(case):
    """OUR item list as the bedGraph text Kent's writer takes: nine significant digits bring every float32 back."""
    return "".join("%s\t%d\t%d\t%.9g\n" % (k, a, b, float(f)) for k, a, b, f in expected_file_items(case))


def data_region(image):
    """The bytes from unzoomedDataOffset to unzoomedIndexOffset: the section count and the sections."""
    data, index = struct.unpack("<QQ", image[16:32])
    return image[data:index]


def load_fixture():
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bigwig_write_fixture.npz"))
