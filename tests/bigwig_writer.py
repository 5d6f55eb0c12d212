"""A bigWig writer for the tests (the project's own, like tests/bam_writer.py): a file from a list of sections, with the
knobs the kernels' seams need -- items per block, the fan-out of both trees, the zlib level per block or no compression
at all, an ``uncompressBufSize`` declared larger than any block, items in any order and overlapping, and a hook that
damages the finished image.  No zoom levels (``zoomLevels = 0``), no total summary.  Layout: header (64 bytes), chromosome
B+ tree, data (u64 section count, then the blocks back to back), R-tree, the magic once more (Kent's bbiFileCheckSigs looks
for it there).

A section is ``Section(chrom_id, kind, items, span=1, step=1, start=0)``: kind ``"bedgraph"`` with items ``(start, end,
value)``, ``"variable"`` with ``(start, value)`` and `span`, ``"fixed"`` with values alone and `start`, `step`, `span`.
One section becomes one block, or several of at most `items_per_block` items each (a fixedStep section's later blocks
start where the earlier ones end)."""
import collections
import struct
import zlib

import numpy as np

MAGIC, BPT_MAGIC, CIR_MAGIC = 0x888FFC26, 0x78CA8C91, 0x2468ACE0
KINDS = {"bedgraph": 1, "variable": 2, "fixed": 3}
Section = collections.namedtuple("Section", "chrom_id kind items span step start")
Section.__new__.__defaults__ = (1, 1, 0)
Layout = collections.namedtuple("Layout", "chrom_tree data index blocks raw_sizes")


def cut(sections, items_per_block):
    """The sections cut into blocks of at most `items_per_block` items (None: a block per section)."""
    out = []
    for s in sections:
        n = len(s.items)
        per = n if not items_per_block else items_per_block
        if n == 0:
            out.append(s)
        for a in range(0, n, max(per, 1)):
            out.append(s._replace(items=s.items[a:a + per], start=s.start + a * s.step if s.kind == "fixed" else s.start))
    return out


ITEM_DTYPES = {1: np.dtype([("start", "<u4"), ("end", "<u4"), ("value", "<f4")]), 2: np.dtype([("start", "<u4"), ("value", "<f4")]), 3: np.dtype("<f4")}


def section_bytes(s):
    """A block's raw bytes: the 24-byte header and the items; and its bounds (start, end) on the contig.  The items may be
    a list of tuples (of floats: fixedStep) or a numpy array of ITEM_DTYPES."""
    t = KINDS[s.kind]
    items = s.items if isinstance(s.items, np.ndarray) else np.array(list(s.items), ITEM_DTYPES[t])
    n = len(items)
    if t == 1:
        lo, hi = (int(items["start"].min()), int(items["end"].max())) if n else (0, 0)
    elif t == 2:
        lo, hi = (int(items["start"].min()), int(items["start"].max()) + s.span) if n else (0, 0)
    else:
        lo, hi = s.start, s.start + max(n - 1, 0) * s.step + s.span
    head = struct.pack("<IIIIIBBH", s.chrom_id, lo, hi, s.step, s.span, t, 0, n)
    return head + items.astype(ITEM_DTYPES[t], copy=False).tobytes(), (lo, hi)


def _tree(leaves, fanout, leaf_item, node_item, first_offset):
    """A tree over `leaves` (any objects) with at most `fanout` items per node, root first, level by level.
    leaf_item(leaf) -> bytes; node_item(children summary, child offset) -> bytes; a node's summary is the list of its leaves.
    Returns the bytes; an empty tree is no bytes."""
    if not leaves:
        return b""
    fanout = max(int(fanout), 2)
    levels = [[leaves[a:a + fanout] for a in range(0, len(leaves), fanout)]]      # the leaf level: groups of leaves
    spans = [[list(g) for g in levels[0]]]                                        # the leaves under every node
    while len(levels[-1]) > 1:
        prev = list(range(len(levels[-1])))
        groups = [prev[a:a + fanout] for a in range(0, len(prev), fanout)]
        levels.append(groups)
        spans.append([[x for k in g for x in spans[-1][k]] for g in groups])
    levels.reverse()
    spans.reverse()
    # sizes, then offsets: the nodes stand root first, level by level
    leaf_size = len(leaf_item(leaves[0]))
    node_size = len(node_item(spans[-1][0], 0))
    offsets, at = [], first_offset
    for depth, lv in enumerate(levels):
        is_leaf = depth == len(levels) - 1
        row = []
        for g in lv:
            row.append(at)
            at += 4 + len(g) * (leaf_size if is_leaf else node_size)
        offsets.append(row)
    out = b""
    for depth, lv in enumerate(levels):
        is_leaf = depth == len(levels) - 1
        for g in lv:
            out += struct.pack("<BBH", 1 if is_leaf else 0, 0, len(g))
            if is_leaf:
                out += b"".join(leaf_item(x) for x in g)
            else:
                out += b"".join(node_item(spans[depth + 1][k], offsets[depth + 1][k]) for k in g)
    return out


def write_bigwig(chroms, sections, items_per_block=None, fanout=256, chrom_fanout=256, level=6, buf_factor=1, version=4, damage=None,
                 edit_raw=None, packed=None, return_layout=False):
    """The image of a bigWig file.  `chroms`: ``[(name, size)]`` -- ids are the places in the list, which is the order of
    the tree's leaves (Kent's own reader searches the tree by name: give it sorted names) -- or ``[(name, id, size)]``.
    `level`: the zlib level of every block, a list the blocks take in turn, or None: stored blocks, ``uncompressBufSize = 0``.
    `buf_factor`: ``uncompressBufSize`` is this many times the largest block.  `edit_raw`: ``{block: f}``, f(bytearray of the
    block's section) -> the bytes to store instead (a damaged header or item, compressed like any other).
    `packed`: ``{block: zlib stream}`` stored for the block as given (a hand-built DEFLATE stream of the block's section).
    `damage(image: bytearray, layout)`: called on the finished image."""
    chroms = [(c[0], k, c[1]) if len(c) == 2 else tuple(c) for k, c in enumerate(chroms)]
    blocks = cut(sections, items_per_block)
    raws, bounds = [], []
    for s in blocks:
        raw, (lo, hi) = section_bytes(s)
        raws.append(raw)
        bounds.append((s.chrom_id, lo, s.chrom_id, hi))
    raws = [bytes(edit_raw[k](bytearray(r))) if edit_raw and k in edit_raw else r for k, r in enumerate(raws)]
    levels = [level[k % len(level)] for k in range(len(raws))] if isinstance(level, (list, tuple)) else [level] * len(raws)
    stored = level is None
    given = packed or {}
    packed = [given[k] if k in given else (r if stored else zlib.compress(r, lv)) for k, (r, lv) in enumerate(zip(raws, levels))]
    assert all(zlib.decompress(given[k]) == raws[k] for k in given), "a given stream does not inflate to its block's section"
    buf = 0 if stored else max([len(r) for r in raws] or [0]) * buf_factor
    key_size = max([len(n.encode()) for n, _, _ in chroms] or [1])
    chrom_tree = 64
    tree = struct.pack("<IIIIQII", BPT_MAGIC, max(chrom_fanout, 2), key_size, 8, len(chroms), 0, 0)
    tree += _tree(chroms, chrom_fanout, lambda c: c[0].encode().ljust(key_size, b"\0") + struct.pack("<II", c[1], c[2]),
                  lambda under, off: under[0][0].encode().ljust(key_size, b"\0") + struct.pack("<Q", off), chrom_tree + 32)
    data = chrom_tree + len(tree)
    at, placed = data + 8, []
    for p in packed:
        placed.append((at, len(p)))
        at += len(p)
    index = at

    def bound(under):
        lo = min((b[0], b[1]) for _, b in under)
        hi = max((b[2], b[3]) for _, b in under)
        return struct.pack("<IIII", lo[0], lo[1], hi[0], hi[1])

    leaves = list(zip(placed, bounds))
    whole = bound(leaves) if leaves else struct.pack("<IIII", 0, 0, 0, 0)
    cir = struct.pack("<IIQ", CIR_MAGIC, max(fanout, 2), len(leaves)) + whole + struct.pack("<QII", index, 1, 0)
    cir += _tree(leaves, fanout, lambda x: struct.pack("<IIII", *x[1]) + struct.pack("<QQ", x[0][0], x[0][1]),
                 lambda under, off: bound(under) + struct.pack("<Q", off), index + 48)
    header = struct.pack("<IHHQQQHHQQIQ", MAGIC, version, 0, chrom_tree, data, index, 0, 0, 0, 0, buf, 0)
    assert len(header) == 64
    image = bytearray(header + tree + struct.pack("<Q", len(packed)) + b"".join(packed) + cir + struct.pack("<I", MAGIC))
    layout = Layout(chrom_tree, data, index, placed, [len(r) for r in raws])
    if damage is not None:
        damage(image, layout)
    return (bytes(image), layout) if return_layout else bytes(image)


# ---------------------------------------------------------------------------------------------------------------------
# a reader of its own (struct + zlib), so that the writer is not judged by the code under test

def read_model(image):
    """``(chroms [(name, id, size)] in leaf order, blocks [(offset, size)] in index order, items [(chrom_id, start, end,
    value float32-as-float, block)])`` of a file this writer (or Kent's) wrote."""
    magic, version, zooms, ct, data, index, _, _, _, _, buf, _ = struct.unpack("<IHHQQQHHQQIQ", image[:64])
    assert magic == MAGIC
    _, _, key_size, val_size, count, _, _ = struct.unpack("<IIIIQII", image[ct:ct + 32])
    chroms, blocks, items = [], [], []

    def walk_chroms(off):
        leaf, _, n = struct.unpack("<BBH", image[off:off + 4])
        for k in range(n):
            p = off + 4 + k * (key_size + 8)
            if leaf:
                cid, size = struct.unpack("<II", image[p + key_size:p + key_size + 8])
                chroms.append((image[p:p + key_size].split(b"\0")[0].decode(), cid, size))
            else:
                walk_chroms(struct.unpack("<Q", image[p + key_size:p + key_size + 8])[0])

    def walk_index(off):
        leaf, _, n = struct.unpack("<BBH", image[off:off + 4])
        for k in range(n):
            if leaf:
                blocks.append(struct.unpack("<QQ", image[off + 4 + k * 32 + 16:off + 4 + k * 32 + 32]))
            else:
                walk_index(struct.unpack("<Q", image[off + 4 + k * 24 + 16:off + 4 + k * 24 + 24])[0])

    if count:
        walk_chroms(ct + 32)
    if struct.unpack("<Q", image[index + 8:index + 16])[0]:
        walk_index(index + 48)
    for b, (off, size) in enumerate(blocks):
        raw = image[off:off + size]
        if buf:
            raw = zlib.decompress(raw)
        cid, start, _, step, span, t, _, n = struct.unpack("<IIIIIBBH", raw[:24])
        assert len(raw) == 24 + n * {1: 12, 2: 8, 3: 4}[t]
        for k in range(n):
            if t == 1:
                a, e, v = struct.unpack("<IIf", raw[24 + 12 * k:36 + 12 * k])
            elif t == 2:
                a, v = struct.unpack("<If", raw[24 + 8 * k:32 + 8 * k])
                e = a + span
            else:
                v, = struct.unpack("<f", raw[24 + 4 * k:28 + 4 * k])
                a = start + k * step
                e = a + span
            items.append((cid, a, e, v, b))
    return chroms, [tuple(int(x) for x in b) for b in blocks], items
