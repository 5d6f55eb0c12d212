"""Shared by tests/test_bam_sort.py and tests/test_gpu_bam_sort.py: BAM files in shuffled record order, and for each its
TWIN -- the same records written in the order the contract of ``sort=True`` asks for, read by the code path without
``sort``.  The expected order is a numpy model: ``np.lexsort((reverse, pos, tid))`` over the placed records (stable:
records with equal (tid, POS, reverse strand) keep their file order), unplaced records last.  Nothing here looks at
what the code under test returns."""
import os

import numpy as np

from tests import bam_writer

COLS = ("tid", "pos", "alen", "flags", "nblk", "blk_start", "blk_len", "wide_idx", "wide_alen", "wide_nblk", "flag16", "mapq", "qlen", "nh")
UNSORTED = "BAM file is not coordinate sorted"
#: FLAG bits beside strand and unmapped that the records carry, so that a FLAG column permuted out of step shows
EXTRA_FLAGS = (0, 0x100, 0x400, 0x1 | 0x40, 0x1 | 0x80, 0x200, 0x1 | 0x2 | 0x40)


def nh_aux(v):
    return b"NHC" + bytes([v])


def model_order(records):
    """(record numbers of the placed records in sorted order, records moved): the contract, in numpy."""
    tid = np.array([r[0] for r in records], np.int64)
    pos = np.array([r[1] for r in records], np.int64)
    rev = np.array([(r[3] >> 4) & 1 for r in records], np.int64)
    placed = np.nonzero(tid >= 0)[0]
    order = placed[np.lexsort((rev[placed], pos[placed], tid[placed]))]
    return order, int((order != placed).sum())


def in_order(records):
    """The order test of a read without ``sort``: (tid, POS) non-decreasing, no placed record behind an unplaced one."""
    seen_unplaced, last = False, None
    for r in records:
        if r[0] < 0:
            seen_unplaced = True
            continue
        if seen_unplaced or (last is not None and (r[0], r[1]) < last):
            return False
        last = (r[0], r[1])
    return True


def twin_of(records):
    order, _ = model_order(records)
    return [records[i] for i in order] + [r for r in records if r[0] < 0]


def with_mapq(records):
    """Every record as a 6-tuple (tid, pos, cigartuples, flag, aux, MAPQ) with a MAPQ of its own, ``(i * 7) % 61`` for the
    i-th record: neighbours and the members of a tie differ, so a MAPQ column permuted out of step shows."""
    return [(r[0], r[1], r[2], r[3], r[4] if len(r) > 4 else b"", (i * 7) % 61) for i, r in enumerate(records)]


def write_fast(path, references, lengths, records, block_bytes=60000):
    """The writer of the shuffled files and their twins: ``bam_writer.write_bam``'s format (same record encoding, same
    members) with the record's MAPQ from its sixth field (``write_bam`` writes 30 everywhere), positions beyond 2^29,
    records given as encoded bytes, and a header that is joined instead of grown reference by reference (70 000 references)."""
    import struct
    text = b"@HD\tVN:1.6\tSO:unknown\n"
    parts = [b"BAM\x01" + struct.pack("<I", len(text)) + text + struct.pack("<I", len(references))]
    for nm, ln in zip(references, lengths):
        nmb = nm.encode() + b"\x00"
        parts.append(struct.pack("<I", len(nmb)) + nmb + struct.pack("<I", ln))
    for i, rec in enumerate(records):
        if isinstance(rec, bytes):   # (an encoded record, for the damaged ones)
            parts.append(rec)
            continue
        far = rec[1] >= 1 << 29      # (encode_record's bin field is that of a BAI: the position is patched in behind it)
        enc = bam_writer.encode_record(rec[0], 0 if far else rec[1], rec[2], rec[3], name=b"r", aux=rec[4] if len(rec) > 4 else b"",
                                       mapq=rec[5] if len(rec) > 5 else 30)
        parts.append(enc[:8] + struct.pack("<i", rec[1]) + enc[12:] if far else enc)
    data = b"".join(parts)
    with open(path, "wb") as fh:
        for off in range(0, len(data), block_bytes):
            fh.write(bam_writer.bgzf_block(data[off:off + block_bytes]))
        fh.write(bam_writer.BGZF_EOF)


def random_records(n, nref, seed, span=None, rich=True):
    """`n` records in random order over `nref` references: positions drawn from a range a third of `n` wide (many ties),
    both strands, FLAG bits and NH tags that vary from record to record, and with `rich` unplaced records (some first),
    placed-unmapped records, reads of 2 to 9 aligned runs and reads with a deletion.  No CIGAR opens with D / N."""
    rng = np.random.default_rng(seed)
    span = span or max(n // 3, 4)
    recs = []
    for i in range(n):
        kind = rng.random() if rich else 1.0
        flag = int(EXTRA_FLAGS[int(rng.integers(len(EXTRA_FLAGS)))]) | (0x10 if rng.random() < 0.5 else 0)
        aux = nh_aux(1 + i % 5) if i % 3 else b""
        if kind < 0.06 or (rich and n > 8 and i < 2):
            recs.append((-1, -1, [], 4 | (flag & 0x10), aux))
            continue
        tid, pos = int(rng.integers(nref)), int(rng.integers(span))
        if kind < 0.10:
            recs.append((tid, pos, [], flag | 4, aux))                      # placed, unmapped
        elif kind < 0.25:
            cig = []
            for k in range(int(rng.integers(2, 10))):
                cig += [(0, int(rng.integers(3, 12))), (3, int(rng.integers(20, 400)))]
            recs.append((tid, pos, cig[:-1], flag, aux))                    # 2 .. 9 aligned runs
        elif kind < 0.30:
            recs.append((tid, pos, [(4, 2), (0, 14), (2, 3), (0, 13), (1, 2), (0, 4)], flag, aux))
        else:
            recs.append((tid, pos, [(0, int(rng.integers(20, 40)))], flag, aux))
    return with_mapq(recs)


def wide_records():
    """Reads beyond the 8-bit / 16-bit columns -- more than 255 aligned runs, more than 65 535 aligned bases -- among
    ordinary ones, out of order and on both strands."""
    many = []
    for k in range(300):
        many += [(0, 5), (3, 7)]
    long_read = [(0, 70000)]
    recs = [(1, 500, [(0, 30)], 0), (0, 900, many[:-1], 16, nh_aux(2)), (0, 40, [(0, 25)], 16), (-1, -1, [], 4),
            (0, 900, long_read, 0, nh_aux(1)), (1, 20, many[:-1] + [(3, 9), (0, 11)], 0), (0, 40, [(0, 31), (3, 100), (0, 4)], 0, nh_aux(1)),
            (0, 10, long_read + [(3, 5), (0, 8)], 0x110), (1, 500, [(0, 28)], 16, nh_aux(3)), (0, 899, [(0, 33)], 0)]
    return with_mapq(recs)


def tie_pile(n=6000):
    """`n` records at one (tid, POS): both strands, aligned lengths cycling through 20 values, interleaved in file order
    -- a tie that spans many workgroups; a few records elsewhere make the file out of order."""
    recs = [(0, 5000, [(0, 30)], 0, nh_aux(1)), (0, 100, [(0, 29)], 16, nh_aux(1))]
    for i in range(n):
        recs.append((0, 3000, [(0, 21 + (i * 7) % 20)], 0x10 if (i % 3 == 1 or i % 5 == 0) else 0, nh_aux(1)))
    recs.append((0, 2990, [(0, 35)], 0, nh_aux(1)))
    return with_mapq(recs)


def write_pair(tmp, name, references, lengths, records, block_bytes=60000):
    """Writes `records` as they are and their twin (both with :func:`write_fast`: per-record MAPQ); returns (path, twin path)."""
    write = write_fast
    path, twin = os.path.join(str(tmp), name + ".bam"), os.path.join(str(tmp), name + ".twin.bam")
    write(path, references, lengths, records, block_bytes=block_bytes)
    write(twin, references, lengths, twin_of(records), block_bytes=block_bytes)
    return path, twin


def same_columns(a, b, what=""):
    for k in COLS:
        assert np.array_equal(getattr(a, k), getattr(b, k)), (what, k)
    assert a.references == b.references and a.lengths == b.lengths and a.mapped == b.mapped and a.n == b.n, what


def expected_file_order(records):
    order, moved = model_order(records)
    return order.astype(np.int64) if moved else None


def same_file_order(got, records, what=""):
    want = expected_file_order(records)
    if want is None:
        assert got.file_order is None, what
    else:
        assert got.file_order is not None and got.file_order.dtype == np.int64 and np.array_equal(got.file_order, want), what


RULES = [("fiveprime", 12), ("threeprime", 0), ("variable", {26: 12, 27: 12, 28: 13, 29: 13, 30: 14, "default": 13}),
         ("stratified", {26: 12, 27: 12, 28: 13, 29: 13, 30: 14, "default": 13}, 25, 35), ("center", 0)]


def oracle_spec(oracle, rule, size_filter=None):
    kind = rule[0]
    if kind in ("fiveprime", "threeprime", "center"):
        return oracle.mapping_spec(kind, rule[1], size_filter=size_filter)
    if kind == "variable":
        return oracle.mapping_spec(kind, 0, rule[1], size_filter=size_filter)
    return oracle.mapping_spec(kind, 0, rule[1], rule[2], rule[3], size_filter=size_filter)


def oracle_counts(oracle, files, rule, segs, size_filter=None):
    """The oracle's count vectors (genome order) of `segs` = [(tid, start, end, strand code)] over `files`, file-major."""
    from plastid_amd.packing import concat_file_major
    arrays, _ = oracle.count_segments(concat_file_major(files), oracle_spec(oracle, rule, size_filter),
                                      np.array([s[0] for s in segs], np.int32), np.array([s[1] for s in segs], np.int64),
                                      np.array([s[2] for s in segs], np.int64), np.array([s[3] for s in segs], np.uint8))
    return arrays
