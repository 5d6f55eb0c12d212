"""The BAI index of a BAM file, record by record, in plain Python: the model the index tests compare with.

What htslib's ``sam_index_build`` writes for a BAM file (BAI: min_shift 14, 5 levels), restated from the SAM
specification section 5 and these rules (kent/src/htslib/sam.c:470-496, bam_endpos sam.c:338-344, hts.c:1150-1169,
1193-1291, 1293-1351, bgzf.c:569-572):

* a record's interval is ``[POS, POS + reference length of the CIGAR)`` when FLAG 0x4 is unset and it has a CIGAR,
  else ``[POS, POS + 1)``;
* its virtual offset is ``header offset of the member << 16 | offset in the payload``; a position where a member begins is
  reported in the FIRST member that begins there with offset 0 (so the end of a member's payload lies in the next member);
* a run -- consecutive placed records with one reference and one bin -- gives the bin one chunk up to the next run's first
  record; mapped records give the 16 kb windows they cover their offset, first come first kept; the pseudo-bin 37450 holds
  the reference's file range and its mapped / unmapped counts; unplaced records are counted;
* the finish fills the uncovered windows forward, moves bins that span fewer than 0x10000 file bytes into an existing
  parent (deepest level first) and merges chunks that touch one BGZF member.

It has its own BGZF / BAM walk (zlib).  An index is ``(refs, n_no_coor)`` with ``refs[t] = (bins, linear)``, ``bins`` a dict
from bin number (37450 included) to a list of ``(begin, end)`` pairs.
"""
import struct
import zlib

import numpy as np

META_BIN = 37450


def parse_bai(bai):
    assert bai[:4] == b"BAI\1"
    o = 4
    nref, = struct.unpack_from("<i", bai, o)
    o += 4
    refs = []
    for _ in range(nref):
        nb, = struct.unpack_from("<i", bai, o)
        o += 4
        bins = {}
        for _ in range(nb):
            b, nc = struct.unpack_from("<Ii", bai, o)
            o += 8
            assert b not in bins
            bins[b] = [struct.unpack_from("<QQ", bai, o + 16 * i) for i in range(nc)]
            o += 16 * nc
        ni, = struct.unpack_from("<i", bai, o)
        o += 4
        lin = list(struct.unpack_from("<%dQ" % ni, bai, o))
        o += 8 * ni
        refs.append((bins, lin))
    nn, = struct.unpack_from("<Q", bai, o)
    assert o + 8 == len(bai)
    return refs, nn


def bin_order(bai):
    """The bin numbers of every reference in the order the bytes have them."""
    o = 8
    nref, = struct.unpack_from("<i", bai, 4)
    out = []
    for _ in range(nref):
        nb, = struct.unpack_from("<i", bai, o)
        o += 4
        ids = []
        for _ in range(nb):
            b, nc = struct.unpack_from("<Ii", bai, o)
            ids.append(b)
            o += 8 + 16 * nc
        ni, = struct.unpack_from("<i", bai, o)
        o += 4 + 8 * ni
        out.append(ids)
    return out


def members(bam):
    """``(file offset of the gzip header, payload)`` of every BGZF member, the empty ones included."""
    o, out = 0, []
    while o < len(bam):
        xlen, = struct.unpack_from("<H", bam, o + 10)
        bsize, p = None, o + 12
        while p < o + 12 + xlen:
            si1, si2, sl = struct.unpack_from("<BBH", bam, p)
            if si1 == 66 and si2 == 67:
                bsize, = struct.unpack_from("<H", bam, p + 4)
            p += 4 + sl
        out.append((o, zlib.decompress(bam[o + 12 + xlen:o + bsize + 1 - 8], -15)))
        o += bsize + 1
    return out


def reg2bin(beg, end):
    end -= 1
    if beg >> 14 == end >> 14:
        return ((1 << 15) - 1) // 7 + (beg >> 14)
    if beg >> 17 == end >> 17:
        return ((1 << 12) - 1) // 7 + (beg >> 17)
    if beg >> 20 == end >> 20:
        return ((1 << 9) - 1) // 7 + (beg >> 20)
    if beg >> 23 == end >> 23:
        return ((1 << 6) - 1) // 7 + (beg >> 23)
    if beg >> 26 == end >> 26:
        return ((1 << 3) - 1) // 7 + (beg >> 26)
    return 0


def level(b):
    return 0 if b == 0 else 1 if b < 9 else 2 if b < 73 else 3 if b < 585 else 4 if b < 4681 else 5


def walk(bam):
    """``dict(nref, lengths, recs, final, members)``: ``recs`` = ``(virtual offset, tid, beg, end, mapped)`` of every record in
    file order, ``final`` the offset behind the last one, ``members`` = ``(header offset, stream begin, length)``."""
    ms = members(bam)
    stream = b"".join(d for _, d in ms)
    uoff = np.cumsum([0] + [len(d) for _, d in ms])

    def tell(p):
        m = int(np.searchsorted(uoff[:-1], p, side="left"))
        if m < len(ms) and uoff[m] == p:
            return ms[m][0] << 16
        if p == len(stream):          # no member begins at the end of the stream: the reader stands at the end of the file
            return len(bam) << 16
        m -= 1
        return (ms[m][0] << 16) | (p - int(uoff[m]))

    assert stream[:4] == b"BAM\1"
    lt, = struct.unpack_from("<i", stream, 4)
    p = 8 + lt
    nref, = struct.unpack_from("<i", stream, p)
    p += 4
    lengths = []
    for _ in range(nref):
        ln, = struct.unpack_from("<i", stream, p)
        lengths.append(struct.unpack_from("<i", stream, p + 4 + ln)[0])
        p += 4 + ln + 4
    first = p
    recs = []
    while p < len(stream):
        bs, = struct.unpack_from("<i", stream, p)
        tid, pos, lname, _mapq, _bin, ncig, flag, _lseq = struct.unpack_from("<iiBBHHHi", stream, p + 4)
        cig = struct.unpack_from("<%dI" % ncig, stream, p + 36 + lname)
        rlen = sum(c >> 4 for c in cig if (c & 15) in (0, 2, 3, 7, 8))
        end = pos + rlen if (not flag & 4 and ncig > 0) else pos + 1
        recs.append((tell(p), tid, pos, end, not flag & 4, p))
        p += 4 + bs
    assert p == len(stream)
    return dict(nref=nref, lengths=lengths, recs=[r[:5] for r in recs], final=tell(p), first_record=first,
                starts=[r[5] for r in recs], members=[(ms[k][0], int(uoff[k]), len(ms[k][1])) for k in range(len(ms))])


def prefinish(w):
    """What the finish takes (the arguments of ``pc_bam_index_finish``): the runs in file order, the linear windows with 0 for
    "not covered", the per-reference file ranges and counts, ``n_no_coor``."""
    nref, recs = w["nref"], w["recs"]
    n = len(recs)
    offs = [r[0] for r in recs] + [w["final"]]
    lin = [[] for _ in range(nref)]
    ref_beg, ref_end = [0] * nref, [0] * nref
    mapped, unmapped = [0] * nref, [0] * nref
    last_of = {}
    nn = 0
    for k, (off, tid, beg, end, mp) in enumerate(recs):
        if tid < 0:
            nn += 1
            continue
        if tid not in last_of:
            ref_beg[tid] = off
        last_of[tid] = k
        if mp:
            mapped[tid] += 1
            a, b = beg >> 14, (end - 1) >> 14
            while len(lin[tid]) < b + 1:
                lin[tid].append(0)
            for x in range(a, b + 1):
                if lin[tid][x] == 0:
                    lin[tid][x] = off
        else:
            unmapped[tid] += 1
    for tid, k in last_of.items():
        ref_end[tid] = offs[k + 1]
    run_tid, run_bin, run_beg, run_end = [], [], [], []
    i = 0
    while i < n:
        off, tid, beg, end, mp = recs[i]
        if tid < 0:
            break
        b = reg2bin(beg, end)
        j = i
        while j + 1 < n and recs[j + 1][1] == tid and reg2bin(recs[j + 1][2], recs[j + 1][3]) == b:
            j += 1
        run_tid.append(tid)
        run_bin.append(b)
        run_beg.append(off)
        run_end.append(offs[j + 1])
        i = j + 1
    lin_start = np.cumsum([0] + [len(x) for x in lin]).astype(np.int64)
    return dict(n_ref=nref, run_tid=np.array(run_tid, np.int32), run_bin=np.array(run_bin, np.uint32), run_beg=np.array(run_beg, np.uint64),
                run_end=np.array(run_end, np.uint64), lin_start=lin_start, linear=np.array([x for l in lin for x in l], np.uint64),
                ref_beg=np.array(ref_beg, np.uint64), ref_end=np.array(ref_end, np.uint64), ref_mapped=np.array(mapped, np.int64),
                ref_unmapped=np.array(unmapped, np.int64), n_no_coor=nn)


def finish(pre):
    nref = pre["n_ref"]
    refs = [({}, []) for _ in range(nref)]
    for t, b, u, v in zip(pre["run_tid"].tolist(), pre["run_bin"].tolist(), pre["run_beg"].tolist(), pre["run_end"].tolist()):
        refs[t][0].setdefault(b, []).append((u, v))
    for tid in range(nref):
        bins, lin = refs[tid]
        has = int(pre["ref_mapped"][tid]) + int(pre["ref_unmapped"][tid]) > 0
        last = int(pre["ref_beg"][tid])
        for v in pre["linear"][int(pre["lin_start"][tid]):int(pre["lin_start"][tid + 1])].tolist():
            if v:
                last = v
            lin.append(last)
        for lv in range(5, 0, -1):
            start = ((1 << (3 * lv)) - 1) // 7
            for b in sorted(k for k in bins if k >= start):
                ch = bins[b]
                if lv < 5 and len(ch) > 1:
                    ch.sort()
                if (ch[-1][1] >> 16) - (ch[0][0] >> 16) < 0x10000:
                    par = (b - 1) >> 3
                    if par not in bins:
                        continue
                    bins[par].extend(ch)
                    del bins[b]
        if 0 in bins:
            bins[0].sort()
        for b, ch in bins.items():
            out = [list(ch[0])]
            for u, v in ch[1:]:
                if out[-1][1] >> 16 >= u >> 16:
                    if out[-1][1] < v:
                        out[-1][1] = v
                else:
                    out.append([u, v])
            bins[b] = [tuple(x) for x in out]
        if has:
            bins[META_BIN] = [(int(pre["ref_beg"][tid]), int(pre["ref_end"][tid])), (int(pre["ref_mapped"][tid]), int(pre["ref_unmapped"][tid]))]
    return refs, pre["n_no_coor"]


def model(bam):
    return finish(prefinish(walk(bam)))
