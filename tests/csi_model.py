"""The CSI index of a BAM file, record by record, in plain Python: the model the CSI tests compare with.

What htslib's ``sam_index_build(fn, min_shift > 0)`` writes (kent/src/htslib/sam.c:477-485, hts.c:1150-1169, 1193-1291,
1293-1351, 1395-1457, 1484-1499; SAM specification 5.3), restated with the index shape ``(min_shift, n_lvls)`` as a
parameter.  The record walk -- intervals, virtual offsets -- is the BAI model's (tests/index_model.py ``walk``); what
differs is the geometry of the bins and windows, and that the windows end as one ``loff`` per bin:

* ``n_lvls`` is the smallest depth with ``max(reference length) + 256 <= 1 << (min_shift + 3 * n_lvls)``;
* a record's bin is found from the leaves (``1 << min_shift`` positions) upwards; mapped records give the windows of
  ``1 << min_shift`` positions they cover their offset, first come first kept;
* the finish fills the windows forward (leading ones: the offset of the reference's first record), gives every bin the
  filled window at its first leaf as ``loff`` (0 beyond the reference's windows), THEN moves small bins into existing
  parents (levels ``n_lvls .. 1``) and merges chunks; the pseudo-bin is ``n_bins + 1`` with ``loff`` 0.

An index is ``(refs, n_no_coor)`` with ``refs[t] = (bins, loff)``: ``bins`` a dict from bin number (pseudo-bin included) to
a list of ``(begin, end)`` pairs, ``loff`` a dict from bin number to its offset.
"""
import struct

import numpy as np

from tests.index_model import walk  # noqa: F401  (re-exported: the record walk is shared)


def depth_for(lengths, min_shift):
    max_len = max([int(x) & 0xffffffff for x in lengths] + [0]) + 256
    n_lvls, s = 0, 1 << min_shift
    while max_len > s:
        n_lvls, s = n_lvls + 1, s << 3
    return n_lvls


def level_first(l):
    return ((1 << (3 * l)) - 1) // 7


def n_bins(n_lvls):
    return level_first(n_lvls + 1)


def meta_bin(n_lvls):
    return n_bins(n_lvls) + 1


def reg2bin(beg, end, min_shift, n_lvls):
    end -= 1
    s = min_shift
    for l in range(n_lvls, 0, -1):
        if beg >> s == end >> s:
            return level_first(l) + (beg >> s)
        s += 3
    return 0


def bin_level(b, n_lvls):
    l = 0
    while l < n_lvls and b >= level_first(l + 1):
        l += 1
    return l


def bin_bot(b, n_lvls):
    l = bin_level(b, n_lvls)
    return (b - level_first(l)) << (3 * (n_lvls - l))


def parse_csi(data):
    """``(min_shift, depth, refs, n_no_coor)`` of a CSI payload (what the BGZF members of a ``.csi`` file hold)."""
    assert data[:4] == b"CSI\1"
    min_shift, depth, l_aux = struct.unpack_from("<iii", data, 4)
    o = 16 + l_aux
    nref, = struct.unpack_from("<i", data, o)
    o += 4
    refs = []
    for _ in range(nref):
        nb, = struct.unpack_from("<i", data, o)
        o += 4
        bins, loff = {}, {}
        for _ in range(nb):
            b, lo, nc = struct.unpack_from("<IQi", data, o)
            o += 16
            assert b not in bins
            bins[b] = [struct.unpack_from("<QQ", data, o + 16 * i) for i in range(nc)]
            loff[b] = lo
            o += 16 * nc
        refs.append((bins, loff))
    nn, = struct.unpack_from("<Q", data, o)
    assert o + 8 == len(data)
    return min_shift, depth, refs, nn


def bin_order(data):
    """The bin numbers of every reference in the order the payload has them."""
    l_aux, = struct.unpack_from("<i", data, 12)
    o = 16 + l_aux
    nref, = struct.unpack_from("<i", data, o)
    o += 4
    out = []
    for _ in range(nref):
        nb, = struct.unpack_from("<i", data, o)
        o += 4
        ids = []
        for _ in range(nb):
            b, _lo, nc = struct.unpack_from("<IQi", data, o)
            ids.append(b)
            o += 16 + 16 * nc
        out.append(ids)
    return out


def prefinish(w, min_shift, n_lvls=None):
    """What the finish takes (the arguments of ``pc_bam_index_finish_csi``): the runs in file order with the ``loff`` of
    their bins, the per-reference file ranges and counts, ``n_no_coor``; ``n_intv``: the windows of every reference."""
    if n_lvls is None:
        n_lvls = depth_for(w["lengths"], min_shift)
    reach = 1 << (min_shift + 3 * n_lvls)
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
        if end > reach:
            raise ValueError("an alignment reaches beyond %d" % reach)
        if tid not in last_of:
            ref_beg[tid] = off
        last_of[tid] = k
        if mp:
            mapped[tid] += 1
            a, b = beg >> min_shift, (end - 1) >> min_shift
            while len(lin[tid]) < b + 1:
                lin[tid].append(None)
            for x in range(a, b + 1):
                if lin[tid][x] is None:
                    lin[tid][x] = off
        else:
            unmapped[tid] += 1
    for tid, k in last_of.items():
        ref_end[tid] = offs[k + 1]
    for tid in range(nref):           # update_loff's forward fill
        last = ref_beg[tid]
        for x, v in enumerate(lin[tid]):
            if v is not None:
                last = v
            lin[tid][x] = last
    run_tid, run_bin, run_beg, run_end, run_loff = [], [], [], [], []
    i = 0
    while i < n:
        off, tid, beg, end, mp = recs[i]
        if tid < 0:
            break
        b = reg2bin(beg, end, min_shift, n_lvls)
        j = i
        while j + 1 < n and recs[j + 1][1] == tid and reg2bin(recs[j + 1][2], recs[j + 1][3], min_shift, n_lvls) == b:
            j += 1
        bot = bin_bot(b, n_lvls)
        run_tid.append(tid)
        run_bin.append(b)
        run_beg.append(off)
        run_end.append(offs[j + 1])
        run_loff.append(lin[tid][bot] if bot < len(lin[tid]) else 0)
        i = j + 1
    return dict(min_shift=min_shift, n_lvls=n_lvls, n_ref=nref, run_tid=np.array(run_tid, np.int32), run_bin=np.array(run_bin, np.uint32),
                run_beg=np.array(run_beg, np.uint64), run_end=np.array(run_end, np.uint64), run_loff=np.array(run_loff, np.uint64),
                ref_beg=np.array(ref_beg, np.uint64), ref_end=np.array(ref_end, np.uint64), ref_mapped=np.array(mapped, np.int64),
                ref_unmapped=np.array(unmapped, np.int64), n_no_coor=nn, n_intv=[len(x) for x in lin], filled=lin)


def finish(pre):
    nref, n_lvls = pre["n_ref"], pre["n_lvls"]
    refs = [({}, {}) for _ in range(nref)]
    for t, b, u, v, lo in zip(pre["run_tid"].tolist(), pre["run_bin"].tolist(), pre["run_beg"].tolist(), pre["run_end"].tolist(), pre["run_loff"].tolist()):
        assert b < n_bins(n_lvls)
        refs[t][0].setdefault(b, []).append((u, v))
        assert refs[t][1].setdefault(b, lo) == lo
    for tid in range(nref):
        bins, loff = refs[tid]
        has = int(pre["ref_mapped"][tid]) + int(pre["ref_unmapped"][tid]) > 0
        for lv in range(n_lvls, 0, -1):
            start = level_first(lv)
            for b in sorted(k for k in bins if k >= start):
                ch = bins[b]
                if lv < n_lvls and len(ch) > 1:
                    ch.sort()
                if (ch[-1][1] >> 16) - (ch[0][0] >> 16) < 0x10000:
                    par = (b - 1) >> 3
                    if par not in bins:
                        continue
                    bins[par].extend(ch)
                    del bins[b]
                    del loff[b]
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
            m = meta_bin(n_lvls)
            bins[m] = [(int(pre["ref_beg"][tid]), int(pre["ref_end"][tid])), (int(pre["ref_mapped"][tid]), int(pre["ref_unmapped"][tid]))]
            loff[m] = 0
    return refs, pre["n_no_coor"]


def model(bam, min_shift, n_lvls=None):
    """``(min_shift, depth, refs, n_no_coor)``, as :func:`parse_csi` gives it."""
    pre = prefinish(walk(bam), min_shift, n_lvls)
    refs, nn = finish(pre)
    return min_shift, pre["n_lvls"], refs, nn
