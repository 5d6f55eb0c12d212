"""Inputs the CSI tests share (CPU and GPU): the cases of ``tests/golden/csi_fixture.npz`` (what htslib wrote and read
back, see tests/golden/make_csi_golden.py), a BAM writer for coordinates up to 2^31 - 1, and the call of
``pc_bam_index_finish_csi``."""
import ctypes
import functools
import os
import struct

import numpy as np

from tests import bam_writer, csi_model

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
COLS = ("tid", "pos", "alen", "flags", "nblk", "blk_start", "blk_len", "wide_idx", "wide_alen", "wide_nblk", "flag16", "mapq", "qlen", "nh")


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(os.path.join(GOLDEN, "csi_fixture.npz")))


def case_shapes():
    """Every ``(case, min_shift)`` of the fixture."""
    fx = fixture()
    return [(str(c), int(s)) for c in fx["cases"] for s in fx[str(c) + "_shapes"]]


@functools.lru_cache(maxsize=None)
def case_bam(case):
    """The BAM bytes of a case (``fixture``: those of hts_fixture.npz)."""
    if case == "fixture":
        return np.load(os.path.join(GOLDEN, "hts_fixture.npz"))["bam"].tobytes()
    return fixture()[case + "_bam"].tobytes()


def case_data(case, min_shift):
    """What htslib gave for one case and shape: dict with ``csi`` (payload bytes), ``rec``, ``regions``, ``region_off``,
    ``region_records``, ``stat``, ``n_no_coor``, ``references``, ``lengths``."""
    fx, k = fixture(), "%s_%d_" % (case, min_shift)
    d = {name: fx[k + name] for name in ("rec", "regions", "region_off", "region_records", "stat")}
    d.update(csi=fx[k + "csi"].tobytes(), n_no_coor=int(fx[k + "n_no_coor"]), references=[str(x) for x in fx[case + "_references"]],
             lengths=[int(x) for x in fx[case + "_lengths"]])
    return d


@functools.lru_cache(maxsize=None)
def case_walk(case):
    return csi_model.walk(case_bam(case))


@functools.lru_cache(maxsize=None)
def case_model(case, min_shift):
    """``(pre-finish arrays, finished index as parse_csi gives it)`` of the model for one case and shape."""
    pre = csi_model.prefinish(case_walk(case), min_shift)
    refs, nn = csi_model.finish(pre)
    return pre, (min_shift, pre["n_lvls"], refs, nn)


def write_case(tmp_path, case, min_shift=None):
    """The case's BAM file in `tmp_path` and, with `min_shift`, htslib's ``.csi`` (BGZF) at ``<bam>.hts.csi``; returns the BAM path."""
    from plastid_amd.bam import _bgzf_wrap
    path = os.path.join(str(tmp_path), case + ".bam")
    if not os.path.exists(path):
        open(path, "wb").write(case_bam(case))
    if min_shift is not None:
        open(path + ".hts.csi", "wb").write(_bgzf_wrap(case_data(case, min_shift)["csi"]))
    return path


def region_want(d, q):
    """Region q of a case as ``(name, beg, end)`` and the indices of the records htslib returned for it."""
    t, b, e = (int(x) for x in d["regions"][q])
    return (d["references"][t], b, e), d["region_records"][d["region_off"][q]:d["region_off"][q + 1]]


def assert_records(got, d, want):
    """The packed alignments `got` are the records `want` (indices into htslib's read-back) in order."""
    rec = d["rec"]
    assert got.n == len(want)
    assert np.array_equal(got.tid, rec[want, 0]) and np.array_equal(got.pos, rec[want, 1]) and np.array_equal(got.flag16, rec[want, 3])
    assert np.array_equal(got.mapq, rec[want, 4]) and np.array_equal(got.qlen, rec[want, 5])


def same(a, b):
    for k in COLS:
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    assert a.references == b.references and a.lengths == b.lengths and a.mapped == b.mapped and a.n == b.n


# ---- a writer for coordinates beyond what bam_writer.encode_record can pack (its 16-bit bin field overflows near 10^9)

def encode_record(tid, pos, cigartuples, flag, name=b"r", mapq=30):
    """One BAM record; the ``bin`` field is the (14, 5) bin truncated to 16 bits, as htslib's ``bam1_core_t`` keeps it."""
    qlen = sum(n for op, n in cigartuples if op in (0, 1, 4, 7, 8))
    ref_len = sum(n for op, n in cigartuples if op in (0, 2, 3, 7, 8))
    name = name + b"\x00"
    cig = b"".join(struct.pack("<I", (n << 4) | op) for op, n in cigartuples)
    body = struct.pack("<iiBBHHHIiii", tid, pos, len(name), mapq, bam_writer.reg2bin(pos, pos + max(ref_len, 1)) & 0xffff, len(cigartuples),
                       flag, qlen, -1, -1, 0) + name + cig + bytes([0x11] * ((qlen + 1) // 2)) + bytes([0xff] * qlen)
    return struct.pack("<I", len(body)) + body


def write_bam(path, references, lengths, records, block_bytes=60000):
    """records: ``(tid, pos, cigartuples, flag)``, named ``r<index>``; members of `block_bytes` payload bytes."""
    text = b"@HD\tVN:1.6\tSO:coordinate\n"
    out = [b"BAM\x01" + struct.pack("<I", len(text)) + text + struct.pack("<I", len(references))]
    for nm, ln in zip(references, lengths):
        nmb = nm.encode() + b"\x00"
        out.append(struct.pack("<I", len(nmb)) + nmb + struct.pack("<I", ln))
    for i, (tid, pos, cig, flag) in enumerate(records):
        out.append(encode_record(tid, pos, cig, flag, name=("r%d" % i).encode()))
    data = b"".join(out)
    with open(path, "wb") as fh:
        for off in range(0, len(data), block_bytes):
            fh.write(bam_writer.bgzf_block(data[off:off + block_bytes]))
        fh.write(bam_writer.BGZF_EOF)


def finish_with_library(pre, min_shift=None, n_lvls=None):
    """``pc_bam_index_finish_csi`` on the model's pre-finish arrays -> ``(payload bytes, stats[8])``."""
    from plastid_amd import _lib
    L = _lib.load()
    h = ctypes.c_void_p()
    keep = [np.ascontiguousarray(pre[k]) for k in ("run_tid", "run_bin", "run_beg", "run_end", "run_loff", "ref_beg", "ref_end", "ref_mapped", "ref_unmapped")]
    _lib.check(L.pc_bam_index_finish_csi(int(pre["min_shift"] if min_shift is None else min_shift), int(pre["n_lvls"] if n_lvls is None else n_lvls),
                                         int(pre["n_ref"]), len(pre["run_tid"]), *[a.ctypes.data_as(ctypes.c_void_p) for a in keep],
                                         int(pre["n_no_coor"]), ctypes.byref(h)))
    try:
        n = ctypes.c_int64(0)
        _lib.check(L.pc_bam_index_bytes(h, None, 0, ctypes.byref(n)))
        buf = ctypes.create_string_buffer(max(int(n.value), 1))
        _lib.check(L.pc_bam_index_bytes(h, buf, int(n.value), ctypes.byref(n)))
        st = np.zeros(8, np.int64)
        _lib.check(L.pc_bam_index_stats(h, st.ctypes.data_as(ctypes.c_void_p)))
    finally:
        L.pc_bam_index_close(h)
    return buf.raw[:int(n.value)], st
