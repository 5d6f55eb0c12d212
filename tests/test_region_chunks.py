"""The chunk list of a region set (``resolve_regions(...)["chunks"]``, ``pb_resolve_chunks``): what a region read on
the GPU uploads instead of the whole span between the first and the last region (``pc_bam_open_chunks``).  CPU only:
the index of the htslib-written fixture and of synthetic files with small BGZF members."""
import ctypes
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from plastid_amd import bam, synth  # noqa: E402
from plastid_amd.bam import read_bam, resolve_regions  # noqa: E402
from tests import bam_writer  # noqa: E402

FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hts_fixture.npz")


def bgzf_members(path):
    """File offsets and compressed lengths of the BGZF members of `path`."""
    offs, lens = [], []
    with open(path, "rb") as fh:
        data = fh.read()
    at = 0
    while at < len(data):
        xlen = struct.unpack("<H", data[at + 10:at + 12])[0]
        extra, bsize, x = data[at + 12:at + 12 + xlen], None, 0
        while x + 4 <= xlen:
            slen = struct.unpack("<H", extra[x + 2:x + 4])[0]
            if extra[x:x + 2] == b"BC":
                bsize = struct.unpack("<H", extra[x + 4:x + 6])[0]
            x += 4 + slen
        offs.append(at)
        lens.append(bsize + 1)
        at += bsize + 1
    return np.array(offs, np.int64), np.array(lens, np.int64)


def touched(offs, chunks):
    """Indices of the members the chunks ``[vb, ve)`` touch: those that start in ``[vb >> 16, ve >> 16)``, and the one at
    ``ve >> 16`` when the chunk ends inside it."""
    hit = set()
    for vb, ve in chunks:
        cb, ce, ue = int(vb) >> 16, int(ve) >> 16, int(ve) & 0xffff
        lo = int(np.searchsorted(offs, cb))
        hi = int(np.searchsorted(offs, ce, side="right" if ue else "left"))
        hit.update(range(lo, hi))
    return np.array(sorted(hit), np.int64)


def check_chunks(sp):
    ch = sp["chunks"]
    assert ch.dtype == np.uint64 and ch.ndim == 2 and ch.shape[1] == 2
    if len(ch) == 0:
        assert sp["voff_begin"] == 0 and sp["voff_end"] == 0
        return
    assert np.all(ch[:, 0] < ch[:, 1])
    assert np.all(ch[1:, 0] > ch[:-1, 1])        # ascending, disjoint (touching ones are merged)
    assert int(ch[0, 0]) == sp["voff_begin"] and int(ch[-1, 1]) == sp["voff_end"]


def span_keys(path, regions):
    """What pb_resolve_regions gives (the existing keys must keep these values)."""
    L = bam._load()
    h = L.pb_open(os.fsencode(path))
    try:
        n = len(regions)
        names = (ctypes.c_char_p * max(n, 1))(*[os.fsencode(c) for c, _, _ in regions])
        starts = np.array([s for _, s, _ in regions], np.int64)
        ends = np.array([e for _, _, e in regions], np.int64)
        vb, ve, mapped, nm = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_int64(0), ctypes.c_int(0)
        tid, beg, end = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int64), np.zeros(max(n, 1), np.int64)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
        assert L.pb_resolve_regions(h, n, names, p(starts), p(ends), ctypes.byref(vb), ctypes.byref(ve), ctypes.byref(mapped), ctypes.byref(nm),
                                    p(tid), p(beg), p(end)) == 0
    finally:
        L.pb_close(h)
    k = nm.value
    return dict(voff_begin=vb.value, voff_end=ve.value, mapped=mapped.value, tid=tid[:k], beg=beg[:k], end=end[:k])


def same_as_span(sp, path, regions):
    old = span_keys(path, regions)
    for key in ("voff_begin", "voff_end", "mapped"):
        assert sp[key] == old[key], key
    for key in ("tid", "beg", "end"):
        assert np.array_equal(sp[key], old[key]), key


@pytest.fixture(scope="module")
def hts_bam(tmp_path_factory):
    hts = np.load(FIX)
    path = str(tmp_path_factory.mktemp("hts") / "htslib.bam")
    open(path, "wb").write(hts["bam"].tobytes())
    open(path + ".bai", "wb").write(hts["bai"].tobytes())
    return hts, path


def test_chunks_of_the_htslib_fixture(hts_bam):
    hts, path = hts_bam
    refs = [str(x) for x in hts["references"]]
    offs, _ = bgzf_members(path)
    for q in range(len(hts["regions"])):
        t, b, e = (int(x) for x in hts["regions"][q])
        reg = [(refs[t], b, e)]
        sp = resolve_regions(path, reg)
        check_chunks(sp)
        same_as_span(sp, path, reg)
        for vb, _ in sp["chunks"]:
            assert (int(vb) >> 16) in set(offs.tolist())          # every chunk starts at a member
        want = hts["region_off"][q + 1] - hts["region_off"][q]
        assert want == 0 or len(sp["chunks"]) > 0
    many = [(refs[int(t)], int(b), int(e)) for t, b, e in hts["regions"][:40]]
    sp = resolve_regions(path, many)
    check_chunks(sp)
    same_as_span(sp, path, many)


def test_an_unknown_contig_has_no_chunks(hts_bam):
    hts, path = hts_bam
    sp = resolve_regions(path, [("nope", 0, 100)])
    assert sp["chunks"].shape == (0, 2) and sp["voff_begin"] == 0 and sp["voff_end"] == 0
    assert sp["mapped"] == int(hts["index_stat"][:, 1].sum())
    sp = resolve_regions(path, [])
    assert sp["chunks"].shape == (0, 2) and len(sp["tid"]) == 0


def _synthetic(path, scale=0.0005, block_bytes=3000):
    genome, tx, reads, _ = synth.make_config("C2", scale=scale, tx_scale=0.002)
    recs = bam_writer.packed_to_records(reads)
    bam_writer.write_bam(path, list(reads.references), [int(x) for x in reads.lengths], recs, block_bytes=block_bytes, index=True)
    return reads


def ends_regions(reads):
    """One region on the first contig with reads, one on the last."""
    on = np.unique(reads.tid)
    t0, t1 = int(on[0]), int(on[-1])
    p0, p1 = reads.pos[reads.tid == t0], reads.pos[reads.tid == t1]
    return [(reads.references[t0], int(np.median(p0)), int(np.median(p0)) + 2000),
            (reads.references[t1], int(np.median(p1)), int(np.median(p1)) + 2000)]


def test_chunks_of_far_apart_regions_touch_a_fraction_of_the_span(tmp_path):
    path = str(tmp_path / "syn.bam")
    reads = _synthetic(path)
    offs, lens = bgzf_members(path)
    assert len(offs) > 500
    regs = ends_regions(reads)
    sp = resolve_regions(path, regs)
    check_chunks(sp)
    same_as_span(sp, path, regs)
    assert len(sp["chunks"]) >= 2
    mine = lens[touched(offs, sp["chunks"])].sum()
    span = lens[touched(offs, [(sp["voff_begin"], sp["voff_end"])])].sum()
    assert 0 < mine < span / 5, (mine, span)
    # the chunks hold every record the region read returns: reading only them gives the same records
    got = read_bam(path, regions=regs)
    assert got.n > 0


def test_random_region_sets_give_well_formed_chunks(tmp_path):
    path = str(tmp_path / "syn.bam")
    reads = _synthetic(path, scale=0.0002)
    refs, lens = list(reads.references), [int(x) for x in reads.lengths]
    rng = np.random.default_rng(7)
    for _ in range(20):
        regs = []
        for _ in range(int(rng.integers(1, 40))):
            t = int(rng.integers(0, len(refs)))
            b = int(rng.integers(0, max(lens[t] - 10, 1)))
            regs.append((refs[t], b, b + int(rng.choice([1, 50, 3000, 200000, lens[t]]))))
        sp = resolve_regions(path, regs)
        check_chunks(sp)
        same_as_span(sp, path, regs)
