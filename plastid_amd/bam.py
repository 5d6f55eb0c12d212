"""BAM files -> :class:`~plastid_amd.packing.PackedAlignments` with the package's own
native reader (``csrc/bam_stager.cpp``: BGZF inflate on a thread pool + BAM record parse).

Replaces what the reference gets from pysam on this path (``pysam.AlignmentFile(X, "rb")``,
``.references/.lengths/.mapped``, ``read.positions``, ``read.is_reverse`` --
plastid/genomics/genome_array.py:660-690, 800-815).  The file must be coordinate sorted
(as for pysam ``fetch``); no index file is needed because the whole file is staged.
"""
import ctypes
import os

import numpy as np

from .build import BAM_LIB, build_bam_library
from .packing import PackedAlignments

_lib = None


def _load():
    global _lib
    if _lib is None:
        if not os.path.exists(BAM_LIB):
            build_bam_library()
        L = ctypes.CDLL(BAM_LIB)
        vp = ctypes.c_void_p
        L.pb_last_error.restype = ctypes.c_char_p
        L.pb_open.restype = vp
        L.pb_open.argtypes = [ctypes.c_char_p]
        L.pb_open_indexed.restype = vp
        L.pb_open_indexed.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
        L.pb_close.argtypes = [vp]
        L.pb_load.argtypes = [vp, ctypes.c_int]
        L.pb_load_regions.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_char_p), vp, vp]
        L.pb_nref.argtypes = [vp]
        L.pb_ref_name.restype = ctypes.c_char_p
        L.pb_ref_name.argtypes = [vp, ctypes.c_int]
        L.pb_ref_length.restype = ctypes.c_int32
        L.pb_ref_length.argtypes = [vp, ctypes.c_int]
        L.pb_counts.argtypes = [vp, vp]
        L.pb_fill.argtypes = [vp] * 8
        L.pb_wide_count.restype = ctypes.c_int64
        L.pb_wide_count.argtypes = [vp]
        L.pb_fill_wide.argtypes = [vp] * 4
        L.pb_fill_sam.argtypes = [vp] * 4
        L.pb_fill_nh.argtypes = [vp] * 2
        L.pb_resolve_regions.argtypes = [vp, ctypes.c_int, ctypes.POINTER(ctypes.c_char_p)] + [vp] * 9
        L.pb_resolve_chunks.argtypes = [vp, ctypes.c_int, ctypes.POINTER(ctypes.c_char_p), vp, vp, ctypes.c_int64] + [vp] * 8
        _lib = L
    return _lib


def bam_header(path):
    """``(references, lengths)`` of a BAM file from its header alone: the leading BGZF members are inflated (zlib) until
    the reference list is complete -- what ``pysam.AlignmentFile(path).references / .lengths`` give
    (genome_array.py:667-670)."""
    import struct
    import zlib
    buf = b""
    with open(path, "rb") as fh:
        def more():
            head = fh.read(12)
            if len(head) < 12:
                return False
            if head[0] != 31 or head[1] != 139 or head[2] != 8 or not (head[3] & 4):
                raise ValueError("not a BGZF file (bad gzip member header)")
            xlen = struct.unpack("<H", head[10:12])[0]
            extra = fh.read(xlen)
            bsize, x = -1, 0
            while x + 4 <= len(extra):
                slen = struct.unpack("<H", extra[x + 2:x + 4])[0]
                if extra[x:x + 2] == b"BC" and slen == 2:
                    bsize = struct.unpack("<H", extra[x + 4:x + 6])[0]
                x += 4 + slen
            if bsize < 0:
                raise ValueError("BGZF member without BC subfield")
            payload = fh.read(bsize + 1 - 12 - xlen)
            if len(payload) < bsize + 1 - 12 - xlen:
                raise ValueError("truncated BGZF member")
            nonlocal buf
            buf += zlib.decompressobj(-15).decompress(payload[:-8])
            return True

        def need(n):
            while len(buf) < n:
                if not more():
                    raise ValueError("truncated BAM header")

        need(12)
        if buf[:4] != b"BAM\x01":
            raise ValueError("not a BAM file (bad magic)")
        l_text = struct.unpack("<i", buf[4:8])[0]
        need(12 + l_text)
        n_ref = struct.unpack("<i", buf[8 + l_text:12 + l_text])[0]
        at = 12 + l_text
        refs, lens = [], []
        for _ in range(n_ref):
            need(at + 4)
            l_name = struct.unpack("<i", buf[at:at + 4])[0]
            need(at + 4 + l_name + 4)
            refs.append(buf[at + 4:at + 4 + l_name - 1].decode())
            lens.append(struct.unpack("<i", buf[at + 4 + l_name:at + 8 + l_name])[0])
            at += 8 + l_name
    return refs, lens


def _region_tuples(regions):
    return [(r.chrom, r.start, r.end) if hasattr(r, "chrom") else tuple(r) for r in regions]


class BamIndex(object):
    """A BAI index (SAM specification 5.2), parsed: what ``samtools index`` writes and :func:`build_index` builds.

    ``bins``: per reference, a dict from bin number to a ``uint64 [k, 2]`` array of chunks ``[begin, end)`` (virtual
    offsets); ``linear``: per reference, the ``uint64`` offsets of its 16 kb windows; ``meta``: per reference, ``None`` or
    ``(file begin, file end, mapped, unmapped)`` from samtools' pseudo-bin 37450; ``n_no_coor``: the records without a
    reference; ``mapped``: the sum of the per-reference mapped counts (pysam's ``AlignmentFile.mapped``), -1 when the
    index carries none.  Two indexes are equal when their parsed content is: the order of the bins in the file is not part of it
    (htslib writes them in the order of its hash table; :meth:`to_bytes` writes them ascending, 37450 last)."""

    META_BIN = 37450

    def __init__(self, bins, linear, meta, n_no_coor=0):
        self.bins, self.linear, self.meta, self.n_no_coor = bins, linear, meta, int(n_no_coor)

    @property
    def n_ref(self):
        return len(self.bins)

    @property
    def mapped(self):
        have = [m for m in self.meta if m is not None]
        return sum(int(m[2]) for m in have) if have else -1

    @classmethod
    def from_bytes(cls, data):
        import struct
        data = bytes(data)
        if len(data) < 8 or data[:4] != b"BAI\x01":
            raise ValueError("not a BAI index")
        n_ref, = struct.unpack_from("<i", data, 4)
        o = 8
        bins, linear, meta = [], [], []
        try:
            for _ in range(n_ref):
                n_bin, = struct.unpack_from("<i", data, o)
                o += 4
                rb, rm = {}, None
                for _ in range(n_bin):
                    b, nc = struct.unpack_from("<Ii", data, o)
                    o += 8
                    if nc < 0 or o + 16 * nc > len(data):
                        raise struct.error("chunks")
                    ch = np.frombuffer(data, "<u8", 2 * nc, o).reshape(nc, 2).copy()
                    o += 16 * nc
                    if b == cls.META_BIN and nc >= 2:
                        rm = tuple(int(x) for x in ch[:2].ravel())
                    elif b != cls.META_BIN:
                        rb[int(b)] = ch
                n_intv, = struct.unpack_from("<i", data, o)
                o += 4
                if n_intv < 0 or o + 8 * n_intv > len(data):
                    raise struct.error("linear")
                linear.append(np.frombuffer(data, "<u8", n_intv, o).copy())
                o += 8 * n_intv
                bins.append(rb)
                meta.append(rm)
            n_no_coor = struct.unpack_from("<Q", data, o)[0] if o + 8 <= len(data) else 0   # (optional in the format)
        except struct.error:
            raise ValueError("truncated BAI index")
        return cls(bins, linear, meta, n_no_coor)

    @classmethod
    def from_file(cls, path):
        with open(path, "rb") as fh:
            return cls.from_bytes(fh.read())

    def to_bytes(self):
        import struct
        out = [b"BAI\x01", struct.pack("<i", self.n_ref)]
        for rb, lin, rm in zip(self.bins, self.linear, self.meta):
            out.append(struct.pack("<i", len(rb) + (rm is not None)))
            for b in sorted(rb):
                ch = np.ascontiguousarray(rb[b], "<u8")
                out.append(struct.pack("<Ii", b, len(ch)))
                out.append(ch.tobytes())
            if rm is not None:
                out.append(struct.pack("<Ii4Q", self.META_BIN, 2, *rm))
            out.append(struct.pack("<i", len(lin)))
            out.append(np.ascontiguousarray(lin, "<u8").tobytes())
        out.append(struct.pack("<Q", self.n_no_coor))
        return b"".join(out)

    def write(self, path):
        with open(path, "wb") as fh:
            fh.write(self.to_bytes())

    def __eq__(self, other):
        if not isinstance(other, BamIndex):
            return NotImplemented
        if self.n_ref != other.n_ref or self.n_no_coor != other.n_no_coor or list(self.meta) != list(other.meta):
            return False
        for a, b, la, lb in zip(self.bins, other.bins, self.linear, other.linear):
            if sorted(a) != sorted(b) or not np.array_equal(la, lb) or any(not np.array_equal(a[k], b[k]) for k in a):
                return False
        return True

    def __ne__(self, other):
        r = self.__eq__(other)
        return r if r is NotImplemented else not r

    __hash__ = None

    def __repr__(self):
        return "BamIndex(%d references, %d bins, %d chunks, n_no_coor=%d, mapped=%d)" % (
            self.n_ref, sum(len(b) for b in self.bins), sum(len(c) for b in self.bins for c in b.values()), self.n_no_coor, self.mapped)


def find_index(path):
    """The index file the region reads find beside `path` (``path + ".bai"``, then ``.bai`` in place of the extension), or ``None``."""
    path = os.fspath(path)
    for cand in (path + ".bai", path[:-4] + ".bai" if len(path) > 4 else None):
        if cand and os.path.isfile(cand):
            return cand
    return None


def build_index(path, engine=None, out=None, overwrite=False, timing=None):
    """Build the BAI index of the coordinate-sorted BAM file `path` ON THE GPU (``pc_bam_index_build``) -- what
    ``samtools index`` / ``pysam.index`` do -- write it to `out` (default ``path + ".bai"``) and return it as a
    :class:`BamIndex`.  The file goes through the decoder of :func:`read_bam_gpu` up to the record fields (a file that
    decoder refuses is refused here with the same message); the bins, runs, linear windows and counts are taken from the
    records in HBM, and the host finishes the index.  `engine`: a :class:`plastid_amd.engine.Engine` (default: the shared
    one of device 0).  The file is written under a temporary name and renamed; an existing `out` is only replaced with
    ``overwrite=True``.  `timing`: optional dict that receives the laps in ms (``upload_ms``, ``inflate_ms``, ``chain_ms``,
    ``fields_ms``, ``index_ms``, ``readback_ms``, ``finish_ms``, ``total_ms``) and the counts (``records``, ``placed``,
    ``runs``, ``chunks``, ``bins``, ``linear``, ``n_no_coor``, ``mapped``, ``index_bytes``).
    ``ValueError``: a reference longer than 2^29 or an alignment that reaches beyond it (BAI cannot hold them)."""
    from . import _lib as clib
    path = os.fspath(path)
    if not os.path.isfile(path):
        raise IOError("No such file: %r" % (path,))
    dest = os.fspath(out) if out is not None else path + ".bai"
    if os.path.exists(dest) and not overwrite:
        raise FileExistsError("%s exists; pass overwrite=True to replace it" % dest)
    if engine is None:
        from .engine import default_engine
        engine = default_engine()
    L = clib.load()
    h = ctypes.c_void_p()
    clib.check(L.pc_bam_index_build(engine._h, os.fsencode(path), ctypes.byref(h)))
    try:
        data = _index_bytes(L, h)
        if timing is not None:
            ms, st = np.zeros(8, np.float64), np.zeros(8, np.int64)
            clib.check(L.pc_bam_index_timing(h, ms.ctypes.data_as(ctypes.c_void_p)))
            clib.check(L.pc_bam_index_stats(h, st.ctypes.data_as(ctypes.c_void_p)))
            timing.update(zip(("upload_ms", "inflate_ms", "chain_ms", "fields_ms", "index_ms", "readback_ms", "finish_ms", "total_ms"), ms.tolist()))
            timing.update(zip(("records", "placed", "runs", "chunks", "bins", "linear", "n_no_coor", "mapped"), st.tolist()))
            timing["index_bytes"] = len(data)
    finally:
        L.pc_bam_index_close(h)
    tmp = "%s.tmp%d" % (dest, os.getpid())
    try:
        with open(tmp, "wb") as fh:
            fh.write(data)
        if os.path.exists(dest) and not overwrite:   # (made by someone else in the meantime)
            raise FileExistsError("%s exists; pass overwrite=True to replace it" % dest)
        os.replace(tmp, dest)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    return BamIndex.from_bytes(data)


def _index_bytes(L, h):
    from . import _lib as clib
    n = ctypes.c_int64(0)
    clib.check(L.pc_bam_index_bytes(h, None, 0, ctypes.byref(n)))
    buf = ctypes.create_string_buffer(max(int(n.value), 1))
    clib.check(L.pc_bam_index_bytes(h, buf, int(n.value), ctypes.byref(n)))
    return buf.raw[:int(n.value)]


def _index_path(path, index, engine=None):
    """The `index` keyword of the region reads: ``None`` -> ``None`` (the lookup beside the file, and its error); a path ->
    that file; ``"build"`` -> the index beside the file, built first (:func:`build_index`) when there is none."""
    if index is None:
        return None
    if isinstance(index, str) and index == "build":
        if find_index(path) is None:
            build_index(path, engine=engine)
        return None
    return os.fspath(index)


def _pb_open(L, path, index_path):
    h = L.pb_open(os.fsencode(path)) if index_path is None else L.pb_open_indexed(os.fsencode(path), os.fsencode(index_path))
    if not h:
        raise IOError(L.pb_last_error().decode())
    return h


def resolve_regions(path, regions, index=None):
    """Resolve `regions` (``(chrom, start, end)`` or |GenomicSegments|) through the BAI index of `path` for a decoder
    that reads the file itself (:func:`read_bam_gpu`, :meth:`Engine.add_bam`): returns a dict with the merged index
    chunks of the regions, ``chunks`` (``uint64 [k, 2]``: ``[voff_beg, voff_end)`` pairs of virtual offsets, ascending and
    disjoint; bins + 16 kb linear index, SAM specification section 5 -- what ``AlignmentFile.fetch`` walks per region,
    genome_array.py:800-809), the span ``voff_begin``, ``voff_end`` that holds them all (0, 0: no chunk), the merged
    regions by reference id (``tid``, ``beg``, ``end`` arrays), the index's whole-file ``mapped`` count (-1: none) and the
    file's ``references`` / ``lengths``.
    `index`: ``None`` -- the index beside the file (``path + ".bai"`` or ``.bai`` in place of ``.bam``); a path -- that index
    file (a BAM file in a read-only directory); ``"build"`` -- the index beside the file, built on the GPU first when there
    is none (:func:`build_index`)."""
    L = _load()
    h = _pb_open(L, path, _index_path(path, index))
    try:
        regs = _region_tuples(regions)
        n = len(regs)
        names = (ctypes.c_char_p * max(n, 1))(*[os.fsencode(str(c)) for c, _, _ in regs])
        starts = np.array([int(s) for _, s, _ in regs], np.int64)
        ends = np.array([int(e) for _, _, e in regs], np.int64)
        nch, mapped, nm = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int(0)
        tid, beg, end = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int64), np.zeros(max(n, 1), np.int64)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
        cap = 8 * n + 64
        while True:
            cb, ce = np.zeros(cap, np.uint64), np.zeros(cap, np.uint64)
            rc = L.pb_resolve_chunks(h, n, names, p(starts), p(ends), cap, p(cb), p(ce), ctypes.byref(nch), ctypes.byref(mapped), ctypes.byref(nm),
                                     p(tid), p(beg), p(end))
            if rc != 0:
                raise ValueError(L.pb_last_error().decode())
            if nch.value <= cap:
                break
            cap = int(nch.value)
        nref = L.pb_nref(h)
        refs = [L.pb_ref_name(h, i).decode() for i in range(nref)]
        lens = [int(L.pb_ref_length(h, i)) for i in range(nref)]
    finally:
        L.pb_close(h)
    k, c = int(nm.value), int(nch.value)
    chunks = np.ascontiguousarray(np.stack([cb[:c], ce[:c]], axis=1))
    return dict(voff_begin=int(chunks[0, 0]) if c else 0, voff_end=int(chunks[:, 1].max()) if c else 0, chunks=chunks,
                tid=tid[:k].copy(), beg=beg[:k].copy(), end=end[:k].copy(), mapped=int(mapped.value), references=refs, lengths=lens)


def read_bam_gpu(path, engine, timing=None, regions=None, index=None):
    """The same :class:`PackedAlignments` as :func:`read_bam` gives for a whole file, decoded ON THE GPU: the file image
    goes to HBM as it is, the BGZF members are inflated there (one wave per member) and the BAM records decoded
    (``pc_bam_open``, ``csrc/bam_kernels.hip.h``); only the packed columns -- 13 bytes per record instead of the ~120 of
    an aligner's record -- come back.  `engine`: a :class:`plastid_amd.engine.Engine` (its device and stream are used).
    `timing`: optional dict that receives the phase times in ms and the member / byte counts.
    `timing` then also has ``uploaded_bytes`` (compressed bytes of the file that went to HBM) and ``runs`` (the contiguous
    stretches they came in).
    `regions`: as for :func:`read_bam` -- only the alignments that overlap one of them, through the BAI index: only the
    BGZF members the index chunks of the regions point to (and the leading ones with the header) are uploaded and
    inflated (``pc_bam_open_chunks``; the overlap test then drops the records of those members that no region wants);
    ``mapped`` is then the index's whole-file count, as pysam's.
    `index` (with `regions`): as for :func:`resolve_regions` -- an index file elsewhere, or ``"build"``."""
    import time
    from . import _lib as clib
    L = clib.load()
    if not os.path.isfile(path):
        raise IOError("No such file: %r" % (path,))
    t_0 = time.perf_counter()
    h = ctypes.c_void_p()
    span = None
    if regions is not None:
        span = resolve_regions(path, regions, index=_index_path(path, index, engine))
        pv = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
        cb, ce = np.ascontiguousarray(span["chunks"][:, 0]), np.ascontiguousarray(span["chunks"][:, 1])
        clib.check(L.pc_bam_open_chunks(engine._h, os.fsencode(path), len(cb), pv(cb), pv(ce), len(span["tid"]),
                                        pv(span["tid"]), pv(span["beg"]), pv(span["end"]), ctypes.byref(h)))
    else:
        # (the library maps the file itself: pages touched by all host threads at once, unmapped on a thread of its own)
        clib.check(L.pc_bam_open_path(engine._h, os.fsencode(path), ctypes.byref(h)))
    t_open = time.perf_counter()
    size = os.path.getsize(path)
    try:
        counts = np.zeros(8, np.int64)
        clib.check(L.pc_bam_counts(h, counts.ctypes.data_as(ctypes.c_void_p)))
        n, nrun, mapped, nw = int(counts[0]), int(counts[1]), int(counts[2]), int(counts[4])
        nref = L.pc_bam_nref(h)
        refs = [L.pc_bam_ref_name(h, i).decode() for i in range(nref)]
        lens = [int(L.pc_bam_ref_length(h, i)) for i in range(nref)]
        tid, pos = np.empty(n, np.int32), np.empty(n, np.int32)
        alen, flags, nblk = np.empty(n, np.uint16), np.empty(n, np.uint8), np.empty(n, np.uint8)
        bs, bl = np.empty(nrun, np.int32), np.empty(nrun, np.int32)
        wi, wa, wn = np.empty(nw, np.int64), np.empty(nw, np.int32), np.empty(nw, np.int32)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
        clib.check(L.pc_bam_read(h, p(tid), p(pos), p(alen), p(flags), p(nblk), p(bs), p(bl), p(wi), p(wa), p(wn)))
        flag16, mapq, qlen = np.empty(n, np.uint16), np.empty(n, np.uint8), np.empty(n, np.int32)
        clib.check(L.pc_bam_read_sam(h, p(flag16), p(mapq), p(qlen)))
        nh = np.empty(n, np.uint16)
        clib.check(L.pc_bam_read_nh(h, p(nh)))
        if timing is not None:
            timing.update(open_wall_ms=(t_open - t_0) * 1e3, read_wall_ms=(time.perf_counter() - t_open) * 1e3)
            ms = np.zeros(4, np.float64)
            clib.check(L.pc_bam_timing(h, p(ms)))
            st = np.zeros(4, np.int64)
            clib.check(L.pc_bam_stats(h, p(st)))
            timing.update(upload_ms=float(ms[0]), inflate_ms=float(ms[1]), chain_ms=float(ms[2]), decode_ms=float(ms[3]),
                          members=int(counts[5]), inflated_bytes=int(counts[6]), compressed_bytes=size, chain_restarts=int(counts[7]),
                          records=int(counts[3]), uploaded_bytes=int(st[0]), runs=int(st[1]))
    finally:
        t_c = time.perf_counter()
        L.pc_bam_close(h)
        if timing is not None:
            timing["close_ms"] = (time.perf_counter() - t_c) * 1e3
    wide = dict(wide_idx=wi, wide_alen=wa, wide_nblk=wn) if nw else {}
    if span is not None:   # `mapped` as pysam reports it: from the index, for the whole file
        if span["mapped"] < 0:
            import warnings
            warnings.warn("the BAI index of %s carries no mapped-read counts; using the number of alignments read" % path)
            mapped = n
        else:
            mapped = span["mapped"]
    out = PackedAlignments(tid, pos, alen, flags, nblk, bs, bl, references=refs, lengths=lens, mapped=mapped,
                           validate=False, flag16=flag16, mapq=mapq, qlen=qlen, nh=nh, **wide)   # the device decoder has checked every invariant validate() checks
    out.filename = path
    return out


def read_bam(path, threads=0, regions=None, index=None):
    """Read a coordinate-sorted BAM file into a :class:`PackedAlignments`.

    `regions`: iterable of ``(chrom, start, end)`` (0-based, half-open) or objects with those
    attributes (|GenomicSegments|): only the alignments that overlap one of them are read, through
    the file's BAI index (``path + ".bai"`` or ``.bai`` in place of ``.bam``) -- what the reference
    does region by region with ``AlignmentFile.fetch`` (genome_array.py:800-809), here for a whole
    query set at once.  Counts over positions inside the regions equal those of the whole file.
    `index` (with `regions`): ``None`` -- the index beside the file; a path -- that index file; ``"build"`` -- build the
    index on the GPU first when there is none (:func:`build_index`).

    ``mapped`` is the number of records with flag 0x4 unset (what ``pysam
    AlignmentFile.mapped`` reports from the index); unplaced reads are not staged
    (``fetch`` never returns them).  Raises ``ValueError`` for unsorted input, as pysam does."""
    L = _load()
    h = _pb_open(L, path, _index_path(path, index) if regions is not None else None)
    try:
        if regions is None:
            rc = L.pb_load(h, int(threads))
        else:
            regs = _region_tuples(regions)
            names = (ctypes.c_char_p * max(len(regs), 1))(*[os.fsencode(str(c)) for c, _, _ in regs])
            starts = np.array([int(s) for _, s, _ in regs], np.int64)
            ends = np.array([int(e) for _, _, e in regs], np.int64)
            rc = L.pb_load_regions(h, int(threads), len(regs), names, starts.ctypes.data_as(ctypes.c_void_p),
                                   ends.ctypes.data_as(ctypes.c_void_p))
        if rc != 0:
            msg = L.pb_last_error().decode()
            raise ValueError(msg)
        counts = np.zeros(4, np.int64)
        L.pb_counts(h, counts.ctypes.data_as(ctypes.c_void_p))
        n, nrun, mapped = int(counts[0]), int(counts[1]), int(counts[2])
        nref = L.pb_nref(h)
        refs = [L.pb_ref_name(h, i).decode() for i in range(nref)]
        lens = [int(L.pb_ref_length(h, i)) for i in range(nref)]
        tid = np.empty(n, np.int32)
        pos = np.empty(n, np.int32)
        alen = np.empty(n, np.uint16)
        flags = np.empty(n, np.uint8)
        nblk = np.empty(n, np.uint8)
        bs = np.empty(nrun, np.int32)
        bl = np.empty(nrun, np.int32)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
        L.pb_fill(h, p(tid), p(pos), p(alen), p(flags), p(nblk), p(bs), p(bl))
        wide = {}
        nw = int(L.pb_wide_count(h))
        if nw > 0:   # reads beyond the 16-bit / 8-bit columns: true lengths / run counts aside (packing.py)
            wi, wa, wn = np.empty(nw, np.int64), np.empty(nw, np.int32), np.empty(nw, np.int32)
            L.pb_fill_wide(h, p(wi), p(wa), p(wn))
            wide = dict(wide_idx=wi, wide_alen=wa, wide_nblk=wn)
        # the SAM FLAG word, MAPQ and l_seq of every record: what read filters may look at (genome_array.py:697-722)
        flag16, mapq, qlen = np.empty(n, np.uint16), np.empty(n, np.uint8), np.empty(n, np.int32)
        L.pb_fill_sam(h, p(flag16), p(mapq), p(qlen))
        nh = np.empty(n, np.uint16)   # ... and the NH:i tag (0: none): read.get_tag("NH") / has_tag("NH")
        L.pb_fill_nh(h, p(nh))
    finally:
        L.pb_close(h)
    if mapped < 0:   # an index without the per-reference counts samtools writes
        import warnings
        warnings.warn("the BAI index of %s carries no mapped-read counts; using the number of alignments read" % path)
        mapped = n
    out = PackedAlignments(tid, pos, alen, flags, nblk, bs, bl, references=refs, lengths=lens, mapped=mapped,
                           validate=False, flag16=flag16, mapq=mapq, qlen=qlen, nh=nh, **wide)   # the native reader has checked every invariant validate() checks
    out.filename = path
    return out
