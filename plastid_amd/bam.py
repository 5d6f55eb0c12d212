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

from ._hostlib import call, load as _load
from .build import BAM_LIB  # noqa: F401  (the path as built; the library is opened at ``build.BAM_LIB``, read at the first load)
from .packing import PackedAlignments


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


def is_sam_path(path):
    """Whether `path` is read as SAM TEXT: its name ends in ``.sam`` (any letter case).  Nothing else makes a path SAM."""
    return isinstance(path, (str, os.PathLike)) and os.fspath(path).lower().endswith(".sam")


def _refuse_compressed_sam(path):
    with open(path, "rb") as fh:
        if fh.read(2) == b"\x1f\x8b":
            raise ValueError("%s: compressed SAM (gzip / BGZF) is not supported: decompress it, or convert it to BAM" % (path,))


def _pb_open_sam(L, path):
    if not os.path.isfile(path):
        raise IOError("No such file: %r" % (path,))
    return call(L.pb_open_sam, os.fsencode(path))   # (ValueError: compressed, or a malformed header)


def sam_header(path):
    """``(references, lengths)`` of a SAM text file from its ``@SQ`` header lines (``SN``, ``LN``; in line order) -- what
    ``pysam.AlignmentFile(path).references / .lengths`` give.  ``ValueError`` for a header the readers refuse (an ``@SQ``
    line without ``SN`` or ``LN``, a repeated ``SN``, alignment lines without any ``@SQ``) and for compressed SAM."""
    L = _load()
    h = _pb_open_sam(L, os.fspath(path))
    try:
        nref = L.pb_nref(h)
        return [L.pb_ref_name(h, i).decode() for i in range(nref)], [int(L.pb_ref_length(h, i)) for i in range(nref)]
    finally:
        L.pb_close(h)


def read_sam(path, threads=0, sort=False, timing=None):
    """Read a SAM TEXT file -- an aligner's output as it is written (bowtie, bowtie2, bwa, hisat2, minimap2; STAR's
    ``Aligned.out.sam``) -- into the :class:`PackedAlignments` that :func:`read_bam` gives for the same records in a BAM
    file, ``flag16``, ``mapq``, ``qlen`` and ``nh`` included: no ``samtools view -b`` in front (``pb_open_sam``; the lines
    are parsed by ``csrc/sam_host.h`` on the worker pool, dealt out by byte ranges cut at line ends).
    The file must be coordinate sorted unless `sort` is true (as for :func:`read_bam`: any record order, ``file_order``
    set when records moved).  ``ValueError``: a malformed line (``"<path>: SAM line <n>: <what>"``, the lowest line
    first), a file out of order without `sort`, compressed SAM.  `timing`: as for :func:`read_bam`."""
    return read_bam(os.fspath(path), threads=threads, sort=sort, timing=timing, _sam=True)


def read_sam_gpu(path, engine, timing=None, sort=False):
    """:func:`read_sam`, parsed ON THE GPU (``pc_sam_open_path_flags``, ``csrc/sam_kernels.hip.h``): the text crosses PCIe
    once, line starts, fields and CIGAR strings are parsed by kernels that run the host reader's line parser, and the
    records go through the placement of :func:`read_bam_gpu` (order checks, or the radix sort with `sort`).  The result
    equals ``read_sam(path, sort=sort)`` array for array, ``file_order`` included, and a refused file raises the same text.
    `timing`: optional dict; receives ``upload_ms``, ``lines_ms`` (line starts), ``fields_ms``, ``place_ms`` (placement and
    columns), ``records``, ``uploaded_bytes`` (the text bytes) and, with `sort`, what :func:`read_bam_gpu` adds."""
    return read_bam_gpu(os.fspath(path), engine, timing=timing, sort=sort, _sam=True)


def _region_tuples(regions):
    return [(r.chrom, r.start, r.end) if hasattr(r, "chrom") else tuple(r) for r in regions]


_BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
_BGZF_PIECE = 0xff00


def _bgzf_wrap(payload):
    """`payload` as a BGZF file: members of at most 0xff00 payload bytes, then the 28-byte EOF block (SAM specification 4.1)."""
    import struct
    import zlib
    out = []
    for at in range(0, len(payload), _BGZF_PIECE):
        piece = payload[at:at + _BGZF_PIECE]
        co = zlib.compressobj(6, zlib.DEFLATED, -15)
        body = co.compress(piece) + co.flush()
        out.append(b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(body) + 25) + body +
                   struct.pack("<II", zlib.crc32(piece) & 0xffffffff, len(piece)))
    out.append(_BGZF_EOF)
    return b"".join(out)


def _bgzf_unwrap(data):
    """The payload of the BGZF file `data`, member by member; ``ValueError`` for a damaged member or one that is cut off.
    A file of whole members without the end-of-file block is read as it is, as htslib and the native reader do."""
    import struct
    import zlib
    o, out = 0, []
    try:
        while o < len(data):
            if len(data) - o < 18 or data[o:o + 4] != b"\x1f\x8b\x08\x04":
                raise ValueError("truncated CSI index (bad BGZF member header)")
            xlen, = struct.unpack_from("<H", data, o + 10)
            bsize, x = -1, o + 12
            while x + 4 <= o + 12 + xlen <= len(data):
                slen, = struct.unpack_from("<H", data, x + 2)
                if data[x:x + 2] == b"BC" and slen == 2 and x + 6 <= len(data):
                    bsize, = struct.unpack_from("<H", data, x + 4)
                x += 4 + slen
            if bsize < 0 or bsize + 1 < 12 + xlen + 8 or o + bsize + 1 > len(data):
                raise ValueError("truncated CSI index (BGZF member)")
            crc, isize = struct.unpack_from("<II", data, o + bsize + 1 - 8)
            piece = zlib.decompressobj(-15).decompress(data[o + 12 + xlen:o + bsize + 1 - 8])
            if len(piece) != isize or zlib.crc32(piece) & 0xffffffff != crc:
                raise ValueError("damaged CSI index (BGZF member)")
            out.append(piece)
            o += bsize + 1
    except zlib.error:
        raise ValueError("damaged CSI index (BGZF member)")
    return b"".join(out)


class BamIndex(object):
    """A BAI or CSI index (SAM specification 5.2, 5.3), parsed: what ``samtools index [-c]`` writes and :func:`build_index` builds.

    ``bins``: per reference, a dict from bin number to a ``uint64 [k, 2]`` array of chunks ``[begin, end)`` (virtual
    offsets); ``linear``: per reference, the ``uint64`` offsets of its 16 kb windows (BAI; empty arrays for a CSI);
    ``meta``: per reference, ``None`` or ``(file begin, file end, mapped, unmapped)`` from samtools' pseudo-bin
    (``meta_bin``: 37450 for a BAI); ``n_no_coor``: the records without a reference; ``mapped``: the sum of the per-reference
    mapped counts (pysam's ``AlignmentFile.mapped``), -1 when the index carries none.
    ``fmt``: ``"bai"`` or ``"csi"``; ``min_shift``, ``depth``: the shape -- leaves of ``2**min_shift`` positions, ``depth``
    levels below the root, (14, 5) for a BAI; ``loff``: per reference, a dict from bin number to the offset of the bin's
    first window (CSI; empty dicts for a BAI).
    Two indexes are equal when their parsed content is: the order of the bins in the file is not part of it
    (htslib writes them in the order of its hash table; :meth:`to_bytes` writes them ascending, the pseudo-bin last)."""

    META_BIN = 37450

    def __init__(self, bins, linear, meta, n_no_coor=0, fmt="bai", min_shift=14, depth=5, loff=None):
        self.bins, self.linear, self.meta, self.n_no_coor = bins, linear, meta, int(n_no_coor)
        if fmt not in ("bai", "csi"):
            raise ValueError("fmt must be 'bai' or 'csi'")
        self.fmt, self.min_shift, self.depth = fmt, int(min_shift), int(depth)
        self.loff = loff if loff is not None else [{} for _ in bins]

    @property
    def n_ref(self):
        return len(self.bins)

    @property
    def meta_bin(self):
        return ((1 << (3 * self.depth + 3)) - 1) // 7 + 1

    @property
    def mapped(self):
        have = [m for m in self.meta if m is not None]
        return sum(int(m[2]) for m in have) if have else -1

    @classmethod
    def from_bytes(cls, data):
        """Parse a BAI file, the payload of a CSI file, or a CSI file as it lies on disk (BGZF)."""
        import struct
        data = bytes(data)
        if data[:2] == b"\x1f\x8b":
            data = _bgzf_unwrap(data)
            if data[:4] != b"CSI\x01":
                raise ValueError("not a CSI index")
        csi = data[:4] == b"CSI\x01"
        if csi:
            if len(data) < 20:
                raise ValueError("truncated CSI index")
            min_shift, depth, l_aux = struct.unpack_from("<iii", data, 4)
            if not (1 <= min_shift <= 30 and 0 <= depth <= 9 and min_shift + 3 * depth <= 40):
                raise ValueError("corrupt CSI index (min_shift / depth)")
            if l_aux < 0 or 16 + l_aux + 4 > len(data):
                raise ValueError("truncated CSI index")
            o = 16 + l_aux
            meta_bin = ((1 << (3 * depth + 3)) - 1) // 7 + 1
        elif len(data) >= 8 and data[:4] == b"BAI\x01":
            o, min_shift, depth, meta_bin = 4, 14, 5, cls.META_BIN
        else:
            raise ValueError("not a BAI index")
        kind = "CSI" if csi else "BAI"
        head = 16 if csi else 8
        n_ref, = struct.unpack_from("<i", data, o)
        o += 4
        bins, linear, meta, loffs = [], [], [], []
        try:
            for _ in range(n_ref):
                n_bin, = struct.unpack_from("<i", data, o)
                o += 4
                if n_bin < 0 or o + head * n_bin > len(data):
                    raise struct.error("bins")
                rb, rm, rl = {}, None, {}
                for _ in range(n_bin):
                    if csi:
                        b, lo, nc = struct.unpack_from("<IQi", data, o)
                    else:
                        (b, nc), lo = struct.unpack_from("<Ii", data, o), 0
                    o += head
                    if nc < 0 or o + 16 * nc > len(data):
                        raise struct.error("chunks")
                    ch = np.frombuffer(data, "<u8", 2 * nc, o).reshape(nc, 2).copy()
                    o += 16 * nc
                    if b == meta_bin and nc >= 2:
                        rm = tuple(int(x) for x in ch[:2].ravel())
                    elif b != meta_bin:
                        rb[int(b)] = ch
                        if csi:
                            rl[int(b)] = int(lo)
                if csi:
                    linear.append(np.zeros(0, np.uint64))
                else:
                    n_intv, = struct.unpack_from("<i", data, o)
                    o += 4
                    if n_intv < 0 or o + 8 * n_intv > len(data):
                        raise struct.error("linear")
                    linear.append(np.frombuffer(data, "<u8", n_intv, o).copy())
                    o += 8 * n_intv
                bins.append(rb)
                meta.append(rm)
                loffs.append(rl)
            n_no_coor = struct.unpack_from("<Q", data, o)[0] if o + 8 <= len(data) else 0   # (optional in the format)
        except struct.error:
            raise ValueError("truncated %s index" % kind)
        return cls(bins, linear, meta, n_no_coor, "csi" if csi else "bai", min_shift, depth, loffs)

    @classmethod
    def from_file(cls, path):
        with open(path, "rb") as fh:
            return cls.from_bytes(fh.read())

    def payload(self):
        """The index serialised without compression: the BAI file, or what the BGZF members of the CSI file hold."""
        import struct
        csi = self.fmt == "csi"
        out = [b"CSI\x01" + struct.pack("<iii", self.min_shift, self.depth, 0) if csi else b"BAI\x01", struct.pack("<i", self.n_ref)]
        for rb, lin, rm, rl in zip(self.bins, self.linear, self.meta, self.loff):
            out.append(struct.pack("<i", len(rb) + (rm is not None)))
            for b in sorted(rb):
                ch = np.ascontiguousarray(rb[b], "<u8")
                out.append(struct.pack("<IQi", b, rl.get(b, 0), len(ch)) if csi else struct.pack("<Ii", b, len(ch)))
                out.append(ch.tobytes())
            if rm is not None:
                out.append(struct.pack("<IQi4Q", self.meta_bin, 0, 2, *rm) if csi else struct.pack("<Ii4Q", self.meta_bin, 2, *rm))
            if not csi:
                out.append(struct.pack("<i", len(lin)))
                out.append(np.ascontiguousarray(lin, "<u8").tobytes())
        out.append(struct.pack("<Q", self.n_no_coor))
        return b"".join(out)

    def to_bytes(self):
        """The bytes of the index FILE: a BAI as it is, a CSI in BGZF members with the end-of-file block."""
        data = self.payload()
        return _bgzf_wrap(data) if self.fmt == "csi" else data

    def write(self, path):
        with open(path, "wb") as fh:
            fh.write(self.to_bytes())

    def __eq__(self, other):
        if not isinstance(other, BamIndex):
            return NotImplemented
        if self.n_ref != other.n_ref or self.n_no_coor != other.n_no_coor or list(self.meta) != list(other.meta):
            return False
        if (self.fmt, self.min_shift, self.depth) != (other.fmt, other.min_shift, other.depth) or list(self.loff) != list(other.loff):
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
        shape = "" if self.fmt == "bai" else "CSI min_shift=%d depth=%d, " % (self.min_shift, self.depth)
        return "BamIndex(%s%d references, %d bins, %d chunks, n_no_coor=%d, mapped=%d)" % (
            shape, self.n_ref, sum(len(b) for b in self.bins), sum(len(c) for b in self.bins for c in b.values()), self.n_no_coor, self.mapped)


def find_index(path):
    """The index file the region reads find beside `path`, or ``None``: ``path + ".bai"``, ``.bai`` in place of the
    extension, then ``path + ".csi"`` and ``.csi`` in place of the extension."""
    path = os.fspath(path)
    stem = path[:-4] if len(path) > 4 else None
    for cand in (path + ".bai", stem + ".bai" if stem else None, path + ".csi", stem + ".csi" if stem else None):
        if cand and os.path.isfile(cand):
            return cand
    return None


def build_index(path, engine=None, out=None, overwrite=False, timing=None, fmt="bai", min_shift=14):
    """Build the index of the coordinate-sorted BAM file `path` ON THE GPU (``pc_bam_index_build`` /
    ``pc_bam_index_build_csi``) -- what ``samtools index [-c]`` / ``pysam.index`` do -- write it to `out` (default
    ``path + ".bai"``, or ``path + ".csi"``) and return it as a :class:`BamIndex`.  The file goes through the decoder of
    :func:`read_bam_gpu` up to the record fields (a file that decoder refuses is refused here with the same message); the
    bins, runs, linear windows and counts are taken from the records in HBM, and the host finishes the index.
    `fmt`: ``"bai"``, or ``"csi"`` -- the index for references longer than 2^29: leaves of ``2**min_shift`` positions
    (8 .. 30) and the depth the longest reference asks for, as htslib's ``sam_index_build(fn, min_shift)``; its windows
    stay on the GPU (at most 2^28 of them: a larger `min_shift` has fewer), and the file is the payload in BGZF members.
    `engine`: a :class:`plastid_amd.engine.Engine` (default: the shared one of device 0).  The file is written under a
    temporary name and renamed; an existing `out` is only replaced with ``overwrite=True``.  `timing`: optional dict that
    receives the laps in ms (``upload_ms``, ``inflate_ms``, ``chain_ms``, ``fields_ms``, ``index_ms``, ``readback_ms``,
    ``finish_ms``, ``total_ms``), the counts (``records``, ``placed``, ``runs``, ``chunks``, ``bins``, ``linear``,
    ``n_no_coor``, ``mapped``, ``index_bytes``) and the shape (``min_shift``, ``depth``).
    ``ValueError``: for a BAI, a reference longer than 2^29 or an alignment that reaches beyond it (BAI cannot hold them)
    and a `min_shift` other than 14; for a CSI, a `min_shift` out of range, an alignment beyond the index's reach, too many windows."""
    from . import _lib as clib
    if fmt not in ("bai", "csi"):
        raise ValueError("fmt must be 'bai' or 'csi', not %r" % (fmt,))
    min_shift = int(min_shift)
    if fmt == "bai" and min_shift != 14:
        raise ValueError("a BAI index has min_shift 14; pass fmt='csi' for another leaf size")
    path = os.fspath(path)
    if is_sam_path(path):
        raise ValueError("build_index: %s is SAM text, which has no index; convert it to BAM for region reads" % (path,))
    if not os.path.isfile(path):
        raise IOError("No such file: %r" % (path,))
    dest = os.fspath(out) if out is not None else path + "." + fmt
    if os.path.exists(dest) and not overwrite:
        raise FileExistsError("%s exists; pass overwrite=True to replace it" % dest)
    if engine is None:
        from .engine import default_engine
        engine = default_engine()
    L = clib.load()
    h = ctypes.c_void_p()
    if fmt == "csi":
        clib.check(L.pc_bam_index_build_csi(engine._h, os.fsencode(path), min_shift, ctypes.byref(h)))
    else:
        clib.check(L.pc_bam_index_build(engine._h, os.fsencode(path), ctypes.byref(h)))
    try:
        data = _index_bytes(L, h)
        if timing is not None:
            ms, st = np.zeros(8, np.float64), np.zeros(8, np.int64)
            clib.check(L.pc_bam_index_timing(h, ms.ctypes.data_as(ctypes.c_void_p)))
            clib.check(L.pc_bam_index_stats(h, st.ctypes.data_as(ctypes.c_void_p)))
            timing.update(zip(("upload_ms", "inflate_ms", "chain_ms", "fields_ms", "index_ms", "readback_ms", "finish_ms", "total_ms"), ms.tolist()))
            timing.update(zip(("records", "placed", "runs", "chunks", "bins", "linear", "n_no_coor", "mapped"), st.tolist()))
    finally:
        L.pc_bam_index_close(h)
    idx = BamIndex.from_bytes(data)
    if fmt == "csi":
        data = _bgzf_wrap(data)   # (the library hands the payload over: it does not link zlib)
    if timing is not None:
        timing.update(index_bytes=len(data), min_shift=idx.min_shift, depth=idx.depth)
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
    return idx


def _index_bytes(L, h):
    from . import _lib as clib
    n = ctypes.c_int64(0)
    clib.check(L.pc_bam_index_bytes(h, None, 0, ctypes.byref(n)))
    buf = ctypes.create_string_buffer(max(int(n.value), 1))
    clib.check(L.pc_bam_index_bytes(h, buf, int(n.value), ctypes.byref(n)))
    return buf.raw[:int(n.value)]


def _index_path(path, index, engine=None):
    """The `index` keyword of the region reads: ``None`` -> ``None`` (the lookup beside the file, and its error); a path ->
    that file; ``"build"`` / ``"build-csi"`` -> the index beside the file, built first (:func:`build_index`, as a BAI / as
    a CSI of min_shift 14) when there is none."""
    if index is None:
        return None
    if isinstance(index, str) and index in ("build", "build-csi"):
        if find_index(path) is None:
            build_index(path, engine=engine, fmt="csi" if index == "build-csi" else "bai")
        return None
    return os.fspath(index)


def _pb_open(L, path, index_path):
    if index_path is None:
        return call(L.pb_open, os.fsencode(path), exc=IOError)
    return call(L.pb_open_indexed, os.fsencode(path), os.fsencode(index_path), exc=IOError)


def resolve_regions(path, regions, index=None):
    """Resolve `regions` (``(chrom, start, end)`` or |GenomicSegments|) through the BAI or CSI index of `path` for a decoder
    that reads the file itself (:func:`read_bam_gpu`, :meth:`Engine.add_bam`): returns a dict with the merged index
    chunks of the regions, ``chunks`` (``uint64 [k, 2]``: ``[voff_beg, voff_end)`` pairs of virtual offsets, ascending and
    disjoint; bins + 16 kb linear index, SAM specification section 5 -- what ``AlignmentFile.fetch`` walks per region,
    genome_array.py:800-809), the span ``voff_begin``, ``voff_end`` that holds them all (0, 0: no chunk), the merged
    regions by reference id (``tid``, ``beg``, ``end`` arrays), the index's whole-file ``mapped`` count (-1: none) and the
    file's ``references`` / ``lengths``.
    `index`: ``None`` -- the index beside the file (``path + ".bai"``, ``.bai`` in place of ``.bam``, then the same with ``.csi``); a path -- that index
    file (a BAM file in a read-only directory), BAI or CSI; ``"build"`` -- the index beside the file, built on the GPU
    first when there is none (:func:`build_index`); ``"build-csi"`` -- the same, built as a CSI (references beyond 2^29)."""
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
            call(L.pb_resolve_chunks, h, n, names, p(starts), p(ends), cap, p(cb), p(ce), ctypes.byref(nch), ctypes.byref(mapped), ctypes.byref(nm),
                 p(tid), p(beg), p(end))
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


def _no_sort_with_regions(sort, regions):
    if sort and regions is not None:
        raise ValueError("sort=True cannot be combined with regions=: a region read goes through the index of a coordinate-sorted file")


def read_bam_gpu(path, engine, timing=None, regions=None, index=None, sort=False, _sam=False):
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
    `index` (with `regions`): as for :func:`resolve_regions` -- an index file elsewhere, ``"build"`` or ``"build-csi"``.
    `sort`: as for :func:`read_bam` -- a whole file in any record order, coordinate sorted on the GPU at decode
    (``pc_bam_open_path_flags`` with ``PC_BAM_SORT``: one key kernel, one stable radix sort of the record numbers, and the
    column kernel scatters by sorted rank); the result equals ``read_bam(path, sort=True)``, ``file_order`` included.
    `timing` then also has ``sort_ms`` (GPU time of the sort phase), ``sorted_input``, ``records_moved`` and ``sort_key_bits``."""
    import time
    from . import _lib as clib
    _no_sort_with_regions(sort, regions)
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
    elif _sam:   # (read_sam_gpu: SAM text)
        clib.check(L.pc_sam_open_path_flags(engine._h, os.fsencode(path), clib.PC_BAM_SORT if sort else 0, ctypes.byref(h)))
    else:
        # (the library maps the file itself: pages touched by all host threads at once, unmapped on a thread of its own)
        if sort:
            clib.check(L.pc_bam_open_path_flags(engine._h, os.fsencode(path), clib.PC_BAM_SORT, ctypes.byref(h)))
        else:
            clib.check(L.pc_bam_open_path(engine._h, os.fsencode(path), ctypes.byref(h)))
    t_open = time.perf_counter()
    file_order = None
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
        if sort:
            sst, sms = np.zeros(4, np.int64), ctypes.c_double(0.0)
            clib.check(L.pc_bam_sort_stats(h, p(sst), ctypes.byref(sms)))
            if int(sst[2]):
                file_order = np.empty(n, np.int64)
                clib.check(L.pc_bam_read_file_order(h, p(file_order)))
            if timing is not None:
                timing.update(sort_ms=float(sms.value), sorted_input=bool(sst[1]), records_moved=int(sst[2]), sort_key_bits=int(sst[3]))
        if timing is not None:
            timing.update(open_wall_ms=(t_open - t_0) * 1e3, read_wall_ms=(time.perf_counter() - t_open) * 1e3)
            ms = np.zeros(4, np.float64)
            clib.check(L.pc_bam_timing(h, p(ms)))
            st = np.zeros(4, np.int64)
            clib.check(L.pc_bam_stats(h, p(st)))
            if _sam:
                timing.update(lines_ms=float(ms[1]), fields_ms=float(ms[2]), place_ms=float(ms[3]))
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
    out.file_order = file_order
    return out


def read_bam(path, threads=0, regions=None, index=None, sort=False, timing=None, _sam=False):
    """Read a coordinate-sorted BAM file into a :class:`PackedAlignments`.

    `regions`: iterable of ``(chrom, start, end)`` (0-based, half-open) or objects with those
    attributes (|GenomicSegments|): only the alignments that overlap one of them are read, through
    the file's BAI or CSI index (``path + ".bai"``, ``.bai`` in place of ``.bam``, then ``.csi`` likewise) -- what the reference
    does region by region with ``AlignmentFile.fetch`` (genome_array.py:800-809), here for a whole
    query set at once.  Counts over positions inside the regions equal those of the whole file.
    `index` (with `regions`): ``None`` -- the index beside the file (BAI or CSI); a path -- that index file; ``"build"`` --
    build the index on the GPU first when there is none (:func:`build_index`); ``"build-csi"`` -- build it as a CSI.

    ``mapped`` is the number of records with flag 0x4 unset (what ``pysam
    AlignmentFile.mapped`` reports from the index); unplaced reads are not staged
    (``fetch`` never returns them).  Raises ``ValueError`` for unsorted input, as pysam does.

    `sort` (whole files only; with `regions` a ``ValueError``): ``True`` -- the file may be in ANY record order (an
    aligner's output, a name-sorted or collated file): the placed records are staged in the stable order of (reference,
    POS, reverse strand), a coordinate sorter's comparator, without a ``samtools sort`` in front.  A file that is in
    order already is returned exactly as without the keyword.  The result's ``file_order`` is ``None`` unless records
    were moved, else the 0-based record number in the file (all records counted) of every staged record.
    `timing`: optional dict; with `sort` it receives ``sort_ms`` (0.0: the host decoder does not time it),
    ``sorted_input`` and ``records_moved``."""
    _no_sort_with_regions(sort, regions)
    L = _load()
    h = _pb_open_sam(L, path) if _sam else _pb_open(L, path, _index_path(path, index) if regions is not None else None)
    try:
        if regions is None:
            call(L.pb_load_sorted if sort else L.pb_load, h, int(threads))
        else:
            regs = _region_tuples(regions)
            names = (ctypes.c_char_p * max(len(regs), 1))(*[os.fsencode(str(c)) for c, _, _ in regs])
            starts = np.array([int(s) for _, s, _ in regs], np.int64)
            ends = np.array([int(e) for _, _, e in regs], np.int64)
            call(L.pb_load_regions, h, int(threads), len(regs), names, starts.ctypes.data_as(ctypes.c_void_p), ends.ctypes.data_as(ctypes.c_void_p))
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
        file_order = None
        if sort:
            sst = np.zeros(3, np.int64)
            L.pb_sort_stats(h, p(sst))
            if int(sst[2]):
                file_order = np.empty(n, np.int64)
                L.pb_file_order(h, p(file_order))
            if timing is not None:
                timing.update(sort_ms=0.0, sorted_input=bool(sst[1]), records_moved=int(sst[2]))
    finally:
        L.pb_close(h)
    if mapped < 0:   # an index without the per-reference counts samtools writes
        import warnings
        warnings.warn("the BAI index of %s carries no mapped-read counts; using the number of alignments read" % path)
        mapped = n
    out = PackedAlignments(tid, pos, alen, flags, nblk, bs, bl, references=refs, lengths=lens, mapped=mapped,
                           validate=False, flag16=flag16, mapq=mapq, qlen=qlen, nh=nh, **wide)   # the native reader has checked every invariant validate() checks
    out.filename = path
    out.file_order = file_order
    return out
