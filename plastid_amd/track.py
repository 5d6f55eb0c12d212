"""Count tracks -- bedGraph, variableStep and fixedStep wiggle text -- read back in.

:class:`GenomeArray` is the reference's ``GenomeArray`` (plastid/genomics/genome_array.py:1323-1533) as a read-and-count
class: float64 values per contig, strand and position in HBM, filled by :meth:`GenomeArray.add_from_wiggle` (:1978-1994;
the text is parsed by the kernels of ``csrc/track_kernels.hip.h``) and read by ``get`` / ``[]``, ``get_counts_batch`` and
``SegmentChain.get_counts`` / ``get_masked_counts`` through one gather kernel.  :func:`read_wiggle` is the reference's
``WiggleReader`` (plastid/readers/wiggle.py:43-174) on the host, built from the same ``csrc/track_host.h`` the kernels
compile: the model of the device import, and the way to read a track without a GPU.

Not here: ``__setitem__``, arithmetic between arrays, ``add_from_bowtie``, ``nonzero``, export, BigWig.
"""
import ctypes
import os
from collections import OrderedDict

import numpy as np

from . import _lib
from ._lib import check
from .roitools import SegmentChain


def _text_of(fh_or_path):
    """``(bytes, name)`` of a path or of an open file (text or binary)."""
    if isinstance(fh_or_path, (str, bytes, os.PathLike)):
        path = os.fspath(fh_or_path)
        if not os.path.isfile(path):
            raise IOError("No such file: %r" % (path,))
        with open(path, "rb") as fh:
            return fh.read(), os.fsdecode(path)
    data = fh_or_path.read()
    if isinstance(data, str):
        data = data.encode("utf-8")
    name = getattr(fh_or_path, "name", None)
    return bytes(data), name if isinstance(name, str) else "<memory>"


class WiggleTable(object):
    """What :func:`read_wiggle` returns: one row per yielded ``(chrom, start, stop, value)`` in file order, as columns.
    ``chrom`` indexes ``names`` (contigs in order of first appearance); ``line`` is the row's 0-based line and ``escaped``
    whether one of its tokens was not *plain* (``csrc/track_host.h``); ``stats``: lines, yielded lines, escaped lines,
    state records."""

    def __init__(self, names, chrom, start, stop, value, line, escaped, stats):
        self.names, self.chrom, self.start, self.stop, self.value = names, chrom, start, stop, value
        self.line, self.escaped, self.stats = line, escaped, stats

    def __len__(self):
        return len(self.chrom)

    def tuples(self):
        """The reader's tuples, as ``WiggleReader`` yields them."""
        return [(self.names[c], int(a), int(b), float(v)) for c, a, b, v in zip(self.chrom, self.start, self.stop, self.value)]


def read_wiggle(fh_or_path):
    """Read a bedGraph / wiggle text on the host (``pb_track_read``): the rows ``WiggleReader(fh)`` yields, 0-based half
    open.  ``ValueError("<path>: track line <n>: <what>")`` for the first malformed line."""
    from .bam import _load
    L = _load()
    if not hasattr(L.pb_track_read, "_bound"):
        vp = ctypes.c_void_p
        L.pb_track_read.restype = vp
        L.pb_track_read.argtypes = [vp, ctypes.c_int64, ctypes.c_char_p]
        L.pb_track_close.argtypes = [vp]
        L.pb_track_rows.restype = ctypes.c_int64
        L.pb_track_rows.argtypes = [vp]
        L.pb_track_nchrom.argtypes = [vp]
        L.pb_track_chrom.restype = ctypes.c_char_p
        L.pb_track_chrom.argtypes = [vp, ctypes.c_int]
        L.pb_track_fill.argtypes = [vp] * 7
        L.pb_track_stats.argtypes = [vp, vp]
        L.pb_track_read._bound = True
    data, name = _text_of(fh_or_path)
    buf = ctypes.create_string_buffer(data, len(data)) if data else None
    h = L.pb_track_read(ctypes.cast(buf, ctypes.c_void_p) if buf is not None else None, len(data), os.fsencode(name))
    if not h:
        raise ValueError(L.pb_last_error().decode("utf-8", "replace"))
    try:
        n = int(L.pb_track_rows(h))
        names = [L.pb_track_chrom(h, i).decode("utf-8", "replace") for i in range(L.pb_track_nchrom(h))]
        chrom, start, stop = np.zeros(n, np.int32), np.zeros(n, np.int64), np.zeros(n, np.int64)
        value, line, escaped = np.zeros(n, np.float64), np.zeros(n, np.int64), np.zeros(n, np.uint8)
        if L.pb_track_fill(h, *[a.ctypes.data for a in (chrom, start, stop, value, line, escaped)]) != 0:
            raise ValueError(L.pb_last_error().decode())
        stats = np.zeros(4, np.int64)
        L.pb_track_stats(h, stats.ctypes.data)
    finally:
        L.pb_track_close(h)
    return WiggleTable(names, chrom, start, stop, value, line, escaped.astype(bool),
                       dict(zip(("lines", "yielded", "escaped", "states"), (int(x) for x in stats))))


class GenomeArray(object):
    """Device-resident ``GenomeArray``: values live in HBM as float64 cells per (contig, strand).

    `chr_lengths`: ``{name: length}`` declared up front (they come first in ``chroms()``); `strands`: the strand names;
    `min_chr_size`: the length a contig met in a file is born with; `engine`: an :class:`~plastid_amd.engine.Engine` to
    share (default: one of its own on GPU 0).  Cells are stored up to the furthest end written, whatever the reported
    length; positions beyond read as zero."""

    def __init__(self, chr_lengths=None, strands=("+", "-"), min_chr_size=10000000, engine=None):
        from .engine import Engine
        self._strands = tuple(strands)
        self.min_chr_size = int(min_chr_size)
        self._own_engine = engine is None
        self._engine = Engine(0) if engine is None else engine
        self._lib = _lib.load()
        self._normalize = False
        self._h = None
        h = ctypes.c_void_p()
        check(self._lib.pc_track_create(self._engine._h, len(self._strands), self.min_chr_size, ctypes.byref(h)), "pc_track_create")
        self._h = h
        for name, length in (chr_lengths or {}).items():
            check(self._lib.pc_track_declare(self._h, os.fsencode(name), int(length)))
        self._names = None

    def close(self):
        if self._h is not None:
            if self._engine._finalizer.alive:      # (an engine that is gone took its tracks with it)
                self._lib.pc_track_destroy(self._h)
            self._h = None
            if self._own_engine:
                self._engine.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- the file side
    def add_from_wiggle(self, fh_or_path, strand):
        """Add the values of a bedGraph / wiggle file (a path, or an open file) onto `strand` (genome_array.py:1978-1994).
        Overlapping lines add in file order, a second call adds on top of the first.  Lines that overlap nothing -- the
        normal case, the formats forbid overlap -- are applied in parallel; a cluster of overlapping lines is applied cell
        by cell, every cell walking the cluster's lines in file order: quadratic in the cluster (cells x lines), exact for
        any overlap.  ``ValueError``: a malformed line
        (the array is unchanged), or normalisation is on."""
        if strand not in self._strands:
            raise ValueError("strand %r is not one of %r" % (strand, self._strands))
        if self._normalize:
            raise ValueError("add_from_wiggle on a normalised GenomeArray: call set_normalize(False) first")
        slot = self._strands.index(strand)
        if isinstance(fh_or_path, (str, bytes, os.PathLike)):
            path = os.fspath(fh_or_path)
            if not os.path.isfile(path):
                raise IOError("No such file: %r" % (path,))
            rc = self._lib.pc_track_add_path(self._h, os.fsencode(path), slot)
        else:
            data, name = _text_of(fh_or_path)
            buf = ctypes.create_string_buffer(data, len(data)) if data else None
            rc = self._lib.pc_track_add_text(self._h, ctypes.cast(buf, ctypes.c_void_p) if buf is not None else None, len(data), os.fsencode(name), slot)
        self._names = None
        check(rc, "pc_track_add_text")

    def import_stats(self):
        """Of the last ``add_from_wiggle``: lines, yielded lines, escaped lines (converted on the host), state records,
        overlapping lines, lines that drove growth."""
        out = np.zeros(6, np.int64)
        check(self._lib.pc_track_stats(self._h, out.ctypes.data))
        return dict(zip(("lines", "yielded", "escaped", "states", "overlapping", "growth"), (int(x) for x in out)))

    def import_timing(self):
        """Milliseconds of the last ``add_from_wiggle``: upload, line starts, classify + state records, fields, apply."""
        out = np.zeros(5, np.float64)
        check(self._lib.pc_track_timing(self._h, out.ctypes.data))
        return dict(zip(("upload", "line_starts", "classify_states", "fields", "apply"), (float(x) for x in out)))

    # ---- the shape
    def chroms(self):
        if self._names is None:
            n = self._lib.pc_track_num_contigs(self._h)
            self._names = [os.fsdecode(self._lib.pc_track_contig_name(self._h, i)) for i in range(n)]
        return list(self._names)

    def keys(self):
        return self.chroms()

    def strands(self):
        return self._strands

    def lengths(self):
        return OrderedDict((c, int(self._lib.pc_track_contig_length(self._h, i))) for i, c in enumerate(self.chroms()))

    def extents(self):
        """``{chrom: {strand: cells stored}}``: the furthest end written (no reference counterpart)."""
        return OrderedDict((c, {st: int(self._lib.pc_track_contig_extent(self._h, i, s)) for s, st in enumerate(self._strands)})
                           for i, c in enumerate(self.chroms()))

    def __contains__(self, chrom):
        return chrom in self.chroms()

    def __len__(self):
        return len(self.chroms())

    def sum(self):
        out = ctypes.c_double()
        check(self._lib.pc_track_sum(self._h, ctypes.byref(out)))
        return float(out.value)

    def reset_sum(self):
        """The sum is recomputed after every write by itself; this only returns to that state (genome_array.py:1389-1392)."""
        self.sum()

    def set_normalize(self, value=True):
        assert value in (True, False)
        self._normalize = value

    # ---- the query side
    def _gather(self, contig, slot, start, end, out_off, out_step, total):
        out = np.zeros(int(total), np.float64)
        if total == 0:
            return out
        arrs = (np.ascontiguousarray(contig, np.int32), np.ascontiguousarray(slot, np.int32), np.ascontiguousarray(start, np.int64),
                np.ascontiguousarray(end, np.int64), np.ascontiguousarray(out_off, np.int64), np.ascontiguousarray(out_step, np.int8))
        check(self._lib.pc_track_gather(self._h, len(arrs[0]), *[a.ctypes.data for a in arrs], int(total), 1 if self._normalize else 0,
                                        out.ctypes.data), "pc_track_gather")
        return out

    def _slot(self, strand):
        if strand not in self._strands:
            raise ValueError("strand %r is not one of %r" % (strand, self._strands))
        return self._strands.index(strand)

    def get(self, roi, roi_order=True):
        """Values over a |GenomicSegment| (or a |SegmentChain|), 5'->3' of `roi` when `roi_order` (genome_array.py:1477-1533).
        Positions below 0, beyond the furthest end written, or on a contig the array does not hold are zero; a read never
        grows the array."""
        if isinstance(roi, SegmentChain):
            return roi.get_counts(self)
        index = {c: i for i, c in enumerate(self.chroms())}
        n = max(int(roi.end) - int(roi.start), 0)
        rev = roi_order is True and roi.strand == "-"
        return self._gather([index.get(roi.chrom, -1)], [self._slot(roi.strand)], [roi.start], [roi.start + n],
                            [n - 1 if rev else 0], [-1 if rev else 1], n)

    def __getitem__(self, roi):
        return self.get(roi, roi_order=True)

    def _get_chain_counts(self, chain, stranded=True):
        """``SegmentChain.get_counts`` for this array: one launch for the whole chain (roitools.pyx:3259-3271)."""
        return self.get_counts_batch([chain], stranded=stranded)[0]

    def get_counts_batch(self, chains, stranded=True):
        """Many |SegmentChains| in ONE launch: a list of float64 arrays, each what ``chain.get_counts(self, stranded)``
        returns."""
        from .engine import chain_layout
        index = {c: i for i, c in enumerate(self.chroms())}
        segs = [[(s.start, s.end) for s in c] for c in chains]
        strands = [c.strand for c in chains]
        seg_chain, out_off, out_step, _, chain_base, chain_len, total = chain_layout(segs, strands, rows=1, stranded=stranded is True)
        contig = [index.get(chains[ci].chrom, -1) for ci in seg_chain]
        slot = [self._slot(chains[ci].strand) for ci in seg_chain]
        flat = [se for chain_segs in segs for se in chain_segs]
        out = self._gather(contig, slot, [s for s, _ in flat], [e for _, e in flat], out_off, out_step, total)
        return [out[chain_base[ci]:chain_base[ci] + chain_len[ci]] for ci in range(len(chains))]

    def to_host(self):
        """The array as a host :class:`~plastid_amd.genome_array.DenseGenomeArray` of the reported lengths."""
        from .genome_array import DenseGenomeArray
        lengths = self.lengths()
        host = DenseGenomeArray(lengths, self._strands)
        norm, self._normalize = self._normalize, False
        try:
            for i, (c, per) in enumerate(self.extents().items()):
                for s, st in enumerate(self._strands):
                    if per[st] > 0:
                        host._chroms[c][st][:per[st]] = self._gather([i], [s], [0], [per[st]], [0], [1], per[st])
        finally:
            self._normalize = norm
        return host
