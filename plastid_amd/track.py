"""Count tracks -- bedGraph, variableStep and fixedStep wiggle text -- read in, changed and written out.

:class:`GenomeArray` is the reference's ``MutableAbstractGenomeArray`` / ``GenomeArray``
(plastid/genomics/genome_array.py:1323-2104): float64 values per contig, strand and position in HBM, filled by
:meth:`GenomeArray.add_from_wiggle` (:1978-1994; the text is parsed by the kernels of ``csrc/track_kernels.hip.h``) and
by ``ga[seg] = val`` (:1535-1611), read by ``get`` / ``[]``, ``get_counts_batch`` and ``SegmentChain.get_counts`` /
``get_masked_counts`` through one gather kernel, combined by ``apply_operation`` / ``+`` / ``-`` / ``*`` (:1697-1928),
compared by ``==``, listed by ``nonzero`` and written by ``to_bedgraph`` / ``to_variable_step`` (:1996-2084), whose text
is formatted by HIP kernels.

The rest of what this module used to hold is re-exported from where it lives now, so ``track.<name>`` goes on working:
the host wiggle reader and writers (:mod:`plastid_amd.track_text`), the host bigWig models
(:mod:`plastid_amd.bigwig_host`) and the device bigWig classes and zlib wrappers (:mod:`plastid_amd.bigwig`, which
imports :class:`GenomeArray` only where it makes one, so that the two modules do not import each other).

Not here: ``add_from_bowtie``, ``plot``, ``SparseGenomeArray``.  Deviations from the
reference (``__eq__``, the ``all`` mode over differing contig sets, operand order, the bigWig classes) are listed in DESIGN.md section 8.
"""
import ctypes
import io
import operator
import os
from collections import OrderedDict

import numpy as np

from . import _lib
from ._hostlib import buffer_of, stats_dict
from ._lib import check
from .bigwig import BigWigGenomeArray, BigWigReader, deflate_zlib, huffman_lengths, inflate_zlib  # noqa: F401
from .bigwig_host import (BIGWIG_WRITE_STATS, BIGWIG_ZOOM_STATS, DEFLATE_CODES, DEFLATE_MAX_INPUT, SUMMARY_ELEMENTS, SUMMARY_KINDS,  # noqa: F401
                          WARN_CHROM_NOT_FOUND, ZOOM_MAX_LEVELS, BigWigTable, BigWigZoomTable, _binary_sink, _check_bigwig_params,
                          _compress_mode, _zoom_level_stats, _zoom_mode, bigwig_info, bigwig_zoom_info, deflate_zlib_host,
                          huffman_lengths_host, read_bigwig, read_bigwig_zoom, sum_ranges, summarize_bigwig, summary_elements_bigwig,
                          write_bigwig)
from .exceptions import DataWarning, warn
from .roitools import SegmentChain
from .track_text import (_EXPORT_STATS, WiggleTable, _track_line, _write_text, float_repr, read_wiggle, write_bedgraph,  # noqa: F401
                         write_count_bedgraph, write_count_variable_step, write_variable_step)


def _export_geometry():
    out = (ctypes.c_int * 2)()
    check(_lib.load().pc_track_export_geometry(out))
    return int(out[0]), int(out[1])


_OPS = {operator.add: 0, operator.sub: 1, operator.mul: 2}


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

    @classmethod
    def _wrap(cls, handle, strands, min_chr_size, engine):
        """A track the library made (``pc_track_combine``) as an array on `engine`."""
        self = cls.__new__(cls)
        self._strands, self.min_chr_size = tuple(strands), int(min_chr_size)
        self._own_engine, self._engine, self._lib = False, engine, _lib.load()
        self._normalize, self._h, self._names = False, handle, None
        return self

    @staticmethod
    def like(other):
        """An empty array of `other`'s contigs, lengths and strands, on its engine (genome_array.py:2086-2100)."""
        return GenomeArray(other.lengths(), strands=other.strands(), min_chr_size=getattr(other, "min_chr_size", 10000000),
                           engine=getattr(other, "_engine", None))

    def close(self):
        """Free the cells; an engine of the array's own is closed with it (and takes the results of arithmetic on this
        array along: they live on the same engine)."""
        self._release(True)

    def _release(self, close_engine):
        if self._h is not None:
            if self._engine._finalizer.alive:      # (an engine that is gone took its tracks with it)
                self._lib.pc_track_destroy(self._h)
            self._h = None
            if self._own_engine and close_engine:
                self._engine.close()

    def __del__(self):
        # (the engine is left to its own finaliser: the results of arithmetic share it and may outlive this array)
        try:
            self._release(False)
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
            ptr, size, name, _keep = buffer_of(fh_or_path)
            rc = self._lib.pc_track_add_text(self._h, ptr, size, name, slot)
        self._names = None
        check(rc, "pc_track_add_text")

    def import_stats(self):
        """Of the last ``add_from_wiggle``: lines, yielded lines, escaped lines (converted on the host), state records,
        overlapping lines, lines that drove growth."""
        out = np.zeros(6, np.int64)
        check(self._lib.pc_track_stats(self._h, out.ctypes.data))
        return stats_dict(("lines", "yielded", "escaped", "states", "overlapping", "growth"), out)

    def import_timing(self):
        """Milliseconds of the last ``add_from_wiggle``: upload, line starts, classify + state records, fields, apply."""
        out = np.zeros(5, np.float64)
        check(self._lib.pc_track_timing(self._h, out.ctypes.data))
        return stats_dict(("upload", "line_starts", "classify_states", "fields", "apply"), out, float)

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

    # ---- writes
    def __setitem__(self, seg, val):
        """``ga[seg] = val`` over a |GenomicSegment| or a |SegmentChain| (genome_array.py:1535-1611).  `val`: a scalar, or a
        vector 5'->3' of `seg` (reversed for '-', the chain as a whole).  The contig is born at ``min_chr_size`` if the array
        does not hold it and grows by the rule of ``add_from_wiggle``; one launch writes every segment of a chain.
        ``ValueError``: the vector's length is not the region's (nothing is written).  A write while normalisation is on
        warns ``DataWarning`` and proceeds."""
        segs = list(seg) if isinstance(seg, SegmentChain) else [seg]
        strand = seg.strand
        slot = self._slot(strand)
        total = sum(max(int(s.end) - int(s.start), 0) for s in segs)
        scalar = np.ndim(val) == 0
        if scalar:
            values, scalar_value = None, float(val)
        else:
            values, scalar_value = np.ascontiguousarray(val, np.float64).ravel(), 0.0
            if len(values) != total:
                raise ValueError("cannot set %d positions from a vector of %d values" % (total, len(values)))
        if any(int(s.start) < 0 for s in segs):
            raise ValueError("cannot set positions below 0")
        if self._normalize:
            warn("Temporarily turning off normalization during value set. It will be re-enabled automatically when complete.", DataWarning)
        if not segs:
            return
        start = np.array([s.start for s in segs], np.int64)
        end = np.maximum(np.array([s.end for s in segs], np.int64), start)
        # genome order within the chain; a '-' vector runs the other way over the whole chain
        before = np.concatenate([[0], np.cumsum(end - start)[:-1]]).astype(np.int64)
        rev = strand == "-"
        val_off = (total - 1 - before) if rev else before
        val_step = np.full(len(segs), -1 if rev else 1, np.int8)
        self._names = None
        check(self._lib.pc_track_set(self._h, os.fsencode(seg.chrom), slot, len(segs), start.ctypes.data, end.ctypes.data,
                                     np.ascontiguousarray(val_off, np.int64).ctypes.data, val_step.ctypes.data,
                                     values.ctypes.data if values is not None else None, 0 if values is None else len(values), scalar_value),
              "pc_track_set")

    # ---- arithmetic
    def apply_operation(self, other, func, mode="same"):
        """A NEW array ``func(self, other)`` elementwise; `self` and `other` are unchanged (genome_array.py:1697-1835).
        `func`: ``operator.add``, ``operator.sub`` or ``operator.mul`` (``TypeError`` otherwise: the cells are not on the
        host).  `other`: a scalar -- it acts on every cell up to each contig's length -- or a :class:`GenomeArray` on the
        same engine (``ValueError`` otherwise), combined under `mode`: ``same`` (equal contigs, strands and lengths are
        asserted; the result reports the reference's lengths, 10000 more per strand, the operands keep theirs), ``truncate`` (common contigs and strands, the shorter length) or ``all`` (the union, the longer length,
        zero for what one side lacks; `self`'s contigs and strands first)."""
        if func not in _OPS:
            raise TypeError("apply_operation runs operator.add, operator.sub or operator.mul on the device; got %r" % (func,))
        if self._normalize:
            warn("Temporarily turning off normalization during value set. It will be re-enabled automatically when complete.", DataWarning)
        out = ctypes.c_void_p()
        if isinstance(other, GenomeArray):
            if other._engine is not self._engine:
                raise ValueError("the arrays live on different engines")
            if mode == "same":
                assert set(self.keys()) == set(other.keys())
                assert self.strands() == other.strands()
                assert self.lengths() == other.lengths()
                strands = list(self._strands)
            elif mode == "all":
                strands = list(self._strands) + [s for s in other._strands if s not in self._strands]
            elif mode == "truncate":
                strands = [s for s in self._strands if s in other._strands]
            else:
                raise ValueError("Mode not understood. Must be 'same', 'all', or 'truncate.'")
            if not strands:
                raise ValueError("the arrays have no strand in common")
            slot_a = np.array([self._strands.index(s) if s in self._strands else -1 for s in strands], np.int32)
            slot_b = np.array([other._strands.index(s) if s in other._strands else -1 for s in strands], np.int32)
            # (the reference writes its `same` result through __setitem__ over whole contigs, and a write that ends at the
            # length grows the contig: its result is 10000 longer per strand, genome_array.py:1771-1775, :1593-1602)
            pad = 10000 * len(strands) if mode == "same" else 0
            check(self._lib.pc_track_combine(self._h, other._h, 0.0, _OPS[func], 0 if mode == "truncate" else 1, pad, len(strands),
                                             slot_a.ctypes.data, slot_b.ctypes.data, ctypes.byref(out)), "pc_track_combine")
        else:
            if np.ndim(other) != 0:
                raise TypeError("the other operand is a scalar or a GenomeArray, not %r" % (type(other),))
            strands = list(self._strands)
            slot_a = np.arange(len(strands), dtype=np.int32)
            check(self._lib.pc_track_combine(self._h, None, float(other), _OPS[func], 1, 0, len(strands), slot_a.ctypes.data, None,
                                             ctypes.byref(out)), "pc_track_combine")
        return GenomeArray._wrap(out, strands, self.min_chr_size, self._engine)

    def __add__(self, other, mode="all"):
        return self.apply_operation(other, operator.add, mode=mode)

    def __mul__(self, other, mode="all"):
        return self.apply_operation(other, operator.mul, mode=mode)

    def __sub__(self, other, mode="all"):
        """``self + other * -1`` (genome_array.py:1927)."""
        return self.__add__(other * -1)

    def __eq__(self, other, tol=1e-10):
        """The same non-zero positions on every contig and strand, and ``|a - b| <= tol`` at each of them; lengths need
        not be equal.  Unlike the reference's test (genome_array.py:1445-1448) the difference counts in both directions
        and at the last non-zero position too.  A reduction on the device."""
        if not isinstance(other, GenomeArray):
            return NotImplemented
        if other._engine is not self._engine:
            raise ValueError("the arrays live on different engines")
        mine, theirs = self.chroms(), other.chroms()
        chroms = mine + [c for c in theirs if c not in mine]
        strands = list(self._strands) + [s for s in other._strands if s not in self._strands]
        ia, ib = {c: i for i, c in enumerate(mine)}, {c: i for i, c in enumerate(theirs)}
        cols = [[], [], [], []]
        for c in chroms:
            for s in strands:
                cols[0].append(ia.get(c, -1))
                cols[1].append(self._strands.index(s) if s in self._strands else -1)
                cols[2].append(ib.get(c, -1))
                cols[3].append(other._strands.index(s) if s in other._strands else -1)
        arrs = [np.array(x, np.int32) for x in cols]
        equal = ctypes.c_int(0)
        check(self._lib.pc_track_equal(self._h, other._h, len(arrs[0]), *[a.ctypes.data for a in arrs], float(tol), ctypes.byref(equal)),
              "pc_track_equal")
        return bool(equal.value)

    def __ne__(self, other):
        r = self.__eq__(other)
        return r if r is NotImplemented else not r

    __hash__ = object.__hash__

    def nonzero(self):
        """``{chrom: {strand: int64 indices of the non-zero positions}}`` (genome_array.py:1679-1695); NaN is non-zero,
        ``-0.0`` is not.  Count, exclusive sum and select on the device; only the indices come back."""
        chroms = self.chroms()
        counts = np.zeros(max(len(chroms) * len(self._strands), 1), np.int64)
        check(self._lib.pc_track_nonzero_count(self._h, counts.ctypes.data), "pc_track_nonzero_count")
        total = int(counts.sum())
        flat = np.zeros(max(total, 1), np.int64)
        check(self._lib.pc_track_nonzero_read(self._h, flat.ctypes.data, total), "pc_track_nonzero_read")
        out, at = OrderedDict(), 0
        for i, c in enumerate(chroms):
            out[c] = {}
            for s, st in enumerate(self._strands):
                n = int(counts[i * len(self._strands) + s])
                out[c][st] = flat[at:at + n].copy()
                at += n
        return out

    # ---- export
    def _export(self, kind, fh, trackname, strand, printer, kwargs):
        assert strand in self._strands
        nbytes = ctypes.c_int64(0)
        check(self._lib.pc_track_export(self._h, kind, self._strands.index(strand), ctypes.byref(nbytes)), "pc_track_export")
        text = np.empty(max(int(nbytes.value), 1), np.uint8)
        check(self._lib.pc_track_export_read(self._h, text.ctypes.data, int(nbytes.value)), "pc_track_export_read")
        if printer is not None:
            for chrom in sorted(self.chroms()):
                printer.write("Writing chromosome %s..." % chrom)
        _write_text(fh, _track_line(kind, trackname, kwargs).encode("utf-8"))
        _write_text(fh, memoryview(text[:int(nbytes.value)]))

    def to_bedgraph(self, fh, trackname, strand, printer=None, **kwargs):
        """Write `strand` as bedGraph, the reference's text byte for byte (genome_array.py:2039-2084): contigs in sorted
        order, only those whose sum is > 0; runs of equal value between the first and the last non-zero position.  The
        text is built in HBM (``csrc/track_kernels.hip.h``: run heads, select, line lengths, format) and read back once."""
        self._export(0, fh, trackname, strand, printer, kwargs)

    def to_variable_step(self, fh, trackname, strand, printer=None, **kwargs):
        """Write `strand` as variableStep wiggle (genome_array.py:1996-2037): every contig's header, a line per non-zero
        position.  See :meth:`to_bedgraph`."""
        self._export(1, fh, trackname, strand, printer, kwargs)

    def export_stats(self):
        """Of the last export: lines, runs (bedGraph) or non-zero positions (variableStep), values listed for the host's
        ``repr`` formatter (integers below 10^16, nan and inf never are), bytes behind the track line."""
        out = np.zeros(4, np.int64)
        check(self._lib.pc_track_export_stats(self._h, out.ctypes.data))
        return stats_dict(_EXPORT_STATS, out)

    def export_timing(self):
        """Milliseconds of the last export: slot sums, run heads + select, listed values, line lengths + offsets, format,
        read-back."""
        out = np.zeros(6, np.float64)
        check(self._lib.pc_track_export_timing(self._h, out.ctypes.data))
        return stats_dict(("slot_sums", "runs", "listed_values", "lengths", "format", "read_back"), out, float)

    def to_bigwig(self, path_or_file, strand, items_per_slot=1024, block_size=256, compress=True, zoom=False):
        """Write `strand` as a bigWig file (a path, or a file object opened in binary mode; a text-mode file is a
        ``TypeError``).  No reference counterpart: the reference reads bigWig and does not write it.

        The stored cells are written, as :meth:`to_bedgraph` writes them -- the normalisation ``get`` would show is NOT
        applied.  A cell is written iff its value ``!= 0.0`` (NaN is, ``-0.0`` is not); neighbouring written cells form
        one item while their float64 values compare equal; values are cast to float32.  Contigs stand in sorted order,
        every contig is in the chromosome tree at ``max(lengths()[c], extents()[c][strand])``; every `items_per_slot`
        items (1 .. 2 048) of a contig make one bedGraph section, `block_size` (2 .. 65 535) is the fan-out of both
        trees, `compress`: ``True`` or ``"fixed"``: every section through the GPU's zlib encoder
        (``csrc/deflate_kernels.hip.h``: LZ77 under the fixed Huffman codes, or a stored block); ``"dynamic"``: the same
        matches under Huffman codes built for every section, never larger and on count data about a third smaller;
        ``False``: stored sections; anything else is a ``ValueError``.  Items, sections, summary and blocks are built in
        HBM; the host lays out the header and the trees.

        `zoom`: ``False`` (the default): no zoom levels, readers fall back to the full data for every summary.  ``True``:
        a pyramid of summary levels on a fixed grid (``csrc/bigwig_write_host.h``, "zoom levels";
        ``csrc/bigwig_zoom_kernels.hip.h``): window ``w`` of level ``k`` on a contig covers
        ``[w * r_k, min((w + 1) * r_k, size))`` with ``r_k = r0 * 4**k``, at most 10 levels, ``r_k <= 2**30``; a window
        with data gives one 32-byte record (valid, min, max, sum, sum of squares); level 0 is written whenever the file
        has items and level ``k + 1`` while it has fewer records than level ``k``.  ``r0 = 4 * max(10, valid // items)``
        capped at ``2**20``; an ``int`` in ``8 .. 2**24`` is ``r0`` itself; anything else is a ``ValueError``.  Every
        ``min(items_per_slot, 768)`` records of a contig form one block, encoded as the sections are.  Kent's readers
        (``bigWigSummary``, genome browsers) answer summary queries from these levels; the windows are not where Kent's
        own writer would put them.  The file is the one :func:`write_bigwig` gives for ``to_host()``."""
        assert strand in self._strands
        _check_bigwig_params(items_per_slot, block_size)
        mode, zoom_mode = _compress_mode(compress), _zoom_mode(zoom)
        if isinstance(path_or_file, io.TextIOBase):
            raise TypeError("a bigWig file is binary: give a path or a file opened in binary mode")
        nbytes = ctypes.c_int64(0)
        if zoom_mode:
            check(self._lib.pc_track_export_bigwig_zoom(self._h, self._strands.index(strand), int(items_per_slot), int(block_size), mode, zoom_mode,
                                                        ctypes.byref(nbytes)), "pc_track_export_bigwig_zoom")
        else:
            check(self._lib.pc_track_export_bigwig(self._h, self._strands.index(strand), int(items_per_slot), int(block_size), mode,
                                                   ctypes.byref(nbytes)), "pc_track_export_bigwig")
        image = np.empty(max(int(nbytes.value), 1), np.uint8)
        check(self._lib.pc_track_export_bigwig_read(self._h, image.ctypes.data, int(nbytes.value)), "pc_track_export_bigwig_read")
        sink, close = _binary_sink(path_or_file)
        try:
            sink.write(memoryview(image[:int(nbytes.value)]))
        finally:
            if close:
                sink.close()

    def bigwig_export_stats(self, block_types=False):
        """Of the last :meth:`to_bigwig`: contigs, items, sections, raw bytes of the sections, bytes of the blocks in the
        file, sections that fell back to a stored DEFLATE block.  `block_types`: also ``fixed_sections`` and
        ``dynamic_sections``, the sections that went out as fixed and as dynamic blocks; with ``stored_sections`` they add
        up to the sections of a compressed file (all three are 0 for ``compress=False``)."""
        out = np.zeros(6, np.int64)
        check(self._lib.pc_track_bigwig_export_stats(self._h, out.ctypes.data))
        stats = stats_dict(BIGWIG_WRITE_STATS, out)
        if block_types:
            types = np.zeros(3, np.int64)
            check(self._lib.pc_track_bigwig_export_block_types(self._h, types.ctypes.data))
            assert int(types[0]) == stats["stored_sections"]
            stats["fixed_sections"], stats["dynamic_sections"] = int(types[1]), int(types[2])
        return stats

    def bigwig_export_timing(self):
        """Milliseconds of the last :meth:`to_bigwig`: item heads and their sum, items + section headers + summary,
        deflate + Adler-32, sizes + compaction, read-back, host layout."""
        out = np.zeros(6, np.float64)
        check(self._lib.pc_track_bigwig_export_timing(self._h, out.ctypes.data))
        return stats_dict(("runs_items", "sections_summary", "deflate_adler", "sizes_compaction", "read_back", "host_layout"), out, float)

    def bigwig_export_zoom_stats(self):
        """Of the last :meth:`to_bigwig`: one dict per zoom level written -- ``reduction``, ``records``, ``blocks``,
        ``raw_bytes`` of the blocks and their ``file_bytes`` (an empty list for ``zoom=False``)."""
        n = ctypes.c_int64(0)
        out = np.zeros(5 * ZOOM_MAX_LEVELS, np.int64)
        check(self._lib.pc_track_bigwig_export_zoom_stats(self._h, ctypes.byref(n), out.ctypes.data))
        return _zoom_level_stats(n.value, out)

    def bigwig_export_zoom_timing(self):
        """Milliseconds of the zoom levels of the last :meth:`to_bigwig` on the engine's stream: level 0 from the items,
        the levels above, flags + record numbers + records + block tables, deflate + compaction of the zoom blocks."""
        out = np.zeros(4, np.float64)
        check(self._lib.pc_track_bigwig_export_zoom_timing(self._h, out.ctypes.data))
        return stats_dict(("level0", "upper_levels", "records", "deflate_compaction"), out, float)

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


def __getattr__(name):
    # EXPORT_TILE (T): cells one workgroup covers in the run-head kernel; FORMAT_RUNS (R): lines one workgroup formats
    if name in ("EXPORT_TILE", "FORMAT_RUNS"):
        return _export_geometry()[0 if name == "EXPORT_TILE" else 1]
    raise AttributeError(name)
