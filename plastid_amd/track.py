"""Count tracks -- bedGraph, variableStep and fixedStep wiggle text -- read in, changed and written out.

:class:`GenomeArray` is the reference's ``MutableAbstractGenomeArray`` / ``GenomeArray``
(plastid/genomics/genome_array.py:1323-2104): float64 values per contig, strand and position in HBM, filled by
:meth:`GenomeArray.add_from_wiggle` (:1978-1994; the text is parsed by the kernels of ``csrc/track_kernels.hip.h``) and
by ``ga[seg] = val`` (:1535-1611), read by ``get`` / ``[]``, ``get_counts_batch`` and ``SegmentChain.get_counts`` /
``get_masked_counts`` through one gather kernel, combined by ``apply_operation`` / ``+`` / ``-`` / ``*`` (:1697-1928),
compared by ``==``, listed by ``nonzero`` and written by ``to_bedgraph`` / ``to_variable_step`` (:1996-2084), whose text
is formatted by HIP kernels.  :func:`write_bedgraph` / :func:`write_variable_step` are the same writers on the host over a
``DenseGenomeArray``: the model of the device export, and the way to write a track without a GPU.  :func:`read_wiggle` is
the reference's ``WiggleReader`` (plastid/readers/wiggle.py:43-174) on the host, built from the same
``csrc/track_host.h`` the kernels compile: the model of the device import, and the way to read a track without a GPU.

:class:`BigWigReader` / :class:`BigWigGenomeArray` are the reference's classes of those names (plastid/readers/bigwig.pyx:109-412,
genome_array.py:1114-1320) over bigWig files whose blocks are inflated and decoded on the GPU (``csrc/bigwig_kernels.hip.h``);
:func:`read_bigwig` is the same reader on the host (``csrc/bigwig_host.h``): the model of the device import.

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
from ._lib import check
from .exceptions import DataWarning, warn
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


def _track_line(kind, trackname, kwargs):
    """The track definition line both writers start with (genome_array.py:2018-2022, :2056-2060)."""
    line = "track type=%s name=%s" % ("bedGraph" if kind == 0 else "wiggle_0", trackname)
    for k, v in sorted(kwargs.items(), key=lambda x: x[0]):
        line += " %s=%s" % (k, v)
    return line + "\n"


def _write_text(fh, text):
    """`text` (bytes or a memoryview of bytes) to a text-mode or binary file."""
    if isinstance(fh, (io.RawIOBase, io.BufferedIOBase)):
        fh.write(text)
        return
    try:
        fh.write(str(text, "utf-8"))
    except TypeError:
        fh.write(text)


def _host_writer():
    from .bam import _load
    L = _load()
    if not hasattr(L.pb_track_writer_open, "_bound"):
        vp = ctypes.c_void_p
        L.pb_track_writer_open.restype = vp
        L.pb_track_writer_open.argtypes = []
        L.pb_track_writer_close.argtypes = [vp]
        L.pb_track_writer_add.argtypes = [vp, ctypes.c_int, ctypes.c_char_p, vp, ctypes.c_int64]
        L.pb_track_writer_add_counts.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_char_p, vp, ctypes.c_int64, ctypes.c_int64]
        L.pb_track_writer_size.restype = ctypes.c_int64
        L.pb_track_writer_size.argtypes = [vp]
        L.pb_track_writer_text.restype = vp
        L.pb_track_writer_text.argtypes = [vp]
        L.pb_track_writer_stats.argtypes = [vp, vp]
        L.pb_float_repr.argtypes = [vp, ctypes.c_int64, vp, vp]
        L.pb_track_writer_open._bound = True
    return L


def _write_host(kind, host_array, fh, trackname, strand, kwargs):
    assert strand in host_array.strands()
    L = _host_writer()
    h = L.pb_track_writer_open()
    try:
        for chrom in sorted(host_array.chroms()):
            cells = np.ascontiguousarray(host_array._chroms[chrom][strand], np.float64)
            if L.pb_track_writer_add(h, kind, chrom.encode("utf-8"), cells.ctypes.data, len(cells)) != 0:
                raise ValueError(L.pb_last_error().decode())
        text = ctypes.string_at(L.pb_track_writer_text(h), int(L.pb_track_writer_size(h)))
        stats = np.zeros(4, np.int64)
        L.pb_track_writer_stats(h, stats.ctypes.data)
    finally:
        L.pb_track_writer_close(h)
    _write_text(fh, _track_line(kind, trackname, kwargs).encode("utf-8"))
    _write_text(fh, text)
    return dict(zip(("lines", "runs", "listed", "bytes"), (int(x) for x in stats)))


def write_bedgraph(host_array, fh, trackname, strand, **kwargs):
    """``GenomeArray.to_bedgraph`` (genome_array.py:2039-2084) of a host ``DenseGenomeArray`` by the serial writer of
    ``csrc/track_host.h``, byte for byte.  Returns the writer's statistics: lines, runs, values that are not plain, bytes."""
    return _write_host(0, host_array, fh, trackname, strand, kwargs)


def write_variable_step(host_array, fh, trackname, strand, **kwargs):
    """``GenomeArray.to_variable_step`` (genome_array.py:1996-2037) of a host ``DenseGenomeArray``; see :func:`write_bedgraph`."""
    return _write_host(1, host_array, fh, trackname, strand, kwargs)


def _count_vectors(vectors):
    """The vectors of a count export as contiguous 1-D arrays of ONE dtype, int64 or float64."""
    out = OrderedDict((c, np.asarray(v)) for c, v in vectors.items())
    is_float = any(v.dtype.kind == "f" and v.size for v in out.values())   # (an empty vector has no say)
    for c, v in out.items():
        if v.ndim != 1 or v.dtype.kind not in "iuf" or (v.size and is_float != (v.dtype.kind == "f")):
            raise TypeError("the vectors of a count export are 1-D arrays, all int64 or all float64 (%r)" % (c,))
    return OrderedDict((c, np.ascontiguousarray(v, np.float64 if is_float else np.int64)) for c, v in out.items()), is_float


def _count_text(kind, vectors, window_size):
    """``(text, stats)`` of the serial writers over ``{contig: vector}``, contigs in sorted order, without the track line."""
    vectors, is_float = _count_vectors(vectors)
    L = _host_writer()
    h = L.pb_track_writer_open()
    try:
        for chrom in sorted(vectors):
            v = vectors[chrom]
            if L.pb_track_writer_add_counts(h, kind, 1 if is_float else 0, chrom.encode("utf-8"), v.ctypes.data, len(v), int(window_size)) != 0:
                raise ValueError(L.pb_last_error().decode())
        text = ctypes.string_at(L.pb_track_writer_text(h), int(L.pb_track_writer_size(h)))
        stats = np.zeros(4, np.int64)
        L.pb_track_writer_stats(h, stats.ctypes.data)
    finally:
        L.pb_track_writer_close(h)
    return text, dict(zip(("lines", "runs", "listed", "bytes"), (int(x) for x in stats)))


def _write_counts(kind, vectors, fh, trackname, window_size, kwargs):
    assert window_size > 0
    text, stats = _count_text(kind, vectors, window_size)
    _write_text(fh, _track_line(kind, trackname, kwargs).encode("utf-8"))
    _write_text(fh, text)
    return stats


def write_count_bedgraph(vectors, fh, trackname, window_size=100000, **kwargs):
    """``BAMGenomeArray.to_bedgraph`` (genome_array.py:1041-1111) over ``{contig: count vector}`` (genome order; 1-D
    arrays, all int64 or all float64) by the serial writer of ``csrc/track_host.h``, byte for byte: contigs in sorted
    order, every vector cut into windows of `window_size`, a line per run of equal value ``> 0`` inside a window.  The
    model of the device export of a :class:`~plastid_amd.genome_array.BAMGenomeArray`, and the way to write such a track
    without a GPU.  Returns the statistics of :func:`write_bedgraph` (``runs``: runs of any value)."""
    return _write_counts(0, vectors, fh, trackname, window_size, kwargs)


def write_count_variable_step(vectors, fh, trackname, window_size=100000, **kwargs):
    """``BAMGenomeArray.to_variable_step`` (genome_array.py:990-1039) over ``{contig: count vector}``: every contig's
    header, a line per non-zero position (`window_size` does not show in the text); see :func:`write_count_bedgraph`."""
    return _write_counts(1, vectors, fh, trackname, window_size, kwargs)


def float_repr(values):
    """``repr(float(x))`` of every value by the formatter of ``csrc/track_host.h`` (the one the export lists values for)."""
    L = _host_writer()
    v = np.ascontiguousarray(values, np.float64).ravel()
    out = np.zeros(max(len(v), 1) * 24, np.uint8)
    lens = np.zeros(max(len(v), 1), np.uint8)
    if L.pb_float_repr(v.ctypes.data, len(v), out.ctypes.data, lens.ctypes.data) != 0:
        raise ValueError(L.pb_last_error().decode())
    raw = out.tobytes()
    return [raw[24 * k:24 * k + int(lens[k])].decode("ascii") for k in range(len(v))]


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
        return dict(zip(("lines", "runs", "listed", "bytes"), (int(x) for x in out)))

    def export_timing(self):
        """Milliseconds of the last export: slot sums, run heads + select, listed values, line lengths + offsets, format,
        read-back."""
        out = np.zeros(6, np.float64)
        check(self._lib.pc_track_export_timing(self._h, out.ctypes.data))
        return dict(zip(("slot_sums", "runs", "listed_values", "lengths", "format", "read_back"), (float(x) for x in out)))

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
        stats = dict(zip(BIGWIG_WRITE_STATS, (int(x) for x in out)))
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
        return dict(zip(("runs_items", "sections_summary", "deflate_adler", "sizes_compaction", "read_back", "host_layout"), (float(x) for x in out)))

    def bigwig_export_zoom_stats(self):
        """Of the last :meth:`to_bigwig`: one dict per zoom level written -- ``reduction``, ``records``, ``blocks``,
        ``raw_bytes`` of the blocks and their ``file_bytes`` (an empty list for ``zoom=False``)."""
        n = ctypes.c_int64(0)
        out = np.zeros(5 * ZOOM_MAX_LEVELS, np.int64)
        check(self._lib.pc_track_bigwig_export_zoom_stats(self._h, ctypes.byref(n), out.ctypes.data))
        return [dict(zip(BIGWIG_ZOOM_STATS, (int(x) for x in out[5 * k:5 * k + 5]))) for k in range(int(n.value))]

    def bigwig_export_zoom_timing(self):
        """Milliseconds of the zoom levels of the last :meth:`to_bigwig` on the engine's stream: level 0 from the items,
        the levels above, flags + record numbers + records + block tables, deflate + compaction of the zoom blocks."""
        out = np.zeros(4, np.float64)
        check(self._lib.pc_track_bigwig_export_zoom_timing(self._h, out.ctypes.data))
        return dict(zip(("level0", "upper_levels", "records", "deflate_compaction"), (float(x) for x in out)))

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


# ---------------------------------------------------------------- bigWig
WARN_CHROM_NOT_FOUND = "No data for chromosome '%s' in file '%s'."      # (plastid/readers/bbifile.pyx:25)


def _image_of(path_or_bytes):
    """``(path, buffer, size)`` for the entry points that take a path or an image."""
    if isinstance(path_or_bytes, (bytes, bytearray, memoryview)):
        data = bytes(path_or_bytes)
        return None, ctypes.create_string_buffer(data, len(data)) if data else ctypes.create_string_buffer(1), len(data)
    path = os.fspath(path_or_bytes)
    if not os.path.isfile(path):
        raise IOError("No such file: %r" % (path,))
    return os.fsencode(path), None, 0


def bigwig_info(path_or_bytes):
    """Header, contigs and block table of a bigWig file (a path, or its bytes) without a GPU (``pc_bigwig_info`` /
    ``pc_bigwig_blocks``): ``chroms`` -- an ``OrderedDict`` name -> size in the order of Kent's ``bbiChromList`` --
    ``blocks`` (file offset, bytes) in index order, ``uncompress_buf_size``, ``version``.  ``ValueError("<path>: bigWig:
    <what>")`` for a file that is refused."""
    L = _lib.load()
    path, buf, size = _image_of(path_or_bytes)
    image = ctypes.cast(buf, ctypes.c_void_p) if buf is not None else None
    out = np.zeros(5, np.int64)
    check(L.pc_bigwig_info(path, image, size, out.ctypes.data, 0, None, 0, None), "pc_bigwig_info")
    nchrom, nblock = int(out[0]), int(out[1])
    names = ctypes.create_string_buffer(max(int(out[4]), 1))
    sizes = np.zeros(max(nchrom, 1), np.int64)
    check(L.pc_bigwig_info(path, image, size, out.ctypes.data, nchrom, names, int(out[4]), sizes.ctypes.data), "pc_bigwig_info")
    parts = names.raw[:int(out[4])].split(b"\0")[:nchrom]
    off, nbytes = np.zeros(max(nblock, 1), np.int64), np.zeros(max(nblock, 1), np.int64)
    check(L.pc_bigwig_blocks(path, image, size, nblock, off.ctypes.data, nbytes.ctypes.data), "pc_bigwig_blocks")
    return {"chroms": OrderedDict((p.decode("utf-8", "replace"), int(s)) for p, s in zip(parts, sizes)),
            "blocks": [(int(a), int(b)) for a, b in zip(off[:nblock], nbytes[:nblock])],
            "uncompress_buf_size": int(out[2]), "version": int(out[3])}


class BigWigTable(object):
    """What :func:`read_bigwig` returns: one row per item in file order -- the order Kent's readers apply them in -- as
    columns.  ``chrom`` indexes ``names`` (``bbiChromList`` order; ``lengths``: their sizes); ``block``: the data block of
    the row; ``block_off`` / ``block_size``: the block table; ``stats``: blocks, compressed blocks, items by section
    type, bytes inflated, ``uncompressBufSize``, version."""

    def __init__(self, names, lengths, chrom, start, stop, value, block, block_off, block_size, stats):
        self.names, self.lengths, self.chrom, self.start, self.stop, self.value = names, lengths, chrom, start, stop, value
        self.block, self.block_off, self.block_size, self.stats = block, block_off, block_size, stats

    def __len__(self):
        return len(self.chrom)

    def tuples(self):
        return [(self.names[c], int(a), int(b), float(v)) for c, a, b, v in zip(self.chrom, self.start, self.stop, self.value)]

    def chromosome_counts(self, chrom):
        """Kent's ``bigWigValsOnChromFetchData`` over the table: the contig's size in float64, the items assigned in file order."""
        i = self.names.index(chrom)
        out = np.zeros(self.lengths[i], np.float64)
        for k in np.flatnonzero(self.chrom == i):
            out[self.start[k]:self.stop[k]] = self.value[k]
        return out


def read_bigwig(path_or_bytes):
    """Read a bigWig file on the host, one thread, zlib (``pb_bigwig_read``; the container and the section decoders are
    ``csrc/bigwig_host.h``, which the kernels compile too): the model of the device import, and the way to read a bigWig
    without a GPU.  ``ValueError("<path>: bigWig: <what>")`` for a file that is refused."""
    from .bam import _load
    L = _load()
    if not hasattr(L.pb_bigwig_read, "_bound"):
        vp = ctypes.c_void_p
        L.pb_bigwig_read.restype = vp
        L.pb_bigwig_read.argtypes = [vp, ctypes.c_int64, ctypes.c_char_p]
        L.pb_bigwig_close.argtypes = [vp]
        for f in (L.pb_bigwig_rows, L.pb_bigwig_nblocks):
            f.restype, f.argtypes = ctypes.c_int64, [vp]
        L.pb_bigwig_nchrom.argtypes = [vp]
        L.pb_bigwig_chrom.restype = ctypes.c_char_p
        L.pb_bigwig_chrom.argtypes = [vp, ctypes.c_int]
        L.pb_bigwig_chrom_size.restype = ctypes.c_int64
        L.pb_bigwig_chrom_size.argtypes = [vp, ctypes.c_int]
        L.pb_bigwig_fill.argtypes = [vp] * 8
        L.pb_bigwig_stats.argtypes = [vp, vp]
        L.pb_bigwig_read._bound = True
    if isinstance(path_or_bytes, (bytes, bytearray, memoryview)):
        data, name = bytes(path_or_bytes), "<memory>"
    else:
        data, name = _text_of(path_or_bytes)
    buf = ctypes.create_string_buffer(data, len(data)) if data else None
    h = L.pb_bigwig_read(ctypes.cast(buf, ctypes.c_void_p) if buf is not None else None, len(data), os.fsencode(name))
    if not h:
        raise ValueError(L.pb_last_error().decode("utf-8", "replace"))
    try:
        n, nb = int(L.pb_bigwig_rows(h)), int(L.pb_bigwig_nblocks(h))
        nchrom = L.pb_bigwig_nchrom(h)
        names = [L.pb_bigwig_chrom(h, i).decode("utf-8", "replace") for i in range(nchrom)]
        lengths = [int(L.pb_bigwig_chrom_size(h, i)) for i in range(nchrom)]
        chrom, start, stop = np.zeros(n, np.int32), np.zeros(n, np.int64), np.zeros(n, np.int64)
        value, block = np.zeros(n, np.float64), np.zeros(n, np.int32)
        block_off, block_size = np.zeros(nb, np.int64), np.zeros(nb, np.int64)
        if L.pb_bigwig_fill(h, *[a.ctypes.data for a in (chrom, start, stop, value, block, block_off, block_size)]) != 0:
            raise ValueError(L.pb_last_error().decode())
        stats = np.zeros(8, np.int64)
        L.pb_bigwig_stats(h, stats.ctypes.data)
    finally:
        L.pb_bigwig_close(h)
    keys = ("blocks", "compressed_blocks", "bedgraph_items", "variable_step_items", "fixed_step_items", "bytes_inflated", "uncompress_buf_size", "version")
    return BigWigTable(names, lengths, chrom, start, stop, value, block, block_off, block_size, dict(zip(keys, (int(x) for x in stats))))


def _bind_zoom_readers(L):
    if not hasattr(L.pb_bigwig_zoom_info, "_bound"):
        vp = ctypes.c_void_p
        L.pb_bigwig_zoom_info.argtypes = [vp, ctypes.c_int64, ctypes.c_char_p, vp, ctypes.c_int, vp]
        L.pb_bigwig_zoom_read.restype = vp
        L.pb_bigwig_zoom_read.argtypes = [vp, ctypes.c_int64, ctypes.c_char_p, ctypes.c_int64]
        L.pb_bigwig_zoom_close.argtypes = [vp]
        L.pb_bigwig_zoom_rows.restype = ctypes.c_int64
        L.pb_bigwig_zoom_rows.argtypes = [vp]
        L.pb_bigwig_zoom_fill.argtypes = [vp] * 9
        L.pb_bigwig_zoom_info._bound = True


def _bigwig_bytes(path_or_bytes):
    """``(ctypes pointer or None, size, name, keep-alive)`` of a bigWig file given as a path or as its bytes."""
    if isinstance(path_or_bytes, (bytes, bytearray, memoryview)):
        data, name = bytes(path_or_bytes), "<memory>"
    else:
        data, name = _text_of(path_or_bytes)
    buf = ctypes.create_string_buffer(data, len(data)) if data else None
    return (ctypes.cast(buf, ctypes.c_void_p) if buf is not None else None), len(data), os.fsencode(name), buf


def bigwig_zoom_info(path_or_bytes):
    """The zoom levels of a bigWig file (a path, or its bytes), without a GPU: a list of ``(reduction, data_offset,
    index_offset, records)``, one per zoom header in the file's order -- ``data_offset`` points at the level's u32 record
    count, ``index_offset`` at its R-tree.  Empty for a file without zoom levels.  ``ValueError("<path>: bigWig: <what>")``
    for a file that is refused."""
    from .bam import _load
    L = _load()
    _bind_zoom_readers(L)
    ptr, size, name, _keep = _bigwig_bytes(path_or_bytes)
    n = ctypes.c_int64(0)
    if L.pb_bigwig_zoom_info(ptr, size, name, ctypes.byref(n), 0, None) != 0:
        raise ValueError(L.pb_last_error().decode("utf-8", "replace"))
    out = np.zeros(4 * max(int(n.value), 1), np.int64)
    if L.pb_bigwig_zoom_info(ptr, size, name, ctypes.byref(n), int(n.value), out.ctypes.data) != 0:
        raise ValueError(L.pb_last_error().decode("utf-8", "replace"))
    return [tuple(int(x) for x in out[4 * k:4 * k + 4]) for k in range(int(n.value))]


class BigWigZoomTable(object):
    """What :func:`read_bigwig_zoom` returns: the records of one zoom level in file order, as columns: ``chrom_id``,
    ``start``, ``end``, ``valid`` (uint32) and ``min``, ``max``, ``sum``, ``sumsq`` (float32)."""
    COLUMNS = ("chrom_id", "start", "end", "valid", "min", "max", "sum", "sumsq")

    def __init__(self, columns):
        for k, v in zip(self.COLUMNS, columns):
            setattr(self, k, v)

    def __len__(self):
        return len(self.chrom_id)


def read_bigwig_zoom(path_or_bytes, level):
    """The records of zoom level `level` of a bigWig file (a path, or its bytes) in file order, walked through that
    level's R-tree and inflated with zlib on the host (``pb_bigwig_zoom_read``; ``csrc/bigwig_write_host.h``:
    ``read_zoom_level``): a :class:`BigWigZoomTable`.  ``ValueError("<path>: bigWig: <what>")`` for a level the file does
    not have and for a file or a level that is refused."""
    from .bam import _load
    L = _load()
    _bind_zoom_readers(L)
    ptr, size, name, _keep = _bigwig_bytes(path_or_bytes)
    h = L.pb_bigwig_zoom_read(ptr, size, name, int(level))
    if not h:
        raise ValueError(L.pb_last_error().decode("utf-8", "replace"))
    try:
        n = int(L.pb_bigwig_zoom_rows(h))
        cols = [np.zeros(n, np.uint32) for _ in range(4)] + [np.zeros(n, np.float32) for _ in range(4)]
        if L.pb_bigwig_zoom_fill(h, *[a.ctypes.data for a in cols]) != 0:
            raise ValueError(L.pb_last_error().decode("utf-8", "replace"))
    finally:
        L.pb_bigwig_zoom_close(h)
    return BigWigZoomTable(cols)


# ---------------------------------------------------------------- binned summaries (csrc/bigwig_summary_host.h)
SUMMARY_KINDS = ("mean", "min", "max", "coverage", "std")
SUMMARY_ELEMENTS = ("valid", "min", "max", "sum", "sumsq")


def _summary_kinds(kind):
    """``(the kinds asked for, whether they came as a tuple)``."""
    kinds = tuple(kind) if isinstance(kind, (tuple, list)) else (kind,)
    for k in kinds:
        if k not in SUMMARY_KINDS:
            raise ValueError("kind %r is none of %r" % (k, SUMMARY_KINDS))
    return kinds, isinstance(kind, (tuple, list))


def _summary_queries(queries, n_bins):
    """``(chrom names, start, end)`` of queries given as ``(chrom, start, end)`` tuples or as segments; the argument errors."""
    if int(n_bins) != n_bins or n_bins < 1 or n_bins >= 2 ** 31:
        raise ValueError("n_bins %r is not in 1 .. 2^31 - 1" % (n_bins,))
    rows = [(q.chrom, q.start, q.end) if hasattr(q, "chrom") else tuple(q) for q in queries]
    names = [r[0] for r in rows]
    start, end = np.array([int(r[1]) for r in rows], np.int64), np.array([int(r[2]) for r in rows], np.int64)
    for k in np.flatnonzero((start < 0) | (start >= 2 ** 31) | (end >= 2 ** 31))[:1]:
        raise ValueError("query %d (%s:%d-%d): a coordinate below 0 or at or beyond 2^31" % (k, names[k], start[k], end[k]))
    for k in np.flatnonzero(start >= end)[:1]:
        raise ValueError("query %d (%s:%d-%d): start >= end" % (k, names[k], start[k], end[k]))
    return names, start, end


def _summary_contigs(names, index, filename):
    """The place of every query's contig in the file's chromosome list, -1 (and one ``DataWarning`` per name) where it has none."""
    contig = np.array([index.get(n, -1) for n in names], np.int32)
    for c in sorted(set(names[k] for k in np.flatnonzero(contig < 0))):
        warn(WARN_CHROM_NOT_FOUND % (c, filename), DataWarning)
    return contig


def _bind_summary(L):
    if not hasattr(L.pb_bigwig_summary_open, "_bound"):
        vp = ctypes.c_void_p
        L.pb_bigwig_summary_open.restype = vp
        L.pb_bigwig_summary_open.argtypes = [vp, ctypes.c_int64, ctypes.c_char_p]
        L.pb_bigwig_summary_close.argtypes = [vp]
        L.pb_bigwig_summary_nchrom.argtypes = [vp]
        L.pb_bigwig_summary_chrom.restype = ctypes.c_char_p
        L.pb_bigwig_summary_chrom.argtypes = [vp, ctypes.c_int]
        L.pb_bigwig_summary_query.argtypes = [vp, ctypes.c_int64, vp, vp, vp, ctypes.c_int64, vp]
        L.pb_bigwig_summary_values.argtypes = [ctypes.c_int64, vp, vp, ctypes.c_int64, vp, ctypes.c_double, ctypes.c_int, vp]
        L.pb_bigwig_summary_stats.argtypes = [vp, vp, ctypes.c_int, vp]
        L.pb_bigwig_summary_open._bound = True


def _summary_values(start, end, n_bins, elements, kinds, as_dict, fill):
    """The kinds of ``float64[5, nq, n_bins]`` elements by the model's formulas (``value_of``), `fill` where valid is 0."""
    from .bam import _load
    L = _load()
    _bind_summary(L)
    nq = len(start)
    out = np.empty((5, nq, int(n_bins)), np.float64)          # (only the columns asked for are filled, and returned)
    mask = sum(1 << SUMMARY_KINDS.index(k) for k in set(kinds))
    if nq and L.pb_bigwig_summary_values(nq, start.ctypes.data, end.ctypes.data, int(n_bins), elements.ctypes.data, float(fill), mask, out.ctypes.data) != 0:
        raise ValueError(L.pb_last_error().decode("utf-8", "replace"))
    if as_dict:
        return {k: out[SUMMARY_KINDS.index(k)] for k in kinds}
    return out[SUMMARY_KINDS.index(kinds[0])]


def _summary_elements_host(path_or_bytes, queries, n_bins):
    from .bam import _load
    L = _load()
    _bind_summary(L)
    names, start, end = _summary_queries(queries, n_bins)
    ptr, size, name, _keep = _bigwig_bytes(path_or_bytes)
    h = L.pb_bigwig_summary_open(ptr, size, name)
    if not h:
        raise ValueError(L.pb_last_error().decode("utf-8", "replace"))
    try:
        index = {L.pb_bigwig_summary_chrom(h, i).decode("utf-8", "replace"): i for i in range(L.pb_bigwig_summary_nchrom(h))}
        contig = _summary_contigs(names, index, name.decode("utf-8", "replace"))
        out = np.empty((5, len(names), int(n_bins)), np.float64)       # (the call fills every element)
        if len(names) and L.pb_bigwig_summary_query(h, len(names), contig.ctypes.data, start.ctypes.data, end.ctypes.data, int(n_bins), out.ctypes.data) != 0:
            raise ValueError(L.pb_last_error().decode("utf-8", "replace"))
    finally:
        L.pb_bigwig_summary_close(h)
    return out, start, end


def summary_elements_bigwig(path_or_bytes, queries, n_bins):
    """The summary elements of ``(chrom, start, end)`` queries over `n_bins` equal bins each, on the host, one thread: a
    dict of ``float64[len(queries), n_bins]`` columns ``valid``, ``min``, ``max``, ``sum``, ``sumsq`` -- Kent's
    ``bbiSummaryElement`` per bin; a bin without data is all zeros.  See :func:`summarize_bigwig`."""
    out, _, _ = _summary_elements_host(path_or_bytes, queries, n_bins)
    return dict(zip(SUMMARY_ELEMENTS, out))


def summarize_bigwig(path_or_bytes, queries, n_bins, kind="mean", fill=np.nan):
    """Binned summaries of a bigWig file (a path, or its bytes) on the host, one thread, without a GPU: what Kent's
    ``bigWigSummaryArray`` gives, bit for bit (``csrc/bigwig_summary_host.h`` states the rules; the kernels of
    :meth:`BigWigReader.summarize_batch` run the same functions).  `queries`: ``(chrom, start, end)`` tuples or segments;
    every query is cut into `n_bins` equal bins and answered from the coarsest zoom level that still gives two records per
    bin, from the items where no level is coarse enough.  `kind`: one of ``mean``, ``min``, ``max``, ``coverage``, ``std``
    -- ``float64[len(queries), n_bins]`` -- or a tuple of them -- a dict.  A bin without data, and every bin on a contig
    the file lacks, is `fill`.  ``ValueError``: ``n_bins < 1``, ``start >= end``, a coordinate at or beyond 2^31, a file
    that is refused, and ``"<path>: bigWig: summarize needs records in coordinate order"`` for a table whose records are
    not sorted (Kent's writer and ours sort them)."""
    kinds, as_dict = _summary_kinds(kind)
    out, start, end = _summary_elements_host(path_or_bytes, queries, n_bins)
    return _summary_values(start, end, n_bins, out, kinds, as_dict, fill)


def sum_ranges(lengths):
    """The positions ``BigWigReader.sum()`` adds, per contig in ``chroms`` order: the reference's position counter is set
    to 0 once, in front of the loop over the contigs (plastid/readers/bigwig.pyx:273-296), so contig k gives only its
    positions from the greatest length of the contigs in front of it on.  ``[(start, end)]``, empty ranges included."""
    out, i = [], 0
    for n in lengths:
        out.append((min(i, n), n))
        i = max(i, n)
    return out


def inflate_zlib(engine, streams, capacity):
    """``pc_inflate_zlib``: every zlib stream of `streams` (bytes) inflated by one wave on `engine` into at most `capacity`
    bytes.  Returns ``[(payload bytes, status)]``; status 0, or why the stream was refused (include/plastid_counts.h)."""
    n = len(streams)
    image = b"".join(streams)
    lens = np.array([len(s) for s in streams], np.int64)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64) if n else np.zeros(0, np.int64)
    buf = ctypes.create_string_buffer(image, len(image)) if image else ctypes.create_string_buffer(1)
    out = np.zeros(max(n * int(capacity), 1), np.uint8)
    out_len, status = np.zeros(max(n, 1), np.int64), np.zeros(max(n, 1), np.int32)
    check(_lib.load().pc_inflate_zlib(engine._h, ctypes.cast(buf, ctypes.c_void_p), n, offs.ctypes.data, lens.ctypes.data, int(capacity),
                                      out.ctypes.data, out_len.ctypes.data, status.ctypes.data), "pc_inflate_zlib")
    return [(out[k * int(capacity):k * int(capacity) + int(out_len[k])].tobytes(), int(status[k])) for k in range(n)]


DEFLATE_MAX_INPUT = 24600     # pcdeflate::kMaxInput: one bedGraph section of 2 048 items


def _deflate(call, inputs, capacity):
    n = len(inputs)
    image = b"".join(bytes(s) for s in inputs)
    lens = np.array([len(s) for s in inputs], np.int64)
    offs = (np.cumsum(lens) - lens).astype(np.int64)
    need = int(lens.sum()) + 11 * n
    capacity = need if capacity is None else int(capacity)
    buf = ctypes.create_string_buffer(image, len(image)) if image else ctypes.create_string_buffer(1)
    out = np.zeros(max(capacity, 1), np.uint8)
    out_off, out_len = np.zeros(max(n, 1), np.int64), np.zeros(max(n, 1), np.int64)
    call(ctypes.cast(buf, ctypes.c_void_p), n, offs.ctypes.data, lens.ctypes.data, out.ctypes.data, capacity, out_off.ctypes.data, out_len.ctypes.data)
    total = int(out_off[n - 1] + out_len[n - 1]) if n else 0
    return out[:total].tobytes(), out_off[:n].copy(), out_len[:n].copy()


DEFLATE_CODES = {"fixed": 1, "dynamic": 2}      # the modes of pc_deflate_zlib_mode


def _codes_mode(codes):
    if codes not in DEFLATE_CODES:
        raise ValueError("codes: %r is neither 'fixed' nor 'dynamic'" % (codes,))
    return DEFLATE_CODES[codes]


def _compress_mode(compress):
    """`compress` of the bigWig writers as the C interface takes it: 0 stored sections, 1 fixed codes, 2 dynamic codes."""
    if isinstance(compress, str):
        if compress in DEFLATE_CODES:
            return DEFLATE_CODES[compress]
    elif compress is None or isinstance(compress, (bool, np.bool_)) or (isinstance(compress, (int, np.integer)) and compress in (0, 1)):
        return 1 if compress else 0
    raise ValueError("compress: %r is none of True, False, 'fixed', 'dynamic'" % (compress,))


def _zoom_mode(zoom):
    """`zoom` of the bigWig writers as the C interface takes it: 0 no zoom levels, -1 the automatic first reduction, or
    the first reduction itself, 8 .. 2**24.  A bool is not an int here."""
    if isinstance(zoom, (bool, np.bool_)):
        return -1 if zoom else 0
    if isinstance(zoom, (int, np.integer)) and 8 <= int(zoom) <= 2 ** 24:
        return int(zoom)
    raise ValueError("zoom: %r is none of False, True, an int in 8 .. 2**24 (the first reduction)" % (zoom,))


def deflate_zlib(engine, inputs, capacity=None, codes="fixed"):
    """``pc_deflate_zlib_mode``: every input of `inputs` (bytes, at most 24 600 each) encoded by one workgroup of ``k_zlib_deflate``
    on `engine` into one zlib stream.  Returns ``(bytes of the streams back to back, offsets, lengths)``; stream k is
    ``out[off[k]:off[k] + len[k]]``, at most ``len(inputs[k]) + 11`` bytes.  `capacity` (default: the sum of the inputs + 11
    each): the room offered; less is a ``ValueError``, as an over-long input is.  `codes`: ``"fixed"`` (the fixed Huffman
    codes) or ``"dynamic"`` (the same tokens under codes built for the block; never longer than the fixed stream).  No
    reference counterpart."""
    L = _lib.load()
    mode = _codes_mode(codes)

    def call(*args):
        check(L.pc_deflate_zlib_mode(engine._h, *(args + (mode,))), "pc_deflate_zlib_mode")
    return _deflate(call, inputs, capacity)


def deflate_zlib_host(inputs, capacity=None, codes="fixed"):
    """``pb_deflate_zlib_mode``: :func:`deflate_zlib` by the serial model encoder of ``csrc/deflate_host.h`` on the host --
    the bytes the kernel must give, and the encoder of :func:`write_bigwig`."""
    from .bam import _load
    L = _load()
    vp = ctypes.c_void_p
    L.pb_deflate_zlib_mode.argtypes = [vp, ctypes.c_int64, vp, vp, vp, ctypes.c_int64, vp, vp, ctypes.c_int]
    mode = _codes_mode(codes)

    def call(*args):
        if L.pb_deflate_zlib_mode(*(args + (mode,))) != 0:
            raise ValueError(L.pb_last_error().decode("utf-8", "replace"))
    return _deflate(call, inputs, capacity)


def _huffman_counts(counts, limit):
    counts = np.ascontiguousarray(counts)
    if counts.ndim != 1 or (len(counts) and (counts.min() < 0 or int(counts.astype(object).sum()) >= 1 << 32)):
        raise ValueError("huffman_lengths: counts must be one row of numbers >= 0 that add up to less than 2^32")
    return counts.astype(np.uint32), np.zeros(max(len(counts), 1), np.uint8), int(limit)


def huffman_lengths(engine, counts, limit):
    """``pc_huffman_lengths``: the code lengths (uint8, 0 for an unused symbol) the encoder's dynamic mode gives `counts`
    (2 .. 286 symbols) under the length `limit` (1 .. 15, ``2 ** limit >= len(counts)``), computed by ``k_huffman_lengths``
    on `engine`: fewer than two used symbols are padded with the lowest-numbered unused ones, the code is complete, and
    length never grows with (count, symbol).  ``ValueError`` for what is out of range.  No reference counterpart."""
    c, out, limit = _huffman_counts(counts, limit)
    check(_lib.load().pc_huffman_lengths(engine._h, c.ctypes.data, len(c), limit, out.ctypes.data), "pc_huffman_lengths")
    return out[:len(c)].copy()


def huffman_lengths_host(counts, limit):
    """``pb_huffman_lengths``: :func:`huffman_lengths` by ``pcdeflate::build_code`` of ``csrc/deflate_host.h`` on the host."""
    from .bam import _load
    L = _load()
    vp = ctypes.c_void_p
    L.pb_huffman_lengths.argtypes = [vp, ctypes.c_int64, ctypes.c_int, vp]
    c, out, limit = _huffman_counts(counts, limit)
    if L.pb_huffman_lengths(c.ctypes.data, len(c), limit, out.ctypes.data) != 0:
        raise ValueError(L.pb_last_error().decode("utf-8", "replace"))
    return out[:len(c)].copy()


BIGWIG_WRITE_STATS = ("contigs", "items", "sections", "raw_bytes", "block_bytes", "stored_sections")
BIGWIG_ZOOM_STATS = ("reduction", "records", "blocks", "raw_bytes", "file_bytes")
ZOOM_MAX_LEVELS = 10


def _binary_sink(path_or_file):
    """``(file object, close it afterwards)`` of a path or a binary file object; a text-mode file is a ``TypeError``."""
    if isinstance(path_or_file, (str, bytes, os.PathLike)):
        return open(os.fspath(path_or_file), "wb"), True
    if isinstance(path_or_file, io.TextIOBase) or not hasattr(path_or_file, "write"):
        raise TypeError("a bigWig file is binary: give a path or a file opened in binary mode")
    return path_or_file, False


def _check_bigwig_params(items_per_slot, block_size):
    if not 1 <= int(items_per_slot) <= 2048:
        raise ValueError("to_bigwig: items_per_slot outside 1 .. 2048")
    if not 2 <= int(block_size) <= 65535:
        raise ValueError("to_bigwig: block_size outside 2 .. 65535")


def write_bigwig(host_array, path_or_file, strand, items_per_slot=1024, block_size=256, compress=True, block_types=False, zoom=False,
                 zoom_stats=False):
    """Write `strand` of a host ``DenseGenomeArray`` as a bigWig file by the serial writer of ``csrc/bigwig_write_host.h``
    (``pb_bigwig_write_*``): the item walk, the model encoder of ``csrc/deflate_host.h`` and the container code the device
    export shares.  The model of :meth:`GenomeArray.to_bigwig`, and the way to write a bigWig without a GPU.

    A cell is written iff its value ``!= 0.0`` (NaN is, ``-0.0`` is not); neighbouring written cells form one item while
    their float64 values compare equal; values are cast to float32.  Contigs stand in sorted order, every contig is in
    the chromosome tree at ``max(reported length, cells stored)``; every `items_per_slot` items of a contig make one
    bedGraph section, `block_size` is the fan-out of the trees.  Normalisation is not applied.
    `compress` and `zoom` as :meth:`GenomeArray.to_bigwig` takes them: ``True`` / ``"fixed"``, ``"dynamic"``, ``False``;
    ``False`` (no zoom levels), ``True`` (the automatic first reduction), or the first reduction, 8 .. 2**24 -- the serial
    model of the zoom levels, window by window.
    Returns the writer's statistics (``BIGWIG_WRITE_STATS``; with `block_types` also ``fixed_sections`` and
    ``dynamic_sections``, as :meth:`GenomeArray.bigwig_export_stats` gives them; with `zoom_stats` also ``zoom``, the list
    :meth:`GenomeArray.bigwig_export_zoom_stats` gives).  No reference counterpart."""
    _check_bigwig_params(items_per_slot, block_size)
    mode, zoom_mode = _compress_mode(compress), _zoom_mode(zoom)
    if isinstance(path_or_file, io.TextIOBase):
        raise TypeError("a bigWig file is binary: give a path or a file opened in binary mode")
    assert strand in host_array.strands()
    from .bam import _load
    L = _load()
    vp = ctypes.c_void_p
    if not hasattr(L.pb_bigwig_write_open, "_bound"):
        L.pb_bigwig_write_open.restype = vp
        L.pb_bigwig_write_open.argtypes = [ctypes.c_int64, ctypes.c_int64, ctypes.c_int]
        L.pb_bigwig_write_close.argtypes = [vp]
        L.pb_bigwig_write_add.argtypes = [vp, ctypes.c_char_p, ctypes.c_int64, vp, ctypes.c_int64]
        L.pb_bigwig_write_finish.argtypes = [vp]
        L.pb_bigwig_write_size.restype = ctypes.c_int64
        L.pb_bigwig_write_size.argtypes = [vp]
        L.pb_bigwig_write_image.restype = vp
        L.pb_bigwig_write_image.argtypes = [vp]
        L.pb_bigwig_write_stats.argtypes = [vp, vp]
        L.pb_bigwig_write_block_types.argtypes = [vp, vp]
        L.pb_bigwig_write_open_zoom.restype = vp
        L.pb_bigwig_write_open_zoom.argtypes = [ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_int64]
        L.pb_bigwig_write_zoom_stats.argtypes = [vp, vp, ctypes.c_int, vp]
        L.pb_bigwig_write_open._bound = True
    h = L.pb_bigwig_write_open_zoom(int(items_per_slot), int(block_size), mode, zoom_mode)
    if not h:
        raise ValueError(L.pb_last_error().decode("utf-8", "replace"))
    try:
        lengths = host_array.lengths()
        for chrom in host_array.chroms():
            cells = np.ascontiguousarray(host_array._chroms[chrom][strand], np.float64)
            if L.pb_bigwig_write_add(h, chrom.encode("utf-8"), int(lengths[chrom]), cells.ctypes.data, len(cells)) != 0:
                raise ValueError(L.pb_last_error().decode("utf-8", "replace"))
        if L.pb_bigwig_write_finish(h) != 0:
            raise ValueError(L.pb_last_error().decode("utf-8", "replace"))
        image = ctypes.string_at(L.pb_bigwig_write_image(h), int(L.pb_bigwig_write_size(h)))
        stats = np.zeros(6, np.int64)
        L.pb_bigwig_write_stats(h, stats.ctypes.data)
        types = np.zeros(3, np.int64)
        L.pb_bigwig_write_block_types(h, types.ctypes.data)
        nlevels, levels = ctypes.c_int64(0), np.zeros(5 * ZOOM_MAX_LEVELS, np.int64)
        L.pb_bigwig_write_zoom_stats(h, ctypes.byref(nlevels), ZOOM_MAX_LEVELS, levels.ctypes.data)
    finally:
        L.pb_bigwig_write_close(h)
    sink, close = _binary_sink(path_or_file)
    try:
        sink.write(image)
    finally:
        if close:
            sink.close()
    out = dict(zip(BIGWIG_WRITE_STATS, (int(x) for x in stats)))
    if block_types:
        out["fixed_sections"], out["dynamic_sections"] = int(types[1]), int(types[2])
    if zoom_stats:
        out["zoom"] = [dict(zip(BIGWIG_ZOOM_STATS, (int(x) for x in levels[5 * k:5 * k + 5]))) for k in range(int(nlevels.value))]
    return out


class BigWigReader(object):
    """The reference's ``BigWigReader`` (plastid/readers/bigwig.pyx:109-412) with the file's values in HBM: the data blocks
    are inflated, checked and decoded on the GPU once, at construction, into a one-strand count track (float64 cells per
    contig up to the furthest end written); every read is a gather.  `maxmem` is accepted and ignored; `engine`: an
    :class:`~plastid_amd.engine.Engine` to share (default: one of its own on GPU 0).  ``fill`` is fixed at 0.0, as in the
    reference, whose setter is commented out.  Not here: ``__iter__`` / ``BigWigIterator``, remote files.
    ``ValueError("<path>: bigWig: <what>")`` for a file that is refused (README: byte-swapped files are).

    :meth:`summarize` / :meth:`summarize_batch` / :meth:`summary_elements_batch` are the batched reader a browser or
    ``bigWigSummary`` is: mean, min, max, coverage and std over `n_bins` equal bins of each of many regions, Kent's
    ``bigWigSummaryArray`` bit for bit.  They do not read the cells (the import keeps no coverage: a stored 0.0 and "no
    data" are the same cell) but the file's ZOOM LEVELS and items: every query is answered from the level with the
    greatest reduction that still gives two records per bin, from the items where no level is that fine.  A table -- one
    level's records, or the items -- goes to HBM at the first query that selects it and stays; ``k_bbi_summarize`` then runs
    one lane per (query, bin), once per table in use, and one buffer of elements comes back.  A lane walks its bin
    serially, because the sums are exact in their order: a file WITHOUT zoom levels asked for bins of millions of items
    is slow by construction -- that case is what ``to_bigwig(zoom=True)`` is for.  A table whose records are not in
    coordinate order (no writer of Kent's or ours makes one) raises ``ValueError("<path>: bigWig: summarize needs records
    in coordinate order")`` on the queries that would use it; ``get`` and the rest are not affected."""

    def __init__(self, filename, maxmem=0, engine=None, **kwargs):
        self.filename = os.fspath(filename)
        if not os.path.isfile(self.filename):
            raise IOError("No such file: %r" % (self.filename,))
        self.fill = 0.0
        self._maxmem = maxmem
        self._sum = None
        self._ga = GenomeArray(strands=(".",), engine=engine)
        try:
            check(self._ga._lib.pc_track_add_bigwig_path(self._ga._h, os.fsencode(self.filename), 0), "pc_track_add_bigwig_path")
        except Exception:
            self._ga.close()
            raise
        self._engine = self._ga._engine
        self._chroms = self._ga.lengths()
        self._index = {c: i for i, c in enumerate(self._chroms)}
        self._summary = None

    def close(self):
        self._close_summary()
        self._ga.close()

    def _close_summary(self):
        if getattr(self, "_summary", None) is not None:
            if self._engine._finalizer.alive:      # (an engine that is gone took its summary readers with it)
                self._ga._lib.pc_bigwig_summary_close(self._summary)
            self._summary = None

    def __del__(self):
        try:
            self._close_summary()
        except Exception:
            pass

    @property
    def chroms(self):
        """``{name: size}`` in the order of Kent's ``bbiChromList`` (bbifile.pyx:211-237)."""
        return OrderedDict(self._chroms)

    def import_stats(self):
        """Of the import: blocks, blocks inflated on the GPU, items of bedGraph / variableStep / fixedStep sections,
        overlapping items, bytes uploaded, bytes inflated."""
        out = np.zeros(8, np.int64)
        check(self._ga._lib.pc_track_bigwig_stats(self._ga._h, out.ctypes.data))
        keys = ("blocks", "inflated_blocks", "bedgraph_items", "variable_step_items", "fixed_step_items", "overlapping", "bytes_in", "bytes_inflated")
        return dict(zip(keys, (int(x) for x in out)))

    def import_timing(self):
        """Milliseconds of the import: upload, inflate + Adler-32, sections + items, sort + apply."""
        out = np.zeros(4, np.float64)
        check(self._ga._lib.pc_track_bigwig_timing(self._ga._h, out.ctypes.data))
        return dict(zip(("upload", "inflate_adler", "sections_items", "sort_apply"), (float(x) for x in out)))

    def get(self, roi, roi_order=True, fill=np.nan):
        """Values over a |GenomicSegment| (a |SegmentChain| goes to ``roi.get_counts(self)``), 0.0 where nothing covers;
        a contig that is not in the file gives zeros and one ``DataWarning``; reversed for ``'-'`` when `roi_order`.
        `fill` other than NaN or 0.0 raises ``NotImplementedError``: it needs a bitmap of the covered positions, which the
        import does not build (the reference's own non-zero fill is commented out for ``get_chromosome_counts``)."""
        if not (np.isnan(fill) or fill == 0.0):
            raise NotImplementedError("a fill other than 0.0 needs the coverage bitmap, which is not built")
        if isinstance(roi, SegmentChain):
            return roi.get_counts(self)
        n = max(int(roi.end) - int(roi.start), 0)
        if roi.chrom not in self._index:
            warn(WARN_CHROM_NOT_FOUND % (roi.chrom, self.filename), DataWarning)
            return np.zeros(n, np.float64)
        rev = roi_order is True and roi.strand == "-"
        return self._ga._gather([self._index[roi.chrom]], [0], [roi.start], [roi.start + n], [n - 1 if rev else 0], [-1 if rev else 1], n)

    def __getitem__(self, roi):
        return self.get(roi)

    # ---- binned summaries from the zoom levels and the items
    def _summary_handle(self):
        if self._summary is None:
            h = ctypes.c_void_p()
            check(self._ga._lib.pc_bigwig_summary_open_path(self._engine._h, os.fsencode(self.filename), ctypes.byref(h)), "pc_bigwig_summary_open_path")
            self._summary = h
        return self._summary

    def _summary_elements(self, segments, n_bins):
        """``(float64[5, len, n_bins] elements, start, end)`` of `segments` in genome order."""
        names, start, end = _summary_queries(segments, n_bins)
        contig = _summary_contigs(names, self._index, self.filename)
        out = np.empty((5, len(names), int(n_bins)), np.float64)       # (the call fills every element)
        if len(names):
            check(self._ga._lib.pc_bigwig_summary_query(self._summary_handle(), len(names), contig.ctypes.data, start.ctypes.data, end.ctypes.data, int(n_bins),
                                                        out.ctypes.data), "pc_bigwig_summary_query")
        return out, start, end

    def summary_elements_batch(self, segments, n_bins):
        """Kent's ``bbiSummaryElement`` per bin of every segment: a dict of ``float64[len(segments), n_bins]`` columns
        ``valid``, ``min``, ``max``, ``sum``, ``sumsq``, bins in genome order; a bin without data is all zeros."""
        out, _, _ = self._summary_elements(segments, n_bins)
        return dict(zip(SUMMARY_ELEMENTS, out))

    def summarize_batch(self, segments, n_bins, kind="mean", fill=np.nan, roi_order=True):
        """`kind` -- ``mean``, ``min``, ``max``, ``coverage`` or ``std`` -- over `n_bins` equal bins of every |GenomicSegment|
        (or ``(chrom, start, end)`` tuple) of `segments`, in one call: ``float64[len(segments), n_bins]``; a tuple of kinds
        gives a dict of such arrays.  Bin ``i`` of a segment is ``[start + span * i // n_bins, start + span * (i + 1) //
        n_bins)``; the bins of a ``'-'`` segment come reversed when `roi_order`, as :meth:`get` returns them.  A bin
        without data is `fill`; so is every bin on a contig the file lacks, with the ``DataWarning`` of :meth:`get`.
        ``ValueError``: ``n_bins < 1``, ``start >= end``, a coordinate at or beyond 2^31, a table that is not in
        coordinate order (the class docstring)."""
        kinds, as_dict = _summary_kinds(kind)
        segments = list(segments)
        el, start, end = self._summary_elements(segments, n_bins)
        out = _summary_values(start, end, n_bins, el, kinds, as_dict, fill)
        if roi_order is True:
            rev = np.array([getattr(s, "strand", "+") == "-" for s in segments], bool)
            for a in (out.values() if as_dict else (out,)):
                a[rev] = a[rev, ::-1]
        return out

    def summarize(self, roi, n_bins=1, kind="mean", fill=np.nan, roi_order=True):
        """:meth:`summarize_batch` of one |GenomicSegment|: ``float64[n_bins]`` (a dict of them for a tuple of kinds)."""
        out = self.summarize_batch([roi], n_bins, kind=kind, fill=fill, roi_order=roi_order)
        return {k: v[0] for k, v in out.items()} if isinstance(out, dict) else out[0]

    def summary_stats(self):
        """Of the summaries so far: ``tables`` the file has (the items and its zoom levels), ``tables_loaded``,
        ``bytes_uploaded``, ``bytes_inflated``, and per table -- ``"items"`` or the level's reduction -- its ``records``
        (``None`` until it is loaded) and the ``queries`` it has answered."""
        L, h = self._ga._lib, self._summary_handle()
        head = np.zeros(4, np.int64)
        check(L.pc_bigwig_summary_stats(h, head.ctypes.data, 0, None))
        per = np.zeros(3 * max(int(head[0]), 1), np.int64)
        check(L.pc_bigwig_summary_stats(h, head.ctypes.data, int(head[0]), per.ctypes.data))
        out = dict(zip(("tables", "tables_loaded", "bytes_uploaded", "bytes_inflated"), (int(x) for x in head)))
        out["per_table"] = OrderedDict(("items" if k == 0 else int(per[3 * k]), {"records": None if per[3 * k + 1] < 0 else int(per[3 * k + 1]), "queries": int(per[3 * k + 2])})
                                       for k in range(int(head[0])))
        return out

    def summary_timing(self):
        """Milliseconds of the last summary call on the engine's stream: upload, inflate + Adler-32, records + order check
        (all 0 when it loaded no table), the summarize kernels, the read-back."""
        out = np.zeros(5, np.float64)
        check(self._ga._lib.pc_bigwig_summary_timing(self._summary_handle(), out.ctypes.data))
        return dict(zip(("upload", "inflate_adler", "records_order_check", "kernel", "read_back"), (float(x) for x in out)))

    def get_chromosome_counts(self, chrom):
        """The whole contig at its size in the chromosome tree, zeros where no data; an unknown contig warns and gives
        ``numpy.array(0, dtype=float)`` (bigwig.pyx:314-412)."""
        if chrom not in self._index:
            warn(WARN_CHROM_NOT_FOUND % (chrom, self.filename), DataWarning)
            warn("Could not retrieve data for chrom '%s' from file '%s'." % (chrom, self.filename), DataWarning)
            return np.array(0, dtype=float)
        n = self._chroms[chrom]
        return self._ga._gather([self._index[chrom]], [0], [0], [n], [0], [1], n)

    def sum(self):
        """The reference's sum (bigwig.pyx:265-302): over the positions :func:`sum_ranges` lists -- its position counter
        is never reset between contigs -- by a fixed-tree reduction on the device, cached."""
        if self._sum is None:
            warn("Summing over a large BigWig file can take a while.", DataWarning)
            ranges = sum_ranges(list(self._chroms.values()))
            n = len(ranges)
            contig, slot = np.arange(n, dtype=np.int32), np.zeros(n, np.int32)
            start, end = np.array([a for a, _ in ranges], np.int64), np.array([b for _, b in ranges], np.int64)
            out = ctypes.c_double()
            check(self._ga._lib.pc_track_sum_ranges(self._ga._h, n, contig.ctypes.data, slot.ctypes.data, start.ctypes.data, end.ctypes.data,
                                                    ctypes.byref(out)), "pc_track_sum_ranges")
            self._sum = float(out.value)
        return self._sum


class BigWigGenomeArray(object):
    """The reference's ``BigWigGenomeArray`` (genome_array.py:1114-1320) over device-resident :class:`BigWigReader` s on one
    engine.  ``get`` / ``get_counts_batch`` add the readers of a strand in their order, ``0.0 + r1 + r2 + ...`` per element,
    one accumulating launch per reader; normalisation is ``v / sum * 1e6`` (:1212; not ``GenomeArray``'s order)."""

    def __init__(self, maxmem=0, engine=None, **kwargs):
        from .engine import Engine
        self._strand_dict = OrderedDict()
        self._normalize = False
        self._chromset = None
        self._sum = None
        self._lengths = None
        self._strands = []
        self._maxmem = maxmem
        self.fill = 0.0
        self._own_engine = engine is None
        self._engine = Engine(0) if engine is None else engine

    def close(self):
        for readers in self._strand_dict.values():
            for bw in readers:
                bw.close()
        self._strand_dict = OrderedDict()
        if self._own_engine:
            self._engine.close()

    def add_from_bigwig(self, filename, strand):
        """Append a reader of `filename` to `strand`'s list; the cached chroms, lengths and sum are dropped (:1271-1292)."""
        bw = BigWigReader(filename, maxmem=self._maxmem, engine=self._engine)
        self._chromset = None
        self._lengths = None
        self._sum = None
        self._strand_dict.setdefault(strand, []).append(bw)
        self._strands = sorted(self._strand_dict.keys())

    def _readers(self):
        return [bw for readers in self._strand_dict.values() for bw in readers]

    def strands(self):
        return self._strands

    def chroms(self):
        if self._chromset is None:
            self._chromset = set(c for bw in self._readers() for c in bw.chroms)
        return self._chromset

    def keys(self):
        return self.chroms()

    def __contains__(self, chrom):
        return chrom in self.chroms()

    def __len__(self):
        return len(self._strands) * sum(self.lengths().values())

    def lengths(self):
        if self._lengths is None:
            lengths = {}
            for bw in self._readers():
                for k, v in bw.chroms.items():
                    lengths[k] = max(lengths.get(k, 0), v)
            self._lengths = lengths
        return self._lengths

    def reset_sum(self):
        my_sum = 0
        for bw in self._readers():
            my_sum += bw.sum()
        self._sum = my_sum
        return my_sum

    def set_sum(self, val):
        self._sum = val

    def sum(self):
        if self._sum is None:
            self.reset_sum()
        return self._sum

    def set_normalize(self, value=True):
        assert value in (True, False)
        self._normalize = value

    def _gather(self, strand, chroms, start, end, out_off, out_step, total):
        """The readers of `strand` over a segment table (``chroms``: the segments' contig names), added in reader order."""
        out = np.zeros(int(total), np.float64)
        readers = self._strand_dict.get(strand)
        if readers is None:
            warn("Strand '%s' not in BigWigGenomeArray (has %s)." % (strand, ", ".join(self._strand_dict.keys())), DataWarning)
            readers = []
        for bw in readers:
            for c in OrderedDict.fromkeys(chroms):
                if c not in bw._index:
                    warn(WARN_CHROM_NOT_FOUND % (c, bw.filename), DataWarning)
        norm = 1 if self._normalize is True else 0
        total_sum = float(self.sum()) if norm else 1.0
        if total == 0:
            return out
        nseg, ntrack = len(chroms), len(readers)
        contig = np.array([[bw._index.get(c, -1) for c in chroms] for bw in readers], np.int32).reshape(ntrack, nseg)
        slot = np.zeros((ntrack, nseg), np.int32)
        handles = (ctypes.c_void_p * max(ntrack, 1))(*[bw._ga._h for bw in readers])
        arrs = (np.ascontiguousarray(start, np.int64), np.ascontiguousarray(end, np.int64), np.ascontiguousarray(out_off, np.int64),
                np.ascontiguousarray(out_step, np.int8))
        check(_lib.load().pc_track_gather_sum(ntrack, handles, nseg, contig.ctypes.data, slot.ctypes.data, *[a.ctypes.data for a in arrs],
                                              int(total), norm, total_sum, out.ctypes.data), "pc_track_gather_sum")
        return out

    def get(self, roi, roi_order=True):
        """Values over a |GenomicSegment| (or a |SegmentChain|): ``zeros(len)`` plus every reader of the strand in order; a
        strand the array lacks gives zeros and a ``DataWarning`` naming the strands it has; then ``v / sum * 1e6`` when
        normalising, then the ``'-'`` reversal (:1171-1217)."""
        if isinstance(roi, SegmentChain):
            return roi.get_counts(self)
        n = max(int(roi.end) - int(roi.start), 0)
        rev = roi_order is True and roi.strand == "-"
        return self._gather(roi.strand, [roi.chrom], [roi.start], [roi.start + n], [n - 1 if rev else 0], [-1 if rev else 1], n)

    def __getitem__(self, roi):
        return self.get(roi, roi_order=True)

    def _get_chain_counts(self, chain, stranded=True):
        return self.get_counts_batch([chain], stranded=stranded)[0]

    def get_counts_batch(self, chains, stranded=True):
        """Many |SegmentChains|: a list of float64 arrays, each what ``chain.get_counts(self, stranded)`` returns.  The
        chains of one strand share one call (one launch per reader of that strand)."""
        from .engine import chain_layout
        out = [None] * len(chains)
        by_strand = OrderedDict()
        for ci, c in enumerate(chains):
            by_strand.setdefault(c.strand, []).append(ci)
        for strand, which in by_strand.items():
            segs = [[(s.start, s.end) for s in chains[ci]] for ci in which]
            seg_chain, out_off, out_step, _, chain_base, chain_len, total = chain_layout(segs, [strand] * len(which), rows=1, stranded=stranded is True)
            flat = [se for chain_segs in segs for se in chain_segs]
            vec = self._gather(strand, [chains[which[k]].chrom for k in seg_chain], [s for s, _ in flat], [e for _, e in flat], out_off, out_step, total)
            for k, ci in enumerate(which):
                out[ci] = vec[chain_base[k]:chain_base[k] + chain_len[k]]
        return out

    def to_genome_array(self):
        """A device :class:`GenomeArray` on the same engine (:1304-1320): every contig at ``lengths()``, every reader added
        onto its strand in order by ``pc_track_combine``, device to device -- no cell visits the host.  The reference fills
        its array through ``__setitem__`` over whole contigs, and the first write that ends at a contig's length grows the
        contig: every contig of the result reports 10000 more than ``lengths()``.  (Where two readers give one contig
        different sizes the reference fails on the shapes; here the shorter one is padded with zeros.)"""
        strands = list(self._strands)
        acc = GenomeArray(chr_lengths=self.lengths(), strands=strands, engine=self._engine)
        pad = 10000
        mine = np.arange(len(strands), dtype=np.int32)
        for strand in strands:
            for bw in self._strand_dict.get(strand, []):
                theirs = np.array([0 if s == strand else -1 for s in strands], np.int32)
                out = ctypes.c_void_p()
                check(acc._lib.pc_track_combine(acc._h, bw._ga._h, 0.0, 0, 1, pad, len(strands), mine.ctypes.data, theirs.ctypes.data, ctypes.byref(out)),
                      "pc_track_combine")
                pad = 0
                nxt = GenomeArray._wrap(out, strands, acc.min_chr_size, self._engine)
                acc._release(False)
                acc = nxt
        return acc


def __getattr__(name):
    # EXPORT_TILE (T): cells one workgroup covers in the run-head kernel; FORMAT_RUNS (R): lines one workgroup formats
    if name in ("EXPORT_TILE", "FORMAT_RUNS"):
        return _export_geometry()[0 if name == "EXPORT_TILE" else 1]
    raise AttributeError(name)
