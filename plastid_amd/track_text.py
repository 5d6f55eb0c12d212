"""Count tracks as text on the host -- bedGraph, variableStep and fixedStep wiggle -- without a GPU.

:func:`read_wiggle` is the reference's ``WiggleReader`` (plastid/readers/wiggle.py:43-174), built from the same
``csrc/track_host.h`` the import kernels compile: the model of :meth:`~plastid_amd.track.GenomeArray.add_from_wiggle`.
:func:`write_bedgraph` / :func:`write_variable_step` are ``GenomeArray.to_bedgraph`` / ``to_variable_step`` over a host
``DenseGenomeArray``, :func:`write_count_bedgraph` / :func:`write_count_variable_step` those of ``BAMGenomeArray`` over count
vectors, by the serial writers of that header: the models of the device exports.
"""
import ctypes
import io
from collections import OrderedDict

import numpy as np

from ._hostlib import buffer_of, call, load, opened, stats_dict

_EXPORT_STATS = ("lines", "runs", "listed", "bytes")      # of the writers here and of the device exports


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
    L = load()
    ptr, size, name, _keep = buffer_of(fh_or_path)
    with opened(L.pb_track_read, L.pb_track_close, ptr, size, name) as h:
        n = int(L.pb_track_rows(h))
        names = [L.pb_track_chrom(h, i).decode("utf-8", "replace") for i in range(L.pb_track_nchrom(h))]
        chrom, start, stop = np.zeros(n, np.int32), np.zeros(n, np.int64), np.zeros(n, np.int64)
        value, line, escaped = np.zeros(n, np.float64), np.zeros(n, np.int64), np.zeros(n, np.uint8)
        call(L.pb_track_fill, h, *[a.ctypes.data for a in (chrom, start, stop, value, line, escaped)])
        stats = np.zeros(4, np.int64)
        L.pb_track_stats(h, stats.ctypes.data)
    return WiggleTable(names, chrom, start, stop, value, line, escaped.astype(bool), stats_dict(("lines", "yielded", "escaped", "states"), stats))


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


def _written(L, h):
    """``(text, stats)`` of the open writer `h`."""
    text = ctypes.string_at(L.pb_track_writer_text(h), int(L.pb_track_writer_size(h)))
    stats = np.zeros(4, np.int64)
    L.pb_track_writer_stats(h, stats.ctypes.data)
    return text, stats_dict(_EXPORT_STATS, stats)


def _write_host(kind, host_array, fh, trackname, strand, kwargs):
    assert strand in host_array.strands()
    L = load()
    with opened(L.pb_track_writer_open, L.pb_track_writer_close) as h:
        for chrom in sorted(host_array.chroms()):
            cells = np.ascontiguousarray(host_array._chroms[chrom][strand], np.float64)
            call(L.pb_track_writer_add, h, kind, chrom.encode("utf-8"), cells.ctypes.data, len(cells))
        text, stats = _written(L, h)
    _write_text(fh, _track_line(kind, trackname, kwargs).encode("utf-8"))
    _write_text(fh, text)
    return stats


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
    L = load()
    with opened(L.pb_track_writer_open, L.pb_track_writer_close) as h:
        for chrom in sorted(vectors):
            v = vectors[chrom]
            call(L.pb_track_writer_add_counts, h, kind, 1 if is_float else 0, chrom.encode("utf-8"), v.ctypes.data, len(v), int(window_size))
        return _written(L, h)


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
    v = np.ascontiguousarray(values, np.float64).ravel()
    out = np.zeros(max(len(v), 1) * 24, np.uint8)
    lens = np.zeros(max(len(v), 1), np.uint8)
    call(load().pb_float_repr, v.ctypes.data, len(v), out.ctypes.data, lens.ctypes.data)
    raw = out.tobytes()
    return [raw[24 * k:24 * k + int(lens[k])].decode("ascii") for k in range(len(v))]
