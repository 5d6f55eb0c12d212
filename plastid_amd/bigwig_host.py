"""bigWig files on the host, without a GPU: the models of the device import, export and summaries.

:func:`read_bigwig` reads a file's items by ``csrc/bigwig_host.h``, :func:`write_bigwig` writes one by
``csrc/bigwig_write_host.h`` with the model encoder of ``csrc/deflate_host.h`` (:func:`deflate_zlib_host`,
:func:`huffman_lengths_host`), :func:`bigwig_zoom_info` / :func:`read_bigwig_zoom` read the zoom levels, and
:func:`summarize_bigwig` / :func:`summary_elements_bigwig` give the binned summaries of ``csrc/bigwig_summary_host.h``.
The argument checks, the constants and the summary helpers here are the ones the device classes of
:mod:`plastid_amd.bigwig` and :meth:`~plastid_amd.track.GenomeArray.to_bigwig` share.
"""
import ctypes
import io
import os
from collections import OrderedDict

import numpy as np

from . import _lib
from ._hostlib import buffer_of, call, load, opened, stats_dict
from ._lib import check
from .exceptions import DataWarning, warn

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
    L = load()
    ptr, size, name, _keep = buffer_of(path_or_bytes, image=True)
    with opened(L.pb_bigwig_read, L.pb_bigwig_close, ptr, size, name) as h:
        n, nb = int(L.pb_bigwig_rows(h)), int(L.pb_bigwig_nblocks(h))
        nchrom = L.pb_bigwig_nchrom(h)
        names = [L.pb_bigwig_chrom(h, i).decode("utf-8", "replace") for i in range(nchrom)]
        lengths = [int(L.pb_bigwig_chrom_size(h, i)) for i in range(nchrom)]
        chrom, start, stop = np.zeros(n, np.int32), np.zeros(n, np.int64), np.zeros(n, np.int64)
        value, block = np.zeros(n, np.float64), np.zeros(n, np.int32)
        block_off, block_size = np.zeros(nb, np.int64), np.zeros(nb, np.int64)
        call(L.pb_bigwig_fill, h, *[a.ctypes.data for a in (chrom, start, stop, value, block, block_off, block_size)])
        stats = np.zeros(8, np.int64)
        L.pb_bigwig_stats(h, stats.ctypes.data)
    keys = ("blocks", "compressed_blocks", "bedgraph_items", "variable_step_items", "fixed_step_items", "bytes_inflated", "uncompress_buf_size", "version")
    return BigWigTable(names, lengths, chrom, start, stop, value, block, block_off, block_size, stats_dict(keys, stats))



def bigwig_zoom_info(path_or_bytes):
    """The zoom levels of a bigWig file (a path, or its bytes), without a GPU: a list of ``(reduction, data_offset,
    index_offset, records)``, one per zoom header in the file's order -- ``data_offset`` points at the level's u32 record
    count, ``index_offset`` at its R-tree.  Empty for a file without zoom levels.  ``ValueError("<path>: bigWig: <what>")``
    for a file that is refused."""
    L = load()
    ptr, size, name, _keep = buffer_of(path_or_bytes, image=True)
    n = ctypes.c_int64(0)
    call(L.pb_bigwig_zoom_info, ptr, size, name, ctypes.byref(n), 0, None)
    out = np.zeros(4 * max(int(n.value), 1), np.int64)
    call(L.pb_bigwig_zoom_info, ptr, size, name, ctypes.byref(n), int(n.value), out.ctypes.data)
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
    L = load()
    ptr, size, name, _keep = buffer_of(path_or_bytes, image=True)
    with opened(L.pb_bigwig_zoom_read, L.pb_bigwig_zoom_close, ptr, size, name, int(level)) as h:
        n = int(L.pb_bigwig_zoom_rows(h))
        cols = [np.zeros(n, np.uint32) for _ in range(4)] + [np.zeros(n, np.float32) for _ in range(4)]
        call(L.pb_bigwig_zoom_fill, h, *[a.ctypes.data for a in cols])
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


def _summary_values(start, end, n_bins, elements, kinds, as_dict, fill):
    """The kinds of ``float64[5, nq, n_bins]`` elements by the model's formulas (``value_of``), `fill` where valid is 0."""
    nq = len(start)
    out = np.empty((5, nq, int(n_bins)), np.float64)          # (only the columns asked for are filled, and returned)
    mask = sum(1 << SUMMARY_KINDS.index(k) for k in set(kinds))
    if nq:
        call(load().pb_bigwig_summary_values, nq, start.ctypes.data, end.ctypes.data, int(n_bins), elements.ctypes.data, float(fill), mask, out.ctypes.data)
    if as_dict:
        return {k: out[SUMMARY_KINDS.index(k)] for k in kinds}
    return out[SUMMARY_KINDS.index(kinds[0])]


def _summary_elements_host(path_or_bytes, queries, n_bins):
    L = load()
    names, start, end = _summary_queries(queries, n_bins)
    ptr, size, name, _keep = buffer_of(path_or_bytes, image=True)
    with opened(L.pb_bigwig_summary_open, L.pb_bigwig_summary_close, ptr, size, name) as h:
        index = {L.pb_bigwig_summary_chrom(h, i).decode("utf-8", "replace"): i for i in range(L.pb_bigwig_summary_nchrom(h))}
        contig = _summary_contigs(names, index, name.decode("utf-8", "replace"))
        out = np.empty((5, len(names), int(n_bins)), np.float64)       # (the call fills every element)
        if len(names):
            call(L.pb_bigwig_summary_query, h, len(names), contig.ctypes.data, start.ctypes.data, end.ctypes.data, int(n_bins), out.ctypes.data)
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


DEFLATE_MAX_INPUT = 24600     # pcdeflate::kMaxInput: one bedGraph section of 2 048 items


def _deflate(encode, inputs, capacity):
    n = len(inputs)
    image = b"".join(bytes(s) for s in inputs)
    lens = np.array([len(s) for s in inputs], np.int64)
    offs = (np.cumsum(lens) - lens).astype(np.int64)
    need = int(lens.sum()) + 11 * n
    capacity = need if capacity is None else int(capacity)
    buf = ctypes.create_string_buffer(image, len(image)) if image else ctypes.create_string_buffer(1)
    out = np.zeros(max(capacity, 1), np.uint8)
    out_off, out_len = np.zeros(max(n, 1), np.int64), np.zeros(max(n, 1), np.int64)
    encode(ctypes.cast(buf, ctypes.c_void_p), n, offs.ctypes.data, lens.ctypes.data, out.ctypes.data, capacity, out_off.ctypes.data, out_len.ctypes.data)
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


def deflate_zlib_host(inputs, capacity=None, codes="fixed"):
    """``pb_deflate_zlib_mode``: :func:`deflate_zlib` by the serial model encoder of ``csrc/deflate_host.h`` on the host --
    the bytes the kernel must give, and the encoder of :func:`write_bigwig`."""
    L, mode = load(), _codes_mode(codes)
    return _deflate(lambda *args: call(L.pb_deflate_zlib_mode, *(args + (mode,))), inputs, capacity)


def _huffman_counts(counts, limit):
    counts = np.ascontiguousarray(counts)
    if counts.ndim != 1 or (len(counts) and (counts.min() < 0 or int(counts.astype(object).sum()) >= 1 << 32)):
        raise ValueError("huffman_lengths: counts must be one row of numbers >= 0 that add up to less than 2^32")
    return counts.astype(np.uint32), np.zeros(max(len(counts), 1), np.uint8), int(limit)


def huffman_lengths_host(counts, limit):
    """``pb_huffman_lengths``: :func:`huffman_lengths` by ``pcdeflate::build_code`` of ``csrc/deflate_host.h`` on the host."""
    c, out, limit = _huffman_counts(counts, limit)
    call(load().pb_huffman_lengths, c.ctypes.data, len(c), limit, out.ctypes.data)
    return out[:len(c)].copy()


BIGWIG_WRITE_STATS = ("contigs", "items", "sections", "raw_bytes", "block_bytes", "stored_sections")
BIGWIG_ZOOM_STATS = ("reduction", "records", "blocks", "raw_bytes", "file_bytes")
ZOOM_MAX_LEVELS = 10


def _zoom_level_stats(n, levels):
    """One dict per zoom level of what ``pb_bigwig_write_zoom_stats`` / ``pc_track_bigwig_export_zoom_stats`` filled in."""
    return [stats_dict(BIGWIG_ZOOM_STATS, levels[5 * k:5 * k + 5]) for k in range(int(n))]


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
    L = load()
    with opened(L.pb_bigwig_write_open_zoom, L.pb_bigwig_write_close, int(items_per_slot), int(block_size), mode, zoom_mode) as h:
        lengths = host_array.lengths()
        for chrom in host_array.chroms():
            cells = np.ascontiguousarray(host_array._chroms[chrom][strand], np.float64)
            call(L.pb_bigwig_write_add, h, chrom.encode("utf-8"), int(lengths[chrom]), cells.ctypes.data, len(cells))
        call(L.pb_bigwig_write_finish, h)
        image = ctypes.string_at(L.pb_bigwig_write_image(h), int(L.pb_bigwig_write_size(h)))
        stats = np.zeros(6, np.int64)
        L.pb_bigwig_write_stats(h, stats.ctypes.data)
        types = np.zeros(3, np.int64)
        L.pb_bigwig_write_block_types(h, types.ctypes.data)
        nlevels, levels = ctypes.c_int64(0), np.zeros(5 * ZOOM_MAX_LEVELS, np.int64)
        L.pb_bigwig_write_zoom_stats(h, ctypes.byref(nlevels), ZOOM_MAX_LEVELS, levels.ctypes.data)
    sink, close = _binary_sink(path_or_file)
    try:
        sink.write(image)
    finally:
        if close:
            sink.close()
    out = stats_dict(BIGWIG_WRITE_STATS, stats)
    if block_types:
        out["fixed_sections"], out["dynamic_sections"] = int(types[1]), int(types[2])
    if zoom_stats:
        out["zoom"] = _zoom_level_stats(nlevels.value, levels)
    return out
