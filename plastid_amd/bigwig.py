"""bigWig files on the GPU.

:class:`BigWigReader` / :class:`BigWigGenomeArray` are the reference's classes of those names
(plastid/readers/bigwig.pyx:109-412, genome_array.py:1114-1320) over bigWig files whose blocks are inflated and decoded
on the GPU (``csrc/bigwig_kernels.hip.h``) into a :class:`~plastid_amd.track.GenomeArray`; :func:`inflate_zlib`,
:func:`deflate_zlib` and :func:`huffman_lengths` run the zlib kernels the import and the export are built on by
themselves.  The host models of all of them are in :mod:`plastid_amd.bigwig_host`.
"""
import ctypes
import os
from collections import OrderedDict

import numpy as np

from . import _lib
from ._hostlib import stats_dict
from ._lib import check
from .bigwig_host import (SUMMARY_ELEMENTS, WARN_CHROM_NOT_FOUND, _codes_mode, _deflate, _huffman_counts, _summary_contigs, _summary_kinds,
                          _summary_queries, _summary_values, sum_ranges)
from .exceptions import DataWarning, warn
from .roitools import SegmentChain


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


def huffman_lengths(engine, counts, limit):
    """``pc_huffman_lengths``: the code lengths (uint8, 0 for an unused symbol) the encoder's dynamic mode gives `counts`
    (2 .. 286 symbols) under the length `limit` (1 .. 15, ``2 ** limit >= len(counts)``), computed by ``k_huffman_lengths``
    on `engine`: fewer than two used symbols are padded with the lowest-numbered unused ones, the code is complete, and
    length never grows with (count, symbol).  ``ValueError`` for what is out of range.  No reference counterpart."""
    c, out, limit = _huffman_counts(counts, limit)
    check(_lib.load().pc_huffman_lengths(engine._h, c.ctypes.data, len(c), limit, out.ctypes.data), "pc_huffman_lengths")
    return out[:len(c)].copy()


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
        from .track import GenomeArray      # (track.py re-exports this module's names)
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
        return stats_dict(keys, out)

    def import_timing(self):
        """Milliseconds of the import: upload, inflate + Adler-32, sections + items, sort + apply."""
        out = np.zeros(4, np.float64)
        check(self._ga._lib.pc_track_bigwig_timing(self._ga._h, out.ctypes.data))
        return stats_dict(("upload", "inflate_adler", "sections_items", "sort_apply"), out, float)

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
        out = stats_dict(("tables", "tables_loaded", "bytes_uploaded", "bytes_inflated"), head)
        out["per_table"] = OrderedDict(("items" if k == 0 else int(per[3 * k]), {"records": None if per[3 * k + 1] < 0 else int(per[3 * k + 1]), "queries": int(per[3 * k + 2])})
                                       for k in range(int(head[0])))
        return out

    def summary_timing(self):
        """Milliseconds of the last summary call on the engine's stream: upload, inflate + Adler-32, records + order check
        (all 0 when it loaded no table), the summarize kernels, the read-back."""
        out = np.zeros(5, np.float64)
        check(self._ga._lib.pc_bigwig_summary_timing(self._summary_handle(), out.ctypes.data))
        return stats_dict(("upload", "inflate_adler", "records_order_check", "kernel", "read_back"), out, float)

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
        from .track import GenomeArray
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
