"""Numpy models of the two derived streams of a staged file (helper, not collected by pytest): the COMPACT stream
(duplicate reads as one entry, ``Engine.stream_entries``) and the CANONICAL stream (one entry per contig, strand and mapped
position under a point rule, ``Engine.canonical_entries``).  Everything here is restated from the code -- the grouping of
``k_compact_tiles`` / ``k_canon_buckets`` (csrc/stage_kernels.hip.h), ``canon_rule`` / ``canon_fits_halo``
(csrc/canon_host.h, pinned to hand-worked values by tests/canon_host_test.cpp), ``choose_halo`` (csrc/host_util.h), the
eligibility line and the weigh-in of ``canonical_for_plan`` (csrc/plastid_counts.hip) -- and nothing is read from an
engine.  tests/test_gpu_canonical_stream.py, tests/test_gpu_compact_stream.py and tests/stateful_cases.py share it."""
import numpy as np

TILE, CAP = 2048, 16        # records per compaction tile; reads per entry
TILE_SPAN = 0x7ffe          # a tile that spans more positions (or two contigs) stays as it is: one entry per record
EXCLUDED = 0x80
STREAM_MAX_LEN = 255        # aligned lengths a 4-byte stream word carries
MAX_SHIFT = 254
KEEP = 0.9                  # PC_COMPACT_KEEP when the knob is not set
#: a world in which the halo is certain (``certain_halo``): every single-run read at most this long ...
CERTAIN_MAX_LEN = 44
#: ... and no span beyond the smallest halo staging ever chooses
MIN_HALO = 64


# ---------------------------------------------------------------------------------------------------- the canonical stream
def rule_index(mapping, L, rev):
    """k(L, strand) of a point rule for arrays of lengths and strands; -1: not mapped."""
    L = L.astype(np.int64)
    if mapping[0] in ("fiveprime", "threeprime"):
        p = mapping[1]
        near_left = (rev == 0) if mapping[0] == "fiveprime" else (rev != 0)
        return np.where(p >= L, -1, np.where(near_left, p, L - 1 - p))
    from plastid_amd import synth
    fac = synth.mapping_factory(mapping)
    fw, rc = np.asarray(fac.forward_offsets, np.int64), np.asarray(fac.reverse_offsets, np.int64)
    return np.where(rev != 0, rc[L], fw[L])


def model_entries(f, flags, mapping, size_filter=None):
    """Entries the grouping implies: the single-run reads that are not excluded and that the rule and the filter keep,
    by (contig, strand, mapped position), one entry per 16 reads of a group."""
    L, rev = f.alen.astype(np.int64), (flags & 1).astype(np.int64)
    k = rule_index(mapping, L, rev)
    keep = (f.nblk == 1) & ((flags & EXCLUDED) == 0) & (k >= 0)
    if size_filter:
        keep &= (L >= size_filter[0]) & ((L <= size_filter[1]) | (size_filter[1] == -1))
    key = (f.tid.astype(np.int64) << 40) | (rev << 39) | (f.pos.astype(np.int64) + k)
    _, cnt = np.unique(key[keep], return_counts=True)
    return int(((cnt + CAP - 1) // CAP).sum())


# ---------------------------------------------------------------------------------------------------- the compact stream
def entries_of_sorted_tiles(f, excluded=None):
    """Entries the format implies for a file whose tiles are all sorted: per tile, ceil(copies / 16) per distinct key."""
    keep = np.ones(f.n, bool) if excluded is None else ~excluded
    total = 0
    for t0 in range(0, f.n, TILE):
        sl = slice(t0, min(t0 + TILE, f.n))
        k = keep[sl]
        key = np.stack([f.pos[sl][k].astype(np.int64), f.alen[sl][k].astype(np.int64), (f.flags[sl][k] & 1).astype(np.int64)], 1)
        if len(key):
            _, cnt = np.unique(key, axis=0, return_counts=True)
            total += int(((cnt + CAP - 1) // CAP).sum())
    return total


def spans_of(f):
    """Reference span of every record as staging measures it (k_cols_pack): the end of the last run minus the start; a
    record without aligned positions spans one."""
    L = f.alen.astype(np.int64)
    span = np.maximum(L, 1)
    multi = np.nonzero(f.nblk >= 2)[0]
    if len(multi):
        off = f.block_offsets()
        last = off[multi] + f.nblk[multi].astype(np.int64) - 1
        span[multi] = f.blk_start[last].astype(np.int64) + f.blk_len[last].astype(np.int64) - f.pos[multi].astype(np.int64)
    return span


def certain_halo(f):
    """True when the halo of `f` needs no quantile: no span beyond MIN_HALO (so wcap = 64 and no record leaves the
    streams for the long-read lists) and every single-run read at most CERTAIN_MAX_LEN long."""
    if f.n == 0:
        return True
    single = f.nblk < 2
    return bool(spans_of(f).max() <= MIN_HALO and (not single.any() or f.alen[single].max() <= CERTAIN_MAX_LEN)
                and f.alen.max() <= STREAM_MAX_LEN)


def compact_entries(f, excluded):
    """Entries of the compact stream of `f` under the exclusion bits `excluded`, tiles that stay as they are included
    (k_compact_tiles): a sorted tile drops the words with the skip bit -- excluded records, multi-run reads -- and merges
    equal (position, length, strand); a tile over two contigs or more than TILE_SPAN positions keeps one entry per record.
    Valid for a file with a certain halo (no record on the long-read lists)."""
    total = 0
    rev = (f.flags & 1).astype(np.int64)
    for t0 in range(0, f.n, TILE):
        t1 = min(t0 + TILE, f.n)
        pos = f.pos[t0:t1].astype(np.int64)
        if f.tid[t0] != f.tid[t1 - 1] or pos[-1] - pos[0] > TILE_SPAN:
            total += t1 - t0
            continue
        k = ~excluded[t0:t1] & (f.nblk[t0:t1] < 2)
        if k.any():
            key = (pos[k] << 20) | (f.alen[t0:t1][k].astype(np.int64) << 1) | rev[t0:t1][k]
            _, cnt = np.unique(key, return_counts=True)
            total += int(((cnt + CAP - 1) // CAP).sum())
    return int(total)


def compact_prediction(f, excluded, no_compact=False, keep=KEEP):
    """Entry count of the compact stream the file keeps, or None when it keeps none (build_compact_stream): no records,
    PC_NO_COMPACT, or more than `keep` of the records left as entries.  `no_compact` / `keep`: the knobs at the time the
    stream was last built."""
    if f.n <= 0 or no_compact:
        return None
    total = compact_entries(f, excluded)
    return None if total > keep * f.n else total


def offset_tables(mapping):
    """(fw, rc) of a variable rule as the engine is handed them (map_factories.build_offset_tables)."""
    import warnings
    from plastid_amd.map_factories import build_offset_tables
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        fw, rc = build_offset_tables(dict(mapping[1]))
    return np.asarray(fw, np.int64), np.asarray(rc, np.int64)


def _scalar_index(mapping, tables, L, rev):
    """canon_host.h rule_index"""
    if mapping[0] == "fiveprime":
        p = mapping[1]
        return -1 if p >= L else (L - 1 - p if rev else p)
    if mapping[0] == "threeprime":
        p = mapping[1]
        return -1 if p >= L else (p if rev else L - 1 - p)
    fw, rc = tables
    if L >= len(fw):
        return -1
    return int(rc[L] if rev else fw[L])


def canon_rule(mapping, size_filter, fast_lo, fast_hi):
    """canon_host.h canon_rule: ``(usable, kc)`` -- per strand the smallest index of a valid length of the entry-table
    range, -1: none; usable: some length is valid and every shift fits."""
    tables = offset_tables(mapping) if mapping[0] == "variable" else None
    lo, hi = max(fast_lo, 0), min(fast_hi, STREAM_MAX_LEN)

    def valid_index(L, s):
        k = _scalar_index(mapping, tables, L, s)
        ok = size_filter is None or (L >= size_filter[0] and (L <= size_filter[1] or size_filter[1] == -1))
        return k if k >= 0 and ok else -1
    kc, fits = [-1, -1], True
    for s in (0, 1):
        ks = [k for k in (valid_index(L, s) for L in range(lo, hi + 1)) if k >= 0]
        if ks:
            kc[s] = min(ks)
            fits = fits and max(ks) - kc[s] <= MAX_SHIFT
    return fits and (kc[0] >= 0 or kc[1] >= 0), kc


def stream_ranges(f):
    """``(fast_lo, fast_hi, Ws)`` of ONE staged file with a certain halo (choose_halo, hist_lds_shape, Engine::Ws): the
    aligned lengths of the single-run records -- whatever their exclusion bits, records without aligned positions
    included -- give Ws (the longest) and, with those of the multi-run reads, the range of the entry table."""
    single, multi = f.alen[f.nblk < 2].astype(np.int64), f.alen[f.nblk >= 2].astype(np.int64)
    smin, smax = (int(single.min()), int(single.max())) if len(single) else (65536, -1)
    rmin, rmax = (int(multi.min()), int(multi.max())) if len(multi) else (65536, -1)
    tmin, tmax = min(smin, rmin), max(smax, rmax)
    slen_max = smax if smax >= smin else 0
    tlen_min, tlen_max = (tmin, tmax) if tmax >= tmin else (0, 0)
    fast_hi = tlen_max
    fast_lo = min(min(STREAM_MAX_LEN, tlen_min), fast_hi)
    return fast_lo, fast_hi, slen_max


def canonical_signature(f, mapping, size_filter, words_gen):
    """What the engine keys the canonical stream of `f` by (CanonSig): rule, size filter, offset tables, fast_lo / fast_hi,
    Ws and the generation of the stream words -- as plain, comparable values."""
    rule = (mapping[0], mapping[1]) if mapping[0] != "variable" else ("variable",) + tuple(t.tobytes() for t in offset_tables(mapping))
    return (rule, None if size_filter is None else tuple(size_filter)) + stream_ranges(f) + (words_gen,)


def plan_modes_eligible(strand, tid, start, end, lens):
    """The `p->modes` test of canonical_for_plan from a segment set: True -- '+' / '-' windows only and at least one;
    False -- some window of another code, or none at all; None -- not certain (a segment of another code that may or may
    not make a window)."""
    strand = np.asarray(strand)
    ntid = len(lens)
    known = (tid >= 0) & (tid < ntid)
    clen = np.array([lens[t] if 0 <= t < ntid else 0 for t in tid], np.int64)
    windowed = known & (end > start) & (start < clen) & (end > 0)
    pm = (strand == 1) | (strand == 2)
    if (windowed & ~pm).any():
        return False
    if (~pm & ~windowed).any():
        return None
    return bool((windowed & pm).any())


def canonical_prediction(nfiles, mapping, size_filter, rows, modes_eligible, f, flags, no_canon=False, compact=None, keep=KEEP):
    """What ``canonical_for_plan`` decides for a plan in this state: ``("none", why)`` -- the plan cannot use the stream;
    ``("built", n)`` -- the stream must exist with `n` entries; ``("unknown",)`` -- the verdict hangs on the halo of a file
    that ``certain_halo`` does not cover, or on segments that may make no window.

    `f`, `flags`: the ONE staged file and its current flag bytes (strand, EXCLUDED: the caller's bits and the filters'
    verdicts); `modes_eligible`: ``plan_modes_eligible``; `compact`: the entry count of the compact stream the file keeps,
    None: it keeps none (``compact_prediction`` with the knobs of its last build); `keep`: PC_COMPACT_KEEP now."""
    if no_canon:
        return ("none", "PC_NO_CANON")
    if nfiles != 1:
        return ("none", "files")
    if mapping[0] not in ("fiveprime", "threeprime", "variable"):
        return ("none", "rule")
    if rows != 1:
        return ("none", "rows")
    if modes_eligible is False:
        return ("none", "modes")
    if f.n <= 0:
        return ("none", "no records")
    if modes_eligible is None or not certain_halo(f):
        return ("unknown",)
    fast_lo, fast_hi, Ws = stream_ranges(f)
    usable, kc = canon_rule(mapping, size_filter, fast_lo, fast_hi)
    if not usable:
        return ("none", "no valid length")
    if not all(k < 0 or k < Ws for k in kc):
        return ("none", "halo")
    total = model_entries(f, flags, mapping, size_filter)
    replaces = compact if compact is not None else f.n
    if total > keep * replaces:
        return ("none", "weigh-in")
    return ("built", total)
