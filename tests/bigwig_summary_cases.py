"""What the tests of the binned bigWig summaries share (test_bigwig_summary_host.py on the CPU, test_gpu_bigwig_summary.py
on the GPU): the files of tests/golden/bigwig_summary_fixture.npz, rebuilt or read and checked against their recorded
CRC-32, their recorded queries grouped by ``n_bins`` (one batch takes one ``n_bins``), and ``restate``: rules 1 to 5 of
csrc/bigwig_summary_host.h written again with Python floats over the host readers' tables, walking Kent's LIST where the
library searches.  Nothing here calls the code under test."""
import functools
import io
import math
import os
import zlib

import numpy as np

import plastid_amd as pa
from tests import bigwig_zoom_cases as zc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KINDS = ("mean", "min", "max", "coverage", "std")
KENT_FILES = ("kent_one", "kent_mixed", "kent_two_per_block", "kent_stored", "py_mixed")


@functools.lru_cache(maxsize=None)
def fixture():
    return np.load(os.path.join(GOLDEN, "bigwig_summary_fixture.npz"))


@functools.lru_cache(maxsize=None)
def read_fixture():
    return np.load(os.path.join(GOLDEN, "bigwig_fixture.npz"))


def tags():
    return [str(t) for t in fixture()["files"]]


@functools.lru_cache(maxsize=None)
def image_of(tag):
    """The file behind `tag`, as the fixture's generator made it; its CRC-32 is the recorded one."""
    if tag in KENT_FILES or tag == "py_overlaps":
        image = read_fixture()["file_" + tag].tobytes()
    else:
        name, comp = tag.rsplit("_", 1)
        case = zc.cases()[name]
        fh = io.BytesIO()
        pa.write_bigwig(zc.host_array(case), fh, "+", compress=comp == "1", zoom=case.zoom)
        image = fh.getvalue()
    if tag != "py_overlaps":
        assert zlib.crc32(image) == int(fixture()["crc_" + tag]), tag
    return image


def batches(tag):
    """``[(n_bins, [(chrom, start, end)], float64[5, nq, n_bins] recorded values)]``: the recorded queries by n_bins."""
    fx = fixture()
    names = [str(x) for x in fx["names_" + tag]]
    q, off, v = fx["q_" + tag], fx["off_" + tag], fx["v_" + tag]
    out = []
    for nb in sorted(set(int(x) for x in q[:, 3])):
        at = np.flatnonzero(q[:, 3] == nb)
        rows = [(names[q[i, 0]] if q[i, 0] >= 0 else "chrNone", int(q[i, 1]), int(q[i, 2])) for i in at]
        out.append((nb, rows, np.stack([v[:, off[i]:off[i + 1]] for i in at], axis=1)))
    return out


def same(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


# ---------------------------------------------------------------------------------------------------------------------
# the restatement

def level_of(reductions, start, end, n_bins):
    want = ((end - start) // n_bins) // 2
    if want <= 1:
        return -1
    best = -1
    for k, r in enumerate(reductions):
        if r <= want and (best < 0 or r > reductions[best]):
            best = k
    return best


def _element(count, lo, hi, s, ss):
    if not count > 0:          # (the items' 0 / 0 reads as no data too)
        return None
    valid = int(math.ceil(count))
    norm = float(valid) / count
    return valid, lo, hi, s * norm, ss * norm


def _walk(recs, bs, be, contribution):
    """Kent's slice over a LIST of records ``(start, end, ...)``: skip while end <= bs, then walk while start < be."""
    i = 0
    while i < len(recs) and recs[i][1] <= bs:
        i += 1
    if i == len(recs):
        return None
    lo, hi = contribution(recs[i])[3:5]
    count = s = ss = 0.0
    while i < len(recs) and recs[i][0] < be:
        a, b = recs[i][0], recs[i][1]
        overlap = min(b, be) - max(a, bs)
        if overlap > 0:
            c, x, xx, mn, mx = contribution(recs[i], overlap)
            count, s, ss = count + c, s + x, ss + xx
            hi = mx if hi < mx else hi
            lo = mn if lo > mn else lo
        i += 1
    return _element(count, lo, hi, s, ss)


def _zoom_part(rec, overlap=0):
    a, b, valid, mn, mx, s, ss = rec
    f = float(overlap) / float(b - a)
    return valid * f, s * f, ss * f, mn, mx


def _item_part(rec, overlap=0):
    a, b, val = rec
    size = float(b - a)
    f = float(overlap) / size
    w = size * f
    return w, val * w, val * val * w, val, val


@functools.lru_cache(maxsize=None)
def _tables(tag):
    image = image_of(tag)
    t = pa.read_bigwig(image)
    zoom = [pa.read_bigwig_zoom(image, k) for k in range(len(pa.bigwig_zoom_info(image)))]
    return t, zoom, [int(z[0]) for z in pa.bigwig_zoom_info(image)]


def restate(tag, chrom, start, end, n_bins, fill=np.nan):
    """``float64[5, n_bins]``: mean, min, max, coverage, std of one query, by the rules.  (In these files a contig's
    chromId is its place in the chromosome list.)"""
    t, zoom, reductions = _tables(tag)
    out = np.full((5, n_bins), fill, np.float64)
    if chrom not in t.names:
        return out
    cid = t.names.index(chrom)
    level = level_of(reductions, start, end, n_bins)
    if level < 0:
        at = np.flatnonzero((t.chrom == cid) & (np.maximum(t.start, start) < np.minimum(t.stop, end)))
        recs = [(max(int(t.start[k]), start), min(int(t.stop[k]), end), float(np.float32(t.value[k]))) for k in at]
        part = _item_part
    else:
        z = zoom[level]
        zs, ze = z.start.astype(np.int64), z.end.astype(np.int64)
        at = np.flatnonzero((z.chrom_id == cid) & (np.maximum(zs, start) < np.minimum(ze, end)))
        recs = [(int(zs[k]), int(ze[k]), float(z.valid[k]), float(z.min[k]), float(z.max[k]), float(z.sum[k]), float(z.sumsq[k])) for k in at]
        part = _zoom_part
    lo = start
    for i in range(n_bins):
        hi = start + (end - start) * (i + 1) // n_bins
        el = _walk(recs, lo, hi + 1 if (level < 0 and hi == lo) else hi, part)
        lo = hi
        if el is None:
            continue
        valid, mn, mx, s, ss = el
        var = ss - s * s / valid
        if valid > 1:
            var = var / (valid - 1)
        with np.errstate(invalid="ignore"):
            out[:, i] = [s / valid, mn, mx, (float(n_bins) / float(end - start)) * valid, float(np.sqrt(np.float64(var)))]
    return out


def seeded_queries(tag, n, seed):
    """`n` queries ``(chrom, start, end, n_bins)`` over the file's contigs (and one name it lacks) at every scale."""
    rng = np.random.default_rng(seed)
    t, _, reductions = _tables(tag)
    out = []
    for _ in range(n):
        c = int(rng.integers(0, len(t.names) + 1))
        size = t.lengths[c] if c < len(t.names) else 1000
        nb = int(rng.choice([1, 2, 3, 4, 6, 11, 33]))
        scale = int(rng.choice([1, 2, 5] + [2 * r for r in reductions] + [3 * r for r in reductions]))
        span = int(rng.integers(1, max(2, min(scale * nb * 2, 3 * size)) + 1))
        start = int(rng.integers(0, size + 5))
        out.append((t.names[c] if c < len(t.names) else "chrNone", start, start + span, nb))
    return out
