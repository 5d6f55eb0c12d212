#!/usr/bin/env python
"""Generate ``tests/golden/bigwig_summary_fixture.npz``: what ``bigWigSummaryArray`` of Kent's bigWig library -- the one
the reference links -- returns for seeded queries whose bins CUT records, over files with Kent's own zoom levels and with
ours.

    python tests/golden/make_bigwig_summary_golden.py

needs the reference checkout (``KENT_SRC``); it reuses ``build_zoom_harness`` of ``make_bigwig_zoom_golden.py`` (the
harness ``bw_zoom_golden.c`` into ``oracle/_ref/bw_zoom_golden``).  Only DATA is committed.

The files (``files``: their tags): the four Kent-written files of ``bigwig_fixture.npz`` and ``py_mixed`` (no levels), and
``write_bigwig(zoom=...)`` of the integer cases of tests/bigwig_zoom_cases.py, compressed (``<case>_1``) and stored
(``<case>_0``).  Per tag: ``crc_<tag>`` the CRC-32 of the file; ``names_<tag>`` / ``sizes_<tag>`` its contigs;
``reductions_<tag>`` its levels as the harness reported them; ``q_<tag>`` int64[nq, 4]: contig (an index into the names,
-1: a name the file lacks, asked as ``chrNone``), start, end, n_bins; ``off_<tag>`` int64[nq + 1]: where a query's bins
stand in ``v_<tag>`` float64[5, total bins]: mean, min, max, coverage, std with NaN as the fill.

Per file the queries reach every level the file has (asserted by RESTATING the choice of a level, not by calling the code
under test) and the items, and include n_bins = 1, n_bins > end - start, a query inside one item, one that runs past the
contig's size, one over a stretch without data and one on a contig without data."""
import io
import os
import subprocess
import sys
import tempfile
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, HERE]
import make_bigwig_zoom_golden as mz  # noqa: E402

KINDS = mz.KINDS
KENT_FILES = ("kent_one", "kent_mixed", "kent_two_per_block", "kent_stored", "py_mixed")
BINS = (1, 2, 3, 5, 7, 70)


def level_of(reductions, start, end, n_bins):
    """Rule 1 restated: -1 the items, else the place of the level."""
    want = ((end - start) // n_bins) // 2
    if want <= 1:
        return -1
    fit = [(r, -k) for k, r in enumerate(reductions) if r <= want]
    return -max(fit)[1] if fit else -1


def files():
    """``[(tag, image)]``."""
    import plastid_amd as pa
    from tests import bigwig_zoom_cases as zc
    fx = np.load(os.path.join(HERE, "bigwig_fixture.npz"))
    out = [(k, fx["file_" + k].tobytes()) for k in KENT_FILES]
    cases = zc.cases()
    for name in zc.integer_cases():
        for comp in (True, False):
            fh = io.BytesIO()
            pa.write_bigwig(zc.host_array(cases[name]), fh, "+", compress=comp, zoom=cases[name].zoom)
            out.append(("%s_%d" % (name, 1 if comp else 0), fh.getvalue()))
    return out


def queries(tag, image):
    """``(names, sizes, reductions, int64[nq, 4])`` of one file: the list the module's docstring promises."""
    import plastid_amd as pa
    rng = np.random.default_rng(zlib.crc32(tag.encode()))
    t = pa.read_bigwig(image)
    names, sizes = list(t.names), [int(x) for x in t.lengths]
    reductions = [int(z[0]) for z in pa.bigwig_zoom_info(image)]
    with_data = sorted(set(int(c) for c in t.chrom))
    big = max(with_data, key=lambda c: sizes[c])
    q = []
    # every level: the span that selects it, from an odd start, once in one bin and once in several
    for k, r in enumerate(reductions):
        above = min([x for x in reductions if x > r] or [4 * r])
        for nb in (1, int(rng.choice(BINS[1:5]))):
            lo, hi = 2 * r * nb, min(2 * above * nb - 1, 2 ** 31 - 2)
            span = int(rng.integers(lo, min(hi, lo + r * nb) + 1))
            start = int(rng.integers(0, max(1, min(sizes[big] // 3, r)))) | 1
            start = min(start, 2 ** 31 - 1 - span)
            q.append((big, start, start + span, nb))
            assert level_of(reductions, start, start + span, nb) == k, (tag, k, q[-1])
    # the items: a single bin, more bins than positions, bins of a few positions, 70 bins
    s0 = int(rng.integers(0, max(1, sizes[big] - 40)))
    q += [(big, s0, s0 + 3, 1), (big, s0 + 1, s0 + 6, 12), (big, s0, s0 + 37, 5), (big, max(0, sizes[big] // 2 - 100), max(0, sizes[big] // 2 - 100) + 141, 70)]
    # inside one item: the longest of the big contig
    at = np.flatnonzero(t.chrom == big)
    k = at[np.argmax(t.stop[at] - t.start[at])]
    a, b = int(t.start[k]), int(t.stop[k])
    q += [(big, a + (1 if b - a > 2 else 0), b - (1 if b - a > 2 else 0), 1), (big, a, b, 2)]
    # past the contig's size: from the items and from every level's scale
    q += [(big, max(0, sizes[big] - 5), sizes[big] + 7, 4), (big, max(0, sizes[big] - 9), sizes[big] + 40, 1)]
    # a stretch without data: the longest uncovered run of the big contig, else beyond its size
    free = np.ones(sizes[big], np.int8)
    for i in at:
        free[int(t.start[i]):int(t.stop[i])] = 0
    step = np.diff(np.concatenate([[0], free, [0]]))
    gaps = list(zip(np.flatnonzero(step == 1).tolist(), np.flatnonzero(step == -1).tolist()))
    if gaps:
        a, b = max(gaps, key=lambda g: g[1] - g[0])
        q += [(big, a, b, 1), (big, a, b, 3)]
    else:
        q += [(big, sizes[big] + 10, sizes[big] + 50, 1), (big, sizes[big] + 10, sizes[big] + 50, 3)]
    # a contig without data: one of the file's, else a name it lacks
    empty = [c for c in range(len(names)) if c not in with_data]
    q += [(empty[0] if empty else -1, 0, 30, 3), (empty[0] if empty else -1, 1, 2 * (reductions[0] if reductions else 8) * 5 + 2, 1)]
    # seeded queries over every contig with data and every scale
    for _ in range(14):
        c = int(rng.choice(with_data))
        nb = int(rng.choice(BINS))
        scale = int(rng.choice([1, 2, 3] + [2 * r for r in reductions]))
        span = int(rng.integers(1, max(2, min(scale * nb * 3, 2 * sizes[c])) + 1))
        start = int(rng.integers(0, sizes[c]))
        q.append((c, start, start + span, nb))
    q = np.array(q, np.int64)
    reached = set(level_of(reductions, int(s), int(e), int(nb)) for c, s, e, nb in q if c >= 0)
    assert reached == set(range(-1, len(reductions))), (tag, reached, reductions)
    assert (q[:, 3] == 1).any() and (q[:, 3] > q[:, 2] - q[:, 1]).any() and (q[:, 1] < q[:, 2]).all() and (q[:, 2] < 2 ** 31).all()
    return names, sizes, reductions, q


def main():
    exe, _ = mz.build_zoom_harness()
    tmp = tempfile.mkdtemp(prefix="bws_golden_")
    out = dict(kent=np.array("kent/src/lib as vendored by the reference"))
    tags, total = [], 0
    for tag, image in files():
        path = os.path.join(tmp, tag + ".bw")
        with open(path, "wb") as fh:
            fh.write(image)
        names, sizes, reductions, q = queries(tag, image)
        values, off = [], [0]
        for c, start, end, nb in q:
            levels, got = mz.summaries(exe, path, names[c] if c >= 0 else "chrNone", int(start), int(end), int(nb))
            assert levels == reductions, (tag, levels, reductions)
            values.append(np.stack([got[k] for k in KINDS]))
            off.append(off[-1] + int(nb))
        tags.append(tag)
        out["crc_" + tag] = np.array(zlib.crc32(image), np.int64)
        out["names_" + tag], out["sizes_" + tag] = np.array(names), np.array(sizes, np.int64)
        out["reductions_" + tag] = np.array(reductions, np.int64)
        out["q_" + tag], out["off_" + tag] = q, np.array(off, np.int64)
        out["v_" + tag] = np.concatenate(values, axis=1)
        total += len(q)
    out["files"] = np.array(tags)
    dst = os.path.join(HERE, "bigwig_summary_fixture.npz")
    np.savez_compressed(dst, **out)
    print("%s: %d files, %d queries, %d bytes" % (dst, len(tags), total, os.path.getsize(dst)))
    assert os.path.getsize(dst) <= 512 * 1024


if __name__ == "__main__":
    main()
