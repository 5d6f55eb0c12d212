"""The chunk table of plastid_amd/csrc/dense_host.h -- a plan's output cut into aligned chunks of 1 024 elements, every
chunk described by the spans of the segments that meet it -- is plain C++: tests/dense_chunks_test.cpp builds the table
in the steps the engine does, compiled with the host compiler under the address and undefined-behaviour sanitizers, and
prints what a workgroup finds through the descriptors.  That is compared element by element with a numpy model of what
the segments write.  No GPU needed."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROW = 128
INLINE = 7


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    tmp = tmp_path_factory.mktemp("dense_chunks")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp / "dense_chunks_test")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(root, "plastid_amd", "csrc"), os.path.join(root, "tests", "dense_chunks_test.cpp"), "-o", out])
    return out


@pytest.fixture(scope="module")
def chunk(exe):
    return int(subprocess.run([exe, "chunk"], stdout=subprocess.PIPE, timeout=300, check=True).stdout)


def run(exe, tmp_path, out_elems, segs):
    path = tmp_path / "plan.txt"
    path.write_text("%d\n" % out_elems + "".join("%d %d %d %d %d %d %d %d %d\n" % tuple(s) for s in segs))
    res = subprocess.run([exe, "table", str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert res.returncode == 0, res.stderr.decode()
    return res.stdout.decode().splitlines()


def lay_out(pieces, rng, tail=0):
    """Segments (out_off step len clip_lo clip_hi start known cell_base ext) for `pieces`, laid left to right:
    ("seg", len) or ("gap", len).  Directions, clips, extents and unknown contigs vary; the order is permuted."""
    segs, at = [], 0
    for what, n in pieces:
        if what == "seg":
            step = 1 if rng.integers(2) else -1
            kind = rng.integers(6)
            start = int(rng.integers(0, 50000))
            clip_lo, clip_hi, known, ext = 0, n, 1, 1 << 20
            if kind == 0 and n > 2:
                clip_lo, clip_hi = int(rng.integers(0, n // 2)), int(rng.integers(n // 2, n + 1))
            elif kind == 1:
                ext = start + int(rng.integers(0, n + 1))       # the contig ends inside the segment
            elif kind == 2:
                known = 0
            elif kind == 3 and n > 1:
                start = -int(rng.integers(1, n))                # starts left of the contig: the clip says so
                clip_lo = -start
            cell_base = int(rng.integers(0, 1 << 20)) * 2
            segs.append((at if step > 0 else at + n - 1, step, n, clip_lo, clip_hi, start, known, cell_base, ext))
        at += n
    order = rng.permutation(len(segs))
    return at + tail, [segs[i] for i in order]


def model(out_elems, segs):
    """cell[e]: the cell element e reads, -1: zero; writers[e]: segments that write e"""
    cell = np.full(out_elems, -1, np.int64)
    writers = np.zeros(out_elems, np.int32)
    for out_off, step, n, clip_lo, clip_hi, start, known, cell_base, ext in segs:
        i = np.arange(n, dtype=np.int64)
        e = out_off + step * i
        writers[e] += 1
        ok = (i >= clip_lo) & (i < clip_hi) & (start + i >= 0) & (start + i < ext) & bool(known)
        cell[e[ok]] = cell_base + start + i[ok]
    return cell, writers


def check(exe, tmp_path, chunk, out_elems, segs):
    cell, writers = model(out_elems, segs)
    assert writers.max() <= 1
    lines = run(exe, tmp_path, out_elems, segs)
    assert lines and lines[0] != "overlap"
    got = np.full(out_elems, -1, np.int64)
    seen = np.zeros(out_elems, np.int32)
    chunks, rows, pairs = {}, {}, {}
    for line in lines:
        f = line.split()
        if f[0] == "elem":
            got[int(f[1])] = int(f[2]); seen[int(f[1])] += 1
        elif f[0] == "pair":
            pairs[int(f[1])] = int(f[2])
        elif f[0] == "chunk":
            chunks[int(f[1])] = (int(f[2]), int(f[3]))
        else:
            rows[(int(f[1]), int(f[2]))] = int(f[3])
    assert seen.max() <= 1                                  # an element reads through one span at most
    assert np.array_equal(got, cell % (1 << 32) * (cell >= 0) - (cell < 0))
    # two cells come by one 4-byte load where they are the halves of one word at an even cell index
    both = [e for e in range(0, out_elems - 1, 2) if cell[e] >= 0 and cell[e + 1] >= 0]
    assert sorted(pairs) == both
    assert all(pairs[e] == int(cell[e] // 2 == cell[e + 1] // 2) for e in both)
    nchunks = -(-out_elems // chunk)
    assert sorted(chunks) == list(range(nchunks))
    # spans of a chunk: the segments that meet it; rows: the segments some element of the row reads through
    lo = np.array([s[0] if s[1] > 0 else s[0] - s[2] + 1 for s in segs], np.int64)
    hi = lo + np.array([s[2] for s in segs], np.int64)
    owner = np.full(out_elems, -1, np.int64)
    for k in range(len(segs)):
        owner[lo[k]:hi[k]] = k
    for c in range(nchunks):
        meets = int(((lo < (c + 1) * chunk) & (hi > c * chunk) & (hi > lo)).sum())
        assert chunks[c] == (meets, max(0, meets - INLINE)), c
        for r in range(-(-min(chunk, out_elems - c * chunk) // ROW)):
            a = c * chunk + r * ROW
            sl = slice(a, min(a + ROW, out_elems))
            assert rows[(c, r)] == len(set(owner[sl][cell[sl] >= 0])), (c, r)
    return chunks, rows


def test_layouts_against_numpy_model(exe, chunk, tmp_path):
    rng = np.random.default_rng(20240611)
    K = chunk
    fixed = [
        # segments ending exactly on row and chunk boundaries, one across three chunks, gaps of one and of more than a chunk
        [("seg", ROW), ("seg", K - ROW), ("seg", 2 * K + 77), ("gap", 1), ("seg", K - 78), ("gap", K + 300), ("seg", 3), ("gap", 1), ("seg", 1), ("seg", 2)],
        # more than 7 spans in a chunk, then a chunk that is all gap, then a short tail
        [("seg", int(n)) for n in rng.integers(30, 61, 40)] + [("gap", 3 * K)] + [("seg", 5)],
        [("seg", 1)], [("seg", 2)], [("gap", 5), ("seg", 1)],
    ]
    for pieces in fixed:
        for tail in (0, 1, 130):
            out_elems, segs = lay_out(pieces, rng, tail)
            check(exe, tmp_path, K, out_elems, segs)
    chunks, _ = check(exe, tmp_path, K, *lay_out(fixed[1], rng))
    assert max(n for n, _ in chunks.values()) > INLINE and min(n for n, _ in chunks.values()) == 0
    for _ in range(12):     # random: tiny to long segments, some gaps
        pieces = []
        for _ in range(int(rng.integers(1, 60))):
            n = int(rng.choice([1, 2, 3, int(rng.integers(4, 200)), int(rng.integers(200, 3 * K))]))
            pieces.append(("seg", n))
            if rng.integers(4) == 0:
                pieces.append(("gap", int(rng.choice([1, 1, int(rng.integers(2, 2 * K))]))))
        out_elems, segs = lay_out(pieces, rng, int(rng.integers(0, 3)))
        assert out_elems > 0
        check(exe, tmp_path, K, out_elems, segs)
    out_elems, segs = lay_out([("seg", 1001), ("gap", 2), ("seg", K)], rng)      # odd, no multiple of a row
    assert out_elems % 2 == 1 and out_elems % ROW
    check(exe, tmp_path, K, out_elems, segs)


@pytest.mark.parametrize("second", [(100, 1, 50), (149, 1, 20), (110, 1, 10), (168, -1, 20), (90, 1, 11)])
def test_overlap_is_detected(exe, chunk, tmp_path, second):
    """the first segment writes [100, 150): an equal range, one shared element at either end (one of them laid out
    downwards), and a range inside it"""
    first = (100, 1, 50, 0, 50, 0, 1, 0, 1 << 20)
    out_off, step, n = second
    seg = (out_off, step, n, 0, n, 7, 1, 0, 1 << 20)
    for segs in ([first, seg], [seg, first], [(0, 1, 40, 0, 40, 0, 1, 0, 1 << 20), seg, (300, 1, 9, 0, 9, 0, 1, 0, 1 << 20), first]):
        _, writers = model(4 * chunk, segs)
        assert writers.max() == 2
        assert run(exe, tmp_path, 4 * chunk, segs) == ["overlap"]


def test_touching_ranges_do_not_overlap(exe, chunk, tmp_path):
    segs = [(150, 1, 10, 0, 10, 0, 1, 0, 1 << 20), (100, 1, 50, 0, 50, 0, 1, 0, 1 << 20), (99, -1, 100, 0, 100, 0, 1, 0, 1 << 20), (500, 1, 0, 0, 0, 0, 1, 0, 1 << 20)]
    check(exe, tmp_path, chunk, 160, segs)
