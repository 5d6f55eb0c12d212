"""plastid_amd/csrc/dense_host.h -- the host arithmetic of the dense vector (extents and cell offsets, the eligibility
decision, the cutting of a plan's segments into gather items) -- is plain C++: tests/dense_host_test.cpp is compiled
with the host compiler under the address and undefined-behaviour sanitizers and run here.  Its `check` mode holds the
hand-worked extents, offsets and decisions; its `items` mode cuts the segments this file writes, and every position of
every item is compared with a numpy model of what a segment position reads and writes.  No GPU needed."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ITEM = 2048


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    tmp = tmp_path_factory.mktemp("dense_host")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp / "dense_host_test")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(root, "plastid_amd", "csrc"), os.path.join(root, "tests", "dense_host_test.cpp"), "-o", out])
    return out


def test_extents_offsets_and_eligibility(exe):
    out = subprocess.run([exe, "check"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert out.returncode == 0, out.stdout.decode()
    assert b"dense_host: ok" in out.stdout


def model(seg):
    """Per position i of the segment: the output element it writes and the cell it reads (-1: zero)."""
    out_off, length, clip_lo, clip_hi, start, step, known, cell_base, ext = seg
    i = np.arange(length, dtype=np.int64)
    g = start + i
    readable = (i >= clip_lo) & (i < clip_hi) & (g >= 0) & (g < ext) & bool(known)
    return out_off + step * i, np.where(readable, cell_base + g, -1)


def segments():
    """(out_off, len, clip_lo, clip_hi, start, step, known, cell_base, ext) -- clip_lo / clip_hi as the plan builder
    leaves them: the segment cut at position 0 of the contig's axis, 0 / 0 for an unknown contig."""
    segs = []
    ext, base = 10000, 777
    out = 0

    def add(start, length, step, known=1, ext=ext, base=base):
        nonlocal out
        lo = min(max(-start, 0), length) if known else 0
        hi = length if known else 0
        if hi <= lo:
            lo = hi = 0
        off = out if step == 1 else out + length - 1
        segs.append((off, length, lo, hi, start, step, known, base, ext))
        out += length

    for length in (1, 2047, 2048, 2049, 4097):
        for step in (1, -1):
            add(100, length, step)
    add(-50, 300, 1)            # starts below 0
    add(-50, 300, -1)
    add(-3000, 2500, 1)         # wholly below 0: all zero
    add(-3000, 5000, -1)        # the first item all zero, the second partly, the third not
    add(9000, 3000, 1)          # clipped at the contig's end (extent 10 000)
    add(9000, 3000, -1)
    add(9999, 1, 1)
    add(10000, 5, 1)            # starts at the end: all zero
    add(20000, 2049, -1)        # beyond the end
    add(500, 2100, 1, known=0)  # unknown contig
    add(500, 2100, -1, known=0)
    add(0, 0, 1)                # empty segment: no item
    add(0, 1, 1, ext=1, base=0)     # a contig of one position
    add(0, 5, 1, ext=0, base=12)    # a contig without cells
    add(-1, 4100, -1, ext=4099, base=5)
    return segs


def test_item_cutting_against_numpy_model(exe, tmp_path):
    segs = segments()
    path = tmp_path / "segs.txt"
    path.write_text("".join(" ".join(str(int(v)) for v in s) + "\n" for s in segs))
    res = subprocess.run([exe, "items", str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert res.returncode == 0, res.stderr.decode()
    rows = np.array([[int(v) for v in line.split()] for line in res.stdout.decode().splitlines()], dtype=np.int64).reshape(-1, 8)
    for s, seg in enumerate(segs):
        want_out, want_cell = model(seg)
        mine = rows[rows[:, 0] == s]
        length = seg[1]
        assert len(mine) == (length + ITEM - 1) // ITEM, (s, seg)
        assert list(mine[:, 1]) == list(range(len(mine)))
        got_out = np.empty(length, np.int64)
        got_cell = np.empty(length, np.int64)
        at = 0
        for _, k, out_off, cell0, n, step, lo, hi in mine:
            assert 1 <= n <= ITEM and (n == ITEM or k == len(mine) - 1), (s, k, n)
            assert step == seg[5] and 0 <= lo <= hi <= n, (s, k, lo, hi, n)
            i = np.arange(n, dtype=np.int64)
            got_out[at:at + n] = out_off + step * i
            got_cell[at:at + n] = np.where((i >= lo) & (i < hi), cell0 + i, -1)
            if hi > lo:   # what the kernel reads stays inside the strand's cells
                assert seg[7] <= cell0 + lo and cell0 + hi <= seg[7] + seg[8], (s, k)
            at += n
        assert at == length
        assert np.array_equal(got_out, want_out), (s, seg)
        assert np.array_equal(got_cell, want_cell), (s, seg)
