"""The pair and batch arithmetic of plastid_amd/csrc/dense_host.h -- how k_dense_gather lays an item out as 16-byte
aligned pairs of output elements with a head and a tail of one element, and how a plan's item list is cut into the
batches a workgroup serves -- is plain C++: tests/dense_batches_test.cpp is compiled with the host compiler under the
address and undefined-behaviour sanitizers and run here.  Every store it prints is compared position by position with a
numpy model of what an item writes.  No GPU needed."""
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
    tmp = tmp_path_factory.mktemp("dense_batches")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp / "dense_batches_test")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(root, "plastid_amd", "csrc"), os.path.join(root, "tests", "dense_batches_test.cpp"), "-o", out])
    return out


def items():
    """(out_off, step, len): every length at which the pairing changes shape, on both parities of the first output
    element and in both directions; large offsets; an item at element 0 going down is impossible (len 1 only)."""
    its = []
    for length in (1, 2, 3, 4, 255, 256, 257, 511, 512, 513, 2046, 2047, 2048):
        for base in (0, 1, 7, 4096, 123457, (1 << 33) + 5, (1 << 33) + 8):
            its.append((base, 1, length))
            its.append((base + length - 1, -1, length))   # laid out downwards from its last element
    its.append((0, -1, 1))
    return its


def test_pairs_against_numpy_model(exe, tmp_path):
    its = items()
    path = tmp_path / "items.txt"
    path.write_text("".join("%d %d %d\n" % it for it in its))
    res = subprocess.run([exe, "pairs", str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert res.returncode == 0, res.stderr.decode()
    stores = {}
    for line in res.stdout.decode().splitlines():
        f = [int(v) for v in line.split()]
        stores.setdefault(f[0], []).append(f[1:])
    for k, (out_off, step, length) in enumerate(its):
        mine = stores.get(k, [])
        widths = [s[0] for s in mine]
        assert widths.count(1) <= 2 and widths.count(2) <= ITEM // 2, (k, its[k])
        assert all(w == 2 for w in widths[1:-1]), (k, its[k])     # order: head, pairs, tail
        elem = np.full(length, -1, np.int64)            # element written for position i
        for s in mine:
            if s[0] == 2:
                lo_elem, lo_pos, hi_elem, hi_pos = s[1:]
                assert lo_elem % 2 == 0 and hi_elem == lo_elem + 1, (k, its[k], s)      # one aligned 16-byte slot
                assert abs(hi_pos - lo_pos) == 1 and (hi_pos - lo_pos) == step, (k, its[k], s)
                for e, p in ((lo_elem, lo_pos), (hi_elem, hi_pos)):
                    assert 0 <= p < length and elem[p] == -1, (k, its[k], s)
                    elem[p] = e
            else:
                e, p = s[1:]
                assert p in (0, length - 1) and elem[p] == -1, (k, its[k], s)
                # a single element only where its slot partner lies outside the item
                partner = e ^ 1
                lo_e, hi_e = (out_off, out_off + length - 1) if step > 0 else (out_off - length + 1, out_off)
                assert not (lo_e <= partner <= hi_e), (k, its[k], s)
                elem[p] = e
        want = out_off + step * np.arange(length, dtype=np.int64)
        assert np.array_equal(elem, want), (k, its[k])


def test_batches_cover_the_item_list(exe):
    BATCH = int(subprocess.run([exe, "batch"], stdout=subprocess.PIPE, timeout=300, check=True).stdout)
    assert 1 <= BATCH <= 8
    sizes = [1, BATCH - 1, BATCH, BATCH + 1, 3 * BATCH + 1, 21013, 1 << 20]
    res = subprocess.run([exe, "batches"] + [str(n) for n in sizes], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert res.returncode == 0, res.stderr.decode()
    rows = [[int(v) for v in line.split()] for line in res.stdout.decode().splitlines()]
    at = 0
    for n in sizes:
        assert rows[at][0] == n and rows[at][1] == -(-n // BATCH), (n, rows[at])
        nb = rows[at][1]
        cover = np.zeros(n, np.int32)
        for first, count in rows[at + 1:at + 1 + nb]:
            assert first % BATCH == 0 and 1 <= count <= BATCH, (n, first, count)
            cover[first:first + count] += 1
        assert (cover == 1).all(), n     # plan order, every item once
        at += 1 + nb
    assert at == len(rows)
