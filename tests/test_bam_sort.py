"""``read_bam(path, sort=True)`` (csrc/bam_stager.cpp ``pb_load_sorted``): a BAM file in any record order comes out as the
same records written in coordinate order do through the reader without ``sort`` -- the twin of tests/bam_sort_cases.py.
The contract (placed records by (tid, POS, reverse strand), ties in file order, unplaced records last) is a numpy model
there; it is this project's statement of a coordinate sorter's comparator, not checked against samtools.  CPU only."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from plastid_amd.bam import read_bam  # noqa: E402
from tests import bam_sort_cases as cases  # noqa: E402

REFS3, LENS3 = ["chrA", "chrB", "chrC"], [5000000, 3000000, 100000]


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as o
    o.lib()
    return o


def case_records(name):
    if name == "wide":
        return REFS3, LENS3, cases.wide_records()
    if name == "pile":
        return REFS3, LENS3, cases.tie_pile(600)
    return REFS3, LENS3, cases.random_records(int(name), 3, seed=int(name) + 7)


@pytest.mark.parametrize("name", ["0", "1", "2", "257", "4097", "wide", "pile"])
def test_shuffled_file_equals_its_twin(tmp_path, name):
    """Every column, the runs, the wide arrays and the SAM / NH columns equal the twin's; ``file_order`` is the model's
    permutation; without ``sort`` the shuffled file is refused as before."""
    refs, lens, recs = case_records(name)
    path, twin = cases.write_pair(tmp_path, "c" + name, refs, lens, recs, block_bytes=700 if len(recs) < 5000 else 20000)
    timing = {}
    got = read_bam(path, sort=True, timing=timing)
    cases.same_columns(got, read_bam(twin), name)
    cases.same_file_order(got, recs, name)
    order, moved = cases.model_order(recs)
    assert timing["records_moved"] == moved and timing["sorted_input"] == cases.in_order(recs)
    if len(getattr(got, "wide_idx", ())):
        assert np.all(np.diff(got.wide_idx) > 0)
    if not cases.in_order(recs):
        with pytest.raises(ValueError) as e:
            read_bam(path)
        assert str(e.value) == "%s: %s" % (cases.UNSORTED, path)
    if name == "pile":   # the tie keeps the file order within each strand
        fo = got.file_order[got.pos == 3000]
        rev = got.flags[got.pos == 3000] & 1
        assert np.all(np.diff(rev) >= 0) and np.all(np.diff(fo[rev == 0]) > 0) and np.all(np.diff(fo[rev == 1]) > 0)


def test_sorted_input_is_not_touched(tmp_path):
    """A file in coordinate order, and one sorted by (tid, POS) only with reverse before forward inside its ties: the
    arrays of ``sort=False``, ``file_order`` None."""
    recs = cases.twin_of(cases.random_records(3000, 3, seed=3))
    ties = [(0, 10, [(0, 30)], 16), (0, 10, [(0, 31)], 0), (0, 10, [(0, 32)], 16), (0, 11, [(0, 25)], 16), (0, 11, [(0, 26)], 0),
            (1, 5, [(0, 27)], 16, cases.nh_aux(2)), (1, 5, [(0, 28), (3, 10), (0, 5)], 0), (-1, -1, [], 4)]
    for k, rr in enumerate((recs, ties)):
        path = str(tmp_path / ("s%d.bam" % k))
        cases.write_fast(path, REFS3, LENS3, rr, block_bytes=900)
        timing = {}
        got, plain = read_bam(path, sort=True, timing=timing), read_bam(path)
        cases.same_columns(got, plain)
        assert got.file_order is None and timing["sorted_input"] is True and timing["records_moved"] == 0
        assert plain.file_order is None


def test_unplaced_records_between_placed_ones_move_nothing(tmp_path):
    """Placed records in order with unplaced records among them: refused without ``sort``; with it the placed records
    are staged where they stood, so nothing moved and ``file_order`` stays None."""
    recs = [(-1, -1, [], 4), (0, 5, [(0, 30)], 0), (-1, -1, [], 4), (0, 9, [(0, 30)], 16), (1, 2, [(0, 22)], 0)]
    path, twin = cases.write_pair(tmp_path, "u", REFS3, LENS3, recs)
    with pytest.raises(ValueError):
        read_bam(path)
    timing = {}
    got = read_bam(path, sort=True, timing=timing)
    cases.same_columns(got, read_bam(twin))
    assert got.file_order is None and timing["sorted_input"] is False and timing["records_moved"] == 0


def test_sort_with_regions_raises(tmp_path):
    path = str(tmp_path / "r.bam")
    cases.bam_writer.write_bam(path, REFS3, LENS3, [(0, 5, [(0, 30)], 0)], index=True)
    with pytest.raises(ValueError) as e:
        read_bam(path, regions=[("chrA", 0, 100)], sort=True)
    assert "sort" in str(e.value) and "regions" in str(e.value)
    with pytest.raises(ValueError) as e:
        read_bam(str(tmp_path / "absent.bam"), regions=[("chrA", 0, 100)], sort=True)   # before any file is opened
    assert "sort" in str(e.value) and "regions" in str(e.value)


def test_defects_with_sort(tmp_path):
    """A deletion-first read that the SORTED order puts out of first-aligned-position order is refused with the existing
    message; a record's own defect and a truncated file are reported as without ``sort``."""
    recs = [(0, 200, [(0, 30)], 0), (0, 100, [(2, 50), (0, 20)], 0), (0, 120, [(0, 30)], 0)]   # POS 100 starts aligning at 150 > 120
    path = str(tmp_path / "d.bam")
    cases.bam_writer.write_bam(path, REFS3, LENS3, recs)
    with pytest.raises(ValueError) as e:
        read_bam(path, sort=True)
    assert "starting with a deletion" in str(e.value)
    recs = [(0, 200, [(0, 30)], 0), (0, 100, [(0, 20)], 0), (0, 120, [(9, 30)], 0), (0, 50, [(0, 30)], 0)]
    path = str(tmp_path / "op.bam")
    cases.bam_writer.write_bam(path, REFS3, LENS3, recs)
    with pytest.raises(ValueError) as e:
        read_bam(path, sort=True)
    assert "unknown CIGAR operation" in str(e.value)
    # cut in the middle of the record stream (members re-written: the BGZF layer stays whole)
    recs = cases.random_records(400, 3, seed=5, rich=False)
    whole = str(tmp_path / "whole.bam")
    cases.write_fast(whole, REFS3, LENS3, recs, block_bytes=100000)
    import gzip
    data = gzip.decompress(open(whole, "rb").read())
    cut = str(tmp_path / "cut.bam")
    with open(cut, "wb") as fh:
        fh.write(cases.bam_writer.bgzf_block(data[:len(data) // 2]) + cases.bam_writer.BGZF_EOF)
    with pytest.raises(ValueError) as e:
        read_bam(cut, sort=True)
    assert str(e.value) == "truncated BAM record"


@pytest.mark.parametrize("name", ["4097", "pile"])
def test_the_oracle_counts_the_result_as_the_twin(tmp_path, oracle, name):
    """All five rules over the sorted result equal the oracle's counts over the twin, bit for bit (the center rule's
    float64 sums depend on the order of the records: the tie order is part of the contract)."""
    refs, lens, recs = case_records(name)
    path, twin = cases.write_pair(tmp_path, "o" + name, refs, lens, recs)
    got, ref = read_bam(path, sort=True), read_bam(twin)
    top = int(max(r[1] for r in recs)) + 4000
    segs = [(t, 0, top, st) for t in range(3) for st in (1, 2, 3)]
    for rule in cases.RULES:
        a = cases.oracle_counts(oracle, [got], rule, segs, size_filter=(22, 36))
        b = cases.oracle_counts(oracle, [ref], rule, segs, size_filter=(22, 36))
        assert sum(float(np.asarray(x).sum()) for x in b) > 0
        for x, y in zip(a, b):
            assert np.array_equal(np.ascontiguousarray(x).view(np.uint64), np.ascontiguousarray(y).view(np.uint64)), rule[0]


def test_sort_kernels_use_no_scratch_memory(tmp_path):
    """The three kernels of csrc/sort_kernels.hip.h in the built gfx950 code object have ``private_segment_fixed_size`` 0
    (tests/test_host_logic.py reads the kernels of namespace ``pc`` the same way; these live in ``pcbam``)."""
    import shutil
    import subprocess
    from plastid_amd import build
    lib = build.build_library()
    objdump, readelf = "/opt/rocm/lib/llvm/bin/llvm-objdump", "/opt/rocm/lib/llvm/bin/llvm-readelf"
    assert os.path.exists(objdump) and os.path.exists(readelf), "llvm-objdump / llvm-readelf of the ROCm toolchain that built the library"
    work = tmp_path / "co"
    work.mkdir()
    copy = str(work / "lib.so")
    shutil.copy(lib, copy)
    subprocess.check_call([objdump, "--offloading", copy], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, cwd=str(work))
    objs = [f for f in os.listdir(str(work)) if "gfx950" in f]
    assert objs, "no gfx950 code object found in %s" % lib
    notes = subprocess.check_output([readelf, "--notes", str(work / objs[0])]).decode()
    sizes = [int(line.split(":")[1]) for line in notes.splitlines() if ".private_segment_fixed_size" in line]
    names = [line.split(":")[1].strip() for line in notes.splitlines() if line.strip().startswith(".name:")]
    assert len(sizes) == len(names)
    own = {n: s for n, s in zip(names, sizes) if "k_bam_sort_" in n}
    assert len(own) == 3 and not any(own.values()), own
