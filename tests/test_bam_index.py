"""The BAI index on the host: the record-by-record model (tests/index_model.py) against the index htslib wrote for the
fixture, the parsed :class:`plastid_amd.bam.BamIndex`, the host half of the build (``pc_bam_index_finish``) against the
model's finish, and region reads through an index file named explicitly."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from plastid_amd.bam import BamIndex, read_bam  # noqa: E402
from tests import index_cases as ic  # noqa: E402
from tests import index_model as im  # noqa: E402


@pytest.fixture(scope="module")
def hts():
    return np.load(ic.FIX)


@pytest.fixture(scope="module")
def synth_path(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("index") / "synth.bam")
    ic.write_synth(path)
    return path


def test_the_model_reproduces_the_index_htslib_wrote(hts):
    """Every bin and chunk, every linear offset, both chunks of every pseudo-bin and n_no_coor of the fixture's ``bai``
    (3 002 records, 3 references, placed-unmapped and unplaced reads), compared parsed."""
    want = im.parse_bai(hts["bai"].tobytes())
    got = im.model(hts["bam"].tobytes())
    assert got[1] == want[1] == 2
    for r, (w, g) in enumerate(zip(want[0], got[0])):
        assert w[1] == g[1], "linear index of reference %d" % r
        assert w[0] == g[0], "bins of reference %d" % r
    assert got == want


def test_bamindex_round_trip(hts):
    data = hts["bai"].tobytes()
    idx = BamIndex.from_bytes(data)
    again = idx.to_bytes()
    assert BamIndex.from_bytes(again) == idx and im.parse_bai(again) == im.parse_bai(data)
    for ids in im.bin_order(again):      # ascending, the pseudo-bin last
        assert ids == sorted(ids) and (not ids or ids[-1] == 37450)
    assert idx.n_ref == 3 and idx.n_no_coor == 2 and idx.mapped == int(hts["index_stat"][:, 1].sum())
    want = im.parse_bai(data)[0]
    for t in range(idx.n_ref):
        assert sorted(idx.bins[t]) == sorted(b for b in want[t][0] if b != 37450)
        assert idx.linear[t].tolist() == want[t][1]
        assert list(idx.meta[t]) == [x for c in want[t][0][37450] for x in c]
    other = BamIndex.from_bytes(data)
    other.linear[0][0] += 1
    assert other != idx
    with pytest.raises(ValueError):
        BamIndex.from_bytes(data[:len(data) // 2])
    with pytest.raises(ValueError):
        BamIndex.from_bytes(b"BAM\x01" + data[4:])


def test_the_host_finish_equals_the_models(hts, synth_path):
    """``pc_bam_index_finish`` (no GPU) on the model's runs and linear arrays: the fixture, the synthetic multi-level file
    (where bins stay, move into parents and merge), the runs in file order and sorted by (tid, bin), and empty input."""
    pre_fix = im.prefinish(im.walk(hts["bam"].tobytes()))
    _, pre_syn, model_syn = ic.synth_model(synth_path)
    ic.assert_synth_shape(model_syn)
    for pre, want in ((pre_fix, im.parse_bai(hts["bai"].tobytes())), (pre_syn, model_syn)):
        data, st = ic.finish_with_library(pre)
        assert im.parse_bai(data) == want
        order = np.lexsort((pre["run_bin"], pre["run_tid"]))          # stable: file order inside a bin
        srt = dict(pre, **{k: pre[k][order] for k in ("run_tid", "run_bin", "run_beg", "run_end")})
        assert ic.finish_with_library(srt)[0] == data
        placed = int(pre["ref_mapped"].sum() + pre["ref_unmapped"].sum())
        chunks = sum(len(c) for bins, _ in want[0] for b, c in bins.items() if b != 37450)
        nbins = sum(1 for bins, _ in want[0] for b in bins if b != 37450)
        assert st.tolist() == [placed + pre["n_no_coor"], placed, len(pre["run_tid"]), chunks, nbins, len(pre["linear"]), pre["n_no_coor"],
                               int(pre["ref_mapped"].sum())]
        for ids in im.bin_order(data):
            assert ids == sorted(ids)
    z64, zu = np.zeros(3, np.int64), np.zeros(3, np.uint64)
    empty = dict(n_ref=3, run_tid=np.zeros(0, np.int32), run_bin=np.zeros(0, np.uint32), run_beg=np.zeros(0, np.uint64), run_end=np.zeros(0, np.uint64),
                 lin_start=np.zeros(4, np.int64), linear=np.zeros(0, np.uint64), ref_beg=zu, ref_end=zu, ref_mapped=z64, ref_unmapped=z64, n_no_coor=0)
    data, st = ic.finish_with_library(empty)
    assert im.parse_bai(data) == ([({}, [])] * 3, 0) and not st.any()
    bad = dict(pre_fix, run_bin=np.full_like(pre_fix["run_bin"], 37450))
    with pytest.raises(ValueError):
        ic.finish_with_library(bad)


def test_region_reads_through_an_index_named_explicitly(hts, tmp_path):
    """``read_bam(path, regions=, index=elsewhere)`` reads what the index beside the file gives; an explicit index that is
    not there raises the message of a missing index."""
    here, there = str(tmp_path / "with.bam"), str(tmp_path / "ro" / "without.bam")
    os.mkdir(str(tmp_path / "ro"))
    for p in (here, there):
        open(p, "wb").write(hts["bam"].tobytes())
    open(here + ".bai", "wb").write(hts["bai"].tobytes())
    elsewhere = str(tmp_path / "elsewhere.idx")
    open(elsewhere, "wb").write(hts["bai"].tobytes())
    refs = [str(x) for x in hts["references"]]
    for lo in (0, 40, 200):
        regs = [(refs[int(t)], int(b), int(e)) for t, b, e in hts["regions"][lo:lo + 20]]
        want, got = read_bam(here, regions=regs), read_bam(there, regions=regs, index=elsewhere)
        assert got.n == want.n and got.mapped == want.mapped
        for col in ("tid", "pos", "alen", "flags", "nblk", "blk_start", "blk_len", "flag16", "mapq", "qlen", "nh"):
            assert np.array_equal(getattr(got, col), getattr(want, col)), col
    with pytest.raises(ValueError, match="cannot read the index of"):
        read_bam(there, regions=[(refs[0], 0, 10)])
    with pytest.raises(ValueError, match="cannot read the index of"):
        read_bam(there, regions=[(refs[0], 0, 10)], index=str(tmp_path / "nowhere.bai"))
