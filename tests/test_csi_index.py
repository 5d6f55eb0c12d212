"""The CSI index without a GPU: the record-by-record model (tests/csi_model.py) against the CSI htslib wrote
(tests/golden/csi_fixture.npz), the host finish ``pc_bam_index_finish_csi`` against the model, ``BamIndex`` on CSI files,
and region reads of the native reader through htslib's ``.csi`` against htslib's own result sets."""
import os
import shutil
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from plastid_amd import bam as pbam  # noqa: E402
from plastid_amd.bam import BamIndex, find_index, read_bam, resolve_regions  # noqa: E402
from tests import csi_cases as cc  # noqa: E402
from tests import csi_model as cm  # noqa: E402
from tests import index_cases as ic  # noqa: E402
from tests import index_model as im  # noqa: E402

SHAPES = cc.case_shapes()
DEPTH = {("fixture", 14): 2, ("fixture", 9): 4, ("long", 14): 6, ("long", 17): 5, ("flat", 14): 0}


@pytest.mark.parametrize("case,min_shift", SHAPES)
def test_model_equals_htslib(case, min_shift):
    d = cc.case_data(case, min_shift)
    want = cm.parse_csi(d["csi"])
    _, got = cc.case_model(case, min_shift)
    assert want[:2] == (min_shift, DEPTH[case, min_shift]) == got[:2]
    assert got[3] == want[3] == d["n_no_coor"]
    for t, ((bins, loff), (hbins, hloff)) in enumerate(zip(got[2], want[2])):
        assert sorted(bins) == sorted(hbins), t
        assert bins == hbins and loff == hloff, t
        m = cm.meta_bin(got[1])
        if m in hbins:
            assert hloff[m] == 0 and tuple(hbins[m][1]) == tuple(int(x) for x in d["stat"][t, 1:])
    # the records the model walked are the records htslib read back
    w = cc.case_walk(case)
    assert [(r[1], r[2], r[3]) for r in w["recs"]] == [tuple(int(x) for x in r[:3]) for r in d["rec"]]


def test_the_long_case_is_what_it_was_made_for():
    d = cc.case_data("long", 14)
    rec = d["rec"]
    assert d["lengths"][:3] == [(1 << 31) - 1, 700_000_000, 1 << 30] and not (rec[:, 0] == 2).any()
    assert rec[:, 2].max() == (1 << 31) - 1 and ((rec[:, 1] < 1 << 29) & (rec[:, 2] > (1 << 29) + 1000)).any()
    only_unmapped = rec[rec[:, 0] == 4]
    assert len(only_unmapped) and (only_unmapped[:, 3] & 4).all()
    assert (rec[:, 0] == -1).sum() == 4 == d["n_no_coor"]
    for ms in (14, 17):
        dd = cc.case_data("long", ms)
        assert (dd["regions"][:, 1] >= 1 << 29).sum() >= 60
        nonempty_high = sum(1 for q in range(len(dd["regions"])) if dd["regions"][q, 1] >= 1 << 29 and dd["region_off"][q + 1] > dd["region_off"][q])
        assert nonempty_high >= 30
        _, (_, n_lvls, refs, _) = cc.case_model("long", ms)
        assert all(v == 0 for v in refs[4][1].values()) and len(refs[4][0]) >= 2       # placed-unmapped only: no window, loff 0
        assert {cm.bin_level(b, n_lvls) for b in refs[0][0] if b < cm.n_bins(n_lvls)} >= {0, n_lvls}


def test_the_bai_shape_ties_the_model_to_the_bai_model():
    """Shape (14, 5) on the fixture BAM: the bins and chunks of the BAI htslib wrote, and every loff is the BAI's filled
    linear window at the bin's first leaf (0 beyond the windows)."""
    hts = np.load(ic.FIX)
    bai_refs, bai_nn = im.parse_bai(hts["bai"].tobytes())
    pre = cm.prefinish(cc.case_walk("fixture"), 14, 5)
    refs, nn = cm.finish(pre)
    assert nn == bai_nn and cm.meta_bin(5) == im.META_BIN
    for (bins, loff), (bbins, lin) in zip(refs, bai_refs):
        assert bins == bbins
        for b, lo in loff.items():
            if b == im.META_BIN:
                assert lo == 0
                continue
            bot = cm.bin_bot(b, 5)
            assert lo == (lin[bot] if bot < len(lin) else 0), b
    assert all(cm.reg2bin(r[2], r[3], 14, 5) == im.reg2bin(r[2], r[3]) for r in cc.case_walk("fixture")["recs"] if r[1] >= 0)


@pytest.mark.parametrize("case,min_shift", SHAPES)
def test_library_finish_equals_model(case, min_shift):
    pre, want = cc.case_model(case, min_shift)
    payload, st = cc.finish_with_library(pre)
    assert cm.parse_csi(payload) == want
    for ids in cm.bin_order(payload):
        assert ids == sorted(ids) and (not ids or ids[-1] == cm.meta_bin(want[1]))
    assert st[2] == len(pre["run_tid"]) and st[6] == want[3] and st[7] == int(pre["ref_mapped"].sum()) and st[5] == 0
    # the runs already in (tid, bin) order, file order kept inside a bin
    order = np.lexsort((np.arange(len(pre["run_tid"])), pre["run_bin"], pre["run_tid"]))
    srt = dict(pre)
    for k in ("run_tid", "run_bin", "run_beg", "run_end", "run_loff"):
        srt[k] = pre[k][order]
    assert cc.finish_with_library(srt)[0] == payload


def test_library_finish_edges():
    empty = dict(min_shift=14, n_lvls=3, n_ref=0, n_no_coor=0, run_tid=np.zeros(0, np.int32), run_bin=np.zeros(0, np.uint32),
                 **{k: np.zeros(0, np.uint64) for k in ("run_beg", "run_end", "run_loff", "ref_beg", "ref_end")},
                 **{k: np.zeros(0, np.int64) for k in ("ref_mapped", "ref_unmapped")})
    payload, st = cc.finish_with_library(empty)
    assert payload == b"CSI\1" + struct.pack("<iiii", 14, 3, 0, 0) + struct.pack("<Q", 0) and not st.any()
    assert cm.parse_csi(payload) == (14, 3, [], 0)
    pre, _ = cc.case_model("flat", 14)
    bad = dict(pre)
    bad["run_bin"] = pre["run_bin"].copy()
    bad["run_bin"][0] = cm.n_bins(0)                 # depth 0 has one bin
    with pytest.raises(ValueError, match="bin out of range"):
        cc.finish_with_library(bad)
    pre6, _ = cc.case_model("long", 14)
    bad = dict(pre6)
    bad["run_bin"] = pre6["run_bin"].copy()
    bad["run_bin"][0] = cm.n_bins(6)
    with pytest.raises(ValueError, match="bin out of range"):
        cc.finish_with_library(bad)
    for ms in (7, 31, 0, -1):
        with pytest.raises(ValueError, match="min_shift"):
            cc.finish_with_library(pre, min_shift=ms)
    with pytest.raises(ValueError, match="n_lvls"):
        cc.finish_with_library(pre, n_lvls=9)


@pytest.mark.parametrize("case,min_shift", SHAPES)
def test_bam_index_on_csi(tmp_path, case, min_shift):
    d = cc.case_data(case, min_shift)
    path = cc.write_case(tmp_path, case, min_shift)
    idx = BamIndex.from_file(path + ".hts.csi")
    assert idx == BamIndex.from_bytes(d["csi"])
    depth = DEPTH[case, min_shift]
    assert (idx.fmt, idx.min_shift, idx.depth, idx.meta_bin) == ("csi", min_shift, depth, cm.meta_bin(depth))
    assert idx.n_no_coor == d["n_no_coor"] and idx.mapped == int(d["stat"][:, 1].sum()) and idx.n_ref == len(d["references"])
    _, _, refs, _ = cm.parse_csi(d["csi"])
    for t, (bins, loff) in enumerate(refs):
        real = {b: c for b, c in bins.items() if b != idx.meta_bin}
        assert sorted(idx.bins[t]) == sorted(real) and all(np.array_equal(idx.bins[t][b], np.array(real[b], np.uint64)) for b in real)
        assert idx.loff[t] == {b: loff[b] for b in real} and len(idx.linear[t]) == 0
        assert idx.meta[t] == (tuple(x for c in bins[idx.meta_bin] for x in c) if idx.meta_bin in bins else None)
    data = idx.to_bytes()
    assert data[:4] == b"\x1f\x8b\x08\x04" and data[-28:] == pbam._BGZF_EOF and data[12:14] == b"BC"
    back = BamIndex.from_bytes(data)
    assert back == idx and cm.parse_csi(idx.payload()) == cm.parse_csi(BamIndex.from_bytes(d["csi"]).payload())
    idx.write(str(tmp_path / "again.csi"))
    assert BamIndex.from_file(str(tmp_path / "again.csi")) == idx
    other = BamIndex.from_bytes(data)
    t_with = next(t for t in range(idx.n_ref) if idx.loff[t])
    b0 = sorted(other.loff[t_with])[0]
    other.loff[t_with][b0] += 1
    assert other != idx
    assert "CSI min_shift=%d depth=%d" % (min_shift, depth) in repr(idx)


def test_a_large_csi_takes_several_bgzf_members():
    idx = BamIndex.from_bytes(cc.case_data("fixture", 9)["csi"])
    big = BamIndex([dict(idx.bins[0])] * 40, [idx.linear[0]] * 40, [idx.meta[0]] * 40, 3, "csi", 9, 4, [dict(idx.loff[0])] * 40)
    data = big.to_bytes()
    assert len(big.payload()) > 2 * 0xff00
    sizes, o = [], 0
    while o < len(data):
        bsize, = struct.unpack_from("<H", data, o + 16)
        sizes.append(struct.unpack_from("<I", data, o + bsize + 1 - 4)[0])
        o += bsize + 1
    assert o == len(data) and sizes[-1] == 0 and max(sizes) == 0xff00 and sum(sizes) == len(big.payload())
    assert BamIndex.from_bytes(data) == big


def test_bai_objects_are_what_they_were():
    hts = np.load(ic.FIX)
    raw = hts["bai"].tobytes()
    idx = BamIndex.from_bytes(raw)
    assert (idx.fmt, idx.min_shift, idx.depth, idx.meta_bin) == ("bai", 14, 5, 37450) and idx.loff == [{}] * idx.n_ref
    assert im.parse_bai(idx.to_bytes()) == im.parse_bai(raw) and idx.to_bytes()[:4] == b"BAI\1"
    assert repr(idx).startswith("BamIndex(3 references")
    assert idx != BamIndex.from_bytes(cc.case_data("fixture", 14)["csi"])


def _stager_refuses(tmp_path, bam_path, index_bytes, name):
    p = str(tmp_path / name)
    open(p, "wb").write(index_bytes)
    with pytest.raises(ValueError):
        read_bam(bam_path, regions=[("chrA", 0, 1000)], index=p)


def test_truncated_and_corrupt_csi_files_are_refused(tmp_path):
    d = cc.case_data("fixture", 9)
    path = cc.write_case(tmp_path, "fixture", 9)
    data = open(path + ".hts.csi", "rb").read()
    for cut in range(0, len(data), 97):
        with pytest.raises(ValueError):
            BamIndex.from_bytes(data[:cut])
    payload = d["csi"]
    for cut in range(0, len(payload) - 8, 97):       # (cut behind the last bin, a payload without n_no_coor is a complete one)
        with pytest.raises(ValueError):
            BamIndex.from_bytes(payload[:cut])
    # counts that promise more than the bytes hold: n_bin of reference 0, n_chunk of its first bin, l_aux; huge and negative
    n_bin_at, n_chunk_at = 20, 24 + 12
    for k, (at, bad) in enumerate([(n_bin_at, 0x7fffffff), (n_bin_at, -1), (n_bin_at, 1 << 20), (n_chunk_at, 0x7fffffff), (n_chunk_at, -5),
                                   (n_chunk_at, 1 << 27), (12, 0x7fffffff), (12, -1), (12, len(payload))]):
        broken = payload[:at] + struct.pack("<i", bad) + payload[at + 4:]
        with pytest.raises(ValueError):
            BamIndex.from_bytes(broken)
        with pytest.raises(ValueError):
            BamIndex.from_bytes(pbam._bgzf_wrap(broken))
        _stager_refuses(tmp_path, path, pbam._bgzf_wrap(broken), "broken%d.csi" % k)
        _stager_refuses(tmp_path, path, broken, "broken%d.payload" % k)
    _stager_refuses(tmp_path, path, data[:len(data) // 2], "half.csi")
    _stager_refuses(tmp_path, path, pbam._bgzf_wrap(b"BAI\1" + payload[4:]), "wrong-magic.csi")
    flipped = bytearray(data)
    flipped[40] ^= 0x55
    with pytest.raises(ValueError):
        BamIndex.from_bytes(bytes(flipped))
    _stager_refuses(tmp_path, path, bytes(flipped), "flipped.csi")


@pytest.mark.parametrize("case,min_shift", SHAPES)
def test_region_reads_through_htslib_csi(tmp_path, case, min_shift):
    d = cc.case_data(case, min_shift)
    path = cc.write_case(tmp_path, case, min_shift)
    bai = None
    if case == "fixture":
        bai = path + ".hts.bai"
        open(bai, "wb").write(np.load(ic.FIX)["bai"].tobytes())
    nonempty = 0
    for q in range(len(d["regions"])):
        reg, want = cc.region_want(d, q)
        got = read_bam(path, regions=[reg], index=path + ".hts.csi")
        cc.assert_records(got, d, want)
        assert got.mapped == int(d["stat"][:, 1].sum())
        nonempty += got.n > 0
        if bai:
            cc.same(got, read_bam(path, regions=[reg], index=bai))
    assert nonempty >= 100
    # a whole query set at once, and the chunk list the GPU decoder would be handed
    regs = [cc.region_want(d, q)[0] for q in range(0, len(d["regions"]), 7)]
    union = np.unique(np.concatenate([cc.region_want(d, q)[1] for q in range(0, len(d["regions"]), 7)]))
    cc.assert_records(read_bam(path, regions=regs, index=path + ".hts.csi"), d, union)
    sp = resolve_regions(path, regs, index=path + ".hts.csi")
    assert sp["mapped"] == int(d["stat"][:, 1].sum()) and len(sp["chunks"]) and (sp["chunks"][1:, 0] > sp["chunks"][:-1, 1]).all()
    assert int(sp["end"].max()) <= 1 << (min_shift + 3 * DEPTH[case, min_shift])


def test_lookup_order(tmp_path):
    d = cc.case_data("fixture", 14)
    path = cc.write_case(tmp_path, "fixture", 14)
    reg, want = next(cc.region_want(d, q) for q in range(300) if len(cc.region_want(d, q)[1]) > 3)
    assert find_index(path) is None
    with pytest.raises(ValueError, match="cannot read the index of"):
        read_bam(path, regions=[reg])
    stem = path[:-4]
    for name in (path + ".csi", stem + ".csi"):
        shutil.copy(path + ".hts.csi", name)
        assert find_index(path) == name
        cc.assert_records(read_bam(path, regions=[reg]), d, want)
        os.remove(name)
    # both present: the BAI is used -- shown with a CSI that cannot be parsed beside a good BAI, and the reverse
    open(path + ".csi", "wb").write(b"\x1f\x8b not an index")
    open(path + ".bai", "wb").write(np.load(ic.FIX)["bai"].tobytes())
    assert find_index(path) == path + ".bai"
    cc.assert_records(read_bam(path, regions=[reg]), d, want)
    shutil.copy(path + ".hts.csi", path + ".csi")
    open(path + ".bai", "wb").write(b"BAI\1 cut")
    with pytest.raises(ValueError, match="BAI index"):
        read_bam(path, regions=[reg])
    os.remove(path + ".bai")
    open(stem + ".bai", "wb").write(np.load(ic.FIX)["bai"].tobytes())
    assert find_index(path) == stem + ".bai"          # x.bai before x.bam.csi
    cc.assert_records(read_bam(path, regions=[reg]), d, want)


def test_build_index_arguments_need_no_gpu(tmp_path):
    path = cc.write_case(tmp_path, "flat")
    with pytest.raises(ValueError, match="min_shift 14"):
        pbam.build_index(path, fmt="bai", min_shift=12)
    with pytest.raises(ValueError, match="fmt"):
        pbam.build_index(path, fmt="tbi")
    assert not [f for f in os.listdir(str(tmp_path)) if f != "flat.bam"]


def test_a_csi_without_the_eof_block_reads_the_same_in_both_readers(tmp_path):
    """htslib only warns about a BGZF file without the end-of-file block; ``BamIndex`` and the native reader take it too."""
    d = cc.case_data("long", 17)
    path = cc.write_case(tmp_path, "long", 17)
    data = open(path + ".hts.csi", "rb").read()
    assert data[-28:] == pbam._BGZF_EOF
    open(path + ".noeof.csi", "wb").write(data[:-28])
    assert BamIndex.from_file(path + ".noeof.csi") == BamIndex.from_bytes(d["csi"])
    q = next(q for q in range(300) if d["regions"][q, 1] >= 1 << 29 and len(cc.region_want(d, q)[1]) > 2)
    reg, want = cc.region_want(d, q)
    cc.assert_records(read_bam(path, regions=[reg], index=path + ".noeof.csi"), d, want)
    assert BamIndex.from_bytes(b"BAI\1" + struct.pack("<i", -1)).n_ref == 0          # (as before CSI was read)


def test_a_whole_reference_region_costs_the_bins_of_the_index_not_the_leaves(tmp_path):
    """Shape (8, 8) has 2^24 leaves under the root; a region over all of them resolves through the bins the index holds."""
    path = str(tmp_path / "deep.bam")
    top = (1 << 31) - 1
    recs = [(0, 5, [(0, 30)], 0), (0, 1 << 30, [(0, 30)], 16), (0, top - 30, [(0, 30)], 0)]
    cc.write_bam(path, ["c1"], [top], recs)
    pre = cm.prefinish(cm.walk(open(path, "rb").read()), 8)
    assert pre["n_lvls"] == 8
    refs, nn = cm.finish(pre)
    bins = {b: np.array(c, np.uint64) for b, c in refs[0][0].items() if b != cm.meta_bin(8)}
    m = refs[0][0][cm.meta_bin(8)]
    idx = BamIndex([bins], [np.zeros(0, np.uint64)], [(m[0][0], m[0][1], m[1][0], m[1][1])], nn, "csi", 8, 8,
                   [{b: refs[0][1][b] for b in bins}])
    idx.write(path + ".csi")
    got = read_bam(path, regions=[("c1", 0, 1 << 40)])
    assert got.n == 3 and got.pos.tolist() == [5, 1 << 30, top - 30]
    assert read_bam(path, regions=[("c1", (1 << 30) + 29, (1 << 30) + 31)]).pos.tolist() == [1 << 30]
    assert read_bam(path, regions=[("c1", (1 << 30) + 30, top - 30)]).n == 0
