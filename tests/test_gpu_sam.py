"""SAM text on the GPU (``pc_sam_open_path_flags``: csrc/sam_decoder.hip.h, csrc/sam_kernels.hip.h): ``read_sam_gpu``,
``Engine.add_sam`` and ``BAMGenomeArray("x.sam")`` against the host reader ``read_sam``, against the BAM twin of the same
records, and against the oracle.  Needs a real MI355X: ``pytest -m gpu``.

ORDER: the kernels run ``sam_parse_line`` of csrc/sam_host.h, the source tests/test_sam_host.py runs on the CPU under the
address and undefined-behaviour sanitizers on every prefix of a line and on lines of 0xff bytes.  The malformed files of
tests/sam_cases.py go through ``read_sam_gpu`` only after tests/test_sam_host.py has passed on the same tree: run
``pytest tests/test_sam_host.py`` (no GPU needed) before ``pytest -m gpu`` whenever csrc/sam_host.h changes.

Shapes: the line-start kernels work on tiles of ``kSamTile`` bytes of the body, the fields kernel on 256 lines per
workgroup and 64 per wave: a newline on the last byte of tile 0 and on the first byte of tile 1, one line that spans four
tiles, files of 1, 63, 64, 65, 256 and 257 records, a body without a final newline; a few thousand records elsewhere."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import plastid_amd as pa  # noqa: E402
from plastid_amd.bam import read_bam, read_bam_gpu, read_sam, read_sam_gpu  # noqa: E402
from plastid_amd.engine import Engine  # noqa: E402
from tests import bam_sort_cases, sam_cases, sam_writer  # noqa: E402
from tests.test_gpu_bam_sort import PA_RULES, bits  # noqa: E402
from tests.test_sam_text import check_against_htslib  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFS3, LENS3 = ["chrA", "chrB", "chrC"], [5000000, 3000000, 100000]


def tile_bytes():
    src = open(os.path.join(ROOT, "plastid_amd", "csrc", "sam_kernels.hip.h")).read()
    return int(re.search(r"constexpr int kSamTile = (\d+);", src).group(1))


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as o
    o.lib()
    return o


@pytest.fixture(scope="module")
def twins(tmp_path_factory):
    return sam_cases.synthetic_twins(tmp_path_factory.mktemp("sam_twins"))


def test_htslib_written_text(eng, tmp_path):
    path, hts, n_lines = sam_cases.hts_sam(tmp_path)
    timing = {}
    got = read_sam_gpu(path, eng, timing=timing)
    check_against_htslib(got, hts, n_lines)
    sam_cases.same_with_order(got, read_sam(path))
    assert timing["records"] == n_lines and timing["members"] == 0 and timing["inflated_bytes"] == 0
    body = open(path, "rb").read()
    assert timing["uploaded_bytes"] == len(body) - body.index(b"\nr") - 1       # the text behind the header lines
    for k in ("upload_ms", "lines_ms", "fields_ms", "place_ms"):
        assert timing[k] >= 0.0


def test_twins_equal_the_host_reader_and_the_bam_decoder(eng, twins):
    for name, bam, sam in twins:
        got = read_sam_gpu(sam, eng)
        assert got.n > 0
        sam_cases.same_with_order(got, read_sam(sam), name)
        sam_cases.same_columns(got, read_bam_gpu(bam, eng), name)
    assert len(read_sam_gpu(twins[-1][2], eng).wide_idx) >= 2


def padded_line(i, length, pos):
    """a good line of exactly `length` bytes (its '\\n' not counted): the read name is padded"""
    base = sam_cases.good_line(i, pos=pos)
    assert len(base) <= length
    return "p" * (length - len(base)) + base


def test_tile_edges(eng, tmp_path):
    T = tile_bytes()
    assert T >= 512
    files = {}
    # the first line's '\n' is the last byte of tile 0 / the first byte of tile 1; ordinary lines follow
    for name, first_len in (("nl_last_of_tile0", T - 1), ("nl_first_of_tile1", T)):
        files[name] = [padded_line(0, first_len, 50)] + [sam_cases.good_line(i) for i in range(1, 40)]
    # ... and the same for a line in the middle of the file, with lines before it
    lines = [sam_cases.good_line(i) for i in range(20)]
    used = sum(len(x) + 1 for x in lines)
    files["nl_last_of_tile1"] = lines + [padded_line(20, 2 * T - 1 - used, 300)] + [sam_cases.good_line(i) for i in range(21, 60)]
    # one record of 3 T aligned bases written as one line: the line spans four tiles
    long_line = "\t".join(["long", "16", "chrA", "1001", "7", "%dM" % (3 * T), "*", "0", "0", "A" * (3 * T), "*", "NH:i:2"])
    files["line_over_four_tiles"] = [sam_cases.good_line(0)] + [long_line] + [sam_cases.good_line(i, pos=2000 + i) for i in range(2, 30)]
    files["only_the_long_line"] = [long_line]
    for n in (1, 63, 64, 65, 256, 257):
        files["n%d" % n] = [sam_cases.good_line(i, cigar="10M5N15M" if i % 3 == 0 else "30M") for i in range(n)]
    for name, body in files.items():
        for final in (True, False):
            path = str(tmp_path / ("%s_%d.sam" % (name, final)))
            sam_cases.write_lines(path, sam_cases.HEAD, body, final_newline=final)
            want = read_sam(path)
            assert want.n == len(body), name
            sam_cases.same_with_order(read_sam_gpu(path, eng), want, (name, final))
    want = read_sam(str(tmp_path / "line_over_four_tiles_1.sam"))
    assert int(want.true_alen()[1]) == 3 * T and want.qlen[1] == 3 * T
    # "\r\n" line ends
    path = str(tmp_path / "crlf.sam")
    sam_cases.write_lines(path, sam_cases.HEAD, files["n257"], eol="\r\n")
    sam_cases.same_with_order(read_sam_gpu(path, eng), read_sam(str(tmp_path / "n257_1.sam")))
    # no record at all: a header only, an empty file
    for k, text in enumerate((sam_writer.join_lines(sam_cases.HEAD), b"")):
        path = str(tmp_path / ("none%d.sam" % k))
        open(path, "wb").write(text)
        got = read_sam_gpu(path, eng)
        assert got.n == 0 and got.mapped == 0 and list(got.references) == (sam_cases.REFS if k == 0 else [])


def sorted_and_shuffled(tmp, n, seed):
    """(records in shuffled order, shuffled SAM, twin SAM in coordinate order, twin BAM)"""
    recs = bam_sort_cases.random_records(n, 3, seed=seed)
    twin = bam_sort_cases.twin_of(recs)
    paths = [os.path.join(str(tmp), x) for x in ("shuffled.sam", "twin.sam", "twin.bam")]
    sam_writer.write_sam(paths[0], REFS3, LENS3, recs)
    sam_writer.write_sam(paths[1], REFS3, LENS3, twin)
    bam_sort_cases.write_fast(paths[2], REFS3, LENS3, twin)
    return [recs] + paths


@pytest.fixture(scope="module")
def counted(tmp_path_factory):
    return sorted_and_shuffled(tmp_path_factory.mktemp("sam_counts"), 4097, 21)


def windows():
    """30 chains of one segment: ten windows on the three references, each on '+', '-' and '.'"""
    return [(t, s, s + 300, st) for t, s in ((0, 0), (0, 250), (0, 700), (0, 1100), (1, 0), (1, 400), (1, 900), (2, 0), (2, 500), (2, 1000)) for st in (1, 2, 3)]


def filtered_array(path, **kw):
    ga = pa.BAMGenomeArray(path, keep_reads=False, **kw)
    ga.add_filter("size", pa.SizeFilterFactory())
    ga.add_filter("flag", pa.FlagFilterFactory(max_nh=1, min_mapq=10))
    return ga


def test_counts_equal_the_bam_twin_and_the_oracle(oracle, counted):
    """``Engine.add_sam`` and ``BAMGenomeArray(sam, keep_reads=False)`` under all five rules, 30 chains on '+', '-' and
    '.', the default size filter and FlagFilterFactory(max_nh=1, min_mapq=10): bit-equal to the array over the BAM twin and
    to the oracle over the twin's reads that pass."""
    recs, shuffled, sam, bam = counted
    ref = read_bam(bam)
    kept = ref.subset(np.nonzero((ref.nh == 1) & (ref.mapq >= 10) & (ref.true_alen() >= 1))[0])
    assert 100 < kept.n < ref.n
    segs = windows()
    assert len(segs) == 30
    e = Engine(0)
    assert e.add_sam(sam) == ref.mapped
    assert e.num_records(0) == ref.n
    e.set_flag_filter(min_mapq=10)
    ga_sam, ga_bam = filtered_array(sam), filtered_array(bam)
    total = 0.0
    for rule, factory in zip(bam_sort_cases.RULES, PA_RULES):
        want = bam_sort_cases.oracle_counts(oracle, [kept], rule, segs)
        exp = np.concatenate([np.asarray(a).reshape(-1) for a in want])
        total += float(exp.sum())
        assert np.array_equal(bits(counts_of(e, rule, segs)), bits(exp)), rule[0]
        ga_sam.set_mapping(factory())
        ga_bam.set_mapping(factory())
        for (t, s, en, st), w in zip(segs, want):
            seg = pa.GenomicSegment(REFS3[t], s, en, "+-."[st - 1])
            g = np.asarray(ga_sam.get(seg, roi_order=False), np.float64)
            assert np.array_equal(bits(g), bits(np.asarray(w, np.float64))), (rule[0], t, s, st)
            assert np.array_equal(bits(g), bits(np.asarray(ga_bam.get(seg, roi_order=False), np.float64))), (rule[0], t, s, st)
    assert total > 0
    assert ga_sam.sum() == ga_bam.sum() == ref.mapped
    e.close()


def counts_of(e, rule, segs):
    """The engine's count vectors of `segs` under `rule` with the default size filter and NH <= 1 (MAPQ: the caller's)."""
    from plastid_amd import synth
    seg_tid = np.array([s[0] for s in segs], np.int32)
    seg_start = np.array([s[1] for s in segs], np.int64)
    seg_end = np.array([s[2] for s in segs], np.int64)
    seg_strand = np.array([s[3] for s in segs], np.uint8)
    synth.mapping_factory(rule)._configure(e)
    e.set_size_filter(1, -1)
    e.set_nh_filter(1)
    rows = e.rows
    lens = seg_end - seg_start
    out_off = np.concatenate([[0], np.cumsum(lens * rows)[:-1]])
    plan = e.plan(seg_tid, seg_start, seg_end, seg_strand, out_off, np.ones(len(lens), np.int8), lens, int((lens * rows).sum()), rows)
    got = plan.count(np.float64 if rule[0] == "center" else np.int64).copy()
    plan.close()
    return got


def test_sort_gives_the_counts_of_the_sorted_twin(eng, counted):
    recs, shuffled, sam, bam = counted
    assert not bam_sort_cases.in_order(recs)
    timing = {}
    got = read_sam_gpu(shuffled, eng, sort=True, timing=timing)
    sam_cases.same_columns(got, read_sam_gpu(sam, eng))
    sam_cases.same_with_order(got, read_sam(shuffled, sort=True))
    bam_sort_cases.same_file_order(got, recs)
    assert timing["records_moved"] == bam_sort_cases.model_order(recs)[1] and timing["sorted_input"] is False and timing["sort_key_bits"] == 35
    with pytest.raises(ValueError) as e:
        read_sam_gpu(shuffled, eng)
    assert str(e.value) == "%s: %s" % (bam_sort_cases.UNSORTED, shuffled)
    a, b = filtered_array(shuffled, sort=True), filtered_array(sam)
    e2 = Engine(0)
    assert e2.add_sam(shuffled, sort=True) == got.mapped
    e2.close()
    for factory in (PA_RULES[0], PA_RULES[4]):
        a.set_mapping(factory())
        b.set_mapping(factory())
        for t, s, en, st in windows():
            seg = pa.GenomicSegment(REFS3[t], s, en, "+-."[st - 1])
            assert np.array_equal(bits(np.asarray(a.get(seg, roi_order=False), np.float64)), bits(np.asarray(b.get(seg, roi_order=False), np.float64)))
    # a file in order with sort=True is not touched
    timing = {}
    plain = read_sam_gpu(sam, eng, sort=True, timing=timing)
    sam_cases.same_with_order(plain, read_sam_gpu(sam, eng))
    assert plain.file_order is None and timing["sorted_input"] is True and timing["records_moved"] == 0


@pytest.mark.parametrize("case", sam_cases.malformed_files(), ids=lambda c: c[0])
def test_malformed_files_raise_the_host_readers_text(eng, tmp_path, case):
    """(See ORDER in the module's docstring.)  The device path raises what the host path raises, and the engine reads the
    next file as if nothing had happened."""
    name, head, body, expected = case
    path = str(tmp_path / (name + ".sam"))
    sam_cases.write_lines(path, head, body)
    with pytest.raises(ValueError) as host:
        read_sam(path)
    assert str(host.value) == sam_cases.expected_message(expected, path)
    with pytest.raises(ValueError) as dev:
        read_sam_gpu(path, eng)
    assert str(dev.value) == str(host.value)
    with pytest.raises(ValueError) as host:
        read_sam(path, sort=True)
    with pytest.raises(ValueError) as dev:
        read_sam_gpu(path, eng, sort=True)
    if name == "deletion-first":
        # the one documented difference of the two sorted reads (include/plastid_counts.h, PC_BAM_SORT): a file that is in
        # order already goes through the device's file-order checks, where the deletion-order pair on the lower line wins;
        # the host's sorted load gives the later line's own defect precedence
        assert str(dev.value) == sam_cases.expected_message(expected, path) and str(host.value) != str(dev.value)
    else:
        assert str(dev.value) == str(host.value)
    good =str(tmp_path / "good.sam")
    sam_cases.write_lines(good, sam_cases.HEAD, [sam_cases.good_line(i) for i in range(70)])
    assert read_sam_gpu(good, eng).n == 70


def test_refusals_and_the_image_entry_point(eng, tmp_path):
    import gzip
    from plastid_amd import _lib as clib
    good = str(tmp_path / "good.sam")
    body = [sam_cases.good_line(i) for i in range(300)]
    sam_cases.write_lines(good, sam_cases.HEAD, body)
    gz = str(tmp_path / "z.sam")
    with gzip.open(gz, "wb") as fh:
        fh.write(open(good, "rb").read())
    for call in (lambda: read_sam_gpu(gz, eng), lambda: eng.add_sam(gz), lambda: pa.BAMGenomeArray(gz, keep_reads=False)):
        with pytest.raises(ValueError) as e:
            call()
        assert "compressed SAM" in str(e.value)
    for kw in (dict(keep_reads=False), dict(decode="gpu"), dict()):
        with pytest.raises(ValueError) as e:
            pa.BAMGenomeArray(good, regions=[("chrA", 0, 100)], **kw)
        assert "SAM text has no index" in str(e.value)
    with pytest.raises(IOError):
        read_sam_gpu(str(tmp_path / "absent.sam"), eng)
    # pc_sam_open_flags: the same file from memory; an unknown flag bit is refused
    L = clib.load()
    image = open(good, "rb").read()
    h = ctypes.c_void_p()
    clib.check(L.pc_sam_open_flags(eng._h, image, len(image), b"good", 0, ctypes.byref(h)))
    counts = np.zeros(8, np.int64)
    clib.check(L.pc_bam_counts(h, counts.ctypes.data_as(ctypes.c_void_p)))
    L.pc_bam_close(h)
    assert list(counts[:4]) == [300, 0, 300, 300] and counts[5] == 0 and counts[6] == 0
    with pytest.raises(ValueError):
        clib.check(L.pc_sam_open_flags(eng._h, image, len(image), b"good", 2, ctypes.byref(h)))


def test_decode_auto_records_the_decoder(eng, tmp_path, monkeypatch):
    from plastid_amd import genome_array
    from plastid_amd.genome_array import _open_alignment_source
    good = str(tmp_path / "good.sam")
    sam_cases.write_lines(good, sam_cases.HEAD, [sam_cases.good_line(i) for i in range(500)])
    assert genome_array.GPU_DECODE_MIN_BYTES_SAM > os.path.getsize(good)
    small = _open_alignment_source(good, engine=eng, decode="auto")
    assert small.decoder == "host"
    monkeypatch.setattr(genome_array, "GPU_DECODE_MIN_BYTES_SAM", 1000)
    large = _open_alignment_source(good, engine=eng, decode="auto")
    assert large.decoder == "gpu"
    sam_cases.same_with_order(large, small)
    assert _open_alignment_source(good, engine=eng, decode="gpu").decoder == "gpu"
    assert _open_alignment_source(good, engine=eng, decode="host").decoder == "host"
    # a file the device decoder refuses gets the host reader's verdict
    name, head, body, expected = sam_cases.malformed_files()[4]
    bad = str(tmp_path / "bad.sam")
    sam_cases.write_lines(bad, head, body + [sam_cases.good_line(i) for i in range(10, 60)])
    with pytest.raises(ValueError) as e:
        _open_alignment_source(bad, engine=eng, decode="auto")
    assert str(e.value) == sam_cases.expected_message(expected, bad)
    ga = pa.BAMGenomeArray(good, sort=True)
    assert ga.bamfiles[0].decoder == "gpu" and ga.sum() == 500
