"""The contig table of a count track (plastid_amd/csrc/track_table.h) without a GPU: tests/track_table_host_test.cpp, compiled
with the host compiler (under the address and undefined-behaviour sanitizers where it has them) and run as a program over
the golden cases as a plain text file -- every import of tests/golden/track_fixture.npz, the construction steps of every
non-raising case of tests/golden/track_export_fixture.npz, and the contigs its golden texts hold."""
import os
import shutil
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import track_cases as tc  # noqa: E402
from tests import track_export_cases as xc  # noqa: E402


def _hex(s):
    return s.encode().hex() or "-"


def _import_cases():
    """declare chr_lengths, every add, then the fixture's chroms / lengths"""
    lines = ["min_chr %d" % tc.fixture()[0]["min_chr_size"]]
    for name in tc.case_names():
        c = tc.case(name)
        lines += ["case %s" % name, "new t 2"]
        lines += ["declare t %s %d" % (_hex(ch), n) for ch, n in (c["chr_lengths"] or {}).items()]
        lines += ["add t %d %s" % ("+-".index(strand), _hex(text)) for text, strand in c["adds"]]
        lines += ["chrom %s %d" % (_hex(ch), c["lengths"][ch]) for ch in c["chroms"]]
        lines.append("expect t 2")
    return lines


def _combine_arguments(strands_a, strands_b, mode):
    """What ``GenomeArray.apply_operation`` hands to ``pc_track_combine``: the result's strands, mode_all, length_pad, the slots."""
    if strands_b is None:
        return list(strands_a), 1, 0, list(range(len(strands_a))), []
    if mode == "truncate":
        strands = [s for s in strands_a if s in strands_b]
    else:
        strands = list(strands_a) + [s for s in strands_b if s not in strands_a]
    slot = lambda own: [own.index(s) if s in own else -1 for s in strands]  # noqa: E731
    return strands, 0 if mode == "truncate" else 1, 10000 * len(strands) if mode == "same" else 0, slot(strands_a), slot(strands_b)


def _replay_cases():
    lines = ["min_chr %d" % xc.MIN_CHR]
    for name in xc.case_names():
        c = xc.case(name)
        lines.append("case %s" % name)
        strands = {}
        for st in c["steps"]:
            t = st["target"]
            if st["op"] == "new":
                strands[t] = ["+", "-"]
                lines.append("new %s 2" % t)
                lines += ["declare %s %s %d" % (t, _hex(ch), n) for ch, n in st["chr_lengths"].items()]
            elif st["op"] == "set":
                segs = " ".join("%d %d" % (a, b) for a, b in st["segments"])
                lines.append("set %s %s %d %d %s" % (t, _hex(st["chrom"]), strands[t].index(st["strand"]), len(st["segments"]), segs))
            elif st["op"] == "wiggle":
                lines.append("add %s %d %s" % (t, strands[t].index(st["strand"]), _hex(st["text"])))
            elif st["op"] == "arith":
                other = st["right"] if isinstance(st["right"], str) else None
                mode = "all" if st["how"] == "operator" else st["mode"]
                strands[t], mode_all, pad, slot_a, slot_b = _combine_arguments(strands[st["left"]], strands[other] if other else None, mode)
                lines.append("arith %s %s %s %d %d %d %s" % (t, st["left"], other or "-", mode_all, pad, len(strands[t]),
                                                         " ".join(str(x) for x in slot_a + slot_b)))
        t, last = c["result"], c["steps"][-1]
        assert sorted(strands[t]) == sorted(c["strands"])
        lines += ["chrom %s %d" % (_hex(ch), c["lengths"][ch]) for ch in c["chroms"]]
        # (the reference takes the order of its `all` result from a set; here it is the left operand's, then the right one's)
        from_set = last["op"] == "arith" and isinstance(last["right"], str) and (last["mode"] == "all" or last["how"] == "operator")
        lines.append("expect %s %d %s" % (t, len(c["strands"]), "%s %s" % (last["left"], last["right"]) if from_set else ""))
    return lines


def _header_contigs(text, kind):
    """The contigs a golden text writes, in its order: bedGraph -- column 0 of its lines; variableStep -- its headers."""
    names = []
    for line in text.split("\n")[1:]:
        if kind == 1 and line.startswith("variableStep chrom="):
            names.append(line[len("variableStep chrom="):].rsplit(" span=", 1)[0])
        elif kind == 0 and line and line.split("\t")[0] not in names:
            names.append(line.split("\t")[0])
    return names


def _export_cases():
    lines = []
    for name in xc.case_names():
        c = xc.case(name)
        lines += ["case %s" % name, "new x %d" % len(c["strands"])]
        lines += ["declare x %s %d" % (_hex(ch), c["lengths"][ch]) for ch in c["chroms"]]
        lines.append("cells x")
        lines += [" ".join(float(v).hex() for v in xc.cells(name, ch, st)) for ch in c["chroms"] for st in c["strands"]]
        for s, st in enumerate(c["strands"]):
            for kind, what in enumerate(("bedgraph", "variable_step")):
                lines.append("want x %d %d %s" % (s, kind, " ".join(_hex(ch) for ch in _header_contigs(c[what][st], kind))))
    return lines


def test_track_table_program(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "track_table_host_test")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    if subprocess.call([cxx] + san + [str(probe), "-o", str(tmp_path / "probe")], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL) != 0 \
            or subprocess.call([str(tmp_path / "probe")]) != 0:
        san = []
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror"] + san + ["-I", os.path.join(root, "plastid_amd", "csrc"),
                           os.path.join(root, "tests", "track_table_host_test.cpp"), "-o", exe])
    cases = tmp_path / "cases.txt"
    cases.write_text("\n".join(_import_cases() + _replay_cases() + _export_cases()) + "\n")
    out = subprocess.run([exe, str(cases)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert out.returncode == 0, out.stdout.decode()
    assert b"track_table_host: ok" in out.stdout
