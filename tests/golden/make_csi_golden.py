#!/usr/bin/env python
"""Generate ``tests/golden/csi_fixture.npz`` by running the reference-held htslib in the build container.

    python tests/golden/make_csi_golden.py

``oracle/build_ref.sh`` compiles that htslib into ``oracle/_ref/libhts_ref.a``; this script compiles the harness
``tests/golden/hts_csi_golden.c`` against it (gcc) into ``oracle/_ref/hts_csi_golden`` (git-ignored) and runs it.  Per
case and index shape the fixture holds what htslib itself wrote and read back: the CSI payload (the ``.csi`` file
inflated), every record, the result sets of 300 seeded regions read through that CSI, and the index's counts.  Only DATA is
committed.  The cases:

``fixture``  the BAM bytes of ``hts_fixture.npz`` (not stored again); min_shift 14 -> depth 2, min_shift 9 -> depth 4
``long``     references up to 2^31 - 1, read clusters around 2^29, 2^30, 2 * 10^9 and the end; 14 -> depth 6, 17 -> depth 5
``flat``     references of at most 16 000; 14 -> depth 0

Keys: ``cases`` (names), ``<case>_shapes`` (the min_shift values), ``<case>_bam`` (``long``, ``flat``), ``<case>_references``,
``<case>_lengths``, and per shape ``<case>_<min_shift>_csi | _rec (tid, pos, endpos, flag, mapq, l_qseq) | _regions (tid, beg,
end) | _region_off | _region_records | _stat (tid, mapped, unmapped) | _n_no_coor``.
"""
import os
import struct
import subprocess
import sys
import tempfile
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
HTSLIB = os.environ.get("HTSLIB_SRC", "/root/reference/kent/src/htslib")
NREG = 300
SEED = 20261018
CASES = (("fixture", (14, 9), (2, 4)), ("long", (14, 17), (6, 5)), ("flat", (14,), (0,)))


def inflate_bgzf(data):
    o, out = 0, []
    while o < len(data):
        xlen, = struct.unpack_from("<H", data, o + 10)
        bsize, = struct.unpack_from("<H", data, o + 16)
        out.append(zlib.decompress(data[o + 12 + xlen:o + bsize + 1 - 8], -15))
        o += bsize + 1
    return b"".join(out)


def main():
    subprocess.check_call(["bash", os.path.join(ROOT, "oracle", "build_ref.sh")])
    ref = os.path.join(ROOT, "oracle", "_ref")
    lib = os.path.join(ref, "libhts_ref.a")
    if not os.path.exists(lib):
        raise SystemExit("oracle/_ref/libhts_ref.a was not built (is the reference present?)")
    exe = os.path.join(ref, "hts_csi_golden")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-I", HTSLIB, os.path.join(HERE, "hts_csi_golden.c"), lib, "-lz", "-lm", "-lpthread", "-o", exe])
    tmp = tempfile.mkdtemp(prefix="csi_golden_")
    out = dict(cases=np.array([c[0] for c in CASES]), htslib_version=np.array("1.3 (vendored: kent/src/htslib)"))
    for case, shapes, depths in CASES:
        bam = os.path.join(tmp, case + ".bam")
        if case == "fixture":
            open(bam, "wb").write(np.load(os.path.join(HERE, "hts_fixture.npz"))["bam"].tobytes())
        else:
            subprocess.check_call([exe, "write-" + case, bam, str(SEED)])
            out[case + "_bam"] = np.frombuffer(open(bam, "rb").read(), np.uint8)
        out[case + "_shapes"] = np.array(shapes, np.int32)
        for min_shift, depth in zip(shapes, depths):
            text = subprocess.check_output([exe, "query", bam, str(min_shift), str(NREG), str(SEED + min_shift)]).decode()
            refs, lens, rec, reg, reg_off, reg_val, stat, nocoor = [], [], [], [], [0], [], [], 0
            for line in text.splitlines():
                f = line.split()
                if f[0] == "REF":
                    refs.append(f[1]); lens.append(int(f[2]))
                elif f[0] == "REC":
                    assert int(f[1]) == len(rec)
                    rec.append([int(x) for x in f[2:8]])
                elif f[0] == "REG":
                    n = int(f[4])
                    v = [int(x) for x in f[5:]]
                    assert len(v) == n
                    reg.append([int(x) for x in f[1:4]]); reg_val.extend(v); reg_off.append(len(reg_val))
                elif f[0] == "STAT":
                    stat.append([int(x) for x in f[1:4]])
                elif f[0] == "NOCOOR":
                    nocoor = int(f[1])
            payload = inflate_bgzf(open(bam + ".csi", "rb").read())
            assert payload[:4] == b"CSI\1" and struct.unpack_from("<iii", payload, 4) == (min_shift, depth, 0), struct.unpack_from("<iii", payload, 4)
            reg = np.array(reg, np.int64)
            if case == "long":
                assert int((reg[:, 1] >= 1 << 29).sum()) >= 60
            k = "%s_%d_" % (case, min_shift)
            out[case + "_references"], out[case + "_lengths"] = np.array(refs), np.array(lens, np.int64)
            out[k + "csi"] = np.frombuffer(payload, np.uint8)
            out[k + "rec"] = np.array(rec, np.int64)
            out[k + "regions"], out[k + "region_off"], out[k + "region_records"] = reg, np.array(reg_off, np.int64), np.array(reg_val, np.int32)
            out[k + "stat"], out[k + "n_no_coor"] = np.array(stat, np.int64), np.array(nocoor, np.int64)
            print("%s min_shift %d depth %d: %d records, %d regions (%d non-empty, %d from 2^29 on), CSI payload %d B" % (
                case, min_shift, depth, len(rec), len(reg), int((np.diff(reg_off) > 0).sum()), int((reg[:, 1] >= 1 << 29).sum()), len(payload)))
            os.remove(bam + ".csi")
        os.remove(bam)
    os.rmdir(tmp)
    dest = os.path.join(HERE, "csi_fixture.npz")
    np.savez_compressed(dest, **out)
    size = os.path.getsize(dest)
    print("wrote %s: %.0f KB" % (dest, size / 1e3))
    assert size <= 512 * 1024


if __name__ == "__main__":
    sys.exit(main())
