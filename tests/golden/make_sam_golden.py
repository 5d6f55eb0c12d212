#!/usr/bin/env python
"""Generate ``tests/golden/sam_fixture.npz`` by running the reference-held htslib in the build container.

    python tests/golden/make_sam_golden.py

``oracle/build_ref.sh`` compiles that htslib into ``oracle/_ref/libhts_ref.a``; this script compiles the harness
``tests/golden/hts_sam_golden.c`` against it (gcc) into ``oracle/_ref/hts_sam_golden`` (git-ignored) and runs it on the
``bam`` bytes of ``hts_fixture.npz``.  The fixture holds the SAM TEXT htslib itself wrote for those records (``sam_open``
in text mode, ``sam_hdr_write``, ``sam_write1``) and nothing else: the expected columns are the existing keys of
``hts_fixture.npz``.  Only DATA is committed.

Keys: ``sam`` (the text, uint8), ``n_lines`` (alignment lines kept: all of them unless the text had to be cut to fit
the size limit of a committed fixture, then the first ``n_lines``), ``n_records`` (records in the BAM file).
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))


def htslib_src():
    """The htslib sources oracle/build_ref.sh builds from: ``HTSLIB_SRC``, or that script's default."""
    import re
    if os.environ.get("HTSLIB_SRC"):
        return os.environ["HTSLIB_SRC"]
    return re.search(r"HTSLIB_SRC:-([^}]+)\}", open(os.path.join(ROOT, "oracle", "build_ref.sh")).read()).group(1)


HTSLIB = htslib_src()
LIMIT = 512 * 1024


def main():
    subprocess.check_call(["bash", os.path.join(ROOT, "oracle", "build_ref.sh")])
    ref = os.path.join(ROOT, "oracle", "_ref")
    lib = os.path.join(ref, "libhts_ref.a")
    if not os.path.exists(lib):
        raise SystemExit("oracle/_ref/libhts_ref.a was not built (is the reference present?)")
    exe = os.path.join(ref, "hts_sam_golden")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-I", HTSLIB, os.path.join(HERE, "hts_sam_golden.c"), lib, "-lz", "-lm", "-lpthread", "-o", exe])
    tmp = tempfile.mkdtemp(prefix="sam_golden_")
    bam, sam = os.path.join(tmp, "fixture.bam"), os.path.join(tmp, "fixture.sam")
    open(bam, "wb").write(np.load(os.path.join(HERE, "hts_fixture.npz"))["bam"].tobytes())
    said = subprocess.check_output([exe, bam, sam]).decode()
    n_records = int(said.split()[0])
    text = open(sam, "rb").read()
    os.remove(bam)
    os.remove(sam)
    os.rmdir(tmp)
    lines = text.splitlines(keepends=True)
    head = [ln for ln in lines if ln.startswith(b"@")]
    body = lines[len(head):]
    assert len(body) == n_records, (len(body), n_records)
    dest = os.path.join(HERE, "sam_fixture.npz")
    keep = len(body)
    while True:
        np.savez_compressed(dest, sam=np.frombuffer(b"".join(head + body[:keep]), np.uint8), n_lines=np.array(keep, np.int64),
                            n_records=np.array(n_records, np.int64), htslib_version=np.array("1.3 (vendored: kent/src/htslib)"))
        size = os.path.getsize(dest)
        if size <= LIMIT:
            break
        keep = int(keep * 0.9 * LIMIT / size)   # the first lines that fit
    print("wrote %s: %.0f KB, %d header lines, %d of %d alignment lines" % (dest, size / 1e3, len(head), keep, n_records))
    assert size <= LIMIT


if __name__ == "__main__":
    sys.exit(main())
