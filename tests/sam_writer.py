"""SAM TEXT twins of what tests/bam_writer.py writes (test infrastructure): the same record tuples and packed arrays as
``write_bam``, ``write_bam_packed`` and ``write_bam_realistic``, written as the text an aligner (or ``samtools view -h``)
would give for them, so that the SAM readers can be pinned against the BAM readers record for record.

Options of every writer: `eol` (``"\\n"`` or ``"\\r\\n"``), `final_newline` (the last line ends with `eol` or not) and
`nh_at` -- where among the optional fields ``NH:i:`` stands: ``"as_is"`` (the order of the BAM record's tags), ``"first"``
or ``"last"``."""
import struct

import numpy as np

CIGAR_OPS = "MIDNSHP=X"

_AUX_SIZE = {b"A": 1, b"c": 1, b"C": 1, b"s": 2, b"S": 2, b"i": 4, b"I": 4, b"f": 4}
_AUX_FMT = {b"c": "<b", b"C": "<B", b"s": "<h", b"S": "<H", b"i": "<i", b"I": "<I", b"f": "<f"}


def aux_text(aux):
    """The optional fields of a BAM record's auxiliary bytes as SAM text fields (htslib's sam_format1 naming: every
    integer type is ``i``).  A field that cannot be sized ends the walk, as htslib's bam_aux_get walk ends there: what
    lies behind it does not exist for a reader, and is not written."""
    out, a = [], 0
    while a + 3 <= len(aux):
        tag, ty = aux[a:a + 2].decode("latin-1"), aux[a + 2:a + 3]
        a += 3
        if ty in _AUX_SIZE:
            sz = _AUX_SIZE[ty]
            if a + sz > len(aux):
                break
            if ty == b"A":
                out.append("%s:A:%s" % (tag, aux[a:a + 1].decode("latin-1")))
            elif ty == b"f":
                out.append("%s:f:%g" % (tag, struct.unpack_from("<f", aux, a)[0]))
            else:
                out.append("%s:i:%d" % (tag, struct.unpack_from(_AUX_FMT[ty], aux, a)[0]))
            a += sz
        elif ty in (b"Z", b"H"):
            z = aux.find(b"\0", a)
            if z < 0:
                break
            out.append("%s:%s:%s" % (tag, ty.decode(), aux[a:z].decode("latin-1")))
            a = z + 1
        elif ty == b"B":
            if a + 5 > len(aux):
                break
            sub = aux[a:a + 1]
            cnt, = struct.unpack_from("<I", aux, a + 1)
            if sub not in _AUX_FMT or a + 5 + cnt * _AUX_SIZE[sub] > len(aux):
                break
            vals = struct.unpack_from("<%d%s" % (cnt, _AUX_FMT[sub][1]), aux, a + 5)
            out.append("%s:B:%s" % (tag, ",".join([sub.decode()] + [("%g" if sub == b"f" else "%d") % v for v in vals])))
            a += 5 + cnt * _AUX_SIZE[sub]
        else:
            break
    return out


def place_nh(fields, nh_at):
    """`fields` with its ``NH:i:`` field (if any) moved to the front or the back."""
    if nh_at == "as_is":
        return fields
    nh = [f for f in fields if f.startswith("NH:i:")]
    rest = [f for f in fields if not f.startswith("NH:i:")]
    if nh_at == "first":
        return nh + rest
    if nh_at == "last":
        return rest + nh
    raise ValueError("nh_at must be 'as_is', 'first' or 'last'")


def header_lines(references, lengths, header_text="@HD\tVN:1.6\tSO:coordinate\n"):
    return [ln for ln in header_text.split("\n") if ln] + ["@SQ\tSN:%s\tLN:%d" % (nm, int(ln)) for nm, ln in zip(references, lengths)]


def record_line(i, rec, references, name=None, mapq=30, nh_at="as_is"):
    tid, pos, cig, flag = rec[:4]
    aux = rec[4] if len(rec) > 4 else b""
    qlen = sum(n for op, n in cig if op in (0, 1, 4, 7, 8))
    if len(rec) > 5:   # (the record tuples of tests/bam_sort_cases.py carry a MAPQ of their own)
        mapq = rec[5]
    fields = [name if name is not None else "r%d" % i, str(int(flag)), references[tid] if tid >= 0 else "*", str(int(pos) + 1), str(mapq),
              "".join("%d%s" % (n, CIGAR_OPS[op]) for op, n in cig) or "*", "*", "0", "0", "A" * qlen if qlen else "*", "*"]
    return "\t".join(fields + place_nh(aux_text(aux), nh_at))


def join_lines(lines, eol="\n", final_newline=True):
    text = eol.join(lines)
    if lines and final_newline:
        text += eol
    return text.encode("latin-1")


def write_sam(path, references, lengths, records, header_text="@HD\tVN:1.6\tSO:coordinate\n", eol="\n", final_newline=True, nh_at="as_is"):
    """The twin of ``bam_writer.write_bam``: records are (tid, pos, cigartuples, flag) or (..., aux bytes); names ``r<i>``,
    MAPQ 30, SEQ ``A`` times the query length."""
    lines = header_lines(references, lengths, header_text) + [record_line(i, r, references, nh_at=nh_at) for i, r in enumerate(records)]
    with open(path, "wb") as fh:
        fh.write(join_lines(lines, eol, final_newline))


def _cigars(packed, gap_ops):
    """CIGAR strings of every record: aligned runs joined by N, or (`gap_ops`) by D where the gap is one position."""
    n = packed.n
    nblk = packed.nblk.astype(np.int64)
    alen = packed.alen.astype(np.int64)
    out = np.char.add(alen.astype("U"), "M").tolist()           # the common record: one run
    wide = {}
    if getattr(packed, "wide_idx", None) is not None and len(packed.wide_idx):
        wide = {int(i): (int(a), int(b)) for i, a, b in zip(packed.wide_idx, packed.wide_alen, packed.wide_nblk)}
    boff = packed.block_offsets() if len(packed.blk_start) else None
    bs, bl = packed.blk_start, packed.blk_len
    for i in sorted(set(np.nonzero(nblk != 1)[0].tolist()) | set(wide)):
        nb = wide[i][1] if i in wide else int(nblk[i])
        if nb <= 1:
            L = wide[i][0] if i in wide else int(alen[i])
            out[i] = "%dM" % L if nb == 1 else "*"
            continue
        o = int(boff[i])
        parts = ["%dM" % bl[o]]
        for j in range(o + 1, o + nb):
            gap = int(bs[j]) - (int(bs[j - 1]) + int(bl[j - 1]))
            parts.append("%d%s%dM" % (gap, "D" if gap_ops and gap == 1 else "N", bl[j]))
        out[i] = "".join(parts)
    return out


def write_sam_packed(path, packed, eol="\n", final_newline=True):
    """The twin of ``bam_writer.write_bam_packed``: name ``r``, MAPQ 30, no sequence, ``<run>M`` joined by ``N``."""
    refs = list(packed.references)
    cig = _cigars(packed, False)
    tid, pos, rev = packed.tid.tolist(), packed.pos.tolist(), (packed.flags & 1).tolist()
    lines = header_lines(refs, packed.lengths)
    lines += ["r\t%d\t%s\t%d\t30\t%s\t*\t0\t0\t*\t*" % (16 if rev[i] else 0, refs[tid[i]], pos[i] + 1, cig[i]) for i in range(packed.n)]
    with open(path, "wb") as fh:
        fh.write(join_lines(lines, eol, final_newline))


def write_sam_realistic(path, packed, seed=5, eol="\n", final_newline=True, nh_at="first", chunk=1 << 20):
    """The twin of ``bam_writer.write_bam_realistic``: a 23-character read name, SEQ of the aligned length, qualities, the
    tags ``NH:i:1`` and ``MD:Z:<n>``, FLAG and MAPQ from the packed file where it carries them; runs joined by ``N`` or (a gap
    of one) ``D``.  Written `chunk` records at a time (tens of millions of records fit a test machine's memory).
    Returns the number of bytes written."""
    rng = np.random.default_rng(seed)
    refs = list(packed.references)
    n = packed.n
    pool_n = 1 << 16
    bases = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, pool_n + 70000)].tobytes().decode()
    quals = np.where(rng.random(pool_n + 70000) < 0.9, ord("F"), np.where(rng.random(pool_n + 70000) < 0.7, ord(":"), ord(","))).astype(np.uint8).tobytes().decode()
    flag16 = getattr(packed, "flag16", None)
    mapq = getattr(packed, "mapq", None)
    cig = _cigars(packed, True)
    eolb = eol.encode()
    tags = ["\t".join(place_nh(["NH:i:1", "MD:Z:%d" % x], nh_at)) for x in range(65536)]   # by aligned length
    total = 0
    with open(path, "wb") as fh:
        head = join_lines(header_lines(refs, packed.lengths, "@HD\tVN:1.6\tSO:coordinate\n@PG\tID:synth\n"), eol, True)
        fh.write(head)
        total += len(head)
        for a in range(0, n, chunk):
            b = min(n, a + chunk)
            tid, pos = packed.tid[a:b].tolist(), packed.pos[a:b].tolist()
            L = packed.alen[a:b].tolist()
            fl = (np.where(packed.flags[a:b] & 1, 16, 0) if flag16 is None else flag16[a:b]).tolist()
            mq = [30] * (b - a) if mapq is None else mapq[a:b].tolist()
            at = rng.integers(0, pool_n, b - a).tolist()
            lines = ["SRR0000000.%012d\t%d\t%s\t%d\t%d\t%s\t*\t0\t0\t%s\t%s\t%s" % (
                a + k, fl[k], refs[tid[k]], pos[k] + 1, mq[k], cig[a + k], bases[at[k]:at[k] + L[k]] or "*", quals[at[k]:at[k] + L[k]] or "*", tags[L[k]])
                for k in range(b - a)]
            blob = eol.join(lines).encode() + (eolb if (b < n or final_newline) else b"")
            fh.write(blob)
            total += len(blob)
    return total
