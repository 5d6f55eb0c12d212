"""Named DEFLATE / BGZF conformance cases for the two inflaters (k_bgzf_inflate on the GPU, the host decoder), built
with tests/deflate_writer.py.  tests/test_inflate_cases.py makes the list trustworthy on the CPU (zlib inflates every
valid member to the modelled payload and refuses every rejected one); tests/test_gpu_inflate.py runs it on the GPU.

A case is one BGZF member: ``Case(name, member, payload, valid, covers, doc)``.  `covers` names the items of the issue's
list that the member holds (a member of the alphabet sweep holds every length symbol, for instance), so that a dropped
item is noticed.  The members of a group ride in ONE BAM file (`group_file`): a zlib-written first member holds the
BAM header and starts a carrier record (placed, unmapped, no CIGAR, l_seq = 0) whose one auxiliary field ``XB:B:C``
is as long as the group's payloads together; the case members follow -- their content is free, and none of them holds
a record start; a last zlib-written member holds a few ordinary records.  Every inflated byte is checked through the
member's CRC-32; the columns that come out are the carrier's and the last member's."""
import collections
import functools
import random
import struct
import zlib

from tests import bam_writer
from tests.deflate_writer import (DIST_BASE, DIST_EXTRA, FIXED_D, FIXED_LL, LEN_BASE, LEN_EXTRA, M, Stream, canonical, chain_lengths,
                                  code_lengths, decode, member, optimal_lengths, random_lengths, subfield, token_symbols)

Case = collections.namedtuple("Case", "name member payload valid covers doc")
REFS, LENS = ["chrA"], [100000]
CARRIER_POS = 100
TAIL = [(0, 200 + 3 * i, [(0, 30)], 16 * (i & 1)) for i in range(5)]     # the ordinary records of the last member


def case(name, stream_or_member, payload=None, valid=True, covers=None, doc=""):
    if isinstance(stream_or_member, Stream):
        payload = bytes(stream_or_member.out) if payload is None else payload
        stream_or_member = stream_or_member.member(payload=payload)
    return Case(name, stream_or_member, bytes(payload), valid, tuple(covers if covers is not None else [name]), doc)


# ---------------------------------------------------------------------------------------------------------------------
# the BAM file around the members

def zmember(data):
    comp = zlib.compressobj(6, zlib.DEFLATED, -15)
    return member(comp.compress(data) + comp.flush(), data)


def lead_payload(n_carried):
    """BAM header + the carrier record up to (not including) the `n_carried` bytes of its XB:B:C array."""
    text = b"@HD\tVN:1.6\tSO:coordinate\n"
    out = b"BAM\x01" + struct.pack("<I", len(text)) + text + struct.pack("<I", len(REFS))
    for nm, ln in zip(REFS, LENS):
        nmb = nm.encode() + b"\x00"
        out += struct.pack("<I", len(nmb)) + nmb + struct.pack("<I", ln)
    assert n_carried + 64 < 1 << 26, "k_bam_chain's plausible_record takes no longer length prefix"
    rec = bam_writer.encode_record(0, CARRIER_POS, [], 4, aux=b"XBBC" + struct.pack("<I", n_carried))
    return out + struct.pack("<I", len(rec) - 4 + n_carried) + rec[4:]


def tail_member():
    return zmember(b"".join(bam_writer.encode_record(t, p, c, f) for t, p, c, f in TAIL))


def group_file(cases):
    """The BAM file that carries the members of `cases` (all valid, or one rejected member among valid ones)."""
    total = sum(len(c.payload) for c in cases)
    return zmember(lead_payload(total)) + b"".join(c.member for c in cases) + tail_member() + bam_writer.BGZF_EOF


def rejected_file(c):
    if c.name == "R.dist.beyond.first":    # the rejected member is the file's first: it holds the BAM header itself
        return c.member + tail_member() + bam_writer.BGZF_EOF
    return group_file([c])


EXPECT_POS = [CARRIER_POS] + [p for _, p, _, _ in TAIL]
EXPECT_FLAG16 = [4] + [f for _, _, _, f in TAIL]


def member_offsets(blob):
    """(file offset, offset of the DEFLATE stream, ISIZE) of every member of a BGZF file."""
    off, out = 0, []
    while off < len(blob):
        xlen = struct.unpack("<H", blob[off + 10:off + 12])[0]
        x, bsize = 0, None
        while x < xlen:
            tag, slen = blob[off + 12 + x:off + 14 + x], struct.unpack("<H", blob[off + 14 + x:off + 16 + x])[0]
            if tag == b"BC":
                bsize = struct.unpack("<H", blob[off + 16 + x:off + 18 + x])[0] + 1
            x += 4 + slen
        out.append((off, off + 12 + xlen, struct.unpack("<I", blob[off + bsize - 4:off + bsize])[0]))
        off += bsize
    return out


# ---------------------------------------------------------------------------------------------------------------------
# building blocks

def rbytes(rng, n, lo=0, hi=255):
    return bytes(rng.randint(lo, hi) for _ in range(n))


def huffman_history(rng, n):
    """Tokens that write >= n bytes of history which is not periodic: random literals, then long matches at varying
    distances (a few hundred bytes of stream for 32 KiB of output)."""
    toks = list(rbytes(rng, 1500))
    size, k = 1500, 0
    while size < n:
        toks.append(M(258 - (k % 5), 700 + (k * 37) % 790))
        size += toks[-1].length
        k += 1
    return toks


def dyn(s, tokens, final=False, **kw):
    ll, dl = optimal_lengths(tokens)
    return s.dynamic(tokens, ll, dl, final=final, **kw)


def length_extremes():
    out = []
    for i in range(29):
        hi = LEN_BASE[i] + (1 << LEN_EXTRA[i]) - 1 - (1 if i == 27 else 0)      # (284 with extra 31 is 258: listed apart)
        out.append(("len%d.min" % (257 + i), LEN_BASE[i], False))
        if i < 28:
            out.append(("len%d.max" % (257 + i), hi, False))
    out.append(("len284.extra31", 258, True))
    return out


def distance_extremes():
    out = []
    for i in range(30):
        out.append(("dist%d.min" % i, DIST_BASE[i]))
        out.append(("dist%d.max" % i, DIST_BASE[i] + (1 << DIST_EXTRA[i]) - 1))
    return out


# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def group_a():
    """A. Alphabet sweep: every length symbol and every distance symbol with its smallest and its largest extra-bit
    value, in a fixed and in a dynamic block, behind a stored block of 32 KiB."""
    out = []
    for kind in ("fixed", "dynamic"):
        for what in ("lengths", "distances"):
            rng = random.Random(len(kind) * 7 + len(what))
            s = Stream().stored(rbytes(rng, 32768))
            toks, covers = [], []
            if what == "lengths":
                for nm, ln, alt in length_extremes():
                    toks += [rng.randint(0, 255), rng.randint(0, 255), M(ln, rng.randint(ln + 1, 30000), alt)]
                    covers.append("%s.%s" % (kind, nm))
            else:
                for nm, d in distance_extremes():
                    toks += [rng.randint(0, 255), M(3 + rng.randint(0, 9), d)]
                    covers.append("%s.%s" % (kind, nm))
            toks += [1, 2, 3]
            s.fixed(toks, final=True) if kind == "fixed" else dyn(s, toks, final=True)
            out.append(case("A.%s.%s" % (kind, what), s, covers=covers))
    return out


B_DIST = list(range(1, 71)) + [127, 128, 129]
B_LEN = [3, 4, 63, 64, 65, 127, 128, 129, 257, 258]


@functools.lru_cache(maxsize=None)
def group_b():
    """B. Overlap matrix: every (distance, length) pair once directly behind literals and once directly behind another
    match (d < len, d = len, d > len); a member per distance and block kind."""
    out = []
    for kind in ("fixed", "dynamic"):
        for d in B_DIST:
            rng = random.Random(1000 + d)
            toks = list(rbytes(rng, d + 3))
            for ln in B_LEN:
                toks += list(rbytes(rng, 5)) + [M(ln, d), M(ln, d)]
            toks += list(rbytes(rng, 4))
            s = Stream()
            s.fixed(toks, final=True) if kind == "fixed" else dyn(s, toks, final=True)
            out.append(case("B.%s.d%d" % (kind, d), s,
                            covers=["%s.d%d.l%d.%s" % (kind, d, ln, w) for ln in B_LEN for w in ("lit", "match")]))
    return out


C_DIST = [1789, 1790, 1791, 1792, 2047, 2048, 2049, 2305, 2306, 3837, 3838, 3839, 4096, 32767, 32768]
C_LEN = [3, 258]
C_PHASE = [0, 1, 15, 16, 17, 511]


@functools.lru_cache(maxsize=None)
def group_c():
    """C. Window edge: distances around the near / far decision of the 2 KiB LDS window (and its multiples, and the
    largest), matches that start at chosen positions mod 512 (the flush piece), history written by a stored block
    and by Huffman blocks.  A member per (history, distance, length) holds the six start positions."""
    out = []
    for hist in ("stored", "huffman"):
        for d in C_DIST:
            for ln in C_LEN:
                rng = random.Random(d * 3 + ln)
                s = Stream()
                if hist == "stored":
                    s.stored(rbytes(rng, 32768 + 7))
                else:
                    dyn(s, huffman_history(rng, 32768 + 7))
                toks, pos, starts = [], len(s.out), []
                for ph in C_PHASE:
                    toks.append(rng.randint(0, 255))
                    pos += 1
                    while pos % 512 != ph:
                        toks.append(rng.randint(0, 255))
                        pos += 1
                    starts.append(pos)
                    toks.append(M(ln, d))
                    pos += ln
                toks += [7, 8, 9]
                first = len(s.trace)
                dyn(s, toks, final=True) if d % 2 else s.fixed(toks, final=True)
                got = [p for t, p, _ in s.trace[first:] if isinstance(t, tuple)]
                assert got == starts and [p % 512 for p in got] == C_PHASE
                out.append(case("C.%s.d%d.l%d" % (hist, d, ln), s,
                                covers=["%s.d%d.l%d.p%d" % (hist, d, ln, ph) for ph in C_PHASE]))
    return out


# the chain codes of group D: a one-bit literal, the end-of-block code in two bits, length symbol 284 and distance
# symbol 29 in 15 bits each
D_LL = chain_lengths([65, 256, 66, 67, 68, 69, 70, 71, 72, 73, 74, 75, 76, 77, 283, 284])
D_DL = chain_lengths(list(range(14)) + [28, 29])


def widest(k):
    """The 48-bit match: 15 bits of length code + 5 extra + 15 bits of distance code + 13 extra."""
    return M(258, 32768, alt=True) if k % 3 == 0 else M(257, 24577 + (k * 2731) % 8192)


@functools.lru_cache(maxsize=None)
def group_d():
    """D. The widest symbol at every bit phase: s one-bit literals, then the 48-bit match, then the end of the block,
    for s in 0..600 -- the match starts at every bit offset of a batch of the kernel's, wherever its batches begin; and
    a second 48-bit match 0..70 one-bit literals behind the first."""
    out = []
    rng = random.Random(4)
    hist_toks = huffman_history(rng, 32768)
    hist_bytes = bytes(decode(hist_toks))
    for s_lits in range(601):
        s = Stream()
        if s_lits % 16 == 0:
            s.stored(hist_bytes[:32768])
        else:
            dyn(s, hist_toks)
        first = len(s.trace)
        b0 = s.bits.bitpos
        s.dynamic([65] * s_lits + [widest(s_lits)], D_LL, D_DL, final=True)
        t, _, bit = s.trace[first + s_lits]
        assert isinstance(t, tuple) and s.bits.bitpos == bit + 48 + 2            # the match is 48 bits, the end-of-block code 2
        assert s_lits == 0 or s.trace[first + 1][2] - s.trace[first][2] == 1
        out.append(case("D.one.s%d" % s_lits, s))
    for gap in range(71):
        s = Stream()
        dyn(s, hist_toks)
        lead = (gap * 29) % 97
        s.dynamic([65] * lead + [widest(gap)] + [65] * gap + [widest(gap + 1)], D_LL, D_DL, final=True)
        out.append(case("D.two.g%d" % gap, s))
    return out


def e_tokens(rng, n=200):
    """Tokens over 16 literals and the length symbols 257..260, every one of them used."""
    toks = list(range(97, 113)) + [M(3, 5), M(4, 9), M(5, 2), M(6, 16)]
    for _ in range(n):
        toks.append(rng.randint(97, 112) if rng.random() < 0.8 else M(rng.randint(3, 6), rng.randint(1, 16)))
    return toks


E_LL = dict([(s, 5) for s in range(97, 113)] + [(256, 2)] + [(s, 4) for s in range(257, 261)])
E_DL = dict((s, 3) for s in range(8))            # distances 1..16


def rle_with(lens, c16=6, c17=10, c18=138):
    """Run-length coding of a code-length list that uses `16` only with count c16, `17` only with c17, `18` only with
    c18 (and plain lengths for what is left)."""
    out, i = [], 0
    while i < len(lens):
        v, j = lens[i], i
        while j < len(lens) and lens[j] == v:
            j += 1
        run = j - i
        if v == 0:
            while run >= c18 >= 11:
                out.append((18, c18))
                run -= c18
            while run >= c17 >= 3:
                out.append((17, c17))
                run -= c17
        else:
            out.append((v,))
            run -= 1
            while run >= c16 >= 3:
                out.append((16, c16))
                run -= c16
        out += [(v,)] * run
        i = j
    return out


def second_level_sizes(ll, root=9):
    """The sizes (in index bits) of the second-level tables a decoder with `root` first-level bits builds."""
    sub = {}
    for s, (c, n) in canonical(ll).items():
        if n > root:
            pre = c >> (n - root)
            sub[pre] = max(sub.get(pre, 0), n - root)
    return sorted(sub.values())


@functools.lru_cache(maxsize=None)
def group_e():
    """E. Header forms of dynamic blocks."""
    out = []
    rng = random.Random(5)

    def add(name, toks, ll, dl, doc="", **kw):
        s = Stream().dynamic(toks, ll, dl, final=True, **kw)
        out.append(case("E." + name, s, doc=doc))
        return s
    toks = e_tokens(rng)
    lens = [E_LL.get(s, 0) for s in range(261)] + [3] * 8
    # HCLEN = 4 gives codes to 16, 17, 18 and 0 alone: every code length is then zero, so no block with HCLEN = 4 has
    # an end-of-block code -- it is in the rejected set; the smallest HCLEN of a valid block is 5 (code length 8 alone)
    ll8 = dict((s, 8) for s in list(range(255)) + [256])
    add("hclen5", list(rbytes(rng, 300, 0, 254)), ll8, {}, cl={0: 1, 8: 1}, rle="none", hdist=1, hclen=5)
    add("hclen19.padded", toks, E_LL, E_DL, hclen=19)
    s = add("hclen19.len15", [65] * 9 + [M(258, 3, alt=True), M(230, 12)], D_LL, D_DL)
    assert any(t[0] == 15 for t in s.cl_symbols)
    add("cl.7bit", toks, E_LL, E_DL, rle=rle_with(lens, 6, 10, 138), cl={0: 1, 5: 2, 4: 3, 3: 4, 2: 5, 16: 6, 17: 7, 18: 7})
    add("hlit257.hdist1", list(rbytes(rng, 200, 97, 112)), dict([(s, 5) for s in range(97, 113)] + [(256, 1)]), {0: 1})
    add("hlit286.padded", toks, E_LL, E_DL, hlit=286)
    t285 = toks + [M(258, 7)]
    ll285 = dict([(s, 5) for s in range(97, 113)] + [(256, 2)] + [(s, 4) for s in (257, 258, 259)] + [(260, 5), (285, 5)])
    add("hlit286.sym285", t285, ll285, E_DL)
    add("hdist30.padded", toks, E_LL, E_DL, hdist=30)
    add("hdist30.sym29", toks + [M(6, 16)] * 5500 + [M(6, 24577 + 8191), M(6, 24577)], E_LL, dict(list(E_DL.items())[:6] + [(6, 4), (7, 4), (28, 4), (29, 4)]))
    for sym, count in ((16, 3), (16, 6), (17, 3), (17, 10), (18, 11), (18, 138)):
        s = add("rle%d.count%d" % (sym, count), toks, E_LL, E_DL, rle=rle_with(lens, *[count if x == sym else 0 for x in (16, 17, 18)]))
        assert (sym, count) in s.cl_symbols and not any(t[0] >= 16 and t != (sym, count) for t in s.cl_symbols)
    # a `16` that starts in the literal/length lengths and ends in the distance lengths: 257..260 have length 4, and
    # so have 16 distance codes
    dl16 = dict((s, 4) for s in range(16))
    head = rle_with([E_LL.get(s, 0) for s in range(257)], 6, 10, 138)
    cross = head + [(4,), (16, 6), (16, 6), (16, 6), (4,)]                      # 257; 258..260 + d0..d2; d3..d8; d9..d14; d15
    add("rle16.across", toks + [M(3, 200)], E_LL, dl16, rle=cross)
    add("rle.none", toks, E_LL, E_DL, rle="none")
    add("dist.single.used", [rng.randint(97, 112) for _ in range(20)] + [M(3, 5), 97, M(6, 6), M(4, 5)] + list(range(97, 113)),
        dict(E_LL), {4: 1}, doc="one distance code of length 1: its code `0` is valid, `1` is not")
    add("dist.all.zero", list(rbytes(rng, 200, 97, 112)) + list(range(97, 113)), dict([(s, 5) for s in range(97, 113)] + [(256, 1)]), {},
        hdist=1, doc="one distance code of length zero (libdeflate before 1.15 for literal-only blocks)")
    # 15-bit codes under several 9-bit prefixes: second-level tables of 2, 2, 4 and 64 entries ...
    multiset = [1, 2, 3, 4, 5, 6, 7] + [10] * 5 + [11] * 3 + [12] * 4 + [13] * 2 + [14] * 3 + [15] * 2
    syms = [256] + list(range(32, 32 + len(multiset) - 1))
    ll = dict(zip(syms, multiset))
    assert second_level_sizes(ll) == [1, 1, 2, 6]
    add("long.prefixes", [rng.choice(syms[1:]) for _ in range(400)] + syms[1:], ll, {})
    # ... and random complete codes over the whole alphabet that reach 15 bits
    k = 0
    for seed in range(1000):
        r = random.Random(seed)
        ll = random_lengths(r, list(range(286)))
        sizes = second_level_sizes(ll)
        if max(ll.values()) == 15 and len(set(sizes)) >= 4:
            dl = random_lengths(r, list(range(30)))
            t = []
            for _ in range(600):
                t.append(r.randint(0, 255) if r.random() < 0.7 else M(r.randint(3, 258), r.randint(1, 256)))
            t = list(range(256)) + [M(ln, 1 + ln % 250) for ln in LEN_BASE] + [M(258, 9, alt=True)] + t
            add("long.random%d" % k, t, ll, dl)
            k += 1
            if k == 4:
                break
    assert k == 4
    return out


def _fixed_block_ending_at(phase, spmod, stored_len, rng):
    """A member: a fixed block that ends at bit `phase` of a byte, a stored block of `stored_len` bytes whose data
    starts at a stream position = spmod (mod 4), a second fixed block."""
    for n8 in range(0, 12):
        for n9 in range(0, 9):
            s = Stream()
            toks = [rng.randint(0, 143) for _ in range(n8)] + [rng.randint(144, 255) for _ in range(n9)] + [M(3, 2)] * 2
            toks = [66, 67, 68] + toks
            s.fixed(toks)
            if s.bits.bitpos % 8 != phase:
                continue
            s.stored(rbytes(rng, stored_len))
            if s.data_pos % 4 != spmod:
                continue
            s.fixed([70, 71, M(5, 4), M(3, len(s.out) + 2), 72], final=True)
            return s
    raise AssertionError("no such block")


@functools.lru_cache(maxsize=None)
def group_f():
    """F. Block sequencing."""
    out = []
    rng = random.Random(6)
    for stored_len, nm in ((0, "empty"), (1, "onebyte")):
        for phase in range(8):
            for spmod in range(4):
                out.append(case("F.stored.%s.bit%d.sp%d" % (nm, phase, spmod), _fixed_block_ending_at(phase, spmod, stored_len, rng)))
    toks = e_tokens(rng)
    s = Stream()
    dyn(s, toks).fixed([]).fixed(toks, final=True)
    out.append(case("F.fixed.empty.middle", s))
    s = Stream()
    dyn(s, toks).fixed([], final=True)
    out.append(case("F.fixed.empty.final", s))
    s = Stream()
    dyn(s, toks).fixed(toks + [M(40, 100)]).stored(rbytes(rng, 700))
    dyn(s, toks + [M(258, 900), M(100, 1500)], final=True)
    out.append(case("F.dynamic.fixed.stored.dynamic", s))
    s = Stream()
    for k in range(1000):
        s.fixed([rng.randint(0, 255)], final=k == 999)
    out.append(case("F.blocks1000", s))
    out.append(case("F.stored.largest", Stream().stored(rbytes(rng, 65536 - 18 - 8 - 5), final=True)))
    s = Stream().stored(rbytes(rng, 5000))
    s.fixed([M(258, 5000), 1, M(3, 5000 + 259), M(258, 5000 + 262 - 1), 2], final=True)
    out.append(case("F.stored.twowindows.match", s))
    # a stored block behind a Huffman block whose last symbols produce most of an LDS window: the batch decoder holds
    # up to 1 790 bytes it has not written out when the stored bytes arrive.  The block is one batch of bit offsets
    # (under 512 bits), so its 1 600 bytes and more are all unflushed at its end, wherever the kernel's batches begin.
    for nlit in (5, 20, 35):
        s = Stream().fixed(list(rbytes(rng, nlit)) + [M(258, nlit - k % 3) for k in range(6)] + [M(52, 3)])
        assert s.bits.bitpos < 512
        s.stored(rbytes(rng, 600)).fixed([M(258, 1500), 3, M(100, 2100)], final=True)
        out.append(case("F.window%d.then.stored" % (1600 + nlit), s))
    return out


def tokens_for(rng, n, alphabet=(0, 255), p_lit=0.5, long_p=0.05):
    """A random token stream of exactly n output bytes, dense in short matches at small and medium distances."""
    toks, pos = [], 0
    while pos < n:
        left = n - pos
        if pos == 0 or left < 3 or rng.random() < p_lit:
            toks.append(rng.randint(*alphabet))
            pos += 1
            continue
        u = rng.random()
        ln = rng.randint(3, 10) if u > long_p else rng.randint(11, 258)
        ln = min(ln, left)
        u = rng.random()
        d = rng.randint(1, 64) if u < 0.5 else (rng.randint(65, 4000) if u < 0.9 else rng.randint(1, 32768))
        d = min(d, pos)
        toks.append(M(ln, d, alt=(ln == 258 and rng.random() < 0.5)))
        pos += ln
    return toks


def write_blocks(s, toks, rng, kinds=("stored", "fixed", "dynamic", "random", "chain"), cuts=None):
    """`toks` into s as blocks of random kinds and lengths (the last one final)."""
    if cuts is None:
        cuts = sorted(set(rng.randrange(1, len(toks)) for _ in range(rng.choice([0, 0, 1, 2, 3, 8])))) if len(toks) > 1 else []
    parts = [toks[a:b] for a, b in zip([0] + cuts, cuts + [len(toks)])]
    for i, part in enumerate(parts):
        final = i == len(parts) - 1
        kind = rng.choice(kinds)
        lf, df = token_symbols(part)
        lu, du = [x for x, c in enumerate(lf) if c], [x for x, c in enumerate(df) if c]
        if kind == "stored":
            data = bytes(decode(part, bytearray(s.out))[len(s.out):])
            if len(data) <= 65535 and len(s.bits.out) + len(data) < 60000:
                s.stored(data, final=final)
                continue
            kind = "dynamic"
        if kind == "chain" and len(lu) <= 16 and len(du) <= 16:
            pad = [x for x in range(286) if not lf[x]]
            rng.shuffle(lu)
            ll = chain_lengths(lu + pad[:16 - len(lu)])
            pad = [x for x in range(30) if not df[x]]
            rng.shuffle(du)
            dl = chain_lengths(du + pad[:16 - len(du)])
            s.dynamic(part, ll, dl, final=final, rle=rng.choice(["none", "greedy"]))
        elif kind in ("random", "chain"):
            extra = [x for x in range(286) if not lf[x]][:rng.randint(1, 20)]
            ll = random_lengths(rng, lu + extra)
            extra = [x for x in range(30) if not df[x]][:rng.randint(2, 6)]
            dl = random_lengths(rng, du + extra)
            s.dynamic(part, ll, dl, final=final, rle=rng.choice(["none", "greedy"]))
        elif kind == "fixed":
            s.fixed(part, final=final)
        else:
            dyn(s, part, final=final)
    return s


G_ISIZE = [1, 2, 15, 16, 17, 63, 64, 65, 1055, 1056, 1057, 2 * 1056, 65535, 65536]


@functools.lru_cache(maxsize=None)
def group_g():
    """G. Member geometry."""
    out = []
    rng = random.Random(7)
    for n in G_ISIZE:
        toks = tokens_for(rng, n, p_lit=0.5 if n < 5000 else 0.1, long_p=0.05 if n < 5000 else 0.5)
        out.append(case("G.isize%d.one" % n, dyn(Stream(), toks, final=True)))
        cuts = sorted(set(rng.randrange(1, len(toks)) for _ in range(9))) if len(toks) > 1 else []
        s = write_blocks(Stream(), toks, rng, cuts=cuts)
        out.append(case("G.isize%d.many" % n, s))
        assert len(out[-1].payload) == len(out[-2].payload) == n
    small = tokens_for(rng, 33)
    out.append(case("G.empty.fixed", member(b"\x03\x00", b""), b""))
    out.append(case("G.between.1", Stream().fixed(small, final=True)))
    out.append(case("G.empty.stored", member(b"\x01\x00\x00\xff\xff", b""), b""))
    out.append(case("G.between.2", Stream().fixed(small, final=True)))
    # other subfields around BC: the DEFLATE stream at every alignment mod 4 of the file image (the members' own lengths
    # move it too; tests/test_inflate_cases.py checks that all four occur)
    for before in (None, 0, 1, 2, 3):
        for after in (None, 0, 1, 3):
            toks = tokens_for(rng, 200 + rng.randint(0, 3))
            s = dyn(Stream(), toks, final=True)
            xb = b"" if before is None else subfield(b"XA", rbytes(rng, before))
            xa = b"" if after is None else subfield(b"ZZ", rbytes(rng, after))
            out.append(case("G.extra.b%s.a%s" % (before, after), s.member(extra=xb, extra_after=xa), bytes(s.out)))
    # payloads of 33 bytes: the members that follow start at every alignment mod 16 of the inflated stream
    for k in range(18):
        out.append(case("G.align16.%d" % k, dyn(Stream(), tokens_for(rng, 33), final=True)))
    out.append(case("G.align16.tail", dyn(Stream(), tokens_for(rng, 3000), final=True)))
    return out


@functools.lru_cache(maxsize=None)
def group_h(seed):
    """H. Random token streams: random block kinds and lengths, optimal, random and chain code lengths, dense in short
    matches at small and medium distances (chains inside the kernel's 64-symbol chunks), payloads of 300 bytes to
    64 KiB."""
    out = []
    rng = random.Random(800 + seed)
    for k in range(200):
        n = 65536 if k == 0 else (300 if k == 1 else int(300 * (65536 / 300.0) ** (rng.random() ** 2.5)))
        small = rng.random() < 0.3
        toks = tokens_for(rng, n, alphabet=(97, 104) if small else (0, 255), p_lit=rng.choice([0.1, 0.3, 0.6]), long_p=rng.choice([0.0, 0.05, 0.3]))
        for attempt in range(8):
            s = write_blocks(Stream(), toks, rng, **({} if attempt < 7 else {"kinds": ("dynamic",)}))
            if len(s.cdata()) + 26 <= 65536:          # (else: incompressible under a costly code -- other blocks then)
                break
        m = s.member()
        out.append(case("H%d.m%d" % (seed, k), m, bytes(s.out)))
        assert len(s.out) == n
    return out


# ---------------------------------------------------------------------------------------------------------------------
# rejected streams

def _fixed_codes():
    return canonical(FIXED_LL), canonical(FIXED_D)


def _fixed_lits(s, data, final=True):
    """Block header of a fixed block and literals (no end of block)."""
    s.bits.put(int(final), 1)
    s.bits.put(1, 2)
    s.symbols(list(data), FIXED_LL, FIXED_D, end=False)


def _raw_fixed_match(s, lsym, lxb, lxv, dsym, dxb, dxv):
    llc, dc = _fixed_codes()
    s.bits.code(*llc[lsym])
    s.bits.put(lxv, lxb)
    s.bits.code(*dc[dsym])
    s.bits.put(dxv, dxb)


def _eob(s):
    s.bits.code(*canonical(FIXED_LL)[256])


@functools.lru_cache(maxsize=None)
def rejected():
    """Streams that an inflater must refuse, each built to reach one check; the kernel's status for it in `doc`.  The
    trailer (CRC-32, ISIZE) is that of the bytes a decoder WITHOUT the check would most likely produce, so that the
    check itself has to refuse the member, not the CRC behind it."""
    out = []
    rng = random.Random(9)
    base = rbytes(rng, 40, 97, 122)

    def add(name, s, payload, doc, **kw):
        cd = s.cdata() if isinstance(s, Stream) else s
        out.append(Case("R." + name, member(cd, payload, **kw), bytes(payload), False, ("R." + name,), doc))
    s = Stream()
    _fixed_lits(s, base, final=False)
    _eob(s)
    s.bits.put(1, 1); s.bits.put(3, 2); s.bits.put(0, 13)
    add("blocktype3", s, base, "kInfBadBlockType")
    s = Stream().fixed(list(base))
    s.bits.put(1, 1); s.bits.put(0, 2); s.bits.align()
    s.bits.put(10, 16); s.bits.put((10 ^ 0xffff) ^ 0x0100, 16); s.bits.out += base[:10]
    add("stored.nlen", s, base + base[:10], "kInfBadStored")
    s = Stream().fixed(list(base))
    s.bits.put(1, 1); s.bits.put(0, 2); s.bits.align()
    s.bits.put(11, 16); s.bits.put(11 ^ 0xffff, 16); s.bits.out += base[:10]
    add("stored.beyond", s, base + base[:10] + b"\x00", "kInfInputOverrun: LEN reaches beyond the compressed data")
    toks = e_tokens(rng)
    for field, nm in ((30, "hlit30"), (31, "hlit31")):
        s = Stream()
        s.bits.put(1, 1); s.bits.put(2, 2)
        s.dynamic_header(E_LL, E_DL, hlit=257 + field, check=False)
        s.symbols(toks, E_LL, E_DL)
        add(nm, s, s.out, "kInfBadCodeLengths: HLIT > 286")
    for field, nm in ((30, "hdist30"), (31, "hdist31")):
        s = Stream()
        s.bits.put(1, 1); s.bits.put(2, 2)
        s.dynamic_header(E_LL, E_DL, hdist=1 + field, check=False)
        s.symbols(toks, E_LL, E_DL)
        add(nm, s, s.out, "kInfBadCodeLengths: HDIST > 30")
    lens = [E_LL.get(x, 0) for x in range(261)] + [3] * 8
    s = Stream()
    s.bits.put(1, 1); s.bits.put(2, 2)
    s.dynamic_header(E_LL, E_DL, rle=[(16, 3)] + rle_with(lens[3:], 6, 10, 138), check=False)
    s.symbols(toks, E_LL, E_DL)
    add("first16", s, s.out, "kInfBadCodeLengths: a repeat of the previous length with no previous length")
    s = Stream()
    s.bits.put(1, 1); s.bits.put(2, 2)
    s.dynamic_header(E_LL, E_DL, rle=rle_with(lens[:-3], 6, 10, 138) + [(16, 4)], check=False)
    s.symbols(toks, E_LL, E_DL)
    add("repeat.past", s, s.out, "kInfBadCodeLengths: a repeat that runs past HLIT + HDIST")
    s = Stream()
    s.bits.put(1, 1); s.bits.put(2, 2)
    ll = dict(E_LL); ll[255] = ll.pop(256)
    s.dynamic_header(ll, E_DL, check=False)
    s.symbols(toks, ll, E_DL, end=False)
    s.bits.put(0, 16)
    add("no256", s, s.out, "kInfBadCodeLengths: no end-of-block code")
    s = Stream()
    s.bits.put(1, 1); s.bits.put(2, 2)
    ll = dict(E_LL); ll[261] = 4
    s.dynamic_header(ll, E_DL, check=False)
    s.symbols(toks, E_LL, E_DL)
    add("ll.over", s, s.out, "kInfOverSubscribed")
    s = Stream()
    s.bits.put(1, 1); s.bits.put(2, 2)
    ll = dict(E_LL); del ll[260]
    t260 = [t for t in toks if not (isinstance(t, tuple) and t.length == 6)]
    s.dynamic_header(ll, E_DL, check=False)
    s.symbols(t260, ll, E_DL)
    add("ll.incomplete", s, s.out, "kInfOverSubscribed (the kernel's one code for a code that is not complete)")
    s = Stream()
    s.bits.put(1, 1); s.bits.put(2, 2)
    dl = {0: 1, 1: 2}
    tt = [t if not isinstance(t, tuple) else M(t.length, 1 + (t.dist & 1)) for t in toks]
    s.dynamic_header(E_LL, dl, check=False)
    s.symbols(tt, E_LL, dl)
    add("dist.incomplete2", s, s.out, "kInfOverSubscribed: two distance codes of lengths 1 and 2")
    s = Stream()
    s.bits.put(1, 1); s.bits.put(2, 2)
    syms = rle_with(lens, 6, 10, 138)
    cl = code_lengths([sum(1 for t in syms if t[0] == x) for x in range(19)], 7)
    cl_over = dict(cl)
    cl_over[[x for x in range(19) if x not in cl][0]] = 7         # one code more than the complete code has room for
    s.dynamic_header(E_LL, E_DL, rle=syms, cl=cl_over, check=False)
    s.symbols(toks, E_LL, E_DL)
    add("cl.over", s, s.out, "kInfOverSubscribed: the code-length code")
    # the unused half of a single one-bit distance code: the valid stream of E.dist.single.used with code `1` for `0`
    s = Stream()
    s.bits.put(1, 1); s.bits.put(2, 2)
    s.dynamic_header(E_LL, {4: 1}, check=False)
    s.symbols([97 + x % 16 for x in base[:20]], E_LL, {4: 1}, end=False)
    llc = canonical(E_LL)
    s.bits.code(*llc[257]); s.bits.put(1, 1); s.bits.put(0, 1)            # length 3, the code `1`, extra bit 0: "distance 5"
    decode([M(3, 5)], s.out)
    s.bits.code(*llc[256])
    add("dist.unusedhalf", s, s.out, "kInfBadSymbol: the code `1` of a single one-bit distance code")
    # HCLEN = 4: no code length but zero can be written, so the block has no end-of-block code (see group E)
    s = Stream()
    s.bits.put(1, 1); s.bits.put(2, 2); s.bits.put(0, 5); s.bits.put(0, 5); s.bits.put(0, 4)
    for v in (0, 0, 1, 1):                    # 16, 17, 18, 0: the codes of `18` and `0`, one bit each
        s.bits.put(v, 3)
    s.bits.code(1, 1); s.bits.put(127, 7); s.bits.code(1, 1); s.bits.put(120 - 11, 7)      # `18` twice: 138 + 120 = 258 zeros
    s.bits.put(0, 16)
    add("hclen4", s, b"\x00", "kInfBadCodeLengths: HCLEN = 4 can only declare zero lengths, so there is no end-of-block code")
    for sym in (286, 287):
        s = Stream()
        _fixed_lits(s, base)
        s.bits.code(*canonical(FIXED_LL)[sym]); s.bits.code(0, 5)
        _eob(s)
        add("fixed%d" % sym, s, base + base[-1:] * 3, "kInfBadSymbol: literal/length symbol %d" % sym)
    for dsym in (30, 31):
        s = Stream()
        _fixed_lits(s, base)
        _raw_fixed_match(s, 257, 0, 0, dsym, 13, 0)
        _eob(s)
        add("fixed.dist%d" % dsym, s, base + base[-1:] * 3, "kInfBadSymbol: distance symbol %d" % dsym)
    # a distance one byte beyond the start of the member: in a later member (the previous member's last byte lies just
    # before it in the inflated stream -- the trailer is that of a decoder which reads it) and in a file's first member
    prev_last = lead_payload(44)[-1:]
    s = Stream()
    _fixed_lits(s, base)
    _raw_fixed_match(s, 258, 0, 0, *_dist_fields(41))
    _eob(s)
    add("dist.beyond.later", s, base + (prev_last + base)[:4], "kInfBadDistance")
    head = lead_payload(200)
    s = Stream()
    _fixed_lits(s, head)
    _raw_fixed_match(s, 258, 0, 0, *_dist_fields(len(head) + 1))
    s.symbols(list(b"\x00" * 196), FIXED_LL, FIXED_D)
    add("dist.beyond.first", s, head + (b"\x00" + head)[:4] + b"\x00" * 196, "kInfBadDistance")
    # output beyond ISIZE by one byte, and one byte short
    s = Stream().fixed(list(base), final=True)
    add("over.literal", s, base[:-1], "kInfOverrun")
    s = Stream().fixed(list(base[:30]) + [M(10, 7)], final=True)
    add("over.match", s, bytes(s.out[:-1]), "kInfOverrun")
    s = Stream().fixed(list(base[:30])).stored(base[:10], final=True)
    add("over.stored", s, bytes(s.out[:-1]), "kInfOverrun")
    s = Stream().fixed(list(base), final=True)
    add("short", s, base + b"\x00", "kInfShort")
    # a stream that ends in the middle of a symbol: the end-of-block code of a fixed block is seven zero bits, cut
    # after its first bits (a decoder that reads zeros behind the end of the data would see it whole); and a literal
    # (nine bits, all ones) cut in the same way
    for n in range(1, 12):
        s = Stream()
        _fixed_lits(s, base[:n])
        if 1 <= s.bits.n <= 4:
            break
    body = s.bits.done()
    assert 8 * len(body) - s.bits.bitpos < 7
    add("ends.in.eob", body, base[:n], "kInfInputOverrun: the data ends inside the end-of-block code")
    s = Stream()
    _fixed_lits(s, base[:n] + b"\xff")
    _eob(s)
    add("ends.in.literal", s.bits.done()[:len(body)], base[:n] + b"\xff", "kInfInputOverrun, kInfBadSymbol or kInfShort: the data ends inside a literal")
    return out


def _dist_fields(d):
    i = max(k for k in range(30) if DIST_BASE[k] <= d)
    return i, DIST_EXTRA[i], d - DIST_BASE[i]


GROUPS = collections.OrderedDict([("A", group_a), ("B", group_b), ("C", group_c), ("D", group_d), ("E", group_e), ("F", group_f),
                                  ("G", group_g), ("H0", functools.partial(group_h, 0)), ("H1", functools.partial(group_h, 1)),
                                  ("H2", functools.partial(group_h, 2))])
