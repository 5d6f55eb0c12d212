"""A token-level DEFLATE (RFC 1951) and BGZF writer in pure Python (test infrastructure).

zlib is one encoder with fixed habits; the streams that libdeflate, zopfli, igzip or 7-zip write freely -- 15-bit
codes, the 48-bit symbol, odd dynamic headers, empty stored blocks at every bit phase -- have to be built by hand.
Here the caller chooses every token, every code length and every header field:

    s = Stream()
    s.stored(b"history ...")
    s.dynamic([65, 66, M(258, 2), M(258, 32768, alt=True)], ll_lens, d_lens, final=True, hclen=19, rle="none")
    blob = s.member()            # the BGZF member;  s.out is what it must inflate to (the model)

A token is a literal byte (int) or ``M(length 3..258, distance 1..32768)``; ``alt=True`` writes length 258 as symbol
284 with extra bits 31 instead of symbol 285, the one place RFC 1951 offers a choice.  ``s.trace`` holds, for every
token written, ``(token, output position, bit position of its code)``.  Code lengths are any complete prefix code
(``code_lengths``: an optimal one, ``chain_lengths``: 1, 2, ..., 14, 15, 15, ``random_lengths``).  Streams that are
not legal are written through ``s.bits`` (``put`` / ``code``) with the code tables below."""
import collections
import heapq
import struct
import zlib

CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]


class Bits(object):
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, value, nbits):            # LSB first (header fields, extra bits)
        self.acc |= value << self.n
        self.n += nbits
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, c, nbits):               # Huffman codes go MSB first
        self.put(int(format(c, "0%db" % nbits)[::-1], 2), nbits)

    def align(self):                        # zero bits up to the byte boundary
        if self.n:
            self.put(0, 8 - self.n)

    @property
    def bitpos(self):
        return 8 * len(self.out) + self.n

    def done(self):
        if self.n:
            self.out.append(self.acc & 255)
        return bytes(self.out)


def code_lengths(freq, limit):
    """Huffman code lengths (<= limit) for the symbols with freq > 0."""
    f = {s: c for s, c in enumerate(freq) if c}
    while True:
        heap = [(c, s, (s,)) for s, c in f.items()]
        heapq.heapify(heap)
        depth = dict.fromkeys(f, 0)
        if len(heap) == 1:
            depth[heap[0][1]] = 1
        while len(heap) > 1:
            a, b = heapq.heappop(heap), heapq.heappop(heap)
            for s in a[2] + b[2]:
                depth[s] += 1
            heapq.heappush(heap, (a[0] + b[0], min(a[1], b[1]), a[2] + b[2]))
        if max(depth.values()) <= limit:
            return depth
        f = {s: (c + 1) // 2 for s, c in f.items()}


def canonical(lengths):
    codes, code = {}, 0
    for ln in range(1, 16):
        for s in sorted(s for s, l in lengths.items() if l == ln):
            codes[s] = (code, ln)
            code += 1
        code <<= 1
    return codes


def kraft(lengths):
    """Sum of 2^-len over the used symbols, in units of 2^-15 (a complete code: 32768)."""
    return sum(1 << (15 - l) for l in lengths.values() if l)


def _reversed_codes(lengths):
    return {s: (int(format(c, "0%db" % n)[::-1], 2), n) for s, (c, n) in canonical(lengths).items()}


def chain_lengths(symbols):
    """The complete code 1, 2, ..., 14, 15, 15 over exactly 16 symbols, in the order given: the first gets the one-bit
    code, the last two the 15-bit ones."""
    symbols = list(symbols)
    assert len(symbols) == 16 and len(set(symbols)) == 16
    return {s: min(i + 1, 15) for i, s in enumerate(symbols)}


def random_lengths(rng, symbols, limit=15):
    """A random complete prefix code over `symbols` (>= 2 of them): leaves of a code tree split at random
    (`rng`: a random.Random)."""
    symbols = list(symbols)
    assert len(symbols) >= 2
    leaves = [1, 1]
    while len(leaves) < len(symbols):
        ok = [i for i, l in enumerate(leaves) if l < limit]
        i = ok[rng.randrange(len(ok))]
        leaves[i] += 1
        leaves.append(leaves[i])
    rng.shuffle(leaves)
    return dict(zip(symbols, leaves))


M_ = collections.namedtuple("M", "length dist alt")


def M(length, dist, alt=False):
    assert 3 <= length <= 258 and 1 <= dist <= 32768 and (not alt or length == 258)
    return M_(length, dist, alt)


def length_symbol(length, alt=False):
    """(symbol, extra bits, extra value) of a match length; `alt`: 258 as 284 + 31."""
    if length == 258:
        return (284, 5, 31) if alt else (285, 0, 0)
    i = max(k for k in range(28) if LEN_BASE[k] <= length)
    return 257 + i, LEN_EXTRA[i], length - LEN_BASE[i]


def distance_symbol(dist):
    i = max(k for k in range(30) if DIST_BASE[k] <= dist)
    return i, DIST_EXTRA[i], dist - DIST_BASE[i]


_LSYM = [None] * 3 + [length_symbol(l) for l in range(3, 259)]
_DSYM = {}


def _dsym(d):
    r = _DSYM.get(d)
    if r is None:
        r = _DSYM[d] = distance_symbol(d)
    return r


def token_symbols(tokens):
    """The literal/length and the distance symbols a token list uses, with their counts (end of block included)."""
    lf, df = [0] * 286, [0] * 30
    for t in tokens:
        if isinstance(t, tuple):
            lf[length_symbol(t.length, t.alt)[0]] += 1
            df[_dsym(t.dist)[0]] += 1
        else:
            lf[t] += 1
    lf[256] += 1
    return lf, df


def optimal_lengths(tokens):
    """Optimal (15-bit limited) code lengths for a token list: what an ordinary encoder would declare.  A block without
    matches gets one distance code of length 1 that is never used; with one distance symbol, that code and a second."""
    lf, df = token_symbols(tokens)
    if sum(1 for c in lf if c) == 1:
        lf[0 if lf[0] == 0 else 1] = 1
    used = [s for s, c in enumerate(df) if c]
    if len(used) == 0:
        df[0] = 1
    if len(used) <= 1:
        df[1 if df[1] == 0 else 2] = 1
    return code_lengths(lf, 15), code_lengths(df, 15)


def decode(tokens, out=None):
    """The bytes a token list inflates to (appended to `out`, the history, when given)."""
    out = bytearray() if out is None else out
    for t in tokens:
        if isinstance(t, tuple):
            n, d = t.length, t.dist
            assert d <= len(out), "distance beyond the start of the member"
            if d >= n:
                out += out[len(out) - d:len(out) - d + n]
            else:
                pat = bytes(out[len(out) - d:])
                out += (pat * (n // d + 1))[:n]
        else:
            out.append(t)
    return out


FIXED_LL = {s: (8 if s < 144 else 9 if s < 256 else 7 if s < 280 else 8) for s in range(288)}
FIXED_D = {s: 5 for s in range(32)}


def rle_lengths(lens, mode):
    """The code-length symbols for a list of code lengths, as (symbol,) or (16 | 17 | 18, count): `mode` "none" uses no
    repeat code, "greedy" the longest repeat at every place."""
    if mode == "none":
        return [(v,) for v in lens]
    out, i = [], 0
    while i < len(lens):
        v, j = lens[i], i
        while j < len(lens) and lens[j] == v:
            j += 1
        run = j - i
        if v == 0:
            while run >= 11:
                k = min(run, 138)
                out.append((18, k))
                run -= k
            if run >= 3:
                out.append((17, run))
                run = 0
            out += [(0,)] * run
        else:
            out.append((v,))
            run -= 1
            while run >= 3:
                k = min(run, 6)
                out.append((16, k))
                run -= k
            out += [(v,)] * run
        i = j
    return out


def expand_rle(syms):
    lens = []
    for t in syms:
        if t[0] < 16:
            lens.append(t[0])
        elif t[0] == 16:
            assert lens and 3 <= t[1] <= 6
            lens += [lens[-1]] * t[1]
        elif t[0] == 17:
            assert 3 <= t[1] <= 10
            lens += [0] * t[1]
        else:
            assert 11 <= t[1] <= 138
            lens += [0] * t[1]
    return lens


class Stream(object):
    """One raw DEFLATE stream under construction, with its model output."""

    def __init__(self):
        self.bits = Bits()
        self.out = bytearray()
        self.trace = []            # (token, output position, bit position of its code)

    # ---- blocks
    def stored(self, data, final=False, align_bits=0):
        assert len(data) <= 65535
        self.bits.put(int(final), 1)
        self.bits.put(0, 2)
        if self.bits.n:
            self.bits.put(align_bits & ((1 << (8 - self.bits.n)) - 1), 8 - self.bits.n)
        self.bits.put(len(data), 16)
        self.bits.put(len(data) ^ 0xffff, 16)
        self.data_pos = len(self.bits.out)             # byte position of the block's data in the stream
        self.bits.out += data
        self.out += data
        return self

    def fixed(self, tokens, final=False):
        self.bits.put(int(final), 1)
        self.bits.put(1, 2)
        self.symbols(tokens, FIXED_LL, FIXED_D)
        return self

    def dynamic(self, tokens, ll, dl, final=False, **header):
        """`ll`, `dl`: {symbol: code length} of the two alphabets (any complete prefix code; the distance code may also
        be one code of length 1, or nothing at all).  Header options: see dynamic_header."""
        self.bits.put(int(final), 1)
        self.bits.put(2, 2)
        self.dynamic_header(ll, dl, **header)
        self.symbols(tokens, ll, dl)
        return self

    def dynamic_header(self, ll, dl, hlit=None, hdist=None, hclen=None, cl=None, rle="greedy", check=True):
        """HLIT / HDIST (default: the smallest that hold the used symbols), HCLEN (default: the smallest), the
        code-length code's own lengths `cl` ({symbol: 1..7}; default: optimal) and the run-length coding of the list:
        "none", "greedy", or the explicit code-length symbols [(len,), (16, count), (17, count), (18, count), ...]."""
        ll = {s: l for s, l in ll.items() if l}
        dl = {s: l for s, l in dl.items() if l}
        hlit = max(257, max(ll) + 1) if hlit is None else hlit
        hdist = max(1, max(dl) + 1 if dl else 1) if hdist is None else hdist
        lens = [ll.get(s, 0) for s in range(hlit)] + [dl.get(s, 0) for s in range(hdist)]
        if check:
            assert max(ll) < hlit <= 286 and (not dl or max(dl) < hdist) and hdist <= 30
            assert kraft(ll) == 32768 and (kraft(dl) == 32768 or list(dl.values()) in ([], [1])), "not a complete code"
        syms = rle_lengths(lens, rle) if isinstance(rle, str) else list(rle)
        if check:
            assert expand_rle(syms) == lens, "the code-length symbols do not spell the code lengths"
        if cl is None:
            freq = [0] * 19
            for t in syms:
                freq[t[0]] += 1
            if sum(1 for c in freq if c) == 1:
                freq[0 if freq[0] == 0 else 1] = 1          # (zlib takes no incomplete code-length code)
            cl = code_lengths(freq, 7)
        cl = {s: l for s, l in cl.items() if l}
        need = max(i for i, s in enumerate(CL_ORDER) if s in cl) + 1
        hclen = max(need, 4) if hclen is None else hclen
        if check:
            assert 4 <= hclen <= 19 and hclen >= need and max(cl.values()) <= 7 and kraft(cl) == 32768
        b = self.bits
        b.put(hlit - 257, 5)
        b.put(hdist - 1, 5)
        b.put(hclen - 4, 4)
        for s in CL_ORDER[:hclen]:
            b.put(cl.get(s, 0), 3)
        clc = canonical(cl)
        for t in syms:
            b.code(*clc[t[0]])
            if t[0] == 16:
                b.put(t[1] - 3, 2)
            elif t[0] == 17:
                b.put(t[1] - 3, 3)
            elif t[0] == 18:
                b.put(t[1] - 11, 7)
        self.cl_symbols = syms

    def symbols(self, tokens, ll, dl, end=True):
        """The tokens in the codes `ll` / `dl` ({symbol: length}), then the end-of-block code."""
        llc, dc = _reversed_codes(ll), _reversed_codes(dl)
        b, out, trace = self.bits, self.out, self.trace
        put = b.put
        for t in tokens:
            trace.append((t, len(out), 8 * len(b.out) + b.n))
            if isinstance(t, tuple):
                sym, xb, xv = (284, 5, 31) if t.alt else _LSYM[t.length]
                put(*llc[sym])
                if xb:
                    put(xv, xb)
                sym, xb, xv = _dsym(t.dist)
                put(*dc[sym])
                if xb:
                    put(xv, xb)
                decode((t,), out)
            else:
                put(*llc[t])
                out.append(t)
        if end:
            put(*llc[256])

    # ---- the results
    def cdata(self):
        return self.bits.done()

    def member(self, extra=b"", extra_after=b"", payload=None):
        return member(self.cdata(), bytes(self.out) if payload is None else payload, extra, extra_after)


def subfield(tag, data):
    return tag + struct.pack("<H", len(data)) + data


def member(cdata, payload, extra=b"", extra_after=b"", isize=None, crc=None):
    """The BGZF member around a raw DEFLATE stream: gzip header with the `BC` subfield (other subfields before and
    after it: `extra`, `extra_after`, as written by `subfield`), CRC-32 and ISIZE of `payload`."""
    xlen = len(extra) + 6 + len(extra_after)
    bsize = 12 + xlen + len(cdata) + 8
    assert bsize <= 65536, "a BGZF member holds at most 64 KiB"
    header = struct.pack("<BBBBIBBH", 31, 139, 8, 4, 0, 0, 255, xlen) + extra + struct.pack("<BBHH", 66, 67, 2, bsize - 1) + extra_after
    return header + cdata + struct.pack("<II", (zlib.crc32(payload) & 0xffffffff) if crc is None else crc,
                                        len(payload) if isize is None else isize)


def literal_only_dynamic_member(data):
    """One BGZF member whose payload is ONE dynamic DEFLATE block of literals only, declaring HDIST = 1 distance code
    of length ZERO (what libdeflate before 1.15 wrote for such blocks; zlib's inflate_table accepts `max == 0`)."""
    freq = [0] * 257
    for b in data:
        freq[b] += 1
    freq[256] = 1
    s = Stream()
    s.dynamic(list(data), code_lengths(freq, 15), {}, final=True, hlit=257, hdist=1, rle="none")
    cdata = s.cdata()
    assert zlib.decompressobj(-15).decompress(cdata) == data   # zlib itself takes the stream
    return member(cdata, data)
