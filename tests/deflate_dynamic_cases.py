"""What the tests of the encoder's DYNAMIC codes share (test_deflate_dynamic_host.py, test_gpu_deflate_dynamic.py):
``block_tokens`` reads a one-block zlib stream of any BTYPE back into its tokens -- and, for a dynamic block, into the three
length tables its header carries --, the checks every code must pass (complete, within its limit, canonical), an independent
Huffman cost by ``heapq``, and the count vectors of the length function's tests."""
import heapq

import numpy as np

from tests import bigwig_write_cases as wc

CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 30


class BitReader(object):
    def __init__(self, body):
        self.bits = np.unpackbits(np.frombuffer(body, np.uint8), bitorder="little")
        self.at = 0

    def take(self, n):            # n bits, first bit lowest
        v = 0
        for i in range(n):
            v |= int(self.bits[self.at + i]) << i
        self.at += n
        return v

    def symbol(self, table):      # one Huffman code, first bit highest; table: (length, code) -> symbol
        code = 0
        for n in range(1, 16):
            code = (code << 1) | int(self.bits[self.at])
            self.at += 1
            if (n, code) in table:
                return table[(n, code)]
        raise AssertionError("no code of 15 bits or fewer at bit %d" % self.at)


def canonical(lengths):
    """{(length, code): symbol} of RFC 1951 3.2.2."""
    count = [0] * 16
    for n in lengths:
        count[n] += 1
    count[0] = 0
    code, nxt = 0, [0] * 16
    for b in range(1, 16):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    table = {}
    for s, n in enumerate(lengths):
        if n:
            table[(n, nxt[n])] = s
            nxt[n] += 1
    return table


def block_tokens(stream):
    """``(btype, tokens, tables)`` of a zlib stream whose body is one block: tokens as ``wc.fixed_tokens`` gives them (None
    for a stored block); tables: None, or for BTYPE 2 ``(literal/length lengths (HLIT), distance lengths (HDIST),
    code-length code lengths by symbol (19), HCLEN)``.  The body must end in the byte the end of block stands in."""
    body = stream[2:-4]
    r = BitReader(body)
    assert r.take(1) == 1
    btype = r.take(2)
    assert btype in (0, 1, 2)
    if btype == 0:
        n = body[1] | (body[2] << 8)
        assert body[0] == 1 and (body[3] | (body[4] << 8)) == (~n & 0xffff) and len(body) == 5 + n
        return 0, None, None
    tables = None
    if btype == 1:
        lit, dist = canonical(FIXED_LIT), canonical(FIXED_DIST)
    else:
        hlit, hdist, hclen = r.take(5) + 257, r.take(5) + 1, r.take(4) + 4
        assert hlit <= 286 and hdist <= 30
        cl = [0] * 19
        for i in range(hclen):
            cl[CL_ORDER[i]] = r.take(3)
        cl_table = canonical(cl)
        lengths = []
        while len(lengths) < hlit + hdist:
            s = r.symbol(cl_table)
            if s < 16:
                lengths.append(s)
            elif s == 16:
                assert lengths
                lengths += [lengths[-1]] * (3 + r.take(2))
            elif s == 17:
                lengths += [0] * (3 + r.take(3))
            else:
                lengths += [0] * (11 + r.take(7))
        assert len(lengths) == hlit + hdist
        tables = (lengths[:hlit], lengths[hlit:], cl, hclen)
        lit, dist = canonical(tables[0]), canonical(tables[1])
    out = []
    while True:
        sym = r.symbol(lit)
        if sym == 256:
            break
        if sym < 256:
            out.append(("lit", sym))
            continue
        k = sym - 257
        length = wc.LENGTH_BASE[k] + r.take(wc.LENGTH_EXTRA[k])
        d = r.symbol(dist)
        out.append(("match", length, wc.DIST_BASE[d] + r.take(wc.DIST_EXTRA[d])))
    assert (r.at + 7) // 8 == len(body)
    return btype, out, tables


def histograms(tokens):
    """The literal/length (286, the end of block once) and distance (30) counts of a token list."""
    lit, dist = [0] * 286, [0] * 30
    lit[256] = 1
    for t in tokens:
        if t[0] == "lit":
            lit[t[1]] += 1
        else:
            lit[257 + max(k for k in range(29) if wc.LENGTH_BASE[k] <= t[1])] += 1
            dist[max(k for k in range(30) if wc.DIST_BASE[k] <= t[2])] += 1
    return lit, dist


def kraft(lengths, limit):
    """The Kraft sum of the non-zero lengths in units of 2^-limit: a complete code gives exactly 2^limit."""
    return sum(1 << (limit - int(n)) for n in lengths if n)


def huffman_cost(counts):
    """The cost (sum of count x length) of an optimal prefix code of the counts above 0 (two or more), by heapq: the sum of
    the weights of the internal nodes."""
    heap = [int(c) for c in counts if c]
    assert len(heap) >= 2
    heapq.heapify(heap)
    cost = 0
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        cost += a + b
        heapq.heappush(heap, a + b)
    return cost


def padded(counts):
    """The counts as the encoder pads them: the lowest-numbered zeros count 1 until two symbols are used."""
    c = [int(x) for x in counts]
    for s in range(len(c)):
        if sum(1 for x in c if x) >= 2:
            break
        if not c[s]:
            c[s] = 1
    return c


def check_lengths(counts, lengths, limit):
    """What the length function promises for `counts`: used symbols (after padding) and only they get a length, within the
    limit; the code is complete; length never grows with (count, symbol); and when no length reached the limit the cost is
    the optimal one."""
    c = padded(counts)
    lengths = [int(x) for x in lengths]
    assert len(lengths) == len(c)
    assert all((n > 0) == (w > 0) for n, w in zip(lengths, c))
    assert max(lengths) <= limit
    assert kraft(lengths, limit) == 1 << limit
    order = sorted((w, s) for s, w in enumerate(c) if w)
    along = [lengths[s] for _, s in order]
    assert all(a >= b for a, b in zip(along, along[1:]))
    if max(lengths) < limit:
        assert sum(w * n for w, n in zip(c, lengths)) == huffman_cost(c)


def fibonacci(n, first=1):
    out = [first, first]
    while len(out) < n:
        out.append(out[-1] + out[-2])
    return out[:n]


def length_cases():
    """name -> (counts, limit): Fibonacci counts, whose Huffman tree is a chain as deep as the alphabet, past both limits;
    equal counts; one and no used symbol; random counts of several shapes."""
    rng = np.random.default_rng(4711)
    out = {}
    out["fib32_15"] = (fibonacci(32), 15)                                  # depth 31 under 15
    out["fib40_in_286_15"] = ([0] * 100 + fibonacci(40) + [0] * 146, 15)     # depth 39, zeros around
    shuffled = fibonacci(36)
    rng.shuffle(shuffled)
    out["fib36_shuffled_15"] = ([int(x) for x in shuffled], 15)
    out["fib19_7"] = (fibonacci(19), 7)                                    # depth 18 under 7
    out["fib17_7"] = (fibonacci(17), 7)
    out["fib17_15"] = (fibonacci(17), 15)                                  # depth 16: one level past the limit
    out["fib16_15"] = (fibonacci(16), 15)                                  # depth 15: the limit reached, nothing to repair
    out["equal286_15"] = ([7] * 286, 15)
    out["equal256_15"] = ([1] * 256, 15)
    out["equal19_7"] = ([3] * 19, 7)
    out["equal128_7"] = ([1] * 128, 7)                                     # 2^limit symbols: every length is the limit
    out["equal30_5"] = ([2] * 30, 5)
    out["one_used_30"] = ([0] * 7 + [12] + [0] * 22, 15)
    out["one_used_first"] = ([5] + [0] * 18, 7)
    out["none_used_286"] = ([0] * 286, 15)
    out["none_used_2"] = ([0, 0], 1)
    out["two_symbols"] = ([9, 1], 1)
    for k in range(6):
        n = int(rng.integers(2, 287))
        out["random%d" % k] = ([int(x) for x in rng.integers(0, 1000, n) * (rng.random(n) < 0.7)], 15)
    out["geometric286_15"] = ([int(x) for x in rng.geometric(0.0005, 286)], 15)
    out["powers30_15"] = ([1 << k for k in range(30)], 15)
    out["powers19_7"] = ([1 << k for k in range(19)], 7)
    out["skewed19_7"] = ([int(x) for x in rng.integers(1, 5, 19) ** 8], 7)
    out["large_counts"] = ([(1 << 32) // 300] * 286, 15)
    return out
