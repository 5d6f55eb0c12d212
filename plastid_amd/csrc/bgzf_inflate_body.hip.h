// The body of the inflate kernels of bam_kernels.hip.h, included once per kernel: k_bgzf_inflate<BATCH> (ZLIB = false) and
// k_zlib_inflate (BATCH = true, ZLIB = true).  It is text, not a function: a shared __device__ function, inlined, did not
// compile to the instructions k_bgzf_inflate had, and a second template parameter would rename that kernel.  Expects the
// kernel's arguments (image, members, first_member, nmembers, out, status) and the constants BATCH and ZLIB in scope.
// No include guard: it is meant to be included more than once.
    __shared__ __attribute__((aligned(16))) InflateShared sh;
    __shared__ __attribute__((aligned(16))) union { HeaderShared hdr; BatchShared bat; } su;
    uint8_t *const s_lens = su.hdr.lens;
    TableScratch &s_ws = su.hdr.ws;
    const int m = first_member + (int)blockIdx.x;   // (the members of one upload piece: pc_bam_open)
    if (m >= nmembers) return;
    if (PC_BGZF_SKIP & 32) { if (threadIdx.x == 0) status[m] = 0u; return; }   // (experiment: the lap without the kernel = the upload)
    const Member mb = members[m];   // (uniform: scalar loads)
    const int lane = threadIdx.x & 63;
    const uint8_t *src = image + mb.coff;
    uint8_t *dst = out + mb.uoff;
    const uint32_t clen = mb.clen, ulen = mb.ulen;
    int err = kInfOk;

    // ---- input: `in` holds the kInBytes of the stream around the read position (ring); refilled a half at a time by
    // the wave when the reader has crossed into the other half (256 bytes: a batch looks 84 bytes ahead of its first bit,
    // and a half is staged before the reader comes within 8 bytes of the staged end -- both fit 128-byte halves)
    uint32_t in_pos = 0;          // next byte of the stream to pull into the bit buffer (always a multiple of 4)
    uint32_t in_loaded = 0;       // bytes of the stream staged so far (multiple of kInHalf)
    auto stage_half = [&]() {     // stage stream bytes [in_loaded, in_loaded + kInHalf)
        const uint32_t base = in_loaded;
        // dwords assembled byte-wise (the stream starts at an arbitrary byte of the image)
        for (int k = lane; k < (int)kInHalf / 4; k += 64) {
            const uint32_t b = base + 4u * (uint32_t)k;
            uint32_t w = 0;
            if (b + 3u < clen) w = (uint32_t)src[b] | ((uint32_t)src[b + 1] << 8) | ((uint32_t)src[b + 2] << 16) | ((uint32_t)src[b + 3] << 24);
            else {
                if (b < clen) w |= (uint32_t)src[b];
                if (b + 1u < clen) w |= (uint32_t)src[b + 1] << 8;
                if (b + 2u < clen) w |= (uint32_t)src[b + 2] << 16;
            }
            sh.in[((base >> 2) + (uint32_t)k) & (kInBytes / 4 - 1)] = w;
        }
        in_loaded += kInHalf;
        __syncthreads();
    };
    stage_half();
    stage_half();
    unsigned long long bb = 0;    // bit buffer
    int nb = 0;                   // valid bits in it
    auto refill = [&]() {         // at least 32 valid bits afterwards (zeros behind the end of the stream)
        if (nb <= 32) {
            // Stage the next half only when the reader is within kInHalf - 8 bytes of the staged end: staging overwrites the
            // ring slots of [in_loaded - kInBytes, in_loaded - kInHalf), and the 8 bytes below in_pos must stay in the ring --
            // the bit buffer may still hold up to 64 unread bits of them when the batch decoder takes over and re-reads the
            // stream from its bit position p = 8 in_pos - nb (invariant: in_pos - 8 >= in_loaded - kInBytes whenever a
            // block's symbols start).  (Zeros behind the end of the stream.)
            if (in_pos + kInHalf - 8u >= in_loaded) stage_half();
            // (every lane reads the same word: readfirstlane tells the compiler so, and what follows stays on the scalar unit)
            const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)sh.in[(in_pos >> 2) & (kInBytes / 4 - 1)]);
            bb |= (unsigned long long)w << nb;
            nb += 32;
            in_pos += 4u;
        }
    };
    auto take = [&](int n) -> uint32_t {   // n <= 16
        const uint32_t v = (uint32_t)bb & ((1u << n) - 1u);
        bb >>= n;
        nb -= n;
        return v;
    };

    uint32_t pos = 0;             // bytes produced
    uint32_t flushed = 0;         // bytes written to HBM
    auto flush_to = [&](uint32_t upto) {   // window bytes [flushed, upto) -> HBM; both multiples of 16 except at the very end
        __syncthreads();
        if (PC_BGZF_SKIP & 8) { flushed = upto; return; }
        for (uint32_t b = flushed + 16u * (uint32_t)lane; b < upto; b += 16u * 64u) {
            if (b + 16u <= upto && ((mb.uoff + b) & 15u) == 0u) {
                const uint4 v = *(const uint4 *)&sh.win[b & (kWinBytes - 1)];
                *(uint4 *)(dst + b) = v;
            } else {
                for (uint32_t k = b; k < upto && k < b + 16u; ++k) dst[k] = sh.win[k & (kWinBytes - 1)];
            }
        }
        flushed = upto;
    };

    bool last = false;
    while (!last && err == kInfOk) {
        refill();
        last = take(1) != 0u;
        const uint32_t type = take(2);
        if (type == 0u) {
            // stored block: skip to the byte boundary, LEN / NLEN, raw bytes
            take(nb & 7);
            refill();
            const uint32_t len = take(16);
            refill();
            const uint32_t nlen = take(16);
            if ((len ^ 0xffffu) != nlen) { err = kInfBadStored; break; }
            if (pos + len > ulen) { err = kInfOverrun; break; }
            // the bit buffer holds whole bytes now: give them back to the stream position
            uint32_t sp = in_pos - (uint32_t)(nb >> 3);
            bb = 0; nb = 0;
            if (sp + len > clen) { err = kInfInputOverrun; break; }
            // (a stored block can be twice the window: copied and flushed piece by piece.  The last batch of a Huffman block
            // may leave up to kWinBytes - 258 bytes unflushed -- a piece on top of that would wrap around the window onto
            // them, so they go out first.)
            if (len != 0u && pos - flushed >= (uint32_t)kFlush) flush_to(pos & ~15u);
            for (uint32_t done = 0; done < len;) {
                const uint32_t piece = len - done < (uint32_t)kFlush ? len - done : (uint32_t)kFlush;
                for (uint32_t k = lane; k < piece; k += 64) sh.win[(pos + k) & (kWinBytes - 1)] = src[sp + done + k];
                __syncthreads();
                pos += piece;
                done += piece;
                while (pos - flushed >= (uint32_t)kFlush + 16u) flush_to((flushed + kFlush) & ~15u);
            }
            sp += len;
            // restart the staged input at the new position (dword aligned below it; the odd bytes are dropped from the bit buffer)
            in_pos = sp & ~3u;
            in_loaded = in_pos & ~(kInHalf - 1u);
            stage_half();
            stage_half();
            refill();
            take((int)((sp & 3u) * 8u));
            continue;
        }
        if (type == 3u) { err = kInfBadBlockType; break; }
        if (type == 1u) {
            // fixed Huffman codes (RFC 1951 3.2.6)
            for (int s = lane; s < 288; s += 64) s_lens[s] = s < 144 ? 8 : (s < 256 ? 9 : (s < 280 ? 7 : 8));
            __syncthreads();
            err = build_table<0>(s_lens, 288, kLitRoot, sh.lit, kLitEntries, &s_ws, lane);
            if (err) break;
            for (int s = lane; s < 32; s += 64) s_lens[s] = 5;
            __syncthreads();
            err = build_table<1>(s_lens, 32, kDistRoot, sh.dist, kDistEntries, &s_ws, lane);   // (32 five-bit codes: 30 and 31 never valid)
            if (err) break;
        } else {
            // dynamic codes: HLIT, HDIST, HCLEN, the code-length code, then the two length lists (RFC 1951 3.2.7)
            refill();
            const int hlit = (int)take(5) + 257, hdist = (int)take(5) + 1, hclen = (int)take(4) + 4;
            if (hlit > 286 || hdist > 30) { err = kInfBadCodeLengths; break; }
            if (lane < 19) s_lens[lane] = 0;
            __syncthreads();
            for (int i = 0; i < hclen; ++i) {
                refill();
                const uint32_t v = take(3);
                if (lane == 0) s_lens[kClOrder[i]] = (uint8_t)v;
            }
            __syncthreads();
            // the code-length code (19 symbols, lengths <= 7) decodes through a 7-bit table in the distance table's space
            err = build_table<2>(s_lens, 19, 7, sh.dist, kDistEntries, &s_ws, lane);
            if (err) break;
            int got = 0, prev = 0;
            const int want = hlit + hdist;
            while (got < want && err == kInfOk) {
                refill();
                const uint32_t ce = (uint32_t)__builtin_amdgcn_readfirstlane((int)sh.dist[(uint32_t)bb & 127u]);
                const int len = (int)ent_bits(ce), sym = (int)(ce >> 4);
                if (len == 0) { err = kInfBadCodeLengths; break; }
                take(len);
                int rep = 1, val = sym;
                if (sym == 16) { if (got == 0) { err = kInfBadCodeLengths; break; } rep = 3 + (int)take(2); val = prev; }
                else if (sym == 17) { rep = 3 + (int)take(3); val = 0; }
                else if (sym == 18) { rep = 11 + (int)take(7); val = 0; }
                if (got + rep > want) { err = kInfBadCodeLengths; break; }
                if (lane == 0) for (int k = 0; k < rep; ++k) s_lens[32 + got + k] = (uint8_t)val;   // (kept clear of the 19 code-length lengths)
                got += rep;
                prev = val;
            }
            if (err) break;
            __syncthreads();
            if (s_lens[32 + 256] == 0) { err = kInfBadCodeLengths; break; }     // no end-of-block code
            err = build_table<0>(s_lens + 32, hlit, kLitRoot, sh.lit, kLitEntries, &s_ws, lane);
            if (err) break;
            // the distance lengths follow the literal/length ones: move them to a 4-byte aligned place of their own
            uint8_t dl = (lane < hdist) ? s_lens[32 + hlit + lane] : 0;
            __syncthreads();
            if (lane < 32) s_lens[lane] = dl;
            __syncthreads();
            err = build_table<1>(s_lens, hdist, kDistRoot, sh.dist, kDistEntries, &s_ws, lane);
            if (err) break;
        }
        // ---- the symbols of the block
        if constexpr (BATCH) {
            BatchShared &bs = su.bat;
            uint32_t p = in_pos * 8u - (uint32_t)nb;       // bit position of the next symbol in the stream
            bool eob = false;
            while (!eob) {
                if (pos - flushed >= (uint32_t)kFlush) flush_to(pos & ~15u);
                // what the batch may produce: everything unflushed plus a maximal match stays inside the LDS window, so that
                // a match source is either whole in the window or whole in what has been flushed
                const uint32_t cap = flushed + (uint32_t)kWinBytes - 258u;
                const uint32_t limit = cap < ulen ? cap : ulen;
                if ((p >> 3) > clen + 8u) { err = kInfInputOverrun; break; }
                while (in_loaded < (p >> 3) + 84u) stage_half();
                __syncthreads();
                // ---- every bit offset's symbol: lane l looks at offsets 8 l .. 8 l + 7
                {
                    const uint32_t a = p + 8u * (uint32_t)lane;
                    const uint32_t di = a >> 5, s0 = a & 31u;
                    const uint32_t d0 = sh.in[di & (kInBytes / 4 - 1)], d1 = sh.in[(di + 1u) & (kInBytes / 4 - 1)];
                    const uint32_t d2 = sh.in[(di + 2u) & (kInBytes / 4 - 1)], d3 = sh.in[(di + 3u) & (kInBytes / 4 - 1)];
                    // the 96 bits from the lane's first offset on
                    const uint32_t A = (uint32_t)((((unsigned long long)d1 << 32) | d0) >> s0), B = (uint32_t)((((unsigned long long)d2 << 32) | d1) >> s0);
                    const uint32_t C = (uint32_t)((((unsigned long long)d3 << 32) | d2) >> s0);
                    uint32_t sy[8];
                    if (PC_BGZF_SKIP & 16) { for (int t = 0; t < 8; ++t) sy[t] = (8u << 2) | ((A >> t) & 0xff00u); }   // (experiment: no lookup -- every offset an 8-bit literal)
                    else symbols_at8(sh.lit, sh.dist, A, B, C, sy);
                    *(uint4 *)&bs.sym[8 * lane] = make_uint4(sy[0], sy[1], sy[2], sy[3]);
                    *(uint4 *)&bs.sym[8 * lane + 4] = make_uint4(sy[4], sy[5], sy[6], sy[7]);
                }
                __syncthreads();
                // ---- which offsets are symbol starts: the walk from offset 0.  It does not look at what it passes: behind an
                // end-of-block code or a symbol that is none it walks on through entries read with the wrong tables (every
                // entry consumes at least a bit, so it ends), and the stage below stops at the first such symbol.
                uint32_t walk, nsym;
                {
                    // seven instructions per symbol (twelve with a scalar bit count and a test for the stop symbols), one LDS
                    // read on the dependent chain; every lane stores the same value to the same place (no mask to set up)
                    uint32_t va = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint32_t *)bs.sym;
                    const uint32_t vn0 = va, vend = va + 4u * (uint32_t)kBatchBits;   // (the chain is written over the offset table: see BatchShared)
                    uint32_t vn = vn0, vs;
                    asm volatile("1:\n\t"
                                 "ds_read_b32 %[vs], %[va]\n\t"
                                 "s_waitcnt lgkmcnt(0)\n\t"
                                 "ds_write_b32 %[vn], %[vs]\n\t"
                                 "v_add_u32 %[vn], 4, %[vn]\n\t"
                                 "v_add_u32_sdwa %[va], %[va], %[vs] dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_0\n\t"
                                 "v_cmp_gt_u32 vcc, %[vend], %[va]\n\t"
                                 "s_cbranch_vccnz 1b\n\t"
                                 "s_waitcnt lgkmcnt(0)"
                                 : [va] "+v"(va), [vn] "+v"(vn), [vs] "=&v"(vs)
                                 : [vend] "v"(vend)
                                 : "vcc", "memory");
                    nsym = (uint32_t)__builtin_amdgcn_readfirstlane((int)(vn - vn0)) >> 2;
                    walk = (uint32_t)__builtin_amdgcn_readfirstlane((int)(va - vn0)) >> 2;
                }
                __syncthreads();
                // ---- per symbol, 64 at a time
                uint32_t done = 0;            // bytes produced by the chunks before
                uint32_t p_next = walk;       // where the next batch starts (bits from p), unless a symbol stops this one
                bool stopped = false;
                uint32_t bits = 0;            // bits consumed by the chunks before
                for (uint32_t c0 = 0; c0 < nsym && !stopped; c0 += 64) {
                    const uint32_t idx = c0 + (uint32_t)lane;
                    const bool have = idx < nsym;
                    const uint32_t sv = have ? bs.sym[idx] : 0u;
                    const uint32_t ol = !have ? 0u : (sym_is_lit(sv) ? 1u : (sym_is_match(sv) ? ((sv >> 8) & 255u) + 3u : 0u));
                    // one prefix sum for both: bytes produced (bits 0-15; <= 64 x 258) and bits consumed (16-31; <= 64 x 48)
                    const uint32_t mine = ol | ((sv & 0xfcu) << 14);   // (sv = 0 without a symbol)
                    uint32_t incl2 = mine;
#pragma unroll
                    for (int d = 1; d < 64; d <<= 1) {
                        const uint32_t y = (uint32_t)__shfl_up((int)incl2, d, 64);
                        if (lane >= d) incl2 += y;
                    }
                    const uint32_t incl = incl2 & 0xffffu;
                    const uint32_t off = bits + ((incl2 - mine) >> 16);
                    const uint32_t chunk_start = pos + done;
                    const uint32_t q = chunk_start + incl - ol, end = chunk_start + incl;
                    const unsigned long long stopm = __ballot(have && (sym_is_special(sv) || end > limit));
                    const int first = stopm ? __builtin_ctzll(stopm) : 64;
                    const uint32_t chunk_bytes = first < 64 ? (uint32_t)__builtin_amdgcn_readlane((int)(incl - ol), first) : (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
                    const uint32_t chunk_end = chunk_start + chunk_bytes;
                    const bool emit = have && lane < first;
                    if (!(PC_BGZF_SKIP & 4) && emit && sym_is_lit(sv)) sh.win[q & (kWinBytes - 1)] = (uint8_t)(sv >> 8);
                    // ---- matches: those whose source lies before the chunk are independent of one another (one per lane);
                    // those that read what this chunk writes follow in stream order, each copied by the whole wave
                    const bool ism = emit && sym_is_match(sv);
                    const uint32_t len = ol, dd = ((sv >> 16) & 0x7fffu) + 1u;
                    if (__ballot(ism && dd > q) != 0ull) { err = kInfBadDistance; break; }
                    const uint32_t src = q - dd;
                    const bool dep = ism && src + len > chunk_start;
                    const bool far = ism && chunk_end - src > (uint32_t)kWinBytes;     // (whole in what has been flushed: see `cap`)
                    if (__ballot(far) != 0ull) __builtin_amdgcn_s_waitcnt(0);         // the flush stores have landed
                    __syncthreads();
                    // The independent matches of the chunk, by OUTPUT BYTE: a lane per byte, 64 bytes a round.  (One lane per
                    // match, copying its own bytes, ran every lane for as long as the longest match of the chunk lasted -- with
                    // read names, quality runs and tags that is often a hundred bytes and more: 16 of the kernel's 42 ms on records as
                    // an aligner writes them, scripts/exp_bam_sections.py.)  Which symbol a byte belongs to: the symbols' first
                    // bytes are marked in 64 flag bytes (the offset table of the batch is free by now), and a byte's owner is the
                    // number of marks up to it -- a ballot and a population count; the owner's source and start come by lane permute.
                    if (!(PC_BGZF_SKIP & 1) && __ballot(ism && !dep) != 0ull) {
                        uint8_t *marks = (uint8_t *)bs.sym;   // (entries 0 .. 15 of the chain: this chunk's symbols are in registers, later chunks read from entry 64 on)
                        const uint32_t startrel = emit ? q - chunk_start : 0xffffu;
                        const uint32_t info = (startrel & 0xffffu) | ((ism && !dep) ? 1u << 16 : 0u) | (far ? 1u << 17 : 0u);
                        for (uint32_t base = 0; base < chunk_bytes; base += 64u) {
                            marks[lane] = 0;
                            __syncthreads();
                            if (emit && ol != 0u && startrel >= base && startrel < base + 64u) marks[startrel - base] = 1;
                            __syncthreads();
                            const unsigned long long mk = __ballot(marks[lane] != 0);
                            const uint32_t before = (uint32_t)__popcll(__ballot(emit && ol != 0u && startrel < base));
                            const uint32_t owner = before + (uint32_t)__popcll(mk & (~0ull >> (63 - lane))) - 1u;   // (the chunk's first symbol starts at its byte 0)
                            const uint32_t o_src = (uint32_t)__shfl((int)src, (int)(owner & 63u), 64);
                            const uint32_t o_info = (uint32_t)__shfl((int)info, (int)(owner & 63u), 64);
                            const uint32_t x = base + (uint32_t)lane;
                            if (x < chunk_bytes && ((o_info >> 16) & 1u)) {
                                const uint32_t from = o_src + (x - (o_info & 0xffffu));
                                const uint8_t b = ((o_info >> 17) & 1u) ? __hip_atomic_load(dst + from, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)   // (past this CU's L1, which may hold an older state of the line)
                                                                        : sh.win[from & (kWinBytes - 1)];
                                sh.win[(chunk_start + x) & (kWinBytes - 1)] = b;
                            }
                            __syncthreads();
                        }
                    }
                    __syncthreads();
                    unsigned long long dm = (PC_BGZF_SKIP & 2) ? 0ull : __ballot(dep);
                    while (dm) {
                        const int l = __builtin_ctzll(dm);
                        dm &= dm - 1ull;
                        const uint32_t q1 = (uint32_t)__builtin_amdgcn_readlane((int)q, l), len1 = (uint32_t)__builtin_amdgcn_readlane((int)len, l);
                        const uint32_t dd1 = (uint32_t)__builtin_amdgcn_readlane((int)dd, l);
                        // byte k comes from `dd1` back; where the match overlaps itself the pattern repeats
                        for (uint32_t k = (uint32_t)lane; k < len1; k += 64u) {
                            const uint32_t from = dd1 >= len1 ? q1 - dd1 + k : q1 - dd1 + (k % dd1);
                            sh.win[(q1 + k) & (kWinBytes - 1)] = sh.win[from & (kWinBytes - 1)];
                        }
                        __syncthreads();
                    }
                    done += chunk_bytes;
                    bits += (uint32_t)__builtin_amdgcn_readlane((int)incl2, 63) >> 16;
                    if (first < 64) {         // the symbol that ends the batch: end of block, none at all, or one that does not fit
                        const uint32_t o1 = (uint32_t)__builtin_amdgcn_readlane((int)off, first);
                        const uint32_t e1 = (uint32_t)__builtin_amdgcn_readlane((int)end, first), s1 = (uint32_t)__builtin_amdgcn_readlane((int)sv, first);
                        stopped = true;
                        if (sym_is_special(s1) && (s1 & kSymBadBit)) err = kInfBadSymbol;
                        else if (sym_is_special(s1)) { eob = true; p_next = o1 + sym_bits(s1); }
                        else if (e1 > ulen) err = kInfOverrun;
                        else p_next = o1;
                    }
                }
                if (err) break;
                pos += done;
                p += p_next;
            }
            if (err) break;
            // hand the stream position back to the uniform reader (block headers, stored blocks)
            __syncthreads();
            in_pos = (p >> 5) << 2;
            bb = 0; nb = 0;
            refill();
            { const int r = (int)(p & 31u); bb >>= r; nb -= r; }
        } else {
            for (;;) {
                refill();
                uint32_t e = (uint32_t)__builtin_amdgcn_readfirstlane((int)sh.lit[(uint32_t)bb & ((1u << kLitRoot) - 1u)]);
                if (ent_is_ptr(e)) {
                    const uint32_t sb = ent_bits(e);
                    e = (uint32_t)__builtin_amdgcn_readfirstlane((int)sh.lit[ent_ptr_start(e) + (((uint32_t)(bb >> kLitRoot)) & ((1u << sb) - 1u))]);
                    bb >>= kLitRoot; nb -= kLitRoot;
                }
                const uint32_t nbits = ent_bits(e);
                if (nbits == 0u) { err = kInfBadSymbol; break; }
                bb >>= nbits; nb -= (int)nbits;
                if (!(e & (kEntLen | kEntSpecial))) {     // literal
                    if (pos >= ulen) { err = kInfOverrun; break; }
                    if (lane == 0) sh.win[pos & (kWinBytes - 1)] = (uint8_t)ent_v8(e);
                    pos += 1u;
                } else if (!(e & kEntLen)) {              // end of block
                    if (e & kEntBadBit) err = kInfBadSymbol;
                    break;
                } else {                                  // length + distance
                    refill();
                    const uint32_t len = 3u + ent_v8(e) + take((int)((e >> 12) & 7u));
                    refill();
                    uint32_t d = (uint32_t)__builtin_amdgcn_readfirstlane((int)sh.dist[(uint32_t)bb & ((1u << kDistRoot) - 1u)]);
                    if (d & kEntPtr) {
                        const uint32_t sb = ent_bits(d);
                        d = (uint32_t)__builtin_amdgcn_readfirstlane((int)sh.dist[ent_ptr_start(d) + (((uint32_t)(bb >> kDistRoot)) & ((1u << sb) - 1u))]);
                        bb >>= kDistRoot; nb -= kDistRoot;
                    }
                    const uint32_t dbits = ent_bits(d);
                    if (dbits == 0u || (d & (kEntPtr | kEntSpecial)) != 0u) { err = kInfBadSymbol; break; }
                    bb >>= dbits; nb -= (int)dbits;
                    refill();
                    const uint32_t dxb = (d >> 4) & 15u;
                    const uint32_t dist = 1u + (((d >> 8) & 3u) << dxb) + take((int)dxb);
                    if (dist > pos) { err = kInfBadDistance; break; }
                    if (pos + len > ulen) { err = kInfOverrun; break; }
                    __syncthreads();
                    if (dist <= (uint32_t)kWinBytes - 258u) {
                        // copy inside the LDS window: byte k comes from `dist` back; where the match overlaps itself the pattern repeats
                        for (uint32_t k = (uint32_t)lane; k < len; k += 64u) {
                            const uint32_t from = dist >= len ? pos - dist + k : pos - dist + (k % dist);
                            sh.win[(pos + k) & (kWinBytes - 1)] = sh.win[from & (kWinBytes - 1)];
                        }
                    } else {
                        // the source lies behind the LDS window: it has been flushed (whatever is older than the window minus a
                        // flush piece has), so read it back from the member's output -- once the stores have landed, and past
                        // this CU's L1, which may hold an older state of the line (dist > len here: no self-overlap)
                        __builtin_amdgcn_s_waitcnt(0);   // vmcnt(0) expcnt(0) lgkmcnt(0)
                        for (uint32_t k = (uint32_t)lane; k < len; k += 64u)
                            sh.win[(pos + k) & (kWinBytes - 1)] = __hip_atomic_load(dst + (pos - dist + k), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
                    __syncthreads();
                    pos += len;
                }
                if (pos - flushed >= (uint32_t)kFlush + 272u) flush_to((flushed + kFlush) & ~15u);   // (unflushed < a piece + two matches: the window keeps the rest as history)
            }
        }
    }
    if (!ZLIB && err == kInfOk && pos != ulen) err = kInfShort;
    // Both symbol decoders read zeros behind the end of the data, and the end-of-block code of a fixed block is seven zero
    // bits: a stream cut inside its last symbol must not pass for a whole one (zlib and libdeflate refuse it).  The
    // reader's bit position is in_pos * 8 - nb after every kind of block.
    if (err == kInfOk && in_pos * 8u - (uint32_t)nb > clen * 8u) err = kInfInputOverrun;   // (a member is < 64 KiB, a zlib block at most 2^28 bytes: no overflow)
    if (ZLIB && err == kInfOk && ((in_pos * 8u - (uint32_t)nb + 7u) >> 3) != clen) err = kInfTrailing;
    if (err == kInfOk) flush_to(ZLIB ? pos : ulen);
    // CRC-32 of the member is checked by k_bgzf_crc (below) on the inflated bytes in HBM
    if (lane == 0) status[m] = (uint32_t)err;
    if (ZLIB && lane == 0) status[nmembers + m] = err == kInfOk ? pos : 0u;
