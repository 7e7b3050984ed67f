// PNG decode core: zlib inflate (RFC 1950 / 1951) and the reversal of the PNG row filters, as plain C++ that compiles into the
// device kernel (csrc/png_decode.hip) and into host code (ssr_png_decode_host, tools/png_inflate_check.cpp) from the same text.
// No inline assembly, no atomics, no tables in memory beyond the caller's `pngi_work`.
//
// Execution shape: a stream is decoded serially by a TEAM of `nlanes` lanes that run this code in lockstep on the same data
// (host: nlanes = 1, lane = 0; device: the 64 lanes of one wave).  Everything that steers control flow (the bit reader, the
// positions, the code counts) is computed redundantly by every lane from the same bytes, so control flow is uniform over the
// team.  Memory is written by lane 0 alone (literals, code lengths, tables) or by all lanes at lane-strided places (match
// copies, stored blocks, None / Up rows); a byte written by one lane is read by another only after PNGI_SYNC().
//
// Hard termination and bounds: every loop iteration consumes at least one input bit or produces at least one output byte, or
// runs a fixed count; every read of the stream is checked against `src_len`, every write against the item's own range
// ([0, out_len) of `out`, [0, h w c) of `dst`).  A malformed stream ends with a PNGI_E* status; 0 is the only success.
//
// The history window is the output buffer itself: the whole raw image is kept, so distances up to 32768 reach back into it
// without a ring buffer.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define PNGI_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define PNGI_FN inline __attribute__((always_inline))
#endif
// order the team's memory accesses: bytes one lane wrote before the point are what any lane reads after it.  The lanes of a wave
// issue their memory instructions together and in program order, so wavefront scope is the whole team.
#if defined(__HIP_DEVICE_COMPILE__)
#define PNGI_SYNC()                                             \
    do {                                                        \
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); \
        __builtin_amdgcn_wave_barrier();                        \
    } while (0)
#else
#define PNGI_SYNC() \
    do {            \
    } while (0)
#endif

enum {
    PNGI_OK = 0,
    PNGI_ETRUNC = 1,     // the input ends inside the stream
    PNGI_EHEADER = 2,    // zlib header: CM != 8, window > 32 K, FDICT, FCHECK
    PNGI_EBTYPE = 3,     // block type 3
    PNGI_ESTORED = 4,    // stored block: LEN != ~NLEN
    PNGI_ECODELEN = 5,   // bad code lengths: counts out of range, over-subscribed or (beyond zlib's rule) incomplete set, bad repeat
    PNGI_ESYMBOL = 6,    // a bit pattern that is no code, or a length / distance symbol that does not exist
    PNGI_EDIST = 7,      // distance too far back
    PNGI_EOVERRUN = 8,   // the stream holds more than the raw image
    PNGI_ESHORT = 9,     // the stream ends before the raw image is complete
    PNGI_EFILTER = 10,   // a scanline's filter byte is not 0..4
    PNGI_EADLER = 11,    // Adler-32 mismatch
    PNGI_EDESC = 12,     // the item's descriptor does not fit its buffers (nothing of the item was read or written)
};

constexpr int PNGI_MAXLANES = 64;
constexpr uint32_t PNGI_MAX_RAW = 1u << 24;     // raw bytes per image (the Adler partial sums stay far below 2^64)

struct pngi_work {                  // per team; LDS on the device
    uint16_t lcount[16], dcount[16];
    uint16_t lsym[288], dsym[32];
    uint16_t offs[16];
    uint16_t fast[1 << 9];          // literal / length code, first level: (symbol << 4) | length for codes of up to 9 bits, else 0
    uint8_t lens[320];
    int32_t ret;
    int32_t pad_[3];
    uint64_t part[PNGI_MAXLANES][2];
};

struct pngi_bits {
    const uint8_t* src;
    uint32_t len, pos;
    uint64_t buf;
    int cnt;
};

// at least 32 bits in the buffer unless the input is exhausted
PNGI_FN void pngi_refill(pngi_bits& b) {
    if (b.cnt >= 32) return;
    if (b.pos + 4 <= b.len) {
        const uint32_t w = (uint32_t)b.src[b.pos] | ((uint32_t)b.src[b.pos + 1] << 8) | ((uint32_t)b.src[b.pos + 2] << 16) |
                           ((uint32_t)b.src[b.pos + 3] << 24);
        b.buf |= (uint64_t)w << b.cnt;
        b.cnt += 32;
        b.pos += 4;
        return;
    }
    while (b.pos < b.len && b.cnt < 32) {
        b.buf |= (uint64_t)b.src[b.pos++] << b.cnt;
        b.cnt += 8;
    }
}

// n <= 16 bits, least significant first; false: the input ends before them
PNGI_FN bool pngi_take(pngi_bits& b, int n, uint32_t& v) {
    pngi_refill(b);
    if (b.cnt < n) return false;
    v = (uint32_t)b.buf & ((1u << n) - 1u);
    b.buf >>= n;
    b.cnt -= n;
    return true;
}

// drop the bits up to the next byte boundary and hand the buffered whole bytes back to the stream
PNGI_FN void pngi_byte_align(pngi_bits& b) {
    b.pos -= (uint32_t)(b.cnt >> 3);
    b.buf = 0;
    b.cnt = 0;
}

// one symbol of a canonical code given as count[len] (in registers: every index below is a constant after unrolling) and the
// symbols in code order.  -1: the input ends inside the code; -2: no such code.
PNGI_FN int pngi_decode(pngi_bits& b, const uint16_t (&count)[16], const uint16_t* sym) {
    pngi_refill(b);
    uint32_t bits = (uint32_t)b.buf;
    int code = 0, first = 0, index = 0;
#pragma unroll
    for (int len = 1; len <= 15; ++len) {
        code |= (int)(bits & 1u);
        bits >>= 1;
        const int c = count[len];
        if (code - c < first) {
            if (b.cnt < len) return -1;
            b.buf >>= len;
            b.cnt -= len;
            return sym[index + (code - first)];
        }
        index += c;
        first += c;
        first <<= 1;
        code <<= 1;
    }
    return b.cnt < 15 ? -1 : -2;
}

// the literal / length code through its first-level table: one lookup for a code of up to PNGI_FAST_BITS bits (nearly every
// literal), the length walk for the rest - longer codes, bit patterns that are no code, and the end of the input
constexpr int PNGI_FAST_BITS = 9;
PNGI_FN int pngi_decode_lit(pngi_bits& b, const uint16_t* fast, const uint16_t (&count)[16], const uint16_t* sym) {
    pngi_refill(b);
    const int e = fast[(uint32_t)b.buf & ((1u << PNGI_FAST_BITS) - 1u)];
    const int len = e & 15;
    if (e != 0 && len <= b.cnt) {
        b.buf >>= len;
        b.cnt -= len;
        return e >> 4;
    }
    return pngi_decode(b, count, sym);
}

// fill the first-level table from a constructed code (lane 0 only): sym[] is in canonical order, so the codes of a length are
// consecutive integers; the table is indexed by the next bits of the stream, which hold a code most significant bit first
PNGI_FN void pngi_fill_fast(uint16_t* fast, const uint16_t* count, const uint16_t* sym) {
    for (int k = 0; k < (1 << PNGI_FAST_BITS); ++k) fast[k] = 0;
    uint32_t code = 0;
    int idx = 0;
    for (int len = 1; len <= PNGI_FAST_BITS; ++len) {
        for (int k = 0; k < count[len]; ++k, ++code) {
            uint32_t r = 0;
            for (int j = 0; j < len; ++j) r |= ((code >> j) & 1u) << (len - 1 - j);
            for (uint32_t at = r; at < (1u << PNGI_FAST_BITS); at += 1u << len) fast[at] = (uint16_t)((sym[idx] << 4) | len);
            ++idx;
        }
        code <<= 1;
    }
}

// canonical code from lengths (lane 0 only).  Returns < 0 over-subscribed, 0 complete, > 0 incomplete.
PNGI_FN int pngi_construct(uint16_t* count, uint16_t* sym, uint16_t* offs, const uint8_t* lens, int n) {
    for (int len = 0; len <= 15; ++len) count[len] = 0;
    for (int s = 0; s < n; ++s) count[lens[s]]++;
    int left = 1;
    for (int len = 1; len <= 15; ++len) {
        left <<= 1;
        left -= count[len];
        if (left < 0) return left;
    }
    offs[1] = 0;
    for (int len = 1; len < 15; ++len) offs[len + 1] = (uint16_t)(offs[len] + count[len]);
    for (int s = 0; s < n; ++s)
        if (lens[s] != 0) sym[offs[lens[s]]++] = (uint16_t)s;
    return left;
}

PNGI_FN void pngi_load_counts(uint16_t (&dst)[16], const uint16_t* src) {
#pragma unroll
    for (int k = 0; k < 16; ++k) dst[k] = src[k];
}

// out[pos .. pos + len) = the bytes `dist` back, repeating when dist < len.  The sources all lie in [pos - dist, pos), written
// before the caller's PNGI_SYNC, so the team's lanes copy independently.
PNGI_FN void pngi_copy_match(uint8_t* out, uint32_t pos, uint32_t dist, uint32_t len, int lane, int nlanes) {
    if (nlanes == 1) {
        for (uint32_t i = 0; i < len; ++i) out[pos + i] = out[pos + i - dist];
        return;
    }
    const uint8_t* from = out + (pos - dist);
    for (uint32_t i = (uint32_t)lane; i < len; i += (uint32_t)nlanes) out[pos + i] = from[i < dist ? i : i % dist];
}

// the compressed data of one literal / length + distance code pair until its end-of-block symbol
PNGI_FN int pngi_codes(pngi_bits& b, uint8_t* out, uint32_t out_len, uint32_t& pos, const pngi_work* wk, const uint16_t (&lc)[16],
                       const uint16_t (&dc)[16], int lane, int nlanes) {
    for (;;) {      // every pass consumes at least one bit (a code is at least one bit long) or returns
        int s = pngi_decode_lit(b, wk->fast, lc, wk->lsym);
        if (s < 0) return s == -1 ? PNGI_ETRUNC : PNGI_ESYMBOL;
        if (s < 256) {
            if (pos >= out_len) return PNGI_EOVERRUN;
            if (lane == 0) out[pos] = (uint8_t)s;
            ++pos;
            continue;
        }
        if (s == 256) return PNGI_OK;
        s -= 257;
        if (s >= 29) return PNGI_ESYMBOL;
        uint32_t eb = 0, len, dist;
        if (s < 8) len = 3u + (uint32_t)s;
        else if (s == 28) len = 258u;
        else {
            const int ext = (s >> 2) - 1;
            if (!pngi_take(b, ext, eb)) return PNGI_ETRUNC;
            len = 3u + ((4u + (uint32_t)(s & 3)) << ext) + eb;
        }
        const int d = pngi_decode(b, dc, wk->dsym);
        if (d < 0) return d == -1 ? PNGI_ETRUNC : PNGI_ESYMBOL;
        if (d >= 30) return PNGI_ESYMBOL;
        if (d < 4) dist = 1u + (uint32_t)d;
        else {
            const int ext = (d >> 1) - 1;      // up to 13
            if (!pngi_take(b, ext, eb)) return PNGI_ETRUNC;
            dist = 1u + ((2u + (uint32_t)(d & 1)) << ext) + eb;
        }
        if (dist > pos) return PNGI_EDIST;
        if (len > out_len - pos) return PNGI_EOVERRUN;
        PNGI_SYNC();
        pngi_copy_match(out, pos, dist, len, lane, nlanes);
        PNGI_SYNC();
        pos += len;
    }
}

// the verdict lane 0 reached, for the whole team
PNGI_FN int pngi_share(pngi_work* wk, int ret, int lane) {
    if (lane == 0) wk->ret = ret;
    PNGI_SYNC();
    const int r = wk->ret;
    PNGI_SYNC();
    return r;
}

// zlib's rule for a literal / length or distance set: complete, or a single code of length 1 (or, for distances, none at all)
PNGI_FN bool pngi_set_ok(int left, const uint16_t* count, int n) { return left == 0 || (left > 0 && n == count[0] + count[1]); }

PNGI_FN int pngi_fixed_tables(pngi_work* wk, int lane) {
    int ret = PNGI_OK;
    if (lane == 0) {
        for (int s = 0; s < 288; ++s) wk->lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8);
        pngi_construct(wk->lcount, wk->lsym, wk->offs, wk->lens, 288);
        pngi_fill_fast(wk->fast, wk->lcount, wk->lsym);
        for (int s = 0; s < 30; ++s) wk->lens[s] = 5;
        pngi_construct(wk->dcount, wk->dsym, wk->offs, wk->lens, 30);     // codes 30 and 31 stay unassigned: PNGI_ESYMBOL
    }
    return pngi_share(wk, ret, lane);
}

PNGI_FN int pngi_dynamic_tables(pngi_bits& b, pngi_work* wk, int lane) {
    static const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    uint32_t v;
    if (!pngi_take(b, 5, v)) return PNGI_ETRUNC;
    const int nlen = (int)v + 257;
    if (!pngi_take(b, 5, v)) return PNGI_ETRUNC;
    const int ndist = (int)v + 1;
    if (!pngi_take(b, 4, v)) return PNGI_ETRUNC;
    const int ncode = (int)v + 4;
    if (nlen > 286 || ndist > 30) return PNGI_ECODELEN;
    for (int i = 0; i < 19; ++i) {
        uint32_t l = 0;
        if (i < ncode && !pngi_take(b, 3, l)) return PNGI_ETRUNC;
        if (lane == 0) wk->lens[order[i]] = (uint8_t)l;
    }
    PNGI_SYNC();
    int ret = PNGI_OK;
    if (lane == 0 && pngi_construct(wk->lcount, wk->lsym, wk->offs, wk->lens, 19) != 0) ret = PNGI_ECODELEN;   // complete sets only
    ret = pngi_share(wk, ret, lane);
    if (ret) return ret;
    uint16_t cc[16];
    pngi_load_counts(cc, wk->lcount);
    PNGI_SYNC();
    const int total = nlen + ndist;
    int index = 0, prev = 0;
    while (index < total) {       // every pass consumes at least one bit or returns
        const int s = pngi_decode(b, cc, wk->lsym);
        if (s < 0) return s == -1 ? PNGI_ETRUNC : PNGI_ESYMBOL;
        if (s < 16) {
            if (lane == 0) wk->lens[index] = (uint8_t)s;
            ++index;
            prev = s;
            continue;
        }
        int val = 0, rep;
        if (s == 16) {
            if (index == 0) return PNGI_ECODELEN;
            val = prev;
            if (!pngi_take(b, 2, v)) return PNGI_ETRUNC;
            rep = 3 + (int)v;
        } else if (s == 17) {
            if (!pngi_take(b, 3, v)) return PNGI_ETRUNC;
            rep = 3 + (int)v;
        } else {
            if (!pngi_take(b, 7, v)) return PNGI_ETRUNC;
            rep = 11 + (int)v;
        }
        if (index + rep > total) return PNGI_ECODELEN;      // a run may cross from the literal lengths into the distances, not past them
        if (lane == 0)
            for (int k = 0; k < rep; ++k) wk->lens[index + k] = (uint8_t)val;
        index += rep;
        prev = val;
    }
    PNGI_SYNC();
    if (lane == 0) {
        if (wk->lens[256] == 0) ret = PNGI_ECODELEN;        // no end-of-block code
        if (!ret && !pngi_set_ok(pngi_construct(wk->lcount, wk->lsym, wk->offs, wk->lens, nlen), wk->lcount, nlen)) ret = PNGI_ECODELEN;
        if (!ret) pngi_fill_fast(wk->fast, wk->lcount, wk->lsym);
        if (!ret && !pngi_set_ok(pngi_construct(wk->dcount, wk->dsym, wk->offs, wk->lens + nlen, ndist), wk->dcount, ndist))
            ret = PNGI_ECODELEN;
    }
    return pngi_share(wk, ret, lane);
}

// Adler-32 of out[0 .. n): lane-strided partial sums (sum b, sum (n - i) b: below 2^56 for n <= PNGI_MAX_RAW), added up by everyone
PNGI_FN uint32_t pngi_adler32(const uint8_t* out, uint32_t n, pngi_work* wk, int lane, int nlanes) {
    uint64_t a = 0, w = 0;
    for (uint32_t i = (uint32_t)lane; i < n; i += (uint32_t)nlanes) {
        const uint64_t v = out[i];
        a += v;
        w += (uint64_t)(n - i) * v;
    }
    wk->part[lane][0] = a;
    wk->part[lane][1] = w;
    PNGI_SYNC();
    a = 0;
    w = 0;
    for (int l = 0; l < nlanes; ++l) {
        a += wk->part[l][0];
        w += wk->part[l][1] % 65521u;
    }
    PNGI_SYNC();
    const uint32_t s1 = (uint32_t)((1u + a) % 65521u), s2 = (uint32_t)((n + w) % 65521u);
    return (s2 << 16) | s1;
}

// a whole zlib stream into out[0 .. out_len): exactly out_len bytes or an error
PNGI_FN int pngi_inflate(const uint8_t* src, uint32_t src_len, uint8_t* out, uint32_t out_len, pngi_work* wk, int lane, int nlanes) {
    if (src_len < 2) return PNGI_ETRUNC;
    const uint32_t cmf = src[0], flg = src[1];
    if ((cmf & 15u) != 8u || (cmf >> 4) > 7u || ((cmf << 8) | flg) % 31u != 0u || (flg & 0x20u)) return PNGI_EHEADER;
    pngi_bits b = {src, src_len, 2u, 0u, 0};
    uint32_t pos = 0, v;
    for (;;) {          // every pass consumes the three header bits of a block or returns
        if (!pngi_take(b, 1, v)) return PNGI_ETRUNC;
        const uint32_t last = v;
        if (!pngi_take(b, 2, v)) return PNGI_ETRUNC;
        if (v == 3) return PNGI_EBTYPE;
        if (v == 0) {
            pngi_byte_align(b);
            if (b.pos + 4 > src_len) return PNGI_ETRUNC;
            const uint32_t len = (uint32_t)src[b.pos] | ((uint32_t)src[b.pos + 1] << 8);
            const uint32_t nlen = (uint32_t)src[b.pos + 2] | ((uint32_t)src[b.pos + 3] << 8);
            if (len != (~nlen & 0xffffu)) return PNGI_ESTORED;
            b.pos += 4;
            if (len > src_len - b.pos) return PNGI_ETRUNC;
            if (len > out_len - pos) return PNGI_EOVERRUN;
            for (uint32_t i = (uint32_t)lane; i < len; i += (uint32_t)nlanes) out[pos + i] = src[b.pos + i];
            PNGI_SYNC();
            b.pos += len;
            pos += len;
        } else {
            const int ret = v == 1 ? pngi_fixed_tables(wk, lane) : pngi_dynamic_tables(b, wk, lane);
            if (ret) return ret;
            uint16_t lc[16], dc[16];
            pngi_load_counts(lc, wk->lcount);
            pngi_load_counts(dc, wk->dcount);
            const int r = pngi_codes(b, out, out_len, pos, wk, lc, dc, lane, nlanes);
            if (r) return r;
            PNGI_SYNC();
        }
        if (last) break;
    }
    if (pos != out_len) return PNGI_ESHORT;
    pngi_byte_align(b);
    if (b.pos + 4 > src_len) return PNGI_ETRUNC;
    const uint32_t want = ((uint32_t)src[b.pos] << 24) | ((uint32_t)src[b.pos + 1] << 16) | ((uint32_t)src[b.pos + 2] << 8) |
                          (uint32_t)src[b.pos + 3];
    PNGI_SYNC();
    return pngi_adler32(out, out_len, wk, lane, nlanes) == want ? PNGI_OK : PNGI_EADLER;
}

PNGI_FN int pngi_paeth(int a, int b, int c) {
    const int p = a + b - c;
    const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

// raw scanlines (h rows of 1 filter byte + w bpp bytes) -> tight [h][w][bpp] bytes at dst.  None and Up rows are spread over the
// team; Sub, Average and Paeth run along the row, one lane per byte of a pixel.
PNGI_FN int pngi_unfilter(const uint8_t* raw, uint32_t w, uint32_t h, uint32_t bpp, uint8_t* dst, int lane, int nlanes) {
    const uint32_t rowb = w * bpp;
    for (uint32_t r = 0; r < h; ++r) {
        const uint8_t* in = raw + (uint64_t)r * (rowb + 1);
        uint8_t* o = dst + (uint64_t)r * rowb;
        const uint8_t* up = r ? o - rowb : o;     // read only when r > 0
        const uint32_t ft = in[0];
        ++in;
        if (ft > 4) return PNGI_EFILTER;
        if (ft == 0) {
            for (uint32_t x = (uint32_t)lane; x < rowb; x += (uint32_t)nlanes) o[x] = in[x];
        } else if (ft == 2) {
            for (uint32_t x = (uint32_t)lane; x < rowb; x += (uint32_t)nlanes) o[x] = (uint8_t)(in[x] + (r ? up[x] : 0));
        } else {
            for (uint32_t ch = (uint32_t)lane; ch < bpp; ch += (uint32_t)nlanes) {
                int a = 0, c = 0;             // left, upper left
                for (uint32_t x = ch; x < rowb; x += bpp) {
                    const int bb = r ? up[x] : 0;
                    const int pred = ft == 1 ? a : ft == 3 ? ((a + bb) >> 1) : pngi_paeth(a, bb, c);
                    a = (in[x] + pred) & 255;
                    c = bb;
                    o[x] = (uint8_t)a;
                }
            }
        }
        PNGI_SYNC();
    }
    return PNGI_OK;
}

// does an item fit its buffers?  (all in 64 bits: nothing here can wrap)
PNGI_FN bool pngi_item_ok(int64_t src_off, int64_t src_len, int64_t w, int64_t h, int64_t c, int64_t dst_off, int64_t raw_off,
                          int64_t streams_len, int64_t dst_len, int64_t scratch_len) {
    if (w < 1 || h < 1 || w > 32768 || h > 32768 || (c != 1 && c != 3)) return false;
    const int64_t raw = h * (w * c + 1);
    if (raw > (int64_t)PNGI_MAX_RAW) return false;
    if (src_off < 0 || src_len < 0 || src_len > 0x7fffffffLL || src_off > streams_len || src_len > streams_len - src_off) return false;
    if (dst_off < 0 || dst_off > dst_len || h * w * c > dst_len - dst_off) return false;
    if (raw_off < 0 || raw_off > scratch_len || raw > scratch_len - raw_off) return false;
    return true;
}

// one PNG image: its zlib stream -> raw scanlines in `raw` (h (w c + 1) bytes) -> pixels at dst
PNGI_FN int pngi_decode_image(const uint8_t* src, uint32_t src_len, uint32_t w, uint32_t h, uint32_t c, uint8_t* raw, uint8_t* dst,
                              pngi_work* wk, int lane, int nlanes) {
    const int st = pngi_inflate(src, src_len, raw, h * (w * c + 1), wk, lane, nlanes);
    if (st) return st;
    PNGI_SYNC();
    return pngi_unfilter(raw, w, h, c, dst, lane, nlanes);
}
