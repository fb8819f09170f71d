/*
 * png_inflate_core.h -- the inflate of one deflate stream (RFC 1951), everything of it that one lane does on its own, written once in
 * the C subset gcc and hipcc both take: lane 0 of mi355_png_inflate's wave (csrc/png_inflate.hip) and the host emulation
 * (png_inflate_emulate.c) run this text.  It follows the host decoder (png.c: zbits, zbuild, zdecode, zdynamic, zblock) check by check,
 * so that a stream is refused here where it is refused there and for the same reason.
 *
 * The bit reader holds up to 64 bits and refills a dword at a time from a WINDOW of the stream: words [base, base + nw) of it at w[]
 * (the kernel keeps the window in LDS and moves it between the rounds; the emulation's window is the whole stream).  A word outside
 * the window reads as zero and nothing outside it is ever read; the callers size the window so that a round cannot leave it
 * (PIC_WINDOW).  Bits past nbytes read as zero -- the stream is followed by zero bytes -- and pic_over says whether any were consumed.
 *
 * What decodes symbols works in ROUNDS: pic_round fills a list of at most PIC_TOKENS tokens (a literal, or length << 16 | distance)
 * and stops at the end of the block, at cap or at an error; placing the tokens' bytes is the callers' part (all lanes in the kernel).
 * Every loop here consumes at least one bit or stores one token or ends, and a consumed bit past the end of the stream ends the
 * decode, so the steps of a stream are bounded by 8 * nbytes plus the reader's 64 bits.
 */
#ifndef DNQ_PNG_INFLATE_CORE_H
#define DNQ_PNG_INFLATE_CORE_H
#include <stdint.h>
#include "../../include/mi355_yolo_int8.h"

#ifdef __HIPCC__
#define PIC_FN __host__ __device__ static inline
#else
#define PIC_FN static inline
#endif

#define PIC_LOOK 10                  /* ZLOOK of png.c */
#define PIC_TOKENS 64                /* tokens of a round: one per lane */
#define PIC_RING 65536u              /* the output ring: the 32 KiB window plus more than a round can produce (64 * 258 bytes) */
#define PIC_WINDOW 256               /* dwords of the input window: a dynamic header is at most 141, a round's tokens at most 98 */
#define PIC_STORED_CHUNK 16384u      /* bytes of a stored block copied between two flushes */
#define PIC_MAX_LENS (288 + 32)

enum { PIC_HEADER = 0, PIC_BUILD, PIC_SYMBOLS, PIC_STORED, PIC_DONE };

typedef struct pic_code {            /* zcode of png.c */
    uint16_t count[16];
    uint16_t symbol[288];
    uint16_t look[1 << PIC_LOOK];    /* (symbol << 4) | bits, 0: a longer code, or none */
} pic_code;

typedef struct pic_bits {
    const uint32_t *w;               /* the window */
    uint32_t base, nw;               /* it holds words base .. base + nw - 1 of the stream */
    uint32_t nbytes;
    uint64_t buf;                    /* LSB first */
    uint32_t cnt;                    /* bits in buf */
    uint32_t next;                   /* the stream's next word to load */
} pic_bits;

typedef struct pic_state {
    pic_bits b;
    uint32_t n, cap;                 /* bytes produced; the stop mark */
    uint32_t n0;                     /* n when the round began */
    int phase, final, status;
    int ntok;                        /* tokens of the round */
    int hlit, hdist;                 /* PIC_BUILD: the lengths at lens[0, hlit) and lens[hlit, hlit + hdist) */
    uint32_t stored_left, stored_at; /* PIC_STORED: bytes still to copy, and where in the stream they start */
    uint32_t skip;                   /* bits (a multiple of 8) the next header drops first */
} pic_state;

/* ---------------------------------------------------------------------------------------------------------------- bits */
/* at least 32 bits in buf */
PIC_FN void pic_fill(pic_bits *b)
{
    if (b->cnt < 32) {
        const uint32_t i = b->next - b->base;
        const uint64_t v = i < b->nw ? b->w[i] : 0u;
        b->buf |= v << b->cnt; b->cnt += 32; ++b->next;
    }
}
/* n <= 16 */
PIC_FN uint32_t pic_take(pic_bits *b, int n)
{
    pic_fill(b);
    const uint32_t v = (uint32_t)b->buf & ((1u << n) - 1);
    b->buf >>= n; b->cnt -= (uint32_t)n;
    return v;
}
PIC_FN uint32_t pic_pos(const pic_bits *b) { return 32u * b->next - b->cnt; }       /* bits consumed */
PIC_FN int pic_over(const pic_bits *b) { return pic_pos(b) > 8u * b->nbytes; }      /* bits beyond the end have been consumed */

/* -------------------------------------------------------------------------------------------------------------- tables */
/* Kept as arithmetic where a table in constant memory would be a scalar or vector load per symbol: the extra bits of length symbol
 * s (0..28) and of distance symbol s (0..29), and the bases they add to. */
PIC_FN int pic_len_extra(int s) { return s < 8 || s == 28 ? 0 : (s - 4) >> 2; }
PIC_FN uint32_t pic_len_start(int s)
{
    if (s < 8) return 3u + (uint32_t)s;
    if (s == 28) return 258u;
    const int e = (s - 4) >> 2;
    return 3u + ((4u + (uint32_t)(s & 3)) << e);
}
PIC_FN int pic_dist_extra(int s) { return s < 4 ? 0 : (s - 2) >> 1; }
PIC_FN uint32_t pic_dist_start(int s)
{
    if (s < 4) return 1u + (uint32_t)s;
    const int e = (s - 2) >> 1;
    return 1u + ((2u + (uint32_t)(s & 1)) << e);
}

/* The serial half of zbuild: counts, the over-subscription check, the symbols in the order of their codes, and every symbol's code
 * (MSB first) at codes[] for pic_look_fill.  0, or MI355_PNG_ELENGTHS; an incomplete set is accepted. */
PIC_FN int pic_build_serial(pic_code *z, const uint8_t *lengths, int n, uint16_t *codes)
{
    uint16_t next[16], at[16];
    for (int i = 0; i < 16; ++i) z->count[i] = 0;
    for (int i = 0; i < n; ++i) ++z->count[lengths[i] & 15];
    z->count[0] = 0;
    int room = 1;
    for (int len = 1; len < 16; ++len) {
        room = 2 * room - z->count[len];
        if (room < 0) return MI355_PNG_ELENGTHS;
    }
    unsigned code = 0;
    next[0] = 0; at[0] = 0;
    for (int len = 1; len < 16; ++len) {
        code = (code + z->count[len - 1]) << 1;
        next[len] = (uint16_t)code;
        at[len] = (uint16_t)(at[len - 1] + z->count[len - 1]);
    }
    for (int i = 0; i < n; ++i) {
        const int len = lengths[i] & 15;
        if (!len) continue;
        z->symbol[at[len]++] = (uint16_t)i;
        codes[i] = next[len]++;
    }
    return 0;
}
/* The look table, by lanes: lane `lane` of `nlanes` zeroes / fills its share; all of pic_look_zero comes before any of pic_look_fill.
 * Codes are prefix-free once pic_build_serial has accepted the lengths, so no two symbols fill the same entry. */
PIC_FN void pic_look_zero(pic_code *z, int lane, int nlanes)
{
    for (int j = lane; j < (1 << PIC_LOOK); j += nlanes) z->look[j] = 0;
}
PIC_FN void pic_look_fill(pic_code *z, const uint8_t *lengths, int n, const uint16_t *codes, int lane, int nlanes)
{
    for (int i = lane; i < n; i += nlanes) {
        const int len = lengths[i] & 15;
        if (!len || len > PIC_LOOK) continue;
        unsigned c = codes[i], lsb = 0; /* the stream carries a code's most significant bit first */
        for (int k = 0; k < len; ++k) lsb |= ((c >> k) & 1u) << (len - 1 - k);
        for (unsigned j = lsb; j < (1u << PIC_LOOK); j += 1u << len) z->look[j] = (uint16_t)(i << 4 | len);
    }
}

/* one symbol, bit by bit against count[] / symbol[]; -1: no code has these bits, nothing is consumed */
PIC_FN int pic_walk(pic_bits *b, const pic_code *z)
{
    int code = 0, first = 0, index = 0;
    for (int len = 1; len < 16; ++len) {
        code |= (int)((b->buf >> (len - 1)) & 1);
        const int count = z->count[len];
        if (code - first < count) {
            b->buf >>= len; b->cnt -= (uint32_t)len;
            return z->symbol[index + (code - first)];
        }
        index += count;
        first = (first + count) << 1;
        code <<= 1;
    }
    return -1;
}
PIC_FN int pic_decode(pic_bits *b, const pic_code *z)
{
    pic_fill(b);
    const unsigned hit = z->look[(uint32_t)b->buf & ((1u << PIC_LOOK) - 1)];
    if (hit) {
        b->buf >>= hit & 15; b->cnt -= hit & 15;
        return (int)(hit >> 4);
    }
    return pic_walk(b, z);
}

/* ------------------------------------------------------------------------------------------------------------- headers */
/* zdynamic up to the lengths: HLIT / HDIST / HCLEN, the code-length code (built in `zc`, walked without a look table) and the
 * lengths with the repeat codes 16 / 17 / 18, into lens[0, hlit + hdist).  0 or the status. */
PIC_FN int pic_dynamic(pic_state *s, pic_code *zc, uint8_t *lens, uint16_t *codes)
{
    const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    pic_bits *b = &s->b;
    uint8_t clens[19];
    const int hlit = (int)pic_take(b, 5) + 257, hdist = (int)pic_take(b, 5) + 1, hclen = (int)pic_take(b, 4) + 4, ntot = hlit + hdist;
    for (int i = 0; i < 19; ++i) clens[i] = 0;
    for (int i = 0; i < hclen; ++i) clens[order[i]] = (uint8_t)pic_take(b, 3);
    if (pic_build_serial(zc, clens, 19, codes)) return MI355_PNG_ELENGTHS;
    int n = 0;
    while (n < ntot) {
        pic_fill(b);
        int c = pic_walk(b, zc);
        if (pic_over(b)) return MI355_PNG_EPREMATURE;
        if (c < 0 || c >= 19) return MI355_PNG_ELENGTHS;
        if (c < 16) { lens[n++] = (uint8_t)c; continue; }
        uint8_t fill = 0;
        if (c == 16) {
            c = (int)pic_take(b, 2) + 3;
            if (n == 0) return MI355_PNG_ELENGTHS;
            fill = lens[n - 1];
        } else if (c == 17) c = (int)pic_take(b, 3) + 3;
        else c = (int)pic_take(b, 7) + 11;
        if (ntot - n < c) return MI355_PNG_ELENGTHS;
        for (int k = 0; k < c; ++k) lens[n + k] = fill;
        n += c;
    }
    if (hlit > 288) return MI355_PNG_ELENGTHS;
    s->hlit = hlit; s->hdist = hdist;
    return 0;
}

/* A block header, phase PIC_HEADER: the three bits, then for a stored block LEN / NLEN (-> PIC_STORED, or the next header where it
 * is empty), for a Huffman block the lengths at lens[] and the serial half of both builds (-> PIC_BUILD: the callers fill the look
 * tables, then set PIC_SYMBOLS).  zl, zd: the block's tables; zd serves the code-length code first.  A status ends the stream. */
PIC_FN void pic_header(pic_state *s, pic_code *zl, pic_code *zd, uint8_t *lens, uint16_t *codes)
{
    pic_bits *b = &s->b;
    for (; s->skip; s->skip -= 8) pic_take(b, 8); /* behind a stored block: the bits of its last word that belong to it */
    s->final = (int)pic_take(b, 1);
    const uint32_t type = pic_take(b, 2);
    int why = 0;
    if (pic_over(b)) why = MI355_PNG_EPREMATURE;
    else if (type == 0) {
        pic_take(b, (int)(b->cnt & 7));
        const uint32_t len = pic_take(b, 16), nlen = pic_take(b, 16);
        if (pic_over(b)) why = MI355_PNG_EPREMATURE;
        else if (nlen != (len ^ 0xffffu)) why = MI355_PNG_ECORRUPT;
        else {
            const uint32_t at = pic_pos(b) >> 3, need = len < s->cap - s->n ? len : s->cap - s->n;
            if (need > b->nbytes - at) why = MI355_PNG_EPAST;
            else if (need) { s->stored_left = need; s->stored_at = at; s->phase = PIC_STORED; }
            else if (s->final) s->phase = PIC_DONE;
        }
    } else if (type == 1) {
        for (int i = 0; i < 144; ++i) lens[i] = 8;
        for (int i = 144; i < 256; ++i) lens[i] = 9;
        for (int i = 256; i < 280; ++i) lens[i] = 7;
        for (int i = 280; i < 288; ++i) lens[i] = 8;
        for (int i = 288; i < 320; ++i) lens[i] = 5;
        s->hlit = 288; s->hdist = 32;
    } else if (type == 2) why = pic_dynamic(s, zd, lens, codes);
    else why = MI355_PNG_EBLOCK;
    if (!why && type) {
        if (!(why = pic_build_serial(zl, lens, s->hlit, codes)) && !(why = pic_build_serial(zd, lens + s->hlit, s->hdist, codes + s->hlit)))
            s->phase = PIC_BUILD;
    }
    if (why) { s->status = why; s->phase = PIC_DONE; }
}

/* The bytes of a stored block (or a chunk of them) have been copied: where the reader goes on. */
PIC_FN void pic_stored_done(pic_state *s, uint32_t copied)
{
    s->n += copied; s->stored_at += copied; s->stored_left -= copied;
    if (s->stored_left) return;
    if (s->n == s->cap || s->final) { s->phase = PIC_DONE; return; }
    s->b.buf = 0; s->b.cnt = 0; s->b.next = s->stored_at >> 2; /* the callers' window moves there before the header is read */
    s->skip = 8u * (s->stored_at & 3);
    s->phase = PIC_HEADER;
}

/* ---------------------------------------------------------------------------------------------------------------- round */
/* zblock for at most PIC_TOKENS tokens.  tok[t]: a literal's byte, or length << 16 | distance of a match, its length cut at cap.
 * Leaves ntok, n (advanced past the tokens; n0: where the round began) and the phase: PIC_SYMBOLS (the list is full), PIC_HEADER (end
 * of block), PIC_DONE (cap, the end of the final block, or a status -- then the tokens in front of it are still placed, as the host
 * has stored their bytes).  window: the window's address once more. */
PIC_FN void pic_round(pic_state *s, const pic_code *zl, const pic_code *zd, uint32_t *tok, const uint32_t *window)
{
    pic_bits b = s->b;
    b.w = window; /* s->b.w, handed in so that the kernel's compiler knows the address space of the refills: LDS reads, not flat ones */
    uint32_t n = s->n;
    const uint32_t cap = s->cap;
    int ntok = 0, why = 0, phase = PIC_SYMBOLS;
    s->n0 = n;
    while (ntok < PIC_TOKENS) {
        int z = pic_decode(&b, zl);
        if (z < 0 || pic_over(&b)) { why = z < 0 ? MI355_PNG_EHUFF : MI355_PNG_EPREMATURE; break; }
        if (z < 256) {
            tok[ntok++] = (uint32_t)z;
            if (++n == cap) { phase = PIC_DONE; break; }
            continue;
        }
        if (z == 256) { phase = s->final ? PIC_DONE : PIC_HEADER; break; }
        z -= 257;
        if (z >= 29) { why = MI355_PNG_EHUFF; break; }
        uint32_t len = pic_len_start(z);
        if (pic_len_extra(z)) len += pic_take(&b, pic_len_extra(z));
        z = pic_decode(&b, zd);
        if (z < 0) { why = MI355_PNG_EHUFF; break; }
        if (z >= 30) { why = MI355_PNG_EDIST; break; }
        uint32_t dist = pic_dist_start(z);
        if (pic_dist_extra(z)) dist += pic_take(&b, pic_dist_extra(z));
        if (pic_over(&b)) { why = MI355_PNG_EPREMATURE; break; }
        if (dist > n) { why = MI355_PNG_EDIST; break; }
        if (len > cap - n) len = cap - n;
        tok[ntok++] = len << 16 | dist;
        n += len;
        if (n == cap) { phase = PIC_DONE; break; }
    }
    s->b = b; s->n = n; s->ntok = ntok;
    if (why) { s->status = why; phase = PIC_DONE; }
    s->phase = phase;
}

/* ---------------------------------------------------------------------------------------------------------------- records */
PIC_FN uint32_t pic_stream_words(uint32_t nbytes) { return ((nbytes + 3) >> 2) + 2; } /* what may be read of z */

/* what is wrong with a stream record (the message mi355_png_inflate refuses it with); NULL: nothing */
PIC_FN const char *pic_stream_check(const mi355_png_stream *s)
{
    if (!s->z || !s->out) return "png_inflate: null z / out pointer";
    if (((size_t)s->z & 3) || ((size_t)s->out & 3)) return "png_inflate: z and out must be 4-byte aligned";
    if (s->nbytes > (1u << 28)) return "png_inflate: a stream of more than 2^28 bytes";
    if (s->cap == 0 || s->cap >= (1u << 31)) return "png_inflate: need 1 <= cap < 2^31";
    if (s->npasses < 1 || s->npasses > 7 || s->reserved) return "png_inflate: need 1 <= npasses <= 7 and reserved == 0";
    uint64_t sum = 0;
    for (int k = 0; k < s->npasses; ++k) {
        if (s->rows[k] < 1 || s->row_bytes[k] < 1) return "png_inflate: a pass without rows or bytes";
        sum += (uint64_t)s->rows[k] * ((uint64_t)s->row_bytes[k] + 1);
    }
    if (sum != s->cap) return "png_inflate: the passes do not add up to cap";
    return 0;
}
#endif
