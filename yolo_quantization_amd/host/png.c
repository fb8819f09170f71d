/*
 * png.c -- chunk parsing and inflate of PNG files (png.h).  The chunk walk follows stb_image v2.19's stbi__parse_png_file (ref:
 * src/stb_image.h:4727-4901) chunk by chunk, so the same files are refused for the same reasons, in stb's words; the inflate is
 * written from RFC 1950 / 1951 -- its code tables are the RFC's counts and ordered symbols, nothing of stb's -- and words its
 * refusals as stb does where stb has the same one.  The compressed bytes are read where they lie, IDAT chunk after
 * IDAT chunk, and the output grows towards the bytes the image needs and never beyond them.
 */
#include "png.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#ifndef DNQ_PNG_REALLOC /* the fuzz program counts what is asked for */
#define DNQ_PNG_REALLOC realloc
#else
void *DNQ_PNG_REALLOC(void *p, size_t n);
#endif

static int fail(char *err, size_t errlen, const char *why)
{
    if (err && errlen) snprintf(err, errlen, "%s", why);
    return -1;
}

static uint32_t be32(const uint8_t *p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]; }
#define CHUNK(a, b, c, d) ((uint32_t)(a) << 24 | (uint32_t)(b) << 16 | (uint32_t)(c) << 8 | (uint32_t)(d))

/* ------------------------------------------------------------------------------------------------------------- inflate */
/* The source of compressed bytes: a plain buffer, or the IDAT chunks of a file whose chunk walk has been validated. */
typedef struct zsrc {
    const uint8_t *file;   /* NULL: a plain buffer */
    size_t file_bytes;
    size_t next;           /* offset of the next chunk header to look at */
    const uint8_t *cur, *end;
    uint64_t buf;          /* LSB first */
    int cnt;               /* bits in buf */
    int pad;               /* zero bytes fed after the end of the data */
} zsrc;

static int zsrc_next_idat(zsrc *s)
{
    if (!s->file) return 0;
    while (s->next + 8 <= s->file_bytes) {
        const uint32_t len = be32(s->file + s->next), type = be32(s->file + s->next + 4);
        const size_t at = s->next + 8;
        if (len > s->file_bytes - at) return 0;
        s->next = at + len + 4 > s->file_bytes ? s->file_bytes : at + len + 4;
        if (type == CHUNK('I', 'E', 'N', 'D')) { s->next = s->file_bytes; return 0; }
        if (type == CHUNK('I', 'D', 'A', 'T')) { s->cur = s->file + at; s->end = s->cur + len; return 1; }
    }
    return 0;
}

static inline void zfill(zsrc *s, int n)
{
    while (s->cnt < n) {
        uint64_t byte = 0;
        while (s->cur == s->end && zsrc_next_idat(s)) {}
        if (s->cur != s->end) byte = *s->cur++;
        else if (s->pad < 64) ++s->pad;
        s->buf |= byte << s->cnt;
        s->cnt += 8;
    }
}
static inline uint32_t zbits(zsrc *s, int n)
{
    zfill(s, n);
    const uint32_t v = (uint32_t)(s->buf & ((1u << n) - 1));
    s->buf >>= n; s->cnt -= n;
    return v;
}
/* bits beyond the end of the data have been consumed */
static inline int zover(const zsrc *s) { return s->pad * 8 > s->cnt; }

/* A canonical Huffman code as RFC 1951 3.2.2 defines it: count[n] codes of n bits, the symbols in the order of their codes (by length,
 * then by value).  A code is walked bit by bit against that list -- of the codes of n bits the first is `first`, and they are
 * consecutive --; `look` answers the codes of at most ZLOOK bits in one step from the next ZLOOK bits of the stream. */
#define ZLOOK 10
typedef struct zcode {
    uint16_t count[16];
    uint16_t symbol[288];
    uint16_t look[1 << ZLOOK];      /* (symbol << 4) | bits, 0: a longer code, or none */
} zcode;

/* n lengths (0: unused).  Over-subscribed lengths are refused; an incomplete set is accepted, as zlib's one-code distance tree is
 * one, and a bit pattern no code has decodes to nothing. */
static const char *zbuild(zcode *z, const uint8_t *lengths, int n)
{
    uint16_t start[16], next[16];   /* per length: index of its first symbol, its next code */
    memset(z, 0, sizeof(*z));
    for (int i = 0; i < n; ++i) ++z->count[lengths[i]];
    z->count[0] = 0;
    int room = 1;                   /* codes still free at this length */
    for (int len = 1; len < 16; ++len) {
        room = 2 * room - z->count[len];
        if (room < 0) return "bad codelengths";
    }
    unsigned code = 0;
    start[0] = 0; next[0] = 0;
    for (int len = 1; len < 16; ++len) {
        code = (code + z->count[len - 1]) << 1;
        next[len] = (uint16_t)code;
        start[len] = (uint16_t)(start[len - 1] + z->count[len - 1]);
    }
    uint16_t at[16];
    memcpy(at, start, sizeof(at));
    for (int i = 0; i < n; ++i) {
        const int len = lengths[i];
        if (!len) continue;
        z->symbol[at[len]++] = (uint16_t)i;
        if (len <= ZLOOK) {
            unsigned c = next[len], lsb = 0; /* the stream carries a code's most significant bit first */
            for (int k = 0; k < len; ++k) lsb |= ((c >> k) & 1u) << (len - 1 - k);
            for (unsigned j = lsb; j < (1u << ZLOOK); j += 1u << len) z->look[j] = (uint16_t)(i << 4 | len);
        }
        ++next[len];
    }
    return NULL;
}

static inline int zdecode(zsrc *s, const zcode *z)
{
    zfill(s, 16);
    const unsigned hit = z->look[s->buf & ((1u << ZLOOK) - 1)];
    if (hit) {
        s->buf >>= hit & 15; s->cnt -= (int)(hit & 15);
        return (int)(hit >> 4);
    }
    int code = 0, first = 0, index = 0;
    for (int len = 1; len < 16; ++len) {
        code |= (int)((s->buf >> (len - 1)) & 1);
        const int count = z->count[len];
        if (code - first < count) {
            s->buf >>= len; s->cnt -= len;
            return z->symbol[index + (code - first)];
        }
        index += count;
        first = (first + count) << 1;
        code <<= 1;
    }
    return -1;
}

typedef struct zout {
    uint8_t *p;
    size_t n, have, cap;
    int grows;             /* p is ours and grows towards cap */
} zout;

static int zroom(zout *o, size_t want)
{
    if (want > o->cap) want = o->cap;
    if (want <= o->have) return 1;
    if (!o->grows) return 0;
    size_t to = o->have ? o->have : 65536;
    while (to < want) to *= 2;
    if (to > o->cap) to = o->cap;
    uint8_t *q = DNQ_PNG_REALLOC(o->p, to);
    if (!q) return 0;
    o->p = q; o->have = to;
    return 1;
}

static const uint16_t zlen_base[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
static const uint8_t zlen_extra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
static const uint16_t zdist_base[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
static const uint8_t zdist_extra[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};

/* One Huffman-coded block.  NULL: the block ended or the output is full (o->n == o->cap). */
static const char *zblock(zsrc *s, zout *o, const zcode *zl, const zcode *zd)
{
    for (;;) {
        if (o->have - o->n < 258 && !zroom(o, o->n + 65536)) return "out of memory";
        int z = zdecode(s, zl);
        if (z < 0 || zover(s)) return z < 0 ? "bad huffman code" : "premature end of the zlib data";
        if (z < 256) {
            o->p[o->n++] = (uint8_t)z;
            if (o->n == o->cap) return NULL;
            continue;
        }
        if (z == 256) return NULL;
        z -= 257;
        if (z >= 29) return "bad huffman code";
        size_t len = zlen_base[z];
        if (zlen_extra[z]) len += zbits(s, zlen_extra[z]);
        z = zdecode(s, zd);
        if (z < 0) return "bad huffman code";
        if (z >= 30) return "bad dist";
        size_t dist = zdist_base[z];
        if (zdist_extra[z]) dist += zbits(s, zdist_extra[z]);
        if (zover(s)) return "premature end of the zlib data";
        if (dist > o->n) return "bad dist";
        if (len > o->cap - o->n) len = o->cap - o->n;
        uint8_t *q = o->p + o->n;
        const uint8_t *from = q - dist;
        for (size_t i = 0; i < len; ++i) q[i] = from[i]; /* byte by byte: the copy may overlap what it writes */
        o->n += len;
        if (o->n == o->cap) return NULL;
    }
}

static const char *zdynamic(zsrc *s, zcode *zl, zcode *zd)
{
    static const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    zcode zc;
    uint8_t lens[288 + 32 + 140], clens[19];
    const int hlit = (int)zbits(s, 5) + 257, hdist = (int)zbits(s, 5) + 1, hclen = (int)zbits(s, 4) + 4, ntot = hlit + hdist;
    memset(clens, 0, sizeof(clens));
    for (int i = 0; i < hclen; ++i) clens[order[i]] = (uint8_t)zbits(s, 3);
    const char *why = zbuild(&zc, clens, 19);
    if (why) return why;
    int n = 0;
    while (n < ntot) {
        int c = zdecode(s, &zc);
        if (zover(s)) return "premature end of the zlib data";
        if (c < 0 || c >= 19) return "bad codelengths";
        if (c < 16) { lens[n++] = (uint8_t)c; continue; }
        uint8_t fill = 0;
        if (c == 16) {
            c = (int)zbits(s, 2) + 3;
            if (n == 0) return "bad codelengths";
            fill = lens[n - 1];
        } else if (c == 17) c = (int)zbits(s, 3) + 3;
        else c = (int)zbits(s, 7) + 11;
        if (ntot - n < c) return "bad codelengths";
        memset(lens + n, fill, (size_t)c);
        n += c;
    }
    if (hlit > 288) return "bad codelengths";
    if ((why = zbuild(zl, lens, hlit))) return why;
    return zbuild(zd, lens + hlit, hdist);
}

static const char *zinflate(zsrc *s, zout *o)
{
    zcode *zl = malloc(2 * sizeof(zcode)), *zd = zl + 1;
    if (!zl) return "out of memory";
    const char *why = NULL;
    const uint32_t cmf = zbits(s, 8), flg = zbits(s, 8);
    if (zover(s) || (cmf * 256 + flg) % 31 != 0) why = "bad zlib header";
    else if (flg & 32) why = "no preset dict";
    else if ((cmf & 15) != 8) why = "bad compression";
    int final = 0;
    while (!why && !final && o->n < o->cap) {
        final = (int)zbits(s, 1);
        const uint32_t type = zbits(s, 2);
        if (zover(s)) { why = "premature end of the zlib data"; break; }
        if (type == 0) {
            zbits(s, s->cnt & 7);
            const uint32_t len = zbits(s, 16), nlen = zbits(s, 16);
            if (zover(s)) why = "premature end of the zlib data";
            else if (nlen != (len ^ 0xffff)) why = "zlib corrupt";
            else if (!zroom(o, o->n + len)) why = "out of memory";
            for (uint32_t i = 0; !why && i < len && o->n < o->cap; ++i) {
                o->p[o->n++] = (uint8_t)zbits(s, 8);
                if (zover(s)) why = "read past buffer";
            }
        } else if (type == 1) {
            uint8_t lens[288 + 32];
            memset(lens, 8, 144); memset(lens + 144, 9, 112); memset(lens + 256, 7, 24); memset(lens + 280, 8, 8);
            memset(lens + 288, 5, 32);
            if (!(why = zbuild(zl, lens, 288)) && !(why = zbuild(zd, lens + 288, 32))) why = zblock(s, o, zl, zd);
        } else if (type == 2) {
            if (!(why = zdynamic(s, zl, zd))) why = zblock(s, o, zl, zd);
        } else why = "bad block type";
    }
    free(zl);
    return why;
}

int png_inflate_host(const uint8_t *z, size_t zbytes, uint8_t *out, size_t cap, size_t *produced, char *err, size_t errlen)
{
    if (!z || (!out && cap) || !produced) return fail(err, errlen, "png_inflate_host: null argument");
    zsrc s = {0};
    s.cur = z; s.end = z + zbytes;
    zout o = {out, 0, cap, cap, 0};
    const char *why = zinflate(&s, &o);
    *produced = o.n;
    return why ? fail(err, errlen, why) : 0;
}

/* ------------------------------------------------------------------------------------------------------------- chunks */
static const uint8_t png_sig[8] = {137, 80, 78, 71, 13, 10, 26, 10};
static const int adam7_xorig[7] = {0, 4, 0, 2, 0, 1, 0}, adam7_yorig[7] = {0, 0, 4, 0, 2, 0, 1};
static const int adam7_xspc[7] = {8, 8, 4, 4, 2, 2, 1}, adam7_yspc[7] = {8, 8, 8, 4, 4, 2, 2};

static void png_layout(dnq_png *p)
{
    size_t at = 0;
    p->npasses = 0;
    for (int k = 0; k < (p->interlace ? 7 : 1); ++k) {
        const int w = p->interlace ? (p->w - adam7_xorig[k] + adam7_xspc[k] - 1) / adam7_xspc[k] : p->w;
        const int rows = p->interlace ? (p->h - adam7_yorig[k] + adam7_yspc[k] - 1) / adam7_yspc[k] : p->h;
        if (w <= 0 || rows <= 0) continue; /* a pass without pixels holds no bytes */
        dnq_png_pass *q = &p->pass[p->npasses++];
        q->w = w; q->rows = rows; q->index = k;
        q->row_bytes = (int)(((size_t)w * (size_t)p->channels * (size_t)p->depth + 7) >> 3);
        q->offset = at;
        at += (size_t)rows * ((size_t)q->row_bytes + 1);
    }
    p->filtered_bytes = at;
}

static int png_parse(const uint8_t *data, size_t bytes, dnq_png *p, int inflate, char *err, size_t errlen)
{
    if (!data || !p) return fail(err, errlen, "png: null argument");
    memset(p, 0, sizeof(*p));
    if (bytes < 8 || memcmp(data, png_sig, 8)) return fail(err, errlen, "bad png sig");
    size_t pos = 8, first_idat = 0;
    int first = 1, seen_idat = 0;
    for (;;) {
        if (pos + 8 > bytes) return fail(err, errlen, "truncated file: no IEND");
        const uint32_t len = be32(data + pos), type = be32(data + pos + 4);
        const uint8_t *d = data + pos + 8;
        if (len > bytes - (pos + 8)) return fail(err, errlen, type == CHUNK('I', 'D', 'A', 'T') ? "outofdata" : "truncated chunk");
        if (type == CHUNK('C', 'g', 'B', 'I')) return fail(err, errlen, "CgBI (Apple) PNG is not supported");
        if (type != CHUNK('I', 'H', 'D', 'R') && first) return fail(err, errlen, "first not IHDR");
        if (type == CHUNK('I', 'H', 'D', 'R')) {
            if (!first) return fail(err, errlen, "multiple IHDR");
            first = 0;
            if (len != 13) return fail(err, errlen, "bad IHDR len");
            const uint32_t w = be32(d), h = be32(d + 4);
            if (w > (1u << 24) || h > (1u << 24)) return fail(err, errlen, "too large");
            p->depth = d[8]; p->color = d[9];
            if (p->depth != 1 && p->depth != 2 && p->depth != 4 && p->depth != 8 && p->depth != 16) return fail(err, errlen, "1/2/4/8/16-bit only");
            if (p->color > 6) return fail(err, errlen, "bad ctype");
            if (p->color == 3 && p->depth == 16) return fail(err, errlen, "bad ctype");
            if (p->color != 3 && (p->color & 1)) return fail(err, errlen, "bad ctype");
            if (d[10]) return fail(err, errlen, "bad comp method");
            if (d[11]) return fail(err, errlen, "bad filter method");
            if (d[12] > 1) return fail(err, errlen, "bad interlace method");
            if (!w || !h) return fail(err, errlen, "0-pixel image");
            if (w > DNQ_PNG_MAX_DIM || h > DNQ_PNG_MAX_DIM) return fail(err, errlen, "width or height above 32768");
            p->w = (int)w; p->h = (int)h; p->interlace = d[12];
            p->channels = p->color == 3 ? 1 : (p->color & 2 ? 3 : 1) + (p->color & 4 ? 1 : 0);
            p->bpp = p->depth < 8 ? 1 : p->channels * p->depth / 8;
        } else if (type == CHUNK('P', 'L', 'T', 'E')) {
            if (len > 256 * 3 || len % 3) return fail(err, errlen, "invalid PLTE");
            p->pal_len = (int)(len / 3);
            memset(p->palette, 0, sizeof(p->palette));
            memcpy(p->palette, d, len);
        } else if (type == CHUNK('t', 'R', 'N', 'S')) {
            if (seen_idat) return fail(err, errlen, "tRNS after IDAT");
            if (p->color == 3) {
                if (p->pal_len == 0) return fail(err, errlen, "tRNS before PLTE");
                if (len > (uint32_t)p->pal_len) return fail(err, errlen, "bad tRNS len");
            } else {
                if (!(p->channels & 1)) return fail(err, errlen, "tRNS with alpha");
                if (len != (uint32_t)p->channels * 2) return fail(err, errlen, "bad tRNS len");
            }
            p->has_trns = 1;
        } else if (type == CHUNK('I', 'D', 'A', 'T')) {
            if (p->color == 3 && !p->pal_len) return fail(err, errlen, "no PLTE");
            if (!seen_idat) first_idat = pos;
            seen_idat = 1;
        } else if (type == CHUNK('I', 'E', 'N', 'D')) {
            if (!seen_idat) return fail(err, errlen, "no IDAT");
            break;
        } else if (!(type & (1u << 29))) {
            char why[40];
            snprintf(why, sizeof(why), "XXXX PNG chunk not known");
            for (int k = 0; k < 4; ++k) why[k] = d[k - 4] >= 32 && d[k - 4] < 127 ? (char)d[k - 4] : '?';
            return fail(err, errlen, why);
        }
        pos += 8 + (size_t)len + 4; /* the CRC is not verified; where the file ends inside it, the next header is missing */
    }
    png_layout(p);
    if (!inflate) return 0;
    zsrc s = {0};
    s.file = data; s.file_bytes = bytes; s.next = first_idat;
    zout o = {NULL, 0, 0, p->filtered_bytes, 1};
    const char *why = zinflate(&s, &o);
    if (!why && o.n < p->filtered_bytes) why = "not enough pixels";
    for (int k = 0; !why && k < p->npasses; ++k) /* the first byte of every row, so that the device needs no status word */
        for (int y = 0; y < p->pass[k].rows; ++y)
            if (o.p[p->pass[k].offset + (size_t)y * ((size_t)p->pass[k].row_bytes + 1)] > 4) { why = "invalid filter"; break; }
    if (why) {
        free(o.p);
        memset(p, 0, sizeof(*p));
        return fail(err, errlen, why);
    }
    p->filtered = o.p;
    return 0;
}

int png_decode_host(const uint8_t *data, size_t bytes, dnq_png *out, char *err, size_t errlen) { return png_parse(data, bytes, out, 1, err, errlen); }
int png_info_host(const uint8_t *data, size_t bytes, dnq_png *out, char *err, size_t errlen) { return png_parse(data, bytes, out, 0, err, errlen); }

void png_free(dnq_png *p)
{
    if (!p) return;
    free(p->filtered);
    p->filtered = NULL;
}
