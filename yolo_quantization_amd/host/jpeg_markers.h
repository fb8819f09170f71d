/*
 * jpeg_markers.h -- the marker parser both host halves of the JPEG path share: jpeg.c (which decodes the scans) and jpeg_scan.c (which
 * only lists them) include it and supply the function that takes over behind a scan header (parser.scan).  Everything here is static:
 * each of the two files compiles on its own.  Written from ITU-T T.81 B.2 with stb_image's refusals (see jpeg.c).
 */
#ifndef DNQ_JPEG_MARKERS_H
#define DNQ_JPEG_MARKERS_H
#include "jpeg.h"
#include <limits.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

/* position in the 8x8 block (row-major) of the k-th coefficient of the zigzag sequence (T.81 figure A.6) */
static const uint8_t zigzag_to_natural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                              41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                              30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

/* total 8x8 blocks of all components an image may have: 256 MB of coefficients */
#define JPEG_MAX_BLOCKS (1L << 21)

typedef struct {
    int defined, nvalues;
    uint8_t values[256];
    int mincode[17], maxcode[17], first[17]; /* per code length 1..16: smallest code, largest code + 1, index of its first symbol */
    uint16_t look[256];                      /* by the next 8 bits: (length << 8) | symbol of a code of <= 8 bits, 0: a longer code */
} huff_table;

typedef struct parser parser;
struct parser {
    const uint8_t *data;
    size_t n, pos;
    char *err;
    size_t errlen;
    dnq_jpeg *j;
    int headers_only, no_coef, got_sof, rgb_ids;
    uint16_t qt[4][64];
    int qt_set[4];
    huff_table hdc[4], hac[4];
    /* behind a scan header (parse_sos_header): consume the entropy-coded data from p->pos on, leave p->pos behind the marker that
     * ended it and that marker in *pending (0: none was reached) */
    int (*scan)(parser *p, int ns, const int *order, const int *hd, const int *ha, int *pending);
    void *user;
};

static int fail(parser *p, const char *fmt, ...)
{
    if (p->err && p->errlen) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(p->err, p->errlen, fmt, ap);
        va_end(ap);
    }
    return -1;
}

/* -1 at the end of the data */
static int get8(parser *p) { return p->pos < p->n ? p->data[p->pos++] : -1; }
static int get16(parser *p)
{
    if (p->n - p->pos < 2) { p->pos = p->n; return -1; }
    const int v = p->data[p->pos] << 8 | p->data[p->pos + 1];
    p->pos += 2;
    return v;
}

/* the next marker code: bytes in front of the 0xFF and repeated 0xFF fill bytes are skipped.  -1: the data ended */
static int next_marker(parser *p)
{
    while (p->pos < p->n && p->data[p->pos] != 0xFF) ++p->pos;
    while (p->pos < p->n && p->data[p->pos] == 0xFF) ++p->pos;
    return get8(p);
}

static int parse_dqt(parser *p)
{
    int L = get16(p);
    if (L < 0) return fail(p, "truncated DQT");
    L -= 2;
    while (L > 0) {
        const int q = get8(p);
        if (q < 0) return fail(p, "truncated DQT");
        const int prec = q >> 4, t = q & 15;
        if (prec != 0 && prec != 1) return fail(p, "bad DQT type");
        if (t > 3) return fail(p, "bad DQT table");
        for (int i = 0; i < 64; ++i) {
            const int v = prec ? get16(p) : get8(p);
            if (v < 0) return fail(p, "truncated DQT");
            p->qt[t][zigzag_to_natural[i]] = (uint16_t)v;
        }
        p->qt_set[t] = 1;
        L -= prec ? 129 : 65;
    }
    return L == 0 ? 0 : fail(p, "bad DQT len");
}

static int parse_dht(parser *p)
{
    int L = get16(p);
    if (L < 0) return fail(p, "truncated DHT");
    L -= 2;
    while (L > 0) {
        const int q = get8(p);
        if (q < 0) return fail(p, "truncated DHT");
        const int tc = q >> 4, th = q & 15;
        if (tc > 1 || th > 3) return fail(p, "bad DHT header");
        huff_table *h = tc ? &p->hac[th] : &p->hdc[th];
        int count[17], n = 0;
        for (int l = 1; l <= 16; ++l) {
            count[l] = get8(p);
            if (count[l] < 0) return fail(p, "truncated DHT");
            n += count[l];
        }
        if (n > 256) return fail(p, "bad DHT symbol count");
        memset(h, 0, sizeof(*h));
        int code = 0, k = 0;
        for (int l = 1; l <= 16; ++l) { /* canonical codes, T.81 C.2 */
            h->mincode[l] = code;
            h->first[l] = k;
            code += count[l];
            k += count[l];
            h->maxcode[l] = code;
            if (code > (1 << l)) return fail(p, "bad code lengths");
            code <<= 1;
        }
        for (int i = 0; i < n; ++i) {
            const int v = get8(p);
            if (v < 0) return fail(p, "truncated DHT");
            h->values[i] = (uint8_t)v;
        }
        h->nvalues = n;
        for (int l = 1; l <= 8; ++l)
            for (int i = 0; i < count[l]; ++i) {
                const int c = (h->mincode[l] + i) << (8 - l);
                for (int f = 0; f < (1 << (8 - l)); ++f) h->look[c + f] = (uint16_t)(l << 8 | h->values[h->first[l] + i]);
            }
        h->defined = 1;
        L -= 17 + n;
    }
    return L == 0 ? 0 : fail(p, "bad DHT len");
}

/* APPn / COM: the JFIF flag and the Adobe colour transform are read, everything else is skipped */
static int parse_app(parser *p, int m)
{
    int L = get16(p);
    if (L < 2) return fail(p, m == 0xFE ? "bad COM len" : "bad APP len");
    L -= 2;
    const size_t start = p->pos;
    if ((size_t)L > p->n - start) return fail(p, "truncated segment");
    if (m == 0xE0 && L >= 5 && !memcmp(p->data + start, "JFIF", 5)) p->j->jfif = 1;
    if (m == 0xEE && L >= 12 && !memcmp(p->data + start, "Adobe", 6)) p->j->adobe_transform = p->data[start + 11];
    p->pos = start + (size_t)L;
    return 0;
}

static int parse_sof(parser *p, int m)
{
    dnq_jpeg *j = p->j;
    if (p->got_sof) return fail(p, "more than one SOF");
    const int Lf = get16(p);
    if (Lf < 11) return fail(p, "bad SOF len");
    const int prec = get8(p);
    if (prec != 8) return fail(p, "only 8-bit: %d-bit samples are not supported", prec);
    j->h = get16(p);
    if (j->h <= 0) return fail(p, "no header height");
    j->w = get16(p);
    if (j->w <= 0) return fail(p, "0 width");
    const int c = get8(p);
    if (c == 4) return fail(p, "4 components (CMYK / YCCK) are not supported");
    if (c != 3 && c != 1) return fail(p, "bad component count");
    if (Lf != 8 + 3 * c) return fail(p, "bad SOF len");
    j->ncomp = c;
    j->sof = m;
    j->h_max = j->v_max = 1;
    for (int i = 0; i < c; ++i) {
        dnq_jpeg_comp *k = &j->comp[i];
        k->id = get8(p);
        const int q = get8(p);
        k->tq = get8(p);
        if (k->tq < 0) return fail(p, "truncated SOF");
        if (c == 3 && k->id == "RGB"[i]) ++p->rgb_ids;
        k->h = q >> 4;
        k->v = q & 15;
        if (!k->h || k->h > 4) return fail(p, "bad H");
        if (!k->v || k->v > 4) return fail(p, "bad V");
        if (k->tq > 3) return fail(p, "bad TQ");
        if (k->h > j->h_max) j->h_max = k->h;
        if (k->v > j->v_max) j->v_max = k->v;
    }
    if (j->w > 32768 || j->h > 32768) return fail(p, "too large: a width or height above 32768 is not supported");
    const int mcu_x = (j->w + 8 * j->h_max - 1) / (8 * j->h_max), mcu_y = (j->h + 8 * j->v_max - 1) / (8 * j->v_max);
    long blocks = 0;
    for (int i = 0; i < c; ++i) {
        dnq_jpeg_comp *k = &j->comp[i];
        if (j->h_max % k->h || j->v_max % k->v)
            return fail(p, "sampling factors that do not divide the largest factor are not supported (component %d: %dx%d of %dx%d)", i, k->h, k->v,
                        j->h_max, j->v_max);
        k->hs = j->h_max / k->h;
        k->vs = j->v_max / k->v;
        k->w = (j->w * k->h + j->h_max - 1) / j->h_max;
        k->rows = (j->h * k->v + j->v_max - 1) / j->v_max;
        k->blocks_w = mcu_x * k->h;
        k->blocks_h = mcu_y * k->v;
        blocks += (long)k->blocks_w * k->blocks_h;
    }
    if (blocks > JPEG_MAX_BLOCKS) return fail(p, "too large: more than %ld blocks of coefficients", JPEG_MAX_BLOCKS);
    if (!p->headers_only && !p->no_coef)
        for (int i = 0; i < c; ++i) {
            dnq_jpeg_comp *k = &j->comp[i];
            k->coef = calloc((size_t)k->blocks_w * k->blocks_h * 64, sizeof(int16_t));
            if (!k->coef) return fail(p, "out of memory");
        }
    p->got_sof = 1;
    return 0;
}

/* SOS: the scan header.  order[i]: the frame component of scan component i, hd / ha: its DC / AC table; the quantiser of each is
 * pinned as it stands now */
static int parse_sos_header(parser *p, int *ns_out, int *order, int *hd, int *ha)
{
    dnq_jpeg *j = p->j;
    const int Ls = get16(p), ns = get8(p);
    if (ns < 1 || ns > 4 || ns > j->ncomp) return fail(p, "bad SOS component count");
    if (Ls != 6 + 2 * ns) return fail(p, "bad SOS len");
    for (int i = 0; i < ns; ++i) {
        const int id = get8(p), q = get8(p);
        if (q < 0) return fail(p, "truncated SOS");
        int which = 0;
        while (which < j->ncomp && j->comp[which].id != id) ++which;
        if (which == j->ncomp) return fail(p, "bad SOS component id");
        hd[i] = q >> 4;
        ha[i] = q & 15;
        if (hd[i] > 3) return fail(p, "bad DC huff");
        if (ha[i] > 3) return fail(p, "bad AC huff");
        order[i] = which;
    }
    const int ss = get8(p), se = get8(p), aa = get8(p);
    (void)se; /* 63, but some writers leave 0 */
    if (aa < 0) return fail(p, "truncated SOS");
    if (ss != 0 || aa != 0) return fail(p, "bad SOS");
    for (int i = 0; i < ns; ++i) {
        dnq_jpeg_comp *k = &j->comp[order[i]];
        if (!p->hdc[hd[i]].defined || !p->hac[ha[i]].defined) return fail(p, "undefined huffman table");
        if (!p->qt_set[k->tq]) return fail(p, "undefined quantiser table");
        memcpy(k->quant, p->qt[k->tq], sizeof(k->quant)); /* the table as it stands now: a later DQT does not reach back */
        ++k->scans;
    }
    ++j->nscans;
    *ns_out = ns;
    return 0;
}

static int parse(parser *p)
{
    dnq_jpeg *j = p->j;
    if (p->n < 2 || p->data[0] != 0xFF || p->data[1] != 0xD8) return fail(p, "no SOI: not a JPEG file");
    p->pos = 2;
    int pending = 0;
    for (;;) {
        int m = pending;
        pending = 0;
        if (!m) m = next_marker(p);
        if (m < 0) return fail(p, j->nscans ? "expected marker: the data ends without EOI" : p->got_sof ? "no SOS" : "no SOF");
        if (m == 0xD9) break;
        if (m == 0x00 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue; /* a stuffed byte or a stray restart behind a scan; TEM */
        int rc = 0;
        if (m == 0xDA) {
            if (!p->got_sof) return fail(p, "SOS before SOF");
            if (p->headers_only) break;
            int ns = 0, order[4], hd[4], ha[4];
            rc = parse_sos_header(p, &ns, order, hd, ha);
            if (!rc) rc = p->scan(p, ns, order, hd, ha, &pending);
        } else if (m == 0xDB) rc = parse_dqt(p);
        else if (m == 0xC4) rc = parse_dht(p);
        else if (m == 0xDD) {
            if (get16(p) != 4) return fail(p, "bad DRI len");
            j->restart_interval = get16(p);
            if (j->restart_interval < 0) return fail(p, "truncated DRI");
        } else if (m == 0xDC) {
            if (get16(p) != 4) return fail(p, "bad DNL len");
            if (get16(p) != j->h) return fail(p, "bad DNL height");
        } else if ((m >= 0xE0 && m <= 0xEF) || m == 0xFE) rc = parse_app(p, m);
        else if (m == 0xC0 || m == 0xC1) rc = parse_sof(p, m);
        else if (m == 0xC2) return fail(p, "progressive JPEG (SOF2) is not supported");
        else if (m == 0xC3 || (m >= 0xC5 && m <= 0xC7)) return fail(p, "lossless / hierarchical JPEG (SOF%d) is not supported", m - 0xC0);
        else if (m == 0xCC || (m >= 0xC9 && m <= 0xCF)) return fail(p, "arithmetic-coded JPEG is not supported");
        else return fail(p, "unknown marker 0x%02X", m);
        if (rc) return rc;
    }
    if (!p->got_sof) return fail(p, "no SOF");
    if (!p->headers_only) {
        if (!j->nscans) return fail(p, "no SOS");
        for (int i = 0; i < j->ncomp; ++i)
            if (!j->comp[i].scans) return fail(p, "component %d has no scan", i);
    }
    /* ref: src/stb_image.h:3587 */
    j->mode = j->ncomp == 1 ? DNQ_JPEG_GREY : (p->rgb_ids == 3 || (j->adobe_transform == 0 && !j->jfif)) ? DNQ_JPEG_RGB : DNQ_JPEG_YCBCR;
    return 0;
}

static int run_parser(const uint8_t *data, size_t bytes, dnq_jpeg *out, char *err, size_t errlen, int headers_only, int no_coef,
                      int (*scan)(parser *, int, const int *, const int *, const int *, int *), void *user)
{
    if (err && errlen) err[0] = 0;
    if (!out) return -1;
    memset(out, 0, sizeof(*out));
    out->adobe_transform = -1;
    parser *p = calloc(1, sizeof(parser));
    if (!p) return -1;
    p->data = data; p->n = data ? bytes : 0; p->err = err; p->errlen = errlen; p->j = out; p->headers_only = headers_only;
    p->no_coef = no_coef; p->scan = scan; p->user = user;
    const int rc = parse(p);
    free(p);
    if (rc) {
        for (int i = 0; i < 3; ++i) free(out->comp[i].coef);
        memset(out, 0, sizeof(*out));
        return -1;
    }
    return 0;
}
#endif
