/*
 * jpeg.c -- marker parsing (jpeg_markers.h, shared with jpeg_scan.c) and Huffman decoding of baseline JPEG files into quantised
 * coefficients (jpeg.h).  Written from the JPEG standard (ITU-T T.81: B.2 marker segments, C / F.2.2 Huffman tables and decoding)
 * with stb_image's refusals and tolerances as the reference loads files with it (ref: src/stb_image.h:2836-3155): the same messages
 * for the same structural errors, its leniency towards fill bytes and padding between segments, its rule that a missing restart
 * marker ends the scan.
 *
 * Nothing here trusts the bytes: the reader never moves past `end`, a Huffman code that names no symbol, a DC category above 15 and a
 * run that leaves the block are errors, and a stream that ends early leaves the remaining blocks zero.
 */
#include "jpeg_markers.h"

/* the entropy-coded segment as a bit stream: byte stuffing removed, stopped by a marker or the end of the data */
typedef struct {
    const uint8_t *p, *end;
    uint64_t buf; /* the next `bits` bits, from the top */
    int bits;
    int pad;     /* of those, zero bits appended after the data stopped */
    int stopped; /* no more data bytes: a marker or the end of the buffer was reached */
    int marker;  /* the marker that stopped the reader, 0: none */
} bit_reader;


static void br_fill(bit_reader *br)
{
    while (br->bits <= 56) {
        unsigned b = 0;
        if (!br->stopped) {
            if (br->p >= br->end) {
                br->stopped = 1;
            } else {
                b = *br->p++;
                if (b == 0xFF) { /* fill bytes, then a stuffed zero (the data byte 0xFF) or a marker */
                    const uint8_t *q = br->p;
                    while (q < br->end && *q == 0xFF) ++q;
                    if (q >= br->end) {
                        br->p = br->end; br->stopped = 1; b = 0;
                    } else if (*q == 0) {
                        br->p = q + 1;
                    } else {
                        br->marker = *q; br->p = q + 1; br->stopped = 1; b = 0;
                    }
                }
            }
        }
        if (br->stopped) br->pad += 8;
        br->buf |= (uint64_t)b << (56 - br->bits);
        br->bits += 8;
    }
}

static inline unsigned br_peek(const bit_reader *br, int n) { return (unsigned)(br->buf >> (64 - n)); }
static inline void br_drop(bit_reader *br, int n) { br->buf <<= n; br->bits -= n; }

/* a Huffman-coded symbol (at most 16 bits; the caller keeps 32 in the buffer), -1: no code of the table matches */
static int huff_symbol(bit_reader *br, const huff_table *h)
{
    const unsigned v = br_peek(br, 16);
    const unsigned e = h->look[v >> 8];
    if (e) { br_drop(br, (int)(e >> 8)); return (int)(e & 255); }
    for (int l = 9; l <= 16; ++l) {
        const int c = (int)(v >> (16 - l));
        if (c < h->maxcode[l]) {
            const int idx = h->first[l] + c - h->mincode[l];
            if (c < h->mincode[l] || idx >= h->nvalues) return -1;
            br_drop(br, l);
            return h->values[idx];
        }
    }
    return -1;
}

/* T.81 F.2.2.1 RECEIVE + EXTEND: n bits, 1 <= n <= 15, as a signed value */
static inline int receive_extend(bit_reader *br, int n)
{
    const int v = (int)br_peek(br, n);
    br_drop(br, n);
    return v < (1 << (n - 1)) ? v - (1 << n) + 1 : v;
}

/* one block into blk[64] (natural order); *pred: the component's DC prediction, kept modulo 2^32 */
static int decode_block(parser *p, bit_reader *br, const huff_table *hdc, const huff_table *hac, uint32_t *pred, int16_t *blk)
{
    memset(blk, 0, 64 * sizeof(int16_t));
    if (br->bits < 32) br_fill(br);
    const int t = huff_symbol(br, hdc);
    if (t < 0) return fail(p, "bad huffman code");
    if (t > 15) return fail(p, "bad DC category");
    if (t) *pred += (uint32_t)receive_extend(br, t);
    blk[0] = (int16_t)(uint16_t)*pred;
    for (int k = 1; k < 64;) {
        if (br->bits < 32) br_fill(br);
        const int rs = huff_symbol(br, hac);
        if (rs < 0) return fail(p, "bad huffman code");
        const int s = rs & 15, r = rs >> 4;
        if (!s) {
            if (r != 15) break; /* end of block */
            k += 16;
            continue;
        }
        k += r;
        if (k > 63) return fail(p, "coefficient index past the end of the block");
        blk[zigzag_to_natural[k++]] = (int16_t)receive_extend(br, s);
    }
    return 0;
}

/* the entropy-coded segment behind a scan header.  p->pos ends behind the marker that stopped the bit reader, which is returned in
 * *pending (0: none was reached). */
static int decode_scan(parser *p, int ns, const int *order, const int *hd, const int *ha, int *pending)
{
    dnq_jpeg *j = p->j;
    bit_reader br = {p->data + p->pos, p->data + p->n, 0, 0, 0, 0, 0};
    uint32_t pred[3] = {0, 0, 0};
    const int interval = j->restart_interval > 0 ? j->restart_interval : INT_MAX;
    int todo = interval, done = 0;
    /* one component: its blocks in raster order over its real size; several: MCU by MCU, every component's h x v blocks */
    const dnq_jpeg_comp *k0 = &j->comp[order[0]];
    const int units_x = ns == 1 ? (k0->w + 7) >> 3 : j->comp[0].blocks_w / j->comp[0].h;
    const int units_y = ns == 1 ? (k0->rows + 7) >> 3 : j->comp[0].blocks_h / j->comp[0].v;
    for (int uy = 0; uy < units_y && !done; ++uy)
        for (int ux = 0; ux < units_x && !done; ++ux) {
            for (int i = 0; i < ns; ++i) {
                dnq_jpeg_comp *k = &j->comp[order[i]];
                const int bh = ns == 1 ? 1 : k->h, bv = ns == 1 ? 1 : k->v;
                for (int y = 0; y < bv; ++y)
                    for (int x = 0; x < bh; ++x) {
                        const size_t bx = (size_t)ux * bh + x, by = (size_t)uy * bv + y; /* < blocks_w, blocks_h by construction */
                        if (decode_block(p, &br, &p->hdc[hd[i]], &p->hac[ha[i]], &pred[order[i]], k->coef + (by * k->blocks_w + bx) * 64))
                            return -1;
                    }
            }
            if (br.bits < br.pad) { done = 1; break; } /* the data ended inside this unit: the rest stays zero */
            if (--todo <= 0) {
                br_fill(&br);
                if (br.marker < 0xD0 || br.marker > 0xD7) { done = 1; break; } /* no restart marker where one is due: the scan ends */
                const uint8_t *at = br.p;
                br = (bit_reader){at, p->data + p->n, 0, 0, 0, 0, 0};
                pred[0] = pred[1] = pred[2] = 0;
                todo = interval;
            }
        }
    if (!br.marker && !br.stopped) { /* pull the reader up to the marker behind the data, if it is next */
        br.bits = 0; br.buf = 0;
        br_fill(&br);
    }
    p->pos = (size_t)(br.p - p->data);
    *pending = br.marker;
    return 0;
}

int jpeg_decode_host(const uint8_t *data, size_t bytes, dnq_jpeg *out, char *err, size_t errlen) { return run_parser(data, bytes, out, err, errlen, 0, 0, decode_scan, NULL); }
int jpeg_info_host(const uint8_t *data, size_t bytes, dnq_jpeg *out, char *err, size_t errlen) { return run_parser(data, bytes, out, err, errlen, 1, 0, decode_scan, NULL); }

void jpeg_free(dnq_jpeg *j)
{
    if (!j) return;
    for (int i = 0; i < 3; ++i) free(j->comp[i].coef);
    memset(j, 0, sizeof(*j));
}
