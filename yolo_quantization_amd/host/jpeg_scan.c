/*
 * jpeg_scan.c -- find the entropy-coded segments of a baseline JPEG without decoding them (jpeg_scan.h).  The markers are parsed by
 * the code jpeg.c parses them with (jpeg_markers.h); behind a scan header this file walks the bytes to the next marker that is neither
 * a stuffed zero nor a restart, and copies each restart interval out unstuffed.
 */
#include "jpeg_scan.h"
#include "jpeg_markers.h"

static int grow(void **buf, size_t elem, size_t need, size_t *cap)
{
    if (need <= *cap) return 0;
    size_t n = *cap ? *cap * 2 : 16;
    while (n < need) n *= 2;
    void *q = realloc(*buf, n * elem);
    if (!q) return -1;
    *buf = q;
    *cap = n;
    return 0;
}

static void huff_out(mi355_jpeg_huff *o, const huff_table *h)
{
    memset(o, 0, sizeof(*o));
    memcpy(o->look, h->look, sizeof(o->look));
    for (int l = 0; l <= 16; ++l) { o->maxcode[l] = h->maxcode[l]; o->mincode[l] = h->mincode[l]; o->first[l] = h->first[l]; }
    o->nvalues = h->nvalues;
    memcpy(o->values, h->values, sizeof(o->values));
}

static int list_scan(parser *p, int ns, const int *order, const int *hd, const int *ha, int *pending)
{
    dnq_jpeg *j = p->j;
    dnq_jpeg_scan_list *L = p->user;
    dnq_jpeg_scan_seg proto;
    memset(&proto, 0, sizeof(proto));
    /* the tables as they stand now */
    size_t cap = (size_t)L->cap_huff;
    if (grow((void **)&L->huff, sizeof(mi355_jpeg_huff), (size_t)L->nhuff + 2 * (size_t)ns, &cap)) return fail(p, "out of memory");
    L->cap_huff = (int)cap;
    const dnq_jpeg_comp *k0 = &j->comp[order[0]];
    proto.ncomp = ns;
    proto.scan = j->nscans - 1;
    proto.units_x = ns == 1 ? (k0->w + 7) >> 3 : j->comp[0].blocks_w / j->comp[0].h;
    proto.units_y = ns == 1 ? (k0->rows + 7) >> 3 : j->comp[0].blocks_h / j->comp[0].v;
    for (int i = 0; i < ns; ++i) {
        const dnq_jpeg_comp *k = &j->comp[order[i]];
        proto.comp[i] = order[i];
        proto.bh[i] = ns == 1 ? 1 : k->h;
        proto.bv[i] = ns == 1 ? 1 : k->v;
        proto.dc[i] = L->nhuff;
        huff_out(&L->huff[L->nhuff++], &p->hdc[hd[i]]);
        proto.ac[i] = L->nhuff;
        huff_out(&L->huff[L->nhuff++], &p->hac[ha[i]]);
    }
    const long units = (long)proto.units_x * proto.units_y;
    const long interval = j->restart_interval > 0 ? j->restart_interval : units;
    const long want = (units + interval - 1) / interval;

    /* the bytes: a segment is at most what is left of the file, plus its padding */
    const uint8_t *s = p->data + p->pos, *end = p->data + p->n;
    long nseg = 0;
    int marker = 0;
    for (;;) {
        /* one segment: up to a marker or the end of the data */
        size_t room = L->cap_bytes;
        if (grow((void **)&L->bytes, 1, L->nbytes + (size_t)(end - s) + 16, &room)) return fail(p, "out of memory");
        L->cap_bytes = room;
        uint8_t *o = L->bytes + L->nbytes;
        size_t n = 0;
        marker = 0;
        while (s < end) {
            const uint8_t *ff = memchr(s, 0xFF, (size_t)(end - s));
            const size_t plain = (size_t)((ff ? ff : end) - s);
            memcpy(o + n, s, plain);
            n += plain;
            s += plain;
            if (!ff) break;
            ++s;
            while (s < end && *s == 0xFF) ++s; /* fill bytes */
            if (s >= end) break;
            const uint8_t m = *s++;
            if (m == 0) { o[n++] = 0xFF; continue; }
            marker = m;
            break;
        }
        if (nseg < want) {
            if (n > (1u << 28)) return fail(p, "too large: a scan segment of more than 2^28 bytes");
            size_t sc = (size_t)L->cap_segs;
            if (grow((void **)&L->segs, sizeof(dnq_jpeg_scan_seg), (size_t)L->nsegs + 1, &sc)) return fail(p, "out of memory");
            L->cap_segs = (int)sc;
            dnq_jpeg_scan_seg *g = &L->segs[L->nsegs++];
            *g = proto;
            g->first_unit = (int)(nseg * interval);
            g->nunits = (int)(units - nseg * interval < interval ? units - nseg * interval : interval);
            g->nbytes = (uint32_t)n;
            g->offset = L->nbytes;
            const size_t padded = ((n + 3) & ~(size_t)3) + 8;
            memset(o + n, 0, padded - n);
            L->nbytes += padded;
        }
        ++nseg;
        if (marker < 0xD0 || marker > 0xD7) break; /* the end of the data or the marker that ends the scan */
    }
    p->pos = (size_t)(s - p->data);
    *pending = marker;
    return 0;
}

void jpeg_scan_free(dnq_jpeg_scan_list *L)
{
    if (!L) return;
    free(L->segs); free(L->huff); free(L->bytes);
    memset(L, 0, sizeof(*L));
}

int jpeg_scan_host(const uint8_t *data, size_t bytes, dnq_jpeg *out, dnq_jpeg_scan_list *scans, char *err, size_t errlen)
{
    if (!scans) return -1;
    memset(scans, 0, sizeof(*scans));
    const int rc = run_parser(data, bytes, out, err, errlen, 0, 1, list_scan, scans);
    if (rc) jpeg_scan_free(scans);
    return rc;
}
