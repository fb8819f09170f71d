/*
 * png_scan.c -- find the deflate stream of a PNG without inflating it (png_scan.h).  png_info_host validates the chunk walk; the walk
 * here then only gathers, IDAT chunk after IDAT chunk, up to IEND.
 */
#include "png_scan.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static int fail(dnq_png_scan *out, char *err, size_t errlen, const char *why)
{
    if (err && errlen) snprintf(err, errlen, "%s", why);
    png_scan_free(out);
    memset(out, 0, sizeof(*out));
    return -1;
}

static uint32_t be32(const uint8_t *p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]; }

void png_scan_free(dnq_png_scan *s)
{
    if (!s) return;
    free(s->z);
    s->z = NULL; s->nbytes = s->zcap = 0;
}

int png_scan_host(const uint8_t *data, size_t bytes, dnq_png_scan *out, char *err, size_t errlen)
{
    if (!out) { if (err && errlen) snprintf(err, errlen, "png: null argument"); return -1; }
    memset(out, 0, sizeof(*out));
    if (png_info_host(data, bytes, &out->im, err, errlen)) { memset(out, 0, sizeof(*out)); return -1; }
    /* two passes over chunks png_info_host has found whole: the size, then the bytes */
    size_t total = 0;
    for (int pass = 0; pass < 2; ++pass) {
        size_t at = 0;
        for (size_t pos = 8; pos + 8 <= bytes;) {
            const uint32_t len = be32(data + pos), type = be32(data + pos + 4);
            if (type == 0x49454e44u) break; /* IEND */
            if (type == 0x49444154u) {      /* IDAT */
                if (pass) {
                    const size_t skip = at < 2 ? (2 - at < len ? 2 - at : len) : 0; /* the zlib header, over however many chunks */
                    if (len > skip) memcpy(out->z + (at + skip - 2), data + pos + 8 + skip, len - skip);
                }
                at += len;
            }
            pos += 12 + (size_t)len;
        }
        if (pass) break;
        total = at;
        uint8_t head[2] = {0, 0};
        size_t got = 0;
        for (size_t pos = 8; pos + 8 <= bytes && got < 2;) {
            const uint32_t len = be32(data + pos), type = be32(data + pos + 4);
            if (type == 0x49454e44u) break;
            if (type == 0x49444154u)
                for (uint32_t k = 0; k < len && got < 2; ++k) head[got++] = data[pos + 8 + k];
            pos += 12 + (size_t)len;
        }
        if (got < 2 || (head[0] * 256 + head[1]) % 31 != 0) return fail(out, err, errlen, "bad zlib header");
        if (head[1] & 32) return fail(out, err, errlen, "no preset dict");
        if ((head[0] & 15) != 8) return fail(out, err, errlen, "bad compression");
        out->nbytes = total - 2;
        out->zcap = ((out->nbytes + 3) & ~(size_t)3) + 8;
        out->z = calloc(out->zcap, 1);
        if (!out->z) return fail(out, err, errlen, "out of memory");
    }
    return 0;
}
