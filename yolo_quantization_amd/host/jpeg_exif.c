/*
 * jpeg_exif.c -- the EXIF orientation of a JPEG file: the marker walk to APP1 "Exif\0\0", the TIFF header in either byte order, IFD0's
 * tag 0x0112.  Everything that is not exactly that gives 1, the value of a file without the tag; every read is checked against the
 * buffer (and the segment) before it is made.  The decoder does not call this: the caller puts the value into a mi355_frame_view.
 */
#include <stddef.h>
#include <stdint.h>
#include "darknet_q.h"

/* big_endian != 0: most significant byte first */
static unsigned rd16(const uint8_t *p, int big_endian) { return big_endian ? (unsigned)p[0] << 8 | p[1] : (unsigned)p[1] << 8 | p[0]; }
static uint32_t rd32(const uint8_t *p, int big_endian)
{
    return big_endian ? (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]
                      : (uint32_t)p[3] << 24 | (uint32_t)p[2] << 16 | (uint32_t)p[1] << 8 | p[0];
}

/* the TIFF block of an Exif segment: n bytes at t */
static int tiff_orientation(const uint8_t *t, size_t n)
{
    if (n < 8) return 1;
    int be;
    if (t[0] == 'I' && t[1] == 'I') be = 0;
    else if (t[0] == 'M' && t[1] == 'M') be = 1;
    else return 1;
    if (rd16(t + 2, be) != 42) return 1;
    const size_t ifd = rd32(t + 4, be);
    if (ifd > n || n - ifd < 2) return 1;
    const size_t entries = rd16(t + ifd, be);
    for (size_t k = 0; k < entries; ++k) {
        const size_t at = ifd + 2 + 12 * k;
        if (at > n || n - at < 12) return 1; /* the directory runs out of the block */
        const uint8_t *e = t + at;
        if (rd16(e, be) != 0x0112) continue;
        if (rd16(e + 2, be) != 3 || rd32(e + 4, be) != 1) return 1; /* SHORT, count 1 */
        const unsigned v = rd16(e + 8, be);
        return v >= 1 && v <= 8 ? (int)v : 1;
    }
    return 1;
}

int jpeg_exif_orientation_host(const uint8_t *data, size_t bytes)
{
    if (!data || bytes < 4 || data[0] != 0xFF || data[1] != 0xD8) return 1;
    size_t at = 2;
    while (bytes - at >= 2) { /* at <= bytes always */
        if (data[at] != 0xFF) return 1;
        const unsigned m = data[at + 1];
        if (m == 0xFF) { ++at; continue; } /* a fill byte */
        at += 2;
        if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue; /* no length */
        if (m == 0xD8 || m == 0xD9 || m == 0xDA || m == 0x00) return 1; /* a second SOI, the end, the scan: no Exif in front of it */
        if (bytes - at < 2) return 1;
        const size_t len = rd16(data + at, 1); /* counts its own two bytes */
        if (len < 2 || len > bytes - at) return 1;
        const uint8_t *p = data + at + 2;
        const size_t n = len - 2;
        if (m == 0xE1 && n >= 6 && p[0] == 'E' && p[1] == 'x' && p[2] == 'i' && p[3] == 'f' && p[4] == 0 && p[5] == 0)
            return tiff_orientation(p + 6, n - 6);
        at += len;
    }
    return 1;
}
