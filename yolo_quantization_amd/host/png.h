/*
 * png.h -- the host half of the PNG input path: chunk parsing and inflate (RFC 1950 / 1951) of PNG files into their filtered scanlines.
 * Plain C, no dependency, no device.  Everything after the inflate -- scanline reconstruction (None / Sub / Up / Average / Paeth),
 * de-interlacing, bit-depth and palette expansion, the reduction to RGB -- runs on the device (csrc/png.hip, mi355_png_unfilter /
 * mi355_png_to_rgb) and is written to give, byte for byte, the pixels stbi_load(file, .., 3) of the reference's stb_image v2.19
 * returns (ref: src/stb_image.h:4307-4931).
 *
 * Accepted: all 15 legal colour-type / depth pairs, plain and Adam7, any number of IDAT chunks of any sizes, tRNS (validated, without
 * effect on RGB), inflated data longer than the image needs.  Ancillary chunks are skipped; chunk CRCs and the Adler-32 are not
 * verified, as stb_image does not verify them.  Refused, each with its own message (stb's words where it has them): see png.c.  Of our
 * own: a width or height above 32768, CgBI files, truncated files.  Every read is checked against the end of the buffer and every
 * Huffman symbol, length and distance against its range; the inflated output is capped at the bytes the image needs, so no input
 * makes the decoder allocate more than that.
 */
#ifndef DNQ_PNG_H
#define DNQ_PNG_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DNQ_PNG_MAX_DIM 32768

typedef struct dnq_png_pass {
    int w, rows;      /* the pass in pixels */
    int row_bytes;    /* bytes of one row without its filter byte: ceil(w * channels * depth / 8) */
    int index;        /* 0..6: the Adam7 pass; 0 for a file that is not interlaced */
    size_t offset;    /* of the pass's first filter byte in `filtered`; rows are row_bytes + 1 apart */
} dnq_png_pass;

struct dnq_png {
    int w, h;         /* pixels */
    int depth;        /* 1, 2, 4, 8, 16 */
    int color;        /* 0 grey, 2 RGB, 3 palette, 4 grey + alpha, 6 RGBA */
    int interlace;    /* 0, or 1: Adam7 */
    int channels;     /* samples per pixel in the file: 1, 3, 1, 2, 4 */
    int bpp;          /* the filter unit in bytes: channels * depth / 8, 1 for depths below 8 */
    int pal_len;      /* PLTE entries, 0: no PLTE */
    int has_trns;
    int npasses;      /* the passes that hold pixels: 1 for a plain file, up to 7 */
    dnq_png_pass pass[7];
    uint8_t palette[768]; /* R, G, B per entry, zero beyond pal_len */
    size_t filtered_bytes; /* what the image needs: the sum over the passes of rows * (row_bytes + 1) */
    uint8_t *filtered;     /* the inflated bytes, exactly filtered_bytes of them; NULL from png_info_host */
};
typedef struct dnq_png dnq_png;

/* Parse the chunks and inflate.  0: *out is filled and owns `filtered` (png_free).  -1: the reason is in err (when errlen > 0), *out
 * holds nothing.  Never exits, never touches a device. */
int png_decode_host(const uint8_t *data, size_t bytes, dnq_png *out, char *err, size_t errlen);
/* The same walk over the chunks with the same refusals, without the inflate: `filtered` stays NULL. */
int png_info_host(const uint8_t *data, size_t bytes, dnq_png *out, char *err, size_t errlen);
void png_free(dnq_png *p);
/* Inflate a zlib stream into at most cap bytes at out; what the stream holds beyond them is not stored.  *produced: the bytes stored.
 * 0, or -1 with the reason in err.  (png_decode_host's inflate, exported for its tests.) */
int png_inflate_host(const uint8_t *z, size_t zbytes, uint8_t *out, size_t cap, size_t *produced, char *err, size_t errlen);

#ifdef __cplusplus
}
#endif
#endif
