/*
 * jpeg.h -- the host half of the JPEG input path: marker parsing and Huffman (entropy) decoding of baseline JPEG files into
 * quantised DCT coefficients.  Plain C, no dependency, no device.  Everything after the entropy decode -- dequantisation, the 8x8
 * inverse DCT, chroma upsampling, YCbCr -> RGB -- runs on the device (csrc/jpeg.hip, mi355_jpeg_idct / mi355_jpeg_to_rgb) and is
 * written to give, byte for byte, the pixels stbi_load(file, .., 3) of the reference's stb_image v2.19 returns
 * (ref: src/stb_image.h, src/image.c:1293-1315).
 *
 * Accepted: SOF0 and 8-bit SOF1 Huffman files of 1 or 3 components, sampling factors 1..4 per axis where every component's factor
 * divides the largest one (4:4:4, 4:2:2, 4:4:0, 4:2:0, 4:1:1, 4:1:0, ...), interleaved and one-component-per-scan scans, restart
 * intervals, 8- and 16-bit quantiser tables (redefinable between scans).  Refused, each with its own message: progressive,
 * arithmetic-coded, lossless / hierarchical and 12-bit files, 4 components (CMYK / YCCK), sampling factors that do not divide the
 * largest, a zero width or height, and the structural errors stb_image names (ref: src/stb_image.h:2841-3032).  Every read is checked
 * against the end of the buffer and every Huffman symbol, run and coefficient index against its range: corrupt bytes give an error or
 * some image, never an access outside the buffers.  What stb_image makes of a corrupt file is not reproduced.
 */
#ifndef DNQ_JPEG_H
#define DNQ_JPEG_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* how the device turns the component planes into RGB (ref: src/stb_image.h:3587, the values of mi355_jpeg_image.mode) */
#define DNQ_JPEG_YCBCR 0 /* three components, YCbCr -> RGB */
#define DNQ_JPEG_RGB   1 /* three components taken as R, G, B: component ids 'R','G','B', or Adobe transform 0 without a JFIF marker */
#define DNQ_JPEG_GREY  2 /* one component, replicated */

typedef struct dnq_jpeg_comp {
    int id;                 /* component id of the frame header */
    int h, v;               /* sampling factors, 1..4 */
    int hs, vs;             /* upsampling factors h_max / h, v_max / v */
    int w, rows;            /* the component's real size in samples: ceil(width * h / h_max) x ceil(height * v / v_max) */
    int blocks_w, blocks_h; /* the MCU-padded plane in 8x8 blocks; block (bx, by) is coef[(by * blocks_w + bx) * 64 ..] */
    int tq;                 /* quantiser table the frame header names */
    int scans;              /* scans that carried this component */
    int16_t *coef;          /* [blocks_h * blocks_w][64] quantised coefficients, natural (de-zigzagged, row-major) order; blocks no
                               scan reached stay zero.  A DC value beyond 16 bits (corrupt files only) keeps its low 16 bits, which
                               is all the 16-bit dequantised product depends on */
    uint16_t quant[64];     /* natural order: the table that was current when this component's (last) scan was decoded */
} dnq_jpeg_comp;

struct dnq_jpeg {
    int w, h;               /* pixels */
    int ncomp;              /* 1 or 3 */
    int mode;               /* DNQ_JPEG_* */
    int h_max, v_max;
    int sof;                /* 0xC0 or 0xC1 */
    int jfif;               /* a JFIF APP0 segment was seen */
    int adobe_transform;    /* APP14 colour transform, -1: no Adobe segment */
    int restart_interval;   /* the last DRI value */
    int nscans;
    dnq_jpeg_comp comp[3];
};
typedef struct dnq_jpeg dnq_jpeg;

/* Parse and entropy-decode `bytes` bytes at data.  0: *out is filled and owns its coefficient arrays (jpeg_free).  -1: the reason is
 * in err (when errlen > 0), *out holds nothing.  Never exits, never touches a device. */
int jpeg_decode_host(const uint8_t *data, size_t bytes, dnq_jpeg *out, char *err, size_t errlen);
/* The headers alone (everything up to the first scan): sizes, sampling, tables named, colour mode as far as the markers before the
 * first SOS decide it; coef is NULL and quant zero.  The same refusals as jpeg_decode_host for what the headers show. */
int jpeg_info_host(const uint8_t *data, size_t bytes, dnq_jpeg *out, char *err, size_t errlen);
void jpeg_free(dnq_jpeg *j);

#ifdef __cplusplus
}
#endif
#endif
