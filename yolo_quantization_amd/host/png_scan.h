/*
 * png_scan.h -- the host half of the PNG path when the inflate runs on the device (mi355_png_inflate): the chunks are walked as
 * png_decode_host walks them (png_info_host: the same headers, the same layout, the same refusals in the same words), the two-byte zlib
 * header is checked with the decoder's three messages, and the payload of every IDAT chunk behind that header is copied into one
 * contiguous buffer.  Nothing is inflated.  Plain C, no device.
 */
#ifndef DNQ_PNG_SCAN_H
#define DNQ_PNG_SCAN_H
#include "png.h"
#include "../../include/mi355_yolo_int8.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dnq_png_scan {
    dnq_png im;        /* what png_info_host gives: filtered == NULL */
    uint8_t *z;        /* raw deflate data: the IDAT payloads minus the zlib header, followed by zero bytes up to zcap */
    size_t nbytes;
    size_t zcap;       /* ((nbytes + 3) & ~3) + 8: what mi355_png_inflate may read */
} dnq_png_scan;

/* 0: *out is filled and owns z (png_scan_free).  -1: the reason is in err, *out holds nothing. */
int png_scan_host(const uint8_t *data, size_t bytes, dnq_png_scan *out, char *err, size_t errlen);
void png_scan_free(dnq_png_scan *s);

/* mi355_png_inflate with host pointers in the table, its rounds run by one thread (png_inflate_emulate.c).  status[s]: 0 or
 * MI355_PNG_E*.  0, or -1: an argument the call refuses (png_inflate_emulate_why names it). */
int png_inflate_emulate_host(const mi355_png_stream *streams, int nstreams, int *status);
const char *png_inflate_emulate_why(void);
/* the words of a status of mi355_png_inflate: the host decoder's */
const char *png_inflate_reason(int status);

#ifdef __cplusplus
}
#endif
#endif
