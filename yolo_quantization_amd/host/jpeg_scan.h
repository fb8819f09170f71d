/*
 * jpeg_scan.h -- the host half of the JPEG path when the entropy decode runs on the device (mi355_jpeg_entropy): the markers are
 * parsed as jpeg_decode_host parses them (jpeg_markers.h: the same headers, colour mode, quantisers and refusals), but the scans are
 * only found and listed, not decoded.  Plain C, no device.
 *
 * A SEGMENT is one restart interval of a scan, or the whole scan where there is none; the end of a scan and the restart markers
 * (FF D0..D7) are found by the marker search.  A scan of u units at interval r lists at most ceil(u / r) segments (bytes behind
 * further restart markers are dropped, as the decoder never reaches them; fewer markers give fewer segments and the blocks of the
 * missing ones stay zero).  Each segment's bytes are copied out unstuffed by the rule of the decoder's bit reader -- FF 00 gives FF,
 * fill FFs in front of a marker are dropped -- to a 4-byte aligned offset of `bytes`, followed by at least 8 zero bytes.  The Huffman
 * tables a scan uses are copied into `huff` as they stand at that scan: a DHT between scans does not reach back.
 */
#ifndef DNQ_JPEG_SCAN_H
#define DNQ_JPEG_SCAN_H
#include "jpeg.h"
#include "../../include/mi355_yolo_int8.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dnq_jpeg_scan_seg {
    int ncomp;             /* components of the scan */
    int comp[3];           /* in scan order: index into dnq_jpeg.comp */
    int bh[3], bv[3];      /* blocks per unit; 1 x 1 in a one-component scan */
    int dc[3], ac[3];      /* index into dnq_jpeg_scan_list.huff */
    int units_x, units_y;  /* the unit grid: MCUs, or the component's real size in blocks in a one-component scan */
    int first_unit, nunits;
    int scan;              /* ordinal of the scan in the file */
    uint32_t nbytes;       /* unstuffed bytes */
    size_t offset;         /* of the first in dnq_jpeg_scan_list.bytes, a multiple of 4 */
} dnq_jpeg_scan_seg;

typedef struct dnq_jpeg_scan_list {
    int nsegs, nhuff;
    dnq_jpeg_scan_seg *segs;
    mi355_jpeg_huff *huff;
    uint8_t *bytes;        /* every segment's bytes, each followed by zeros up to ((nbytes + 3) & ~3) + 8 */
    size_t nbytes;
    int cap_segs, cap_huff; /* allocation */
    size_t cap_bytes;
} dnq_jpeg_scan_list;

/* 0: *out holds the headers as jpeg_decode_host fills them (coef == NULL) and *scans owns its arrays (jpeg_scan_free).  -1: the reason
 * is in err, both hold nothing. */
int jpeg_scan_host(const uint8_t *data, size_t bytes, dnq_jpeg *out, dnq_jpeg_scan_list *scans, char *err, size_t errlen);
void jpeg_scan_free(dnq_jpeg_scan_list *scans);

/* mi355_jpeg_entropy with host pointers in the table, its lanes run one after another (jpeg_entropy_emulate.c).  status[s]: 0 or
 * MI355_JPEG_E*; steps_out (may be NULL): per segment, the settle steps of its slowest round.  -1: a refused argument. */
int jpeg_entropy_emulate_host(const mi355_jpeg_segment *segments, int nsegments, int subseq_bits, int *status, int *steps_out);

#ifdef __cplusplus
}
#endif
#endif
