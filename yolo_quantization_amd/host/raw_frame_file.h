/* The CLI's reader of raw video frames (`detector test ... -frames nv12 | nv21 | i420 | yv12 | i422 | i444 | rgba | bgra | argb | abgr |
 * yuyv | uyvy | yvyu | p010 | rggb | bggr | grbg | gbrg | mono`).  Part of ./darknet, not of the library. */
#ifndef RAW_FRAME_FILE_H
#define RAW_FRAME_FILE_H
#include <stddef.h>
#include <stdint.h>

/* The kinds of raw files.  The planar ones are the formats' ids (MI355_PLANAR_I420 .. MI355_PLANAR_I444 = 0 .. 3); NV12 lies away from
 * them, so a planar id one past either end is no kind at all. */
enum { RAW_FRAME_I420 = 0, RAW_FRAME_YV12 = 1, RAW_FRAME_I422 = 2, RAW_FRAME_I444 = 3, RAW_FRAME_NV12 = 16,
       /* the packed kinds are 32 + the formats' ids (MI355_PACKED_RGBA .. MI355_PACKED_YVYU = 0 .. 6); P010 lies away from them too */
       RAW_FRAME_RGBA = 32, RAW_FRAME_BGRA = 33, RAW_FRAME_ARGB = 34, RAW_FRAME_ABGR = 35, RAW_FRAME_YUYV = 36, RAW_FRAME_UYVY = 37,
       RAW_FRAME_YVYU = 38, RAW_FRAME_P010 = 48,
       /* the raw sensor kinds are 64 + 8 * the sample layout's id (MI355_RAW_U8 .. MI355_RAW_MIPI12 = 0 .. 3) + the pattern's id
        * (MI355_BAYER_RGGB .. MI355_BAYER_MONO = 0 .. 4): 64 .. 68, 72 .. 76, 80 .. 84, 88 .. 92 */
       RAW_FRAME_SENSOR = 64 };

/* Reads a raw frame from a file named `<anything>_<W>x<H>.<ext>`, as raw video usually is, ext = nv12 | i420 | yv12 | i422 | i444 |
 * rgba | bgra | argb | abgr | yuyv | uyvy | yvyu | p010 being the kind the caller asks for.  W and H are plain decimal digits,
 * 1..32768.  A file of the first five kinds holds, exactly and tightly packed, W * H luma bytes and then
 *   nv12:        (H + 1) / 2 rows of (W + 1) / 2 chroma pairs (an NV21 frame has the same shape);
 *   the others:  the two chroma planes in the order the format names them, each (W + 1) / 2 x (H + 1) / 2 (i420, yv12),
 *                (W + 1) / 2 x H (i422) or W x H (i444) bytes.
 * A file of a packed kind holds one plane and no more, plane_bytes[1] = 0:
 *   rgba, bgra, argb, abgr:  H rows of W pixels of four bytes: 4 * W * H bytes;
 *   yuyv, uyvy, yvyu:        H rows of (W + 1) / 2 macropixels of four bytes: 4 * ((W + 1) / 2) * H bytes.
 * A p010 file has nv12's shape with samples of two bytes (little-endian, the significant bits at the top):
 * 2 * W * H + 4 * ((W + 1) / 2) * ((H + 1) / 2) bytes.
 * A file of a raw sensor kind is named by its pattern, ext = rggb | bggr | grbg | gbrg | mono, whatever the sample layout, and holds
 * one plane of H tightly packed rows and no more, plane_bytes[1] = 0: W * H bytes (u8), 2 * W * H (u16, little-endian),
 * 5 * ((W + 3) / 4) * H (mipi10: four pixels in five bytes) or 3 * ((W + 1) / 2) * H (mipi12: two pixels in three bytes).
 * Returns the malloc'd bytes and the size; plane_bytes[0] = the length of plane 0, plane_bytes[1] = that of every plane after it (plane
 * 1 starts at plane_bytes[0], a planar kind's plane 2 at plane_bytes[0] + plane_bytes[1]).  NULL with the reason written to `why` when
 * the kind is none of these, the name carries no size or another extension, the file cannot be opened or read into memory, or its
 * length is another: the message says which.  Needs no device. */
uint8_t *load_raw_frame_file(const char *path, int kind, int *w, int *h, size_t plane_bytes[2], char *why, size_t why_len);

#endif
