/* The CLI's reader of raw planar YUV frames (`detector test ... -frames i420 | yv12 | i422 | i444`).  Part of ./darknet, not of the
 * library. */
#ifndef PLANAR_FILE_H
#define PLANAR_FILE_H
#include <stddef.h>
#include <stdint.h>

/* Reads a raw frame of three tightly packed planes from a file named `<anything>_<W>x<H>.<ext>`, ext = i420 | yv12 | i422 | i444
 * being the format (MI355_PLANAR_I420 .. MI355_PLANAR_I444 = 0 .. 3) the caller asks for: W * H luma bytes, then the two chroma planes
 * in the order the format names them, each (W + 1) / 2 x (H + 1) / 2 (i420, yv12), (W + 1) / 2 x H (i422) or W x H (i444) bytes,
 * exactly.  W and H are plain decimal digits, 1..32768.  Returns the malloc'd bytes and the size, *plane_bytes = the length of plane 0
 * and of each chroma plane (plane 1 starts at plane_bytes[0], plane 2 at plane_bytes[0] + plane_bytes[1]); NULL with the reason
 * written to `why` when the format is none of the four, the name carries no size or another extension, the file cannot be opened or
 * read into memory, or its length is another: the message says which.  Needs no device. */
uint8_t *load_planar_file(const char *path, int format, int *w, int *h, size_t plane_bytes[2], char *why, size_t why_len);

#endif
