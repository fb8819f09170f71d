/* The CLI's reader of raw NV12 / NV21 frames (`detector test ... -frames nv12 | nv21`).  Part of ./darknet, not of the library. */
#ifndef NV12_FILE_H
#define NV12_FILE_H
#include <stddef.h>
#include <stdint.h>

/* Reads a raw NV12 / NV21 frame from a file named `<anything>_<W>x<H>.nv12`, as raw video usually is: W * H luma bytes followed by
 * ((H + 1) / 2) rows of (W + 1) / 2 chroma pairs, exactly.  W and H are plain decimal digits, 1..32768.  Returns the malloc'd bytes
 * (the chroma plane starts at W * H) and the size; NULL with the reason written to `why` when the name carries no size, the file
 * cannot be opened or read into memory, or its length is another: the message says which.  Needs no device. */
uint8_t *load_nv12_file(const char *path, int *w, int *h, char *why, size_t why_len);

#endif
