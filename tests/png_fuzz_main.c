/* png_fuzz_main.c -- hostile input for the host PNG decoder (yolo_quantization_amd/host/png.c), as a stand-alone program that is
 * compiled with -fsanitize=address,undefined together with png.c (tests/test_png_cpu.py): nothing of it is loaded into Python.
 *
 *   png_fuzz_main <corruptions> <file>...   the first three files are also cut at every length
 *
 * Every file is decoded as it is (must succeed), then from a heap copy of exactly its size -- so that a read one byte past the data is
 * a report -- at every truncation (the first three files) and with <corruptions> seeded single-byte changes spread over all files.
 * A decode may fail or give some scanlines; the bytes it returns are read in full.  png.c is compiled with DNQ_PNG_REALLOC naming
 * fuzz_realloc below, so every allocation of the inflated output passes through here: none may ask for more than the bytes the image
 * of the file's own header needs (png_info_host's filtered_bytes; nothing where the chunk walk refuses the file), nor for more than a
 * deflate stream of the file's size can produce.  Exit status 0 and no sanitizer report is the pass. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "png.h"

static unsigned long long rng_state = 88172645463325252ULL;
static unsigned rnd(void)
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (unsigned)(rng_state >> 32);
}

static long decoded, refused;
static size_t cap, largest;

void *fuzz_realloc(void *p, size_t n)
{
    if (n > cap) { fprintf(stderr, "an allocation of %zu bytes, the cap is %zu\n", n, cap); exit(4); }
    if (n > largest) largest = n;
    return realloc(p, n);
}

/* decode an exact-size heap copy; the result is walked so that its bytes are really there */
static int decode(const uint8_t *data, size_t n)
{
    uint8_t *copy = malloc(n ? n : 1);
    if (n) memcpy(copy, data, n);
    dnq_png info, p;
    char err[200];
    cap = 0;
    if (png_info_host(copy, n, &info, err, sizeof(err)) == 0) {
        const size_t by_ratio = 65536 + 2 * 1032 * n; /* deflate expands by at most 1032; the buffer doubles */
        cap = info.filtered_bytes < by_ratio ? info.filtered_bytes : by_ratio;
    }
    err[0] = 0;
    const int rc = png_decode_host(copy, n, &p, err, sizeof(err));
    if (rc == 0) {
        long sum = 0;
        for (size_t i = 0; i < p.filtered_bytes; ++i) sum += p.filtered[i];
        for (int k = 0; k < p.npasses; ++k)
            if (p.pass[k].offset + (size_t)p.pass[k].rows * ((size_t)p.pass[k].row_bytes + 1) > p.filtered_bytes) { fprintf(stderr, "a pass beyond the bytes\n"); exit(5); }
        if (sum == 0x7fffffffffffL) puts("");
        png_free(&p);
        ++decoded;
    } else {
        if (!err[0]) { fprintf(stderr, "a refusal without a message\n"); exit(2); }
        ++refused;
    }
    free(copy);
    return rc;
}

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    const long corruptions = atol(argv[1]);
    const int nfiles = argc - 2;
    uint8_t **data = calloc((size_t)nfiles, sizeof(uint8_t *));
    size_t *size = calloc((size_t)nfiles, sizeof(size_t));
    for (int f = 0; f < nfiles; ++f) {
        FILE *fp = fopen(argv[2 + f], "rb");
        if (!fp) { perror(argv[2 + f]); return 2; }
        fseek(fp, 0, SEEK_END);
        size[f] = (size_t)ftell(fp);
        fseek(fp, 0, SEEK_SET);
        data[f] = malloc(size[f]);
        if (fread(data[f], 1, size[f], fp) != size[f]) return 2;
        fclose(fp);
        if (decode(data[f], size[f])) { fprintf(stderr, "%s: refused as it is\n", argv[2 + f]); return 3; }
    }
    for (int f = 0; f < nfiles && f < 3; ++f)
        for (size_t n = 0; n < size[f]; ++n) decode(data[f], n);
    for (long i = 0; i < corruptions; ++i) {
        const int f = (int)(i % nfiles);
        uint8_t *copy = malloc(size[f]);
        memcpy(copy, data[f], size[f]);
        const size_t at = rnd() % size[f];
        const unsigned how = rnd() % 4;
        copy[at] = how == 0 ? 0xFF : how == 1 ? 0x00 : how == 2 ? (uint8_t)(copy[at] ^ (1u << (rnd() % 8))) : (uint8_t)rnd();
        decode(copy, size[f]);
        free(copy);
    }
    printf("png_fuzz: %ld decoded, %ld refused, largest allocation %zu bytes\n", decoded, refused, largest);
    for (int f = 0; f < nfiles; ++f) free(data[f]);
    free(data); free(size);
    return 0;
}
