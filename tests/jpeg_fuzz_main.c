/* jpeg_fuzz_main.c -- hostile input for the host JPEG decoder (yolo_quantization_amd/host/jpeg.c), as a stand-alone program that is
 * compiled with -fsanitize=address,undefined together with jpeg.c (tests/test_jpeg_cpu.py): nothing of it is loaded into Python.
 *
 *   jpeg_fuzz_main <corruptions> <file>...   the first three files are also cut at every length
 *
 * Every file is decoded as it is (must succeed), then from a heap copy of exactly its size -- so that a read one byte past the data is
 * a report -- at every truncation (the first three files) and with <corruptions> seeded single-byte changes spread over all files.
 * A decode may fail or give some image; every coefficient array it returns is read in full.  Exit status 0 and no sanitizer report
 * is the pass. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "jpeg.h"

static unsigned long long rng_state = 88172645463325252ULL;
static unsigned rnd(void)
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (unsigned)(rng_state >> 32);
}

static long decoded, refused;

/* decode an exact-size heap copy; the result is walked so that its arrays are really there */
static int decode(const uint8_t *data, size_t n)
{
    uint8_t *copy = malloc(n ? n : 1);
    if (n) memcpy(copy, data, n);
    dnq_jpeg j;
    char err[200];
    const int rc = jpeg_decode_host(copy, n, &j, err, sizeof(err));
    if (rc == 0) {
        long sum = 0;
        for (int k = 0; k < j.ncomp; ++k) {
            const size_t cnt = (size_t)j.comp[k].blocks_w * j.comp[k].blocks_h * 64;
            for (size_t i = 0; i < cnt; i += 61) sum += j.comp[k].coef[i];
            for (int i = 0; i < 64; ++i) sum += j.comp[k].quant[i];
        }
        if (sum == 0x7fffffffffffL) puts("");
        jpeg_free(&j);
        ++decoded;
    } else {
        if (!err[0]) { fprintf(stderr, "a refusal without a message\n"); exit(2); }
        ++refused;
    }
    dnq_jpeg info;
    jpeg_info_host(copy, n, &info, err, sizeof(err));
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
    printf("jpeg_fuzz: %ld decoded, %ld refused\n", decoded, refused);
    for (int f = 0; f < nfiles; ++f) free(data[f]);
    free(data); free(size);
    return 0;
}
