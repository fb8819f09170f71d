/* jpeg_exif_fuzz_main.c -- jpeg_exif_orientation_host (host/jpeg_exif.c) on hostile bytes, as a stand-alone program to be built with
 * -fsanitize=address,undefined: every file as it is, every truncation of the first one, and N seeded corruptions of each.  Every buffer
 * is a heap block of exactly the bytes handed over, so that a read one byte outside it is reported.  Each result must be in 1..8.
 * usage: jpeg_exif_fuzz N file... */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "darknet_q.h"

static uint32_t rng_state = 12345;
static uint32_t rng(void) { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

static int once(const uint8_t *src, size_t n)
{
    uint8_t *tight = malloc(n ? n : 1); /* a block of its own: the sanitizer guards both ends */
    if (n) memcpy(tight, src, n);
    const int o = jpeg_exif_orientation_host(tight, n);
    free(tight);
    if (o < 1 || o > 8) { fprintf(stderr, "orientation %d outside 1..8\n", o); exit(2); }
    return o;
}

int main(int argc, char **argv)
{
    if (argc < 3) return 1;
    const int rounds = atoi(argv[1]);
    long calls = 0, not_one = 0;
    for (int f = 2; f < argc; ++f) {
        FILE *fp = fopen(argv[f], "rb");
        if (!fp) { fprintf(stderr, "cannot open %s\n", argv[f]); return 1; }
        fseek(fp, 0, SEEK_END);
        const long n = ftell(fp);
        fseek(fp, 0, SEEK_SET);
        uint8_t *data = malloc((size_t)n + 1), *work = malloc((size_t)n + 1);
        if (fread(data, 1, (size_t)n, fp) != (size_t)n) return 1;
        fclose(fp);
        not_one += once(data, (size_t)n) != 1; ++calls;
        if (f == 2)
            for (long cut = 0; cut < n; ++cut) { once(data, (size_t)cut); ++calls; }
        const long head = n < 256 ? n : 256; /* the markers and the Exif block live at the front */
        for (int r = 0; r < rounds && head > 0; ++r) {
            memcpy(work, data, (size_t)n);
            const int hits = 1 + (int)(rng() % 3);
            for (int k = 0; k < hits; ++k) work[rng() % (uint32_t)head] = (uint8_t)rng();
            not_one += once(work, (size_t)n) != 1; ++calls;
        }
        free(data); free(work);
    }
    once(NULL, 0); ++calls;
    printf("jpeg_exif_fuzz: %ld calls, %ld gave an orientation other than 1\n", calls, not_one);
    return 0;
}
