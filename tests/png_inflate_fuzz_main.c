/* png_inflate_fuzz_main.c -- hostile input for the host half and the emulation of the inflate on the device
 * (yolo_quantization_amd/host/png_scan.c, png_inflate_emulate.c, png_inflate_core.h: the text the kernel's lane 0 runs), as a
 * stand-alone program compiled with -fsanitize=address,undefined together with them and png.c (tests/test_png_inflate_cpu.py):
 * nothing of it is loaded into Python.
 *
 *   png_inflate_fuzz_main <corruptions> <file>...   the first three files are also cut at every length
 *
 * Every file goes through png_scan_host and png_inflate_emulate_host as it is (must be accepted), then from a heap copy of exactly
 * its size at every truncation (the first three files) and with <corruptions> seeded single-byte changes spread over all files.  The
 * stream the scan returns lies in a heap block of exactly the bytes mi355_png_inflate may read, so a read beyond them is a report;
 * the output lies between guard bytes, which are checked after every run.  The verdict must be the host decoder's (png_decode_host),
 * and where both accept, the bytes too.  Exit status 0 and no sanitizer report is the pass. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "png.h"
#include "png_scan.h"

enum { GUARD = 64 };

static unsigned long long rng_state = 88172645463325252ULL;
static unsigned rnd(void)
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (unsigned)(rng_state >> 32);
}

static long accepted, refused, refused_by_scan;

static int run(const uint8_t *data, size_t n)
{
    uint8_t *copy = malloc(n ? n : 1);
    if (n) memcpy(copy, data, n);
    dnq_png host;
    dnq_png_scan sc;
    char herr[200] = "", serr[200] = "";
    const int hrc = png_decode_host(copy, n, &host, herr, sizeof(herr));
    const int src = png_scan_host(copy, n, &sc, serr, sizeof(serr));
    int rc = -1;
    if (src) {
        if (!serr[0]) { fprintf(stderr, "a refusal without a message\n"); exit(2); }
        if (!hrc) { fprintf(stderr, "the scan refuses (%s) what the host decoder accepts\n", serr); exit(3); }
        if (sc.z || sc.im.w) { fprintf(stderr, "a refused scan holds something\n"); exit(3); }
        ++refused_by_scan;
    } else {
        const size_t cap = sc.im.filtered_bytes;
        uint8_t *buf = malloc(cap + 2 * GUARD + 3);
        memset(buf, 0xA5, cap + 2 * GUARD + 3);
        mi355_png_stream t;
        memset(&t, 0, sizeof(t));
        t.z = (const uint32_t *)sc.z; t.nbytes = (uint32_t)sc.nbytes; t.out = buf + GUARD; t.cap = (uint32_t)cap;
        t.npasses = sc.im.npasses;
        for (int k = 0; k < sc.im.npasses; ++k) { t.rows[k] = sc.im.pass[k].rows; t.row_bytes[k] = sc.im.pass[k].row_bytes; }
        int status = -1;
        if (png_inflate_emulate_host(&t, 1, &status)) { fprintf(stderr, "the emulation refuses its table: %s\n", png_inflate_emulate_why()); exit(4); }
        for (size_t i = 0; i < GUARD; ++i)
            if (buf[i] != 0xA5 || buf[GUARD + cap + i] != 0xA5) { fprintf(stderr, "a guard byte changed\n"); exit(5); }
        if ((status == 0) != (hrc == 0)) {
            fprintf(stderr, "verdicts differ: host %d (%s), emulation %d (%s)\n", hrc, herr, status, png_inflate_reason(status));
            exit(6);
        }
        if (!status && memcmp(buf + GUARD, host.filtered, cap)) { fprintf(stderr, "bytes differ\n"); exit(7); }
        if (status) ++refused; else { ++accepted; rc = 0; }
        free(buf);
        png_scan_free(&sc);
    }
    if (!hrc) png_free(&host);
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
        if (run(data[f], size[f])) { fprintf(stderr, "%s: refused as it is\n", argv[2 + f]); return 3; }
    }
    for (int f = 0; f < nfiles && f < 3; ++f)
        for (size_t n = 0; n < size[f]; ++n) run(data[f], n);
    for (long i = 0; i < corruptions; ++i) {
        const int f = (int)(i % nfiles);
        uint8_t *copy = malloc(size[f]);
        memcpy(copy, data[f], size[f]);
        const size_t at = rnd() % size[f];
        const unsigned how = rnd() % 4;
        copy[at] = how == 0 ? 0xFF : how == 1 ? 0x00 : how == 2 ? (uint8_t)(copy[at] ^ (1u << (rnd() % 8))) : (uint8_t)rnd();
        run(copy, size[f]);
        free(copy);
    }
    printf("png_inflate_fuzz: %ld accepted, %ld refused by the inflate, %ld by the scan\n", accepted, refused, refused_by_scan);
    for (int f = 0; f < nfiles; ++f) free(data[f]);
    free(data); free(size);
    return 0;
}
