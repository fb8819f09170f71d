/* jpeg_entropy_fuzz_main.c -- hostile input for the scan lister (yolo_quantization_amd/host/jpeg_scan.c) and for the lane routine of
 * mi355_jpeg_entropy as the host emulation runs it (jpeg_entropy_emulate.c through jpeg_entropy_core.h, the text the kernel's lanes
 * run), as a stand-alone program compiled with -fsanitize=address,undefined (tests/test_jpeg_entropy_cpu.py): nothing of it is loaded
 * into Python.
 *
 *   jpeg_entropy_fuzz_main <corruptions> <file>...   the first three files are also cut at every length
 *   jpeg_entropy_fuzz_main --damaged <file>...       files the host decoder refuses: scanned and emulated, nothing is compared
 *
 * Every file goes through jpeg_scan_host from a heap copy of exactly its size; every segment's bytes are copied to a heap block of
 * exactly ((nbytes + 3) & ~3) + 8 bytes and every coefficient plane is a heap block of exactly its size, so that a read or a store one
 * byte outside what the contract names is a report.  The emulation then runs at 32 and 1024 bits a subsequence.  An untouched file
 * must scan, decode with status 0 and give jpeg_decode_host's coefficients; a cut or corrupted one may be refused, give a status or
 * some coefficients.  Exit status 0 and no sanitizer report is the pass. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "jpeg.h"
#include "jpeg_scan.h"

static unsigned long long rng_state = 88172645463325252ULL;
static unsigned rnd(void)
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (unsigned)(rng_state >> 32);
}

static long scanned, refused, flagged;

/* 0: scanned and emulated; with `pristine`, compared against the host decoder as well (2: they differ) */
static int run(const uint8_t *data, size_t n, int pristine)
{
    uint8_t *copy = malloc(n ? n : 1);
    if (n) memcpy(copy, data, n);
    dnq_jpeg j;
    dnq_jpeg_scan_list sl;
    char err[200];
    int rc = jpeg_scan_host(copy, n, &j, &sl, err, sizeof(err));
    if (rc) {
        if (!err[0]) { fprintf(stderr, "a refusal without a message\n"); exit(2); }
        ++refused;
        free(copy);
        return 1;
    }
    ++scanned;
    rc = 0;
    for (int pass = 0; pass < 2 && sl.nsegs > 0; ++pass) {
        int16_t *plane[3] = {NULL, NULL, NULL};
        for (int k = 0; k < j.ncomp; ++k) plane[k] = calloc((size_t)j.comp[k].blocks_w * j.comp[k].blocks_h * 64, sizeof(int16_t));
        mi355_jpeg_segment *t = calloc((size_t)sl.nsegs, sizeof(*t));
        int *status = calloc((size_t)sl.nsegs, sizeof(int)), *steps = calloc((size_t)sl.nsegs, sizeof(int));
        mi355_jpeg_huff *huff = malloc(sizeof(*huff) * (size_t)sl.nhuff);
        memcpy(huff, sl.huff, sizeof(*huff) * (size_t)sl.nhuff);
        for (int s = 0; s < sl.nsegs; ++s) {
            const dnq_jpeg_scan_seg *z = &sl.segs[s];
            const size_t padded = (((size_t)z->nbytes + 3) & ~(size_t)3) + 8;
            uint8_t *bits = malloc(padded);
            memcpy(bits, sl.bytes + z->offset, padded);
            for (size_t i = z->nbytes; i < padded; ++i)
                if (bits[i]) { fprintf(stderr, "a segment's padding is not zero\n"); exit(2); }
            t[s].bits = (const uint32_t *)bits;
            t[s].huff = huff;
            t[s].nhuff = sl.nhuff;
            t[s].nbytes = z->nbytes;
            t[s].ncomp = z->ncomp;
            for (int c = 0; c < z->ncomp; ++c) {
                const dnq_jpeg_comp *k = &j.comp[z->comp[c]];
                t[s].coef[c] = plane[z->comp[c]];
                t[s].bh[c] = z->bh[c]; t[s].bv[c] = z->bv[c];
                t[s].blocks_w[c] = k->blocks_w; t[s].blocks_h[c] = k->blocks_h;
                t[s].dc[c] = z->dc[c]; t[s].ac[c] = z->ac[c];
            }
            t[s].units_x = z->units_x; t[s].units_y = z->units_y; t[s].first_unit = z->first_unit; t[s].nunits = z->nunits;
        }
        if (jpeg_entropy_emulate_host(t, sl.nsegs, pass ? 1024 : 32, status, steps)) { fprintf(stderr, "the emulation refused a scanned table\n"); exit(2); }
        int any = 0;
        for (int s = 0; s < sl.nsegs; ++s) {
            any |= status[s];
            if (steps[s] < 0 || steps[s] > 256) { fprintf(stderr, "settle steps outside 0 .. 256\n"); exit(2); }
        }
        if (any) ++flagged;
        if (pristine) {
            dnq_jpeg want;
            if (jpeg_decode_host(copy, n, &want, err, sizeof(err)) == 0) {
                if (any) rc = 2;
                for (int k = 0; k < j.ncomp; ++k)
                    if (memcmp(plane[k], want.comp[k].coef, (size_t)j.comp[k].blocks_w * j.comp[k].blocks_h * 128) || memcmp(j.comp[k].quant, want.comp[k].quant, 128)) rc = 2;
                jpeg_free(&want);
            }
        }
        for (int s = 0; s < sl.nsegs; ++s) free((void *)t[s].bits);
        for (int k = 0; k < 3; ++k) free(plane[k]);
        free(t); free(status); free(steps); free(huff);
    }
    jpeg_free(&j);
    jpeg_scan_free(&sl);
    free(copy);
    return rc;
}

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    const int damaged = !strcmp(argv[1], "--damaged");
    const long corruptions = damaged ? 0 : atol(argv[1]);
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
        const int rc = run(data[f], size[f], !damaged);
        if (rc && !damaged) { fprintf(stderr, "%s: %s\n", argv[2 + f], rc == 1 ? "refused as it is" : "the emulation and the host decoder differ"); return 3; }
    }
    for (int f = 0; f < nfiles && f < 3 && !damaged; ++f)
        for (size_t n = 0; n < size[f]; ++n) run(data[f], n, 0);
    for (long i = 0; i < corruptions; ++i) {
        const int f = (int)(i % nfiles);
        uint8_t *copy = malloc(size[f]);
        memcpy(copy, data[f], size[f]);
        const size_t at = rnd() % size[f];
        const unsigned how = rnd() % 4;
        copy[at] = how == 0 ? 0xFF : how == 1 ? 0x00 : how == 2 ? (uint8_t)(copy[at] ^ (1u << (rnd() % 8))) : (uint8_t)rnd();
        run(copy, size[f], 0);
        free(copy);
    }
    printf("jpeg_entropy_fuzz: %ld scanned, %ld refused, %ld runs with a status word set\n", scanned, refused, flagged);
    for (int f = 0; f < nfiles; ++f) free(data[f]);
    free(data); free(size);
    return 0;
}
