#include "nv12_file.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

/* decimal digits only (no blank, no sign), value 1..32768; returns the first character after them, or NULL */
static const char *side(const char *s, int *out)
{
    int v = 0, n = 0;
    for (; *s >= '0' && *s <= '9'; ++s, ++n) {
        v = 10 * v + (*s - '0');
        if (v > 32768) return NULL; /* checked digit by digit: a long string of digits never overflows */
    }
    if (!n || v < 1) return NULL;
    *out = v;
    return s;
}

uint8_t *load_nv12_file(const char *path, int *w, int *h, char *why, size_t why_len)
{
    const char *us = strrchr(path, '_'), *slash = strrchr(path, '/');
    int fw = 0, fh = 0;
    const char *p = us && !(slash && us < slash) ? side(us + 1, &fw) : NULL;
    p = p && *p == 'x' ? side(p + 1, &fh) : NULL;
    if (!p || strcmp(p, ".nv12")) {
        snprintf(why, why_len, "%s: the name of a raw NV12 file must end in _<W>x<H>.nv12 (1 <= W, H <= 32768)", path);
        return NULL;
    }
    const size_t want = (size_t)fw * fh + (size_t)((fh + 1) / 2) * 2 * (size_t)((fw + 1) / 2);
    FILE *f = fopen(path, "rb");
    if (!f) { snprintf(why, why_len, "%s: cannot open the file", path); return NULL; }
    uint8_t *raw = malloc(want + 1);
    if (!raw) {
        fclose(f);
        snprintf(why, why_len, "%s: no memory for the %zu bytes of a %d x %d NV12 frame", path, want, fw, fh);
        return NULL;
    }
    const size_t got = fread(raw, 1, want + 1, f); /* one byte more than wanted: a longer file is told from an exact one */
    fclose(f);
    if (got != want) {
        snprintf(why, why_len, "%s: a %d x %d NV12 frame holds %zu bytes, the file holds %s%zu", path, fw, fh, want,
                 got > want ? "more than " : "", got > want ? want : got);
        free(raw);
        return NULL;
    }
    *w = fw; *h = fh;
    return raw;
}
