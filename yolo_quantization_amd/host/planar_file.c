#include "planar_file.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static const char *const planar_ext[4] = {".i420", ".yv12", ".i422", ".i444"}; /* by format id */

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

uint8_t *load_planar_file(const char *path, int format, int *w, int *h, size_t plane_bytes[2], char *why, size_t why_len)
{
    if (format < 0 || format > 3) {
        snprintf(why, why_len, "%s: raw planar files are i420, yv12, i422 or i444", path);
        return NULL;
    }
    const char *ext = planar_ext[format];
    const char *us = strrchr(path, '_'), *slash = strrchr(path, '/');
    int fw = 0, fh = 0;
    const char *p = us && !(slash && us < slash) ? side(us + 1, &fw) : NULL;
    p = p && *p == 'x' ? side(p + 1, &fh) : NULL;
    if (!p || strcmp(p, ext)) {
        snprintf(why, why_len, "%s: the name of a raw %s file must end in _<W>x<H>%s (1 <= W, H <= 32768)", path, ext + 1, ext);
        return NULL;
    }
    const size_t cw = format == 3 ? (size_t)fw : (size_t)((fw + 1) / 2), ch = format <= 1 ? (size_t)((fh + 1) / 2) : (size_t)fh;
    const size_t luma = (size_t)fw * fh, chroma = cw * ch, want = luma + 2 * chroma;
    FILE *f = fopen(path, "rb");
    if (!f) { snprintf(why, why_len, "%s: cannot open the file", path); return NULL; }
    uint8_t *raw = malloc(want + 1);
    if (!raw) {
        fclose(f);
        snprintf(why, why_len, "%s: no memory for the %zu bytes of a %d x %d %s frame", path, want, fw, fh, ext + 1);
        return NULL;
    }
    const size_t got = fread(raw, 1, want + 1, f); /* one byte more than wanted: a longer file is told from an exact one */
    fclose(f);
    if (got != want) {
        snprintf(why, why_len, "%s: a %d x %d %s frame holds %zu bytes, the file holds %s%zu", path, fw, fh, ext + 1, want,
                 got > want ? "more than " : "", got > want ? want : got);
        free(raw);
        return NULL;
    }
    *w = fw; *h = fh;
    plane_bytes[0] = luma; plane_bytes[1] = chroma;
    return raw;
}
