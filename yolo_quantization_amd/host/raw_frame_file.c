#include "raw_frame_file.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

/* what a kind brings: the extension, the name messages call it by, the shifts of its chroma size, the number of chroma planes, the
 * bytes of a sample and, for the packed kinds (one plane, no chroma plane), how many pixels share a 4-byte group */
typedef struct { int kind; const char *ext, *name; int sx, sy, chroma_planes, sample_bytes, group_pixels; } raw_kind;
#define N_KINDS 13
static const raw_kind kinds[N_KINDS] = {{RAW_FRAME_I420, ".i420", "i420", 1, 1, 2, 1, 0}, {RAW_FRAME_YV12, ".yv12", "yv12", 1, 1, 2, 1, 0},
                                        {RAW_FRAME_I422, ".i422", "i422", 1, 0, 2, 1, 0}, {RAW_FRAME_I444, ".i444", "i444", 0, 0, 2, 1, 0},
                                        {RAW_FRAME_NV12, ".nv12", "NV12", 1, 1, 1, 1, 0}, /* one plane of pairs: twice the width */
                                        {RAW_FRAME_RGBA, ".rgba", "rgba", 0, 0, 0, 1, 1}, {RAW_FRAME_BGRA, ".bgra", "bgra", 0, 0, 0, 1, 1},
                                        {RAW_FRAME_ARGB, ".argb", "argb", 0, 0, 0, 1, 1}, {RAW_FRAME_ABGR, ".abgr", "abgr", 0, 0, 0, 1, 1},
                                        {RAW_FRAME_YUYV, ".yuyv", "yuyv", 0, 0, 0, 1, 2}, {RAW_FRAME_UYVY, ".uyvy", "uyvy", 0, 0, 0, 1, 2},
                                        {RAW_FRAME_YVYU, ".yvyu", "yvyu", 0, 0, 0, 1, 2},
                                        {RAW_FRAME_P010, ".p010", "P010", 1, 1, 1, 2, 0}}; /* NV12's shape, two bytes a sample */

/* the raw sensor kinds, RAW_FRAME_SENSOR + 8 * layout + pattern: extensions by pattern (MI355_BAYER_RGGB .. _MONO), names of the
 * sample layouts (MI355_RAW_U8 .. _MIPI12) */
static const char *const sensor_ext[5] = {".rggb", ".bggr", ".grbg", ".gbrg", ".mono"};
static const char *const sensor_layout[4] = {"u8", "u16", "mipi10", "mipi12"};

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

uint8_t *load_raw_frame_file(const char *path, int kind, int *w, int *h, size_t plane_bytes[2], char *why, size_t why_len)
{
    const raw_kind *k = NULL;
    raw_kind sensor;
    char sensor_name[24];
    for (int i = 0; i < N_KINDS; ++i)
        if (kinds[i].kind == kind) k = &kinds[i];
    const int pattern = (kind - RAW_FRAME_SENSOR) & 7, layout = (kind - RAW_FRAME_SENSOR) >> 3;
    if (kind >= RAW_FRAME_SENSOR && pattern < 5 && layout < 4) { /* one plane of raw samples: the pattern names the extension */
        snprintf(sensor_name, sizeof(sensor_name), "%s %s", sensor_ext[pattern] + 1, sensor_layout[layout]);
        sensor = (raw_kind){kind, sensor_ext[pattern], sensor_name, 0, 0, 0, 1, 0};
        k = &sensor;
    }
    if (!k) {
        snprintf(why, why_len, "%s: raw planar files are i420, yv12, i422 or i444", path);
        return NULL;
    }
    const char *us = strrchr(path, '_'), *slash = strrchr(path, '/');
    int fw = 0, fh = 0;
    const char *p = us && !(slash && us < slash) ? side(us + 1, &fw) : NULL;
    p = p && *p == 'x' ? side(p + 1, &fh) : NULL;
    if (!p || strcmp(p, k->ext)) {
        snprintf(why, why_len, "%s: the name of a raw %s file must end in _<W>x<H>%s (1 <= W, H <= 32768)", path, k->name, k->ext);
        return NULL;
    }
    const size_t cw = (size_t)((fw + k->sx) >> k->sx) * (k->chroma_planes == 1 ? 2 : 1), ch = (size_t)((fh + k->sy) >> k->sy);
    size_t row = k->group_pixels ? 4 * (((size_t)fw + k->group_pixels - 1) / k->group_pixels) : (size_t)fw * k->sample_bytes;
    if (k == &sensor) row = layout == 1 ? 2 * (size_t)fw : layout == 2 ? 5 * (((size_t)fw + 3) / 4) : layout == 3 ? 3 * (((size_t)fw + 1) / 2) : (size_t)fw;
    const size_t luma = row * fh, chroma = k->chroma_planes ? cw * ch * k->sample_bytes : 0, want = luma + (size_t)k->chroma_planes * chroma;
    FILE *f = fopen(path, "rb");
    if (!f) { snprintf(why, why_len, "%s: cannot open the file", path); return NULL; }
    uint8_t *raw = malloc(want + 1);
    if (!raw) {
        fclose(f);
        snprintf(why, why_len, "%s: no memory for the %zu bytes of a %d x %d %s frame", path, want, fw, fh, k->name);
        return NULL;
    }
    const size_t got = fread(raw, 1, want + 1, f); /* one byte more than wanted: a longer file is told from an exact one */
    fclose(f);
    if (got != want) {
        snprintf(why, why_len, "%s: a %d x %d %s frame holds %zu bytes, the file holds %s%zu", path, fw, fh, k->name, want,
                 got > want ? "more than " : "", got > want ? want : got);
        free(raw);
        return NULL;
    }
    *w = fw; *h = fh;
    plane_bytes[0] = luma; plane_bytes[1] = chroma;
    return raw;
}
