/*
 * png_inflate_emulate.c -- mi355_png_inflate on the CPU: the rounds of the kernel (csrc/png_inflate.hip) run by one thread, lane 0's
 * part through the text the kernel's lane 0 runs (png_inflate_core.h), the lanes' parts -- look tables, token positions, literals,
 * matches, stored bytes, flushes of the ring, filter bytes -- as loops over what the lanes do.  The pointers of the stream table are
 * host pointers here.  For tests and for running hostile streams under sanitizers; no device.
 */
#include "png_scan.h"
#include "png_inflate_core.h"
#include <stdlib.h>
#include <string.h>

static _Thread_local const char *emu_why = "";
const char *png_inflate_emulate_why(void) { return emu_why; }

const char *png_inflate_reason(int status)
{
    static const char *const words[] = {"", "bad block type", "zlib corrupt", "bad codelengths", "bad huffman code", "bad dist",
                                        "premature end of the zlib data", "read past buffer", "not enough pixels", "invalid filter"};
    return status >= 1 && status <= 9 ? words[status] : status ? "unknown status" : "";
}

typedef struct {
    pic_code zl, zd;
    uint8_t ring[PIC_RING];
    uint8_t lens[PIC_MAX_LENS];
    uint16_t codes[PIC_MAX_LENS];
    uint32_t tok[PIC_TOKENS];
} emu_mem;

/* the ring's bytes [from, to) go out; to <= cap */
static void flush(const emu_mem *m, uint8_t *out, uint32_t from, uint32_t to)
{
    for (uint32_t i = from; i < to; ++i) out[i] = m->ring[i & (PIC_RING - 1)];
}

static int emulate_stream(const mi355_png_stream *t, emu_mem *m)
{
    pic_state s;
    memset(&s, 0, sizeof(s));
    s.b.w = t->z; s.b.base = 0; s.b.nw = pic_stream_words(t->nbytes); s.b.nbytes = t->nbytes; /* the window: the whole stream */
    s.cap = t->cap;
    uint32_t flushed = 0;
    while (s.phase != PIC_DONE) {
        if (s.phase == PIC_HEADER) {
            pic_header(&s, &m->zl, &m->zd, m->lens, m->codes);
            if (s.phase != PIC_BUILD) continue;
            pic_look_zero(&m->zl, 0, 1); pic_look_zero(&m->zd, 0, 1);
            pic_look_fill(&m->zl, m->lens, s.hlit, m->codes, 0, 1);
            pic_look_fill(&m->zd, m->lens + s.hlit, s.hdist, m->codes + s.hlit, 0, 1);
            s.phase = PIC_SYMBOLS;
        } else if (s.phase == PIC_SYMBOLS) {
            pic_round(&s, &m->zl, &m->zd, m->tok, t->z);
            uint32_t at[PIC_TOKENS], p = s.n0;
            for (int k = 0; k < s.ntok; ++k) { at[k] = p; p += m->tok[k] >> 16 ? m->tok[k] >> 16 : 1; } /* the scan */
            for (int k = 0; k < s.ntok; ++k)
                if (!(m->tok[k] >> 16)) m->ring[at[k] & (PIC_RING - 1)] = (uint8_t)m->tok[k];
            for (int k = 0; k < s.ntok; ++k) {
                const uint32_t len = m->tok[k] >> 16, dist = m->tok[k] & 0xffff;
                for (uint32_t j = 0; j < len; ++j) /* any order of j: the source lies in front of the match */
                    m->ring[(at[k] + j) & (PIC_RING - 1)] = m->ring[(at[k] - dist + j % dist) & (PIC_RING - 1)];
            }
        } else { /* PIC_STORED */
            const uint32_t chunk = s.stored_left < PIC_STORED_CHUNK ? s.stored_left : PIC_STORED_CHUNK;
            const uint8_t *src = (const uint8_t *)t->z + s.stored_at;
            for (uint32_t j = 0; j < chunk; ++j) m->ring[(s.n + j) & (PIC_RING - 1)] = src[j];
            pic_stored_done(&s, chunk);
        }
        if (s.n - flushed >= PIC_STORED_CHUNK || s.phase == PIC_DONE) {
            const uint32_t to = s.phase == PIC_DONE ? s.n : s.n & ~3u;
            flush(m, t->out, flushed, to);
            flushed = to;
        }
    }
    if (s.status) return s.status;
    if (s.n < s.cap) return MI355_PNG_EPIXELS;
    const uint8_t *row = t->out;
    for (int k = 0; k < t->npasses; ++k)
        for (int y = 0; y < t->rows[k]; ++y, row += (size_t)t->row_bytes[k] + 1)
            if (*row > 4) return MI355_PNG_EFILTER;
    return 0;
}

int png_inflate_emulate_host(const mi355_png_stream *streams, int nstreams, int *status)
{
    if (!streams || !status || nstreams < 1 || nstreams > 65535) { emu_why = "png_inflate: null table / need 1 <= nstreams <= 65535"; return -1; }
    for (int i = 0; i < nstreams; ++i)
        if ((emu_why = pic_stream_check(&streams[i]))) return -1;
    emu_why = "";
    emu_mem *m = malloc(sizeof(emu_mem));
    if (!m) { emu_why = "out of memory"; return -1; }
    for (int i = 0; i < nstreams; ++i) status[i] = emulate_stream(&streams[i], m);
    free(m);
    return 0;
}
