/*
 * jpeg_entropy_core.h -- the decode of one subsequence of a JPEG segment, written once in the C subset gcc and hipcc both take: the
 * lanes of mi355_jpeg_entropy (csrc/jpeg_entropy.hip) and the host emulation (jpeg_entropy_emulate.c) run this text.  See
 * mi355_yolo_int8.h for what a segment and a unit are.
 *
 * A lane's state is (bit position, block slot inside the unit, zigzag index k; k == 0: the next symbol is a DC).  jec_run decodes
 * every symbol that STARTS in [bit, end_bit) -- a symbol is 1..31 bits (a code of <= 16 bits and <= 15 value bits), so the exit
 * position lies less than 31 bits past end_bit -- and returns the exit state, the blocks it finished, the sum of the DC differences
 * per scan component and an error (MI355_JPEG_E*, as decode_block of jpeg.c names them).  An error ends the run: the exit state is
 * then (end_bit, 0, 0), a pure function of the entry as every other exit.
 *
 * Writing mode (write != 0) also takes the ordinal of the block the entry state stands in (counted from the segment's first) and the
 * DC predictions at entry, stores every non-zero coefficient, and stops in front of the segment's last block + 1: nothing is stored
 * for a block at or beyond sg->total_blocks, whatever the bits say (the 1-bits that pad the last byte decode to something).
 *
 * Every loop is bounded: at most end_bit - bit symbols are taken (each is at least one bit in a table that parse_dht accepted; a
 * table with a zero-length code cannot hold a lane longer than that either).  Reads: the two dwords at bit >> 5 for bit < nbits,
 * which the zero padding behind the segment covers.
 */
#ifndef DNQ_JPEG_ENTROPY_CORE_H
#define DNQ_JPEG_ENTROPY_CORE_H
#include "../../include/mi355_yolo_int8.h"

#if defined(__HIPCC__)
#define JEC_FN __host__ __device__ static inline
#else
#define JEC_FN static inline
#endif

#define JEC_LANES 256

/* what the lanes of a segment share (the kernel keeps it in LDS) */
typedef struct jec_seg {
    const uint32_t *bits;
    uint32_t nbits;
    uint32_t total_blocks;  /* nunits * nslots */
    int ncomp, nslots;      /* blocks per unit */
    int slot_start[3];      /* first slot of component c; nslots for c >= ncomp */
    int bh[3], bv[3], blocks_w[3];
    int units_x, first_unit;
    int16_t *coef[3];
} jec_seg;

typedef struct jec_out {
    uint32_t bit;
    int slot, k;
    uint32_t blocks;    /* finished */
    uint32_t dc0, dc1, dc2; /* sums of the DC differences, modulo 2^32 (the stored coefficient keeps 16 bits) */
    int err;
} jec_out;

/* position in the 8x8 block (row-major) of the k-th coefficient of the zigzag sequence (T.81 figure A.6): the `zigzag` of jec_run */
#define JEC_ZIGZAG {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28, \
                    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63}

/* what is wrong with a segment record, as far as the record shows it (the message mi355_jpeg_entropy refuses it with); NULL: nothing.
 * Host only: the pointers are compared, not followed. */
static inline const char *jec_segment_check(const mi355_jpeg_segment *s)
{
    if (!s->bits || !s->huff) return "jpeg_entropy: null bits / huff pointer";
    if (((size_t)s->bits & 3) || ((size_t)s->huff & 3)) return "jpeg_entropy: bits and huff must be 4-byte aligned";
    if (s->nbytes > (1u << 28)) return "jpeg_entropy: a segment of more than 2^28 bytes";
    if (s->ncomp < 1 || s->ncomp > 3) return "jpeg_entropy: need 1 <= ncomp <= 3";
    if (s->nhuff < 1 || s->reserved) return "jpeg_entropy: need nhuff >= 1 and reserved == 0";
    if (s->units_x < 1 || s->units_y < 1 || s->units_x > 32768 || s->units_y > 32768) return "jpeg_entropy: need 1 <= units_x, units_y <= 32768";
    if (s->first_unit < 0 || s->nunits < 1 || (long)s->first_unit + s->nunits > (long)s->units_x * s->units_y)
        return "jpeg_entropy: first_unit .. first_unit + nunits - 1 must lie in the unit grid";
    for (int c = 0; c < s->ncomp; ++c) {
        if (!s->coef[c] || ((size_t)s->coef[c] & 1)) return "jpeg_entropy: null or misaligned coefficient plane";
        if (s->bh[c] < 1 || s->bh[c] > 4 || s->bv[c] < 1 || s->bv[c] > 4) return "jpeg_entropy: need 1 <= bh, bv <= 4";
        if (s->blocks_w[c] < 1 || s->blocks_h[c] < 1 || s->blocks_w[c] > 32768 || s->blocks_h[c] > 32768) return "jpeg_entropy: need 1 <= blocks_w, blocks_h <= 32768";
        if ((long)s->units_x * s->bh[c] > s->blocks_w[c] || (long)s->units_y * s->bv[c] > s->blocks_h[c])
            return "jpeg_entropy: the unit grid is larger than a component's plane";
        if (s->dc[c] < 0 || s->dc[c] >= s->nhuff || s->ac[c] < 0 || s->ac[c] >= s->nhuff) return "jpeg_entropy: a table index outside 0 .. nhuff - 1";
    }
    return 0;
}

JEC_FN void jec_seg_init(jec_seg *sg, const mi355_jpeg_segment *s)
{
    int n = 0;
    sg->bits = s->bits;
    sg->nbits = s->nbytes * 8u;
    sg->ncomp = s->ncomp;
    for (int c = 0; c < 3; ++c) {
        sg->slot_start[c] = n;
        sg->bh[c] = c < s->ncomp ? s->bh[c] : 1;
        sg->bv[c] = c < s->ncomp ? s->bv[c] : 1;
        sg->blocks_w[c] = c < s->ncomp ? s->blocks_w[c] : 1;
        sg->coef[c] = c < s->ncomp ? s->coef[c] : s->coef[0];
        if (c < s->ncomp) n += s->bh[c] * s->bv[c];
    }
    sg->nslots = n;
    sg->total_blocks = (uint32_t)s->nunits * (uint32_t)n;
    sg->units_x = s->units_x;
    sg->first_unit = s->first_unit;
}

/* the next 64 bits from position `bit` on, of which the top 33 at least are the stream's (bit < nbits) */
JEC_FN uint64_t jec_window(const uint32_t *bits, uint32_t bit)
{
    const uint32_t a = __builtin_bswap32(bits[bit >> 5]), b = __builtin_bswap32(bits[(bit >> 5) + 1]);
    return ((uint64_t)a << 32 | b) << (bit & 31);
}

/* the symbol of the code at the top of v16 (16 bits), its length in *len; -1: no code of the table matches */
JEC_FN int jec_symbol(const mi355_jpeg_huff *h, uint32_t v16, int *len)
{
    const uint32_t e = h->look[v16 >> 8];
    if (e) {
        *len = (int)(e >> 8);
        return *len <= 8 ? (int)(e & 255) : -1;
    }
    for (int l = 9; l <= 16; ++l) {
        const int c = (int)(v16 >> (16 - l));
        if (c < h->maxcode[l]) {
            const int idx = h->first[l] + c - h->mincode[l];
            if (c < h->mincode[l] || (uint32_t)idx >= 256u || idx >= h->nvalues) return -1;
            *len = l;
            return h->values[idx];
        }
    }
    return -1;
}

/* where block `block` (ordinal in the segment) of slot `slot`, component c, lies in its plane */
JEC_FN int16_t *jec_block_at(const jec_seg *sg, uint32_t block, int slot, int c)
{
    const int unit = sg->first_unit + (int)(block / (uint32_t)sg->nslots);
    const int uy = unit / sg->units_x, ux = unit - uy * sg->units_x;
    const int s = slot - sg->slot_start[c], bh = sg->bh[c];
    const int y = s / bh, x = s - y * bh;
    return sg->coef[c] + ((size_t)(uy * sg->bv[c] + y) * (size_t)sg->blocks_w[c] + (size_t)(ux * bh + x)) * 64;
}

/* tabs: the DC table of component c at tabs[2 c], its AC table at tabs[2 c + 1] */
JEC_FN jec_out jec_run(const jec_seg *sg, const mi355_jpeg_huff *tabs, const uint8_t *zigzag, uint32_t bit, int slot, int k, uint32_t end_bit,
                       int write, uint32_t block, uint32_t p0, uint32_t p1, uint32_t p2)
{
    jec_out o;
    o.blocks = 0; o.dc0 = o.dc1 = o.dc2 = 0; o.err = 0;
    const uint32_t total = sg->total_blocks;
    const int nslots = sg->nslots, s1 = sg->slot_start[1], s2 = sg->slot_start[2];
    uint32_t budget = end_bit > bit ? end_bit - bit : 0;
    int c = (slot >= s1) + (slot >= s2);
    int16_t *blk = 0;
    if (write && block < total) blk = jec_block_at(sg, block, slot, c);
    while (bit < end_bit && budget--) {
        if (write && block >= total) break;
        uint64_t win = jec_window(sg->bits, bit);
        int len = 0, done = 0;
        if (k == 0) {
            const int t = jec_symbol(tabs + 2 * c, (uint32_t)(win >> 48), &len);
            if (t < 0) { o.err = MI355_JPEG_EHUFF; break; }
            if (t > 15) { o.err = MI355_JPEG_EDC; break; }
            win <<= len;
            uint32_t diff = 0;
            if (t) { /* T.81 F.2.2.1 RECEIVE + EXTEND */
                const int v = (int)(win >> (64 - t));
                diff = (uint32_t)(v < (1 << (t - 1)) ? v - (1 << t) + 1 : v);
            }
            bit += (uint32_t)(len + t);
            if (c == 0) o.dc0 += diff;
            else if (c == 1) o.dc1 += diff;
            else o.dc2 += diff;
            if (write) {
                const uint32_t dc = c == 0 ? p0 + o.dc0 : c == 1 ? p1 + o.dc1 : p2 + o.dc2;
                if ((uint16_t)dc) blk[0] = (int16_t)(uint16_t)dc;
            }
            k = 1;
        } else {
            const int rs = jec_symbol(tabs + 2 * c + 1, (uint32_t)(win >> 48), &len);
            if (rs < 0) { o.err = MI355_JPEG_EHUFF; break; }
            const int s = rs & 15, r = rs >> 4;
            if (!s) {
                bit += (uint32_t)len;
                if (r != 15) done = 1; /* end of block */
                else {
                    k += 16;
                    if (k > 63) done = 1;
                }
            } else {
                k += r;
                if (k > 63) { o.err = MI355_JPEG_EINDEX; break; }
                win <<= len;
                const int v = (int)(win >> (64 - s));
                const int coef = v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
                bit += (uint32_t)(len + s);
                if (write && (int16_t)coef) blk[zigzag[k]] = (int16_t)coef;
                if (++k > 63) done = 1;
            }
        }
        if (done) {
            k = 0;
            ++o.blocks;
            ++block;
            if (++slot == nslots) slot = 0;
            c = (slot >= s1) + (slot >= s2);
            if (write && block < total) blk = jec_block_at(sg, block, slot, c);
        }
    }
    if (o.err) { bit = end_bit; slot = 0; k = 0; }
    o.bit = bit; o.slot = slot; o.k = k;
    return o;
}
#endif
