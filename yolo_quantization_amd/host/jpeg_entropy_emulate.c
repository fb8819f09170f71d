/*
 * jpeg_entropy_emulate.c -- mi355_jpeg_entropy on the CPU: the four phases of the kernel (csrc/jpeg_entropy.hip) with the 256 lanes of
 * a workgroup run one after another, every lane through the routine the kernel's lanes run (jpeg_entropy_core.h).  The pointers of
 * the segment table are host pointers here.  For tests and for running hostile streams under sanitizers; no device.
 */
#include "jpeg_scan.h"
#include "jpeg_entropy_core.h"
#include <string.h>

static const uint8_t zigzag[64] = JEC_ZIGZAG;

typedef struct { uint32_t bit; int slot, k; } lane_state;

static int same(lane_state a, lane_state b) { return a.bit == b.bit && a.slot == b.slot && a.k == b.k; }

static int emulate_segment(const mi355_jpeg_segment *s, int subseq_bits, int *steps_out)
{
    jec_seg sg;
    mi355_jpeg_huff tabs[6];
    jec_seg_init(&sg, s);
    memset(tabs, 0, sizeof(tabs));
    for (int c = 0; c < s->ncomp; ++c) {
        tabs[2 * c] = s->huff[s->dc[c]];
        tabs[2 * c + 1] = s->huff[s->ac[c]];
    }
    const uint32_t S = (uint32_t)subseq_bits, nsub = (sg.nbits + S - 1) / S;
    lane_state carry = {0, 0, 0};
    uint32_t block = 0, pred[3] = {0, 0, 0};
    int status = 0, slowest = 0;
    for (uint32_t base = 0; base < nsub && !status; base += JEC_LANES) {
        lane_state entry[JEC_LANES], ex[JEC_LANES];
        jec_out res[JEC_LANES];
        uint32_t end[JEC_LANES];
        /* 1. speculate */
        for (int i = 0; i < JEC_LANES; ++i) {
            const uint64_t lo = (uint64_t)(base + (uint32_t)i) * S, hi = lo + S;
            end[i] = lo >= sg.nbits ? 0 : hi < sg.nbits ? (uint32_t)hi : sg.nbits; /* 0: a lane behind the last subsequence decodes nothing */
            entry[i] = i ? (lane_state){lo < sg.nbits ? (uint32_t)lo : sg.nbits, 0, 0} : carry;
            res[i] = jec_run(&sg, tabs, zigzag, entry[i].bit, entry[i].slot, entry[i].k, end[i], 0, 0, 0, 0, 0);
            ex[i] = (lane_state){res[i].bit, res[i].slot, res[i].k};
        }
        /* 2. settle: every lane looks at the exit its predecessor had BEFORE this step, as the lanes of the kernel do */
        int steps = 0;
        for (; steps < JEC_LANES; ++steps) {
            lane_state seen[JEC_LANES];
            int changed = 0;
            memcpy(seen, ex, sizeof(seen));
            for (int i = 1; i < JEC_LANES; ++i)
                if (end[i] && !same(seen[i - 1], entry[i])) {
                    entry[i] = seen[i - 1];
                    res[i] = jec_run(&sg, tabs, zigzag, entry[i].bit, entry[i].slot, entry[i].k, end[i], 0, 0, 0, 0, 0);
                    ex[i] = (lane_state){res[i].bit, res[i].slot, res[i].k};
                    changed = 1;
                }
            if (!changed) break;
        }
        if (steps > slowest) slowest = steps;
        /* 3. scan, 4. write: lanes up to the first whose error lies in front of the segment's last block */
        for (int i = 0; i < JEC_LANES; ++i) {
            const int real = res[i].err && block + res[i].blocks < sg.total_blocks;
            jec_run(&sg, tabs, zigzag, entry[i].bit, entry[i].slot, entry[i].k, end[i], 1, block, pred[0], pred[1], pred[2]);
            if (real) { status = res[i].err; break; }
            block += res[i].blocks;
            pred[0] += res[i].dc0; pred[1] += res[i].dc1; pred[2] += res[i].dc2;
        }
        carry = ex[JEC_LANES - 1];
    }
    if (steps_out) *steps_out = slowest;
    return status;
}

int jpeg_entropy_emulate_host(const mi355_jpeg_segment *segments, int nsegments, int subseq_bits, int *status, int *steps_out)
{
    if (!segments || !status || nsegments < 1 || subseq_bits < 32 || subseq_bits > 8192 || (subseq_bits & 31)) return -1;
    for (int i = 0; i < nsegments; ++i) {
        const mi355_jpeg_segment *s = &segments[i];
        if (jec_segment_check(s)) return -1;
        status[i] = emulate_segment(s, subseq_bits, steps_out ? &steps_out[i] : NULL);
    }
    return 0;
}
