// jpeg_entropy.hip -- mi355_jpeg_entropy: Huffman decoding of baseline JPEG scans on the device, the step in front of jpeg.hip.
// One 256-thread workgroup per segment (a restart interval, or a whole scan), the segment's Huffman tables, the zigzag table and the
// segment's geometry in LDS.  The segment's bits are cut into subsequences of S bits; the workgroup walks them in rounds of 256, one
// per lane, and every lane decodes through jec_run (host/jpeg_entropy_core.h: the routine the host emulation runs, the same text):
//   1. speculate  lane i decodes from (i S, slot 0, k 0); lane 0 from the true state the round before left;
//   2. settle     a lane whose predecessor's exit state differs from the entry it last decoded from takes that exit and decodes again,
//                 until a workgroup-wide vote says nobody changed (lane t is right after t steps: at most 255 steps; Huffman streams
//                 resynchronise, real ones settle in a few).  All three fields of the state are compared;
//   3. scan       exclusive scan of the blocks finished and of the DC sums over the lanes, plus what the rounds before carried;
//   4. write      every lane decodes once more from its settled state and stores its non-zero coefficients.  A lane's error counts if
//                 it lies in front of the segment's last block; lanes behind the first such lane store nothing, the status word takes
//                 its code and the segment ends.
// The lanes diverge by nature (each follows its own symbols); the table lookups are LDS reads, the stream reads two dwords a symbol.
// No atomics: one thread of the one workgroup that owns the segment stores its status word.
#include "kargs.h"
#include "../host/jpeg_entropy_core.h"

__device__ static const uint8_t jpeg_zigzag_dev[64] = JEC_ZIGZAG;

struct JpegLaneScan {  // what the scan adds up
    uint32_t blocks, dc0, dc1, dc2;
};

__global__ __launch_bounds__(JEC_LANES) void jpeg_entropy_kernel(const mi355_jpeg_segment *table, int S, int *status)
{
    __shared__ mi355_jpeg_huff tabs[6];
    __shared__ jec_seg sg;
    __shared__ uint8_t zigzag[64];
    __shared__ uint32_t ex_bit[JEC_LANES], ex_sk[JEC_LANES];  // exit states: bit position, slot << 8 | k
    __shared__ JpegLaneScan sums[2][JEC_LANES];
    __shared__ unsigned long long err_mask[JEC_LANES / 64];
    const int i = threadIdx.x;
    const mi355_jpeg_segment &seg = table[blockIdx.x];

    // the tables of this segment's components, dword by dword
    {
        uint32_t *dst = reinterpret_cast<uint32_t *>(tabs);
        constexpr int words = (int)(sizeof(mi355_jpeg_huff) / 4);
        const int ncomp = seg.ncomp;
        for (int t = 0; t < 2 * ncomp; ++t) {
            const int which = (t & 1) ? seg.ac[t >> 1] : seg.dc[t >> 1];
            const uint32_t *src = reinterpret_cast<const uint32_t *>(seg.huff + which);
            for (int w = i; w < words; w += JEC_LANES) dst[t * words + w] = src[w];
        }
        if (i < 64) zigzag[i] = jpeg_zigzag_dev[i];
        if (i == 0) jec_seg_init(&sg, &seg);
    }
    __syncthreads();

    const uint32_t nbits = sg.nbits, total = sg.total_blocks;
    const uint32_t nsub = (nbits + (uint32_t)S - 1) / (uint32_t)S;
    uint32_t carry_bit = 0, carry_block = 0, p0 = 0, p1 = 0, p2 = 0;  // the same in every lane
    int carry_slot = 0, carry_k = 0, code = 0;

    for (uint32_t base = 0; base < nsub && !code; base += JEC_LANES) {
        const unsigned long long lo = (unsigned long long)(base + (uint32_t)i) * (uint32_t)S, hi = lo + (uint32_t)S;
        const uint32_t end = hi < nbits ? (uint32_t)hi : nbits;
        uint32_t e_bit = i ? (lo < nbits ? (uint32_t)lo : nbits) : carry_bit;
        int e_slot = i ? 0 : carry_slot, e_k = i ? 0 : carry_k;
        // a lane behind the segment's last subsequence (the last round only) has nothing to decode and nobody reads its exit
        const bool active = lo < nbits;
        // 1. speculate
        jec_out r = jec_run(&sg, tabs, zigzag, e_bit, e_slot, e_k, active ? end : 0u, 0, 0, 0, 0, 0);
        ex_bit[i] = r.bit;
        ex_sk[i] = (uint32_t)r.slot << 8 | (uint32_t)r.k;
        __syncthreads();
        // 2. settle
        for (int step = 0; step < JEC_LANES; ++step) {
            int changed = 0;
            if (i && active) {
                const uint32_t pb = ex_bit[i - 1], ps = ex_sk[i - 1];
                if (pb != e_bit || ps != ((uint32_t)e_slot << 8 | (uint32_t)e_k)) {
                    e_bit = pb; e_slot = (int)(ps >> 8); e_k = (int)(ps & 255);
                    r = jec_run(&sg, tabs, zigzag, e_bit, e_slot, e_k, end, 0, 0, 0, 0, 0);
                    changed = 1;
                }
            }
            __syncthreads();  // every lane has read its predecessor's exit of the step before
            if (changed) {
                ex_bit[i] = r.bit;
                ex_sk[i] = (uint32_t)r.slot << 8 | (uint32_t)r.k;
            }
            if (!__syncthreads_or(changed)) break;
        }
        // 3. inclusive scan over the lanes (Hillis-Steele, two buffers), read back exclusively
        JpegLaneScan mine = {r.blocks, r.dc0, r.dc1, r.dc2};
        int cur = 0;
        sums[0][i] = mine;
        __syncthreads();
        for (int d = 1; d < JEC_LANES; d <<= 1) {
            JpegLaneScan v = sums[cur][i];
            if (i >= d) {
                const JpegLaneScan o = sums[cur][i - d];
                v.blocks += o.blocks; v.dc0 += o.dc0; v.dc1 += o.dc1; v.dc2 += o.dc2;
            }
            sums[cur ^ 1][i] = v;
            cur ^= 1;
            __syncthreads();
        }
        const JpegLaneScan incl = sums[cur][i], all = sums[cur][JEC_LANES - 1];
        const uint32_t my_block = carry_block + incl.blocks - mine.blocks;
        // the first lane whose error lies in front of the segment's last block
        const int real = r.err && my_block + r.blocks < total;
        const unsigned long long ballot = __ballot(real);
        if ((i & 63) == 0) err_mask[i >> 6] = ballot;
        __syncthreads();
        int first_err = JEC_LANES;
        for (int w = JEC_LANES / 64 - 1; w >= 0; --w)
            if (err_mask[w]) first_err = w * 64 + __ffsll((long long)err_mask[w]) - 1;
        // 4. write
        if (active && i <= first_err && my_block < total)
            jec_run(&sg, tabs, zigzag, e_bit, e_slot, e_k, end, 1, my_block, p0 + incl.dc0 - mine.dc0, p1 + incl.dc1 - mine.dc1, p2 + incl.dc2 - mine.dc2);
        if (first_err < JEC_LANES) {
            if (i == first_err) ex_bit[0] = (uint32_t)r.err;  // nobody reads the exit states any more in this segment
            __syncthreads();
            code = (int)ex_bit[0];
        } else {
            carry_bit = ex_bit[JEC_LANES - 1];
            carry_slot = (int)(ex_sk[JEC_LANES - 1] >> 8);
            carry_k = (int)(ex_sk[JEC_LANES - 1] & 255);
            carry_block += all.blocks;
            p0 += all.dc0; p1 += all.dc1; p2 += all.dc2;
        }
        __syncthreads();  // the exit states, the sums and the masks are rewritten by the next round
    }
    if (i == 0) status[blockIdx.x] = code;
}

const char *jpeg_entropy_check(const mi355_jpeg_segment *host, int nsegments, int subseq_bits)
{
    if (!host || nsegments < 1 || nsegments > (1 << 24)) return "jpeg_entropy: null table / need 1 <= nsegments <= 2^24";
    if (subseq_bits < 32 || subseq_bits > 8192 || (subseq_bits & 31)) return "jpeg_entropy: subseq_bits must be a multiple of 32 in 32 .. 8192";
    for (int s = 0; s < nsegments; ++s) {
        const char *why = jec_segment_check(&host[s]);
        if (why) return why;
    }
    return nullptr;
}

int jpeg_entropy_launch(const mi355_jpeg_segment *table_dev, int nsegments, int subseq_bits, int *status_dev, hipStream_t st)
{
    hipLaunchKernelGGL(jpeg_entropy_kernel, dim3((unsigned)nsegments), dim3(JEC_LANES), 0, st, table_dev, subseq_bits, status_dev);
    return hipGetLastError() == hipSuccess ? MI355_OK : MI355_EHIP;
}
