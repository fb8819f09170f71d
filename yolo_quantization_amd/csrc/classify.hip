// classify.hip -- the classifier tail: the global average pool and the fully connected layer.
//
// connected (kernel id 14).  acc[b][j] = sum_k (w[j][k] - zp_w[j]) x[b][k] over K = C H W is a skinny GEMM: n filters by a handful of
// images, every weight byte used once.  On V_MFMA_I32_16X16X64_I8: M = 16 filters, N = 16 IMAGES, a K-step 64 bytes of the input in
// the tensor's cell order -- cell (y, x) after cell, cp = round_up(C, 16) bytes a cell ("packed K", Kp = H W cp; the tensor's own cell
// size cs >= cp is only the stride of the gather).  mi355_connected_pack permutes the reference's (c, y, x) record into that order,
// stores w - 128 with zeros on the spare channels C..cp of every cell and on the last step's padding, in MFMA lane order
// [M tile][K step][lane][16 B]: the A fragment of a lane is one 16-byte global load, coalesced to 1 KB per wave, straight into registers (read one step ahead), and no weight byte is read twice in a launch or passes through LDS.
//
// Work split.  A workgroup owns up to four M tiles (one per wave), one K slice and one group of up to 64 images (four N tiles).  It
// walks its slice in chunks: the chunk's bytes of every image of the group are gathered into LDS cell by cell (pad cells are never
// read; bytes at or beyond C and images past the batch are written as x' = 0), image after image at a pitch of chunk bytes + 16, so
// that the sixteen lanes of a B-fragment read (sixteen images, one 16-byte column) fall on sixteen different 16-byte bank groups.
// Per K-step a wave issues one A load, and per N tile one LDS read, one MFMA and four v_dot4 that add the fragment's bytes into the
// lane's sum of x'; two shuffles across the four K groups of the wave give every lane the whole sum of x' of its own image -- the
// column its accumulators belong to.  acc = acc1 + (128 - zp_w) sum x' + [128 sum w' + 128 K (128 - zp_w)]  (DESIGN.md 2).
//
// Split-K.  int32 sums are exact in any order, so S slices change no bit and need no atomics: with S > 1 the workgroups store their
// partial accumulators [S][B][16 mtiles] (16-byte vector stores) and partial sums of x' [S][B] into the caller's workspace and
// connected_sum_kernel adds them, corrects and runs the epilogue; with S = 1 the main kernel runs it itself.
//
// avgpool_u8.  One workgroup per (image, 64-byte channel chunk); lane = (16-byte column, pixel phase of 64): one 16-byte load a cell,
// sixteen channel sums in registers over cells phase, phase + 64, ..; the phases meet in LDS; q = (2 S + HW) / (2 HW) in unsigned
// 32-bit integers.
#include "kargs.h"

namespace {

__device__ __forceinline__ uint32_t fc_epilogue(uint32_t acct, const GrpRow &rw, const FcArgs &a, int b, int oc)
{
    const uint32_t u8 = requant_u8((int32_t)acct, rw.bias, rw.mval, rw.sval, a.zp_act, a.act, a.store_mode);
    const size_t ridx = (size_t)b * a.n + oc;
    if (a.acc_out) a.acc_out[ridx] = (int32_t)acct;
    if (a.y_f32) a.y_f32[ridx] = (float)((int)u8 - a.zp_act) * a.s_act;
    return u8;
}

// bytes of rows row0 .. row0 + 3 (those below n) into image b's one cell of y
__device__ __forceinline__ void fc_store(const FcArgs &a, int b, int row0, const uint32_t (&bytes)[4])
{
    if (!a.y) return;
    uint8_t *dst = a.y + (size_t)((long)a.out_lead + ((long)b * 2 + 1) * 2) * a.out_cs + row0;
    if (row0 + 3 < a.n) {
        *reinterpret_cast<uint32_t *>(dst) = (bytes[0] | bytes[1] << 8 | bytes[2] << 16 | bytes[3] << 24) ^ 0x80808080u;
    } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (row0 + r < a.n) dst[r] = (uint8_t)(bytes[r] ^ 0x80u);
    }
}

// the blob in device memory is the one packed for this launch's (n, C, H, W): the host side of the call cannot read it
__device__ __forceinline__ bool fc_blob_matches(const FcArgs &a)
{
    const FcBlobHeader *h = a.hdr;
    return h->magic == MI355_FC_MAGIC && h->n == a.n && h->C == a.C && h->H == a.H && h->W == a.W && h->cp == a.cp && h->nsteps == a.nsteps;
}

__global__ __launch_bounds__(FC_THREADS) void connected_kernel(const FcArgs a)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];  // [image of the group][pitch] staged x' bytes of the chunk
    if (!fc_blob_matches(a)) return;  // (uniform: before any barrier)

    const int tid = threadIdx.x, lane = tid & 63, nthreads = blockDim.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lp = lane & 15, q = lane >> 4;

    const int fb = blockIdx.x % a.fblocks;
    const int rest = blockIdx.x / a.fblocks;
    const int sl = rest % a.S, ig = rest / a.S;
    const int tile = fb * FC_MB + wave;
    const bool live = tile < a.mtiles;
    const int b0 = ig * 64, nimg = min(64, a.B - b0), nt = (nimg + 15) >> 4;
    const int st0 = sl * a.sps, st1 = min(st0 + a.sps, a.nsteps);
    const int hw = a.H * a.W, W1 = a.W + 1;

    v4i acc[4] = {};
    int sx[4] = {0, 0, 0, 0};
    const v4i *fr = reinterpret_cast<const v4i *>(a.frag) + (size_t)(live ? tile : 0) * a.nsteps * 64 + lane;

#pragma unroll 1
    for (int c0 = st0; c0 < st1; c0 += a.chunk) {
        const int c1 = min(c0 + a.chunk, st1);
        const int units = (c1 - c0) * 4, total = nt * 16 * units;
        __syncthreads();  // the previous chunk's bytes are read
        for (int i = tid; i < total; i += nthreads) {
            const int img = i / units, u = i - img * units;
            const int k = c0 * 64 + u * 16;
            const int cell = k / a.cp, ch = k - cell * a.cp;
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (img < nimg && cell < hw && ch < a.C) {
                const int yy = cell / a.W, xx = cell - yy * a.W;
                v = *reinterpret_cast<const uint4 *>(a.x + (size_t)((long)a.in_lead + ((long)(b0 + img) * (a.H + 1) + yy + 1) * W1 + xx) * a.in_cs + ch);
                const int keep = a.C - ch;  // data bytes of this piece
                if (keep < 16) {
                    uint32_t d[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int kb = keep - 4 * e;
                        d[e] = kb >= 4 ? d[e] : (kb <= 0 ? 0u : d[e] & (0xFFFFFFFFu >> (8 * (4 - kb))));
                    }
                    v = make_uint4(d[0], d[1], d[2], d[3]);
                }
            }
            *reinterpret_cast<uint4 *>(smem + (size_t)img * a.pitch + (size_t)u * 16) = v;
        }
        __syncthreads();
        if (!live) continue;
        v4i wn = fr[(size_t)c0 * 64];
#pragma unroll 1
        for (int st = c0; st < c1; ++st) {
            const v4i wf = wn;
            if (st + 1 < c1) wn = fr[(size_t)(st + 1) * 64];
            const char *col = smem + (size_t)lp * a.pitch + (size_t)(st - c0) * 64 + q * 16;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (j < nt) {
                    const v4i bf = *reinterpret_cast<const v4i *>(col + (size_t)j * 16 * a.pitch);
                    acc[j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(wf, bf, acc[j], 0, 0, 0);
                    int t = sx[j];
                    t = __builtin_amdgcn_sdot4(bf[0], 0x01010101, t, false);
                    t = __builtin_amdgcn_sdot4(bf[1], 0x01010101, t, false);
                    t = __builtin_amdgcn_sdot4(bf[2], 0x01010101, t, false);
                    t = __builtin_amdgcn_sdot4(bf[3], 0x01010101, t, false);
                    sx[j] = t;
                }
            }
        }
    }
    if (!live) return;  // (no barrier follows)

    // lane (lp, q): image 16 j + lp of the group, filter rows 4 q .. 4 q + 3 of the tile; the K groups' sums of x' meet in every lane
    const int row0 = tile * 16 + 4 * q;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (j >= nt) break;
        int sxt = sx[j];
        sxt += __shfl_xor(sxt, 16);
        sxt += __shfl_xor(sxt, 32);
        const int b = b0 + 16 * j + lp;
        if (b >= a.B) continue;
        if (a.S > 1) {
            *reinterpret_cast<v4i *>(a.ws_acc + ((size_t)sl * a.B + b) * a.npad + row0) = acc[j];
            if (fb == 0 && wave == 0 && q == 0) a.ws_sx[(size_t)sl * a.B + b] = sxt;
            continue;
        }
        if (row0 >= a.n) continue;
        uint32_t bytes[4] = {0, 0, 0, 0};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (row0 + r >= a.n) break;
            const GrpRow rw = a.rows[row0 + r];
            bytes[r] = fc_epilogue((uint32_t)acc[j][r] + (uint32_t)rw.d * (uint32_t)sxt + (uint32_t)rw.cst, rw, a, b, row0 + r);
        }
        fc_store(a, b, row0, bytes);
    }
}

// S > 1: one thread per (image, four filter rows) adds the slices' partial sums, corrects and runs the epilogue
__global__ __launch_bounds__(256) void connected_sum_kernel(const FcArgs a)
{
    if (!fc_blob_matches(a)) return;
    const int quads = a.npad >> 2;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)a.B * quads) return;
    const int b = (int)(idx / quads), row0 = 4 * (int)(idx - (long)b * quads);
    if (row0 >= a.n) return;
    v4i t = {0, 0, 0, 0};
    int sxt = 0;
    for (int s = 0; s < a.S; ++s) {
        t += *reinterpret_cast<const v4i *>(a.ws_acc + ((size_t)s * a.B + b) * a.npad + row0);
        sxt += a.ws_sx[(size_t)s * a.B + b];
    }
    uint32_t bytes[4] = {0, 0, 0, 0};
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if (row0 + r >= a.n) break;
        const GrpRow rw = a.rows[row0 + r];
        bytes[r] = fc_epilogue((uint32_t)t[r] + (uint32_t)rw.d * (uint32_t)sxt + (uint32_t)rw.cst, rw, a, b, row0 + r);
    }
    fc_store(a, b, row0, bytes);
}

__global__ __launch_bounds__(256) void avgpool_u8_kernel(const AvgArgs a)
{
    __shared__ uint32_t part[64][65];  // [phase][channel of the chunk], odd pitch
    const int tid = threadIdx.x, qc = tid & 3, phase = tid >> 2;
    const int b = blockIdx.x / a.nchunks, chunk = blockIdx.x - b * a.nchunks;
    const int ch0 = chunk * 64 + qc * 16;  // first channel of this lane's 16-byte piece; a piece of spare channels only is never read
    const int hw = a.H * a.W, W1 = a.W + 1;
    uint32_t s[16] = {};
    if (ch0 < a.C) {
        const uint8_t *img = a.x + ((size_t)a.in_lead + (size_t)b * (a.H + 1) * W1 + W1) * a.in_cs + ch0;  // cell (0, 0) of image b
        int yy = phase / a.W, xx = phase - yy * a.W;
        for (int p = phase; p < hw; p += 64) {
            const uint4 v = *reinterpret_cast<const uint4 *>(img + ((size_t)yy * W1 + xx) * a.in_cs);
            const uint32_t d[4] = {v.x ^ 0x80808080u, v.y ^ 0x80808080u, v.z ^ 0x80808080u, v.w ^ 0x80808080u};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                s[4 * e] += d[e] & 0xFFu; s[4 * e + 1] += (d[e] >> 8) & 0xFFu; s[4 * e + 2] += (d[e] >> 16) & 0xFFu; s[4 * e + 3] += d[e] >> 24;
            }
            yy += a.dq; xx += a.dr;  // 64 cells on
            if (xx >= a.W) { xx -= a.W; ++yy; }
        }
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) part[phase][qc * 16 + i] = s[i];
    __syncthreads();
    const int ch = chunk * 64 + tid;
    if (tid < 64 && ch < a.C) {
        uint32_t t = 0;
#pragma unroll 8
        for (int p = 0; p < 64; ++p) t += part[p][tid];
        const uint32_t qv = (2u * t + (uint32_t)hw) / (2u * (uint32_t)hw);  // round-half-up of the mean: at most 255
        a.y[((size_t)a.out_lead + (size_t)b * 4 + 2) * a.out_cs + ch] = (uint8_t)(qv ^ 0x80u);
    }
}

}  // namespace

// ceil(nsteps / slices) K-steps a slice and the number of non-empty slices for the rule's S (fc_split, kargs.h)
int connected_launch(FcArgs &a, hipStream_t st)
{
    if (a.n < 1 || a.B < 1 || a.nsteps < 1 || a.in_cs % 16 || ((uintptr_t)a.x & 15) || ((uintptr_t)a.frag & 15)) return MI355_EINVAL;
    a.mtiles = (a.n + 15) / 16;
    a.npad = a.mtiles * 16;
    a.fblocks = (a.mtiles + FC_MB - 1) / FC_MB;
    const int igroups = (a.B + 63) / 64;
    const int rule = fc_split(a.n, a.ktrue, a.B);
    a.sps = (a.nsteps + rule - 1) / rule;
    a.S = (a.nsteps + a.sps - 1) / a.sps;
    if (a.S > 1 && (!a.ws_acc || ((uintptr_t)a.ws_acc & 15))) return MI355_EINVAL;
    a.ws_sx = a.ws_acc ? a.ws_acc + (size_t)a.S * a.B * a.npad : nullptr;
    // the chunk: as many K-steps of every image of a group as fit in 64 KB at a pitch of chunk bytes + 16 (both plans: two
    // workgroups a CU; the plan changes nothing here)
    const int ipad = a.B >= 64 ? 64 : (a.B + 15) / 16 * 16;
    int chunk = (FC_LDS_MAX / ipad - 16) / 64;
    if (chunk > a.sps) chunk = a.sps;
    a.chunk = chunk;
    a.pitch = chunk * 64 + 16;
    const size_t lds = (size_t)ipad * a.pitch;
    const long grid = (long)a.fblocks * a.S * igroups;
    if (grid > 0x7FFFFFFF) return MI355_EINVAL;
    const int threads = 64 * (a.mtiles < FC_MB ? a.mtiles : FC_MB);
    conv_launch_note(grid, threads, lds);
    hipLaunchKernelGGL(connected_kernel, dim3((int)grid), dim3(threads), lds, st, a);
    if (hipGetLastError() != hipSuccess) return MI355_EHIP;
    if (a.S > 1) {
        const long work = (long)a.B * (a.npad / 4);
        hipLaunchKernelGGL(connected_sum_kernel, dim3((int)((work + 255) / 256)), dim3(256), 0, st, a);
        if (hipGetLastError() != hipSuccess) return MI355_EHIP;
    }
    return MI355_OK;
}

int avgpool_launch(AvgArgs &a, hipStream_t st)
{
    a.nchunks = (a.C + 63) / 64;
    a.dq = 64 / a.W; a.dr = 64 % a.W;
    const long grid = (long)a.B * a.nchunks;
    if (grid > 0x7FFFFFFF) return MI355_EINVAL;
    hipLaunchKernelGGL(avgpool_u8_kernel, dim3((int)grid), dim3(256), 0, st, a);
    return hipGetLastError() == hipSuccess ? MI355_OK : MI355_EHIP;
}
