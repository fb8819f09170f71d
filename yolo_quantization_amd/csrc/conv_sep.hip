// conv_sep.hip -- the depthwise-separable block: a depthwise k x k layer and the dense 1x1 layer that reads it, in one launch
// (kernel id 15).  sep(x) = pw(dw(x)) byte for byte:
//        m[c][p]   = dw epilogue( sum_taps (wd_u8[c][tap] - zp_wd[c]) x_u8[c][tap(p)] )          conv_dw.hip, out-of-image taps = zp_in
//        acc[j][p] = sum_c (w_u8[j][c] - zp_w[j]) m[c][p]                                        exact int32, zp_in(pw) = zp_act(dw)
// then the pw layer's epilogue.  The intermediate m lives in LDS only.
//
// Work split.  A workgroup (256 threads) owns one image, a tile of 128 output pixels (conv_dw.hip's 16 x 8 / 8 x 16 / 4 x 32 choice)
// and a block of 128 (MS = 1) or 256 (MS = 2) filters, and walks the channels in chunks of 64.  Per chunk:
//   dw stage   conv_dw.hip's lane layout: a lane owns four channels (one dword of a cell) and a run of DW_RUN = 8 pixels along x, 16
//              lanes x 16 runs.  The patch with its halo is staged in LDS (16-byte loads, un-biased, out-of-image cells and channels
//              >= c written as zp_in: no bounds check in the MAC loop); 3x3 / 5x5 at stride 1 | 2 keep (w - zp_w) in VGPRs, every
//              other size reads int16 weights from LDS.  The dw epilogue (common.h requant_group / requant_u8) runs in registers and
//              the BIASED bytes (u8 ^ 0x80) go to the intermediate tile T[pixel][64 channels], SEP_TPITCH = 80 bytes a pixel: the 16
//              lanes of a B-fragment quarter-wave read 16 bytes each at 80-byte steps, which are 16 different bank quads.  Channels
//              >= c are stored as biased 0, i.e. x' = 0: nothing for the GEMM, nothing for sum x'.
//   pw stage   V_MFMA_I32_32X32X32_I8.  Wave w owns filters [(4 fb + w) 32 MS, + 32 MS) of the block and all 128 pixels: MS x 4
//              accumulator tiles, 64 MS registers.  B fragments are 16-byte LDS reads of T; A fragments come from the pw layer's own
//              mi355_conv_pack blob in global memory, one K-step ahead.  sum_c x' per pixel (the zp_w correction) is a V_DOT4 of
//              every B fragment against ones.
// The pw blob has one of two forms and the kernel reads either (GEN):
//   generic (c % 16 != 0)       the general-kernel plane [mpad / 32][ceil(c / 16)][64 lanes][16 B]: a K-step is 16 channels in lane
//                               half 0 against zero weights in half 1 (the second tap slot of a 1x1 layer is empty)
//   specialised (c % 16 == 0)   the row plane [mpad / 16][ksteps][4 units][16 rows][16 B] of the 1x1 kernels: lane (row, kh) of
//                               K-step q reads the 16 bytes of row `row`, 16-channel block 2 q + kh -- a full 32-channel K-step
// Pipeline.  T is double-buffered, and the patch too where LDS allows: between two barriers a wave multiplies chunk i, runs the
// depthwise stage of chunk i + 1 into the other T buffer and issues the loads of chunk i + 2's patch.  One barrier per chunk (two
// with a single patch buffer).
#include "kargs.h"
#include <mutex>

namespace {

constexpr int SEP_THREADS = 256;
constexpr int SEP_PIX = 128;                          // output pixels of a workgroup: 16 runs of DW_RUN
constexpr int SEP_TPITCH = 80;                        // bytes between two pixels of the intermediate tile (64 channels + 16)
constexpr int SEP_TBYTES = SEP_PIX * SEP_TPITCH;      // one intermediate tile
constexpr size_t SEP_LDS_MAX = 160 * 1024, SEP_LDS_SHARED = 80 * 1024;
static_assert(SEP_PIX == 16 * DW_RUN, "the tile is the depthwise kernel's");

__device__ __forceinline__ void sep_mac4(int (&acc)[4], const int (&w)[4], uint32_t d)
{
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[c] += __mul24(w[c], (int)((d >> (8 * c)) & 0xFFu));
}

// requant_u8's second half (common.h): activation, zero point, store mode, uint8 wrap
__device__ __forceinline__ uint32_t sep_finish(int32_t q, int zp_act, int act, int store_mode)
{
    int32_t v;
    if (act == MI355_ACT_LEAKY) {
        const uint32_t uq = 0u - (uint32_t)q;
        v = q < 0 ? zp_act - (int32_t)((uq + 5u) / 10u) : q + zp_act;
    } else if (act == MI355_ACT_RELU6) {
        v = q <= 0 ? zp_act : q + zp_act;
    } else {
        v = q + zp_act;
    }
    if (store_mode == MI355_STORE_SATURATE) v = v < 0 ? 0 : (v > 255 ? 255 : v);
    return (uint32_t)v & 0xFFu;
}

// the dw epilogue of a lane's four channels x DW_RUN pixels when every shift_value is a power of two: biased packed bytes
template <int ACT, bool SAT>
__device__ __forceinline__ void sep_dw_group(const int (&acc)[DW_RUN][4], const int32_t *bias, const double *mprime, int zp,
                                             uint32_t (&packed)[DW_RUN])
{
    int32_t accb[4][DW_RUN];
    double mp[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int bv = bias[c];
        mp[c] = mprime[c];
#pragma unroll
        for (int j = 0; j < DW_RUN; ++j) accb[c][j] = acc[j][c] + bv;
    }
    requant_group<ACT, SAT, DW_RUN>(accb, mp, zp, packed);
}

// KS, S: compile-time depthwise size and stride (3 | 5, 1 | 2) or 0, 0 = both read from the arguments; GEN: the pw blob's form;
// MS: 32-filter accumulator tiles per wave
template <int KS, int S, bool GEN, int MS>
__global__ __launch_bounds__(SEP_THREADS) void conv_sep_kernel(const SepArgs a)
{
    constexpr int RUN = DW_RUN, NS = SEP_PIX / 32;
    constexpr int SPC = GEN ? 4 : 2;  // K-steps per 64-channel chunk
    extern __shared__ __attribute__((aligned(16))) char smem[];

    // both blobs must be the launch's layers: a foreign header ends the workgroup before it reads or writes anything else
    if (a.dhdr->magic != MI355_DW_MAGIC || a.dhdr->c != a.c || a.dhdr->ksize != a.ksize || a.hdr->magic != MI355_BLOB_MAGIC ||
        a.hdr->n != a.n || a.hdr->c != a.c || a.hdr->ksize != 1)
        return;

    const int tid = threadIdx.x, lane = tid & 63, cl = tid & 15, run = tid >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kh = lane >> 5, lj = lane & 31;
    const int k = KS ? KS : a.ksize, s = KS ? S : a.stride, kk = k * k;
    const int pitch = a.pitch, pw = a.pw;
    int idx = blockIdx.x;
    const int fb = idx % a.fblocks;
    idx /= a.fblocks;
    const int tpi = a.tiles_x * a.tiles_y;
    const int b = idx / tpi;
    idx -= b * tpi;
    const int ty = idx / a.tiles_x, tx = idx - ty * a.tiles_x;
    const int RY = 1 << a.ry_sh, TW = (16 >> a.ry_sh) * RUN;
    const int oy0 = ty * RY, ox0 = tx * TW;
    const int iy0 = oy0 * s - a.pad, ix0 = ox0 * s - a.pad;
    const int nch = a.nchunks;

    char *T = smem;                       // [2][SEP_PIX][SEP_TPITCH]
    char *PB = smem + 2 * SEP_TBYTES;     // [pbufs] patch [ph][pitch] cells of 16 dwords, then (KS == 0) the chunk's weights [kk][64] int16
    const size_t wl_off = (size_t)a.ph * pitch * 64;

    // ---- stage chunk `ch` into patch buffer `buf`: 16-byte pieces, plain bytes; outside the image or beyond the channels: zp_in
    auto stage = [&](int ch, int buf) {
        uint32_t *P = reinterpret_cast<uint32_t *>(PB + (size_t)buf * a.pbytes);
        const int vp = min(4, a.pieces16 - 4 * ch);
        const uint32_t fill = (uint32_t)(a.zp_in & 0xFF) * 0x01010101u;
        const int npieces = a.ph * pw * 4;
        const size_t W1 = (size_t)a.W + 1;
        const uint8_t *xb = a.x + (size_t)ch * 64;
        for (int i = tid; i < npieces; i += SEP_THREADS) {
            const int cell = i >> 2, q = i & 3;
            const int r = fd_div(cell, a.fd_pw), cc = cell - r * pw;
            const int iy = iy0 + r, ix = ix0 + cc;
            uint4 v = make_uint4(fill, fill, fill, fill);
            if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W && q < vp) {
                const size_t src = ((size_t)a.in_lead + ((size_t)b * (a.H + 1) + iy + 1) * W1 + ix) * a.in_cs + q * 16;
                v = *reinterpret_cast<const uint4 *>(xb + src);
                v.x ^= 0x80808080u; v.y ^= 0x80808080u; v.z ^= 0x80808080u; v.w ^= 0x80808080u;
            }
            *reinterpret_cast<uint4 *>(P + (size_t)(r * pitch + cc) * 16 + q * 4) = v;
        }
        if constexpr (KS == 0) {
            uint32_t *WL = reinterpret_cast<uint32_t *>(reinterpret_cast<char *>(P) + wl_off);
            const uint32_t *src = reinterpret_cast<const uint32_t *>(a.wd + (size_t)ch * kk * 64);
            for (int i = tid; i < kk * 32; i += SEP_THREADS) WL[i] = src[i];
        }
    };

    // ---- depthwise stage of chunk `ch`: patch buffer `buf` -> intermediate tile `tb`
    const int ry = run & (RY - 1), rx = run >> a.ry_sh;
    const bool dpow2 = a.dhdr->pow2 == 1;
    auto dw = [&](int ch, int buf, int tb) {
        const uint32_t *P = reinterpret_cast<const uint32_t *>(PB + (size_t)buf * a.pbytes);
        const uint32_t *row0 = P + (size_t)(ry * s * pitch + rx * RUN * s) * 16 + cl;  // tap (0, 0) of the run's first output
        const int16_t *wg = a.wd + (size_t)ch * kk * 64;
        int acc[RUN][4];
#pragma unroll
        for (int j = 0; j < RUN; ++j)
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[j][c] = 0;
        if constexpr (KS != 0) {
            int w[KS * KS][4];
#pragma unroll
            for (int t = 0; t < KS * KS; ++t) {
                const short4 q = *reinterpret_cast<const short4 *>(wg + t * 64 + 4 * cl);
                w[t][0] = q.x; w[t][1] = q.y; w[t][2] = q.z; w[t][3] = q.w;
            }
            constexpr int L = (RUN - 1) * S + KS;
#pragma unroll
            for (int ky = 0; ky < KS; ++ky) {
                uint32_t st[L];
#pragma unroll
                for (int i = 0; i < L; ++i) st[i] = row0[(size_t)(ky * pitch + i) * 16];
#pragma unroll
                for (int j = 0; j < RUN; ++j)
#pragma unroll
                    for (int kx = 0; kx < KS; ++kx) sep_mac4(acc[j], w[ky * KS + kx], st[j * S + kx]);
            }
        } else {
            const uint32_t *WL = reinterpret_cast<const uint32_t *>(reinterpret_cast<const char *>(P) + wl_off);
#pragma unroll 1
            for (int ky = 0; ky < k; ++ky)
#pragma unroll 1
                for (int kx = 0; kx < k; ++kx) {
                    const uint2 wq = *reinterpret_cast<const uint2 *>(WL + (ky * k + kx) * 32 + 2 * cl);
                    const int w[4] = {(int)(short)(wq.x & 0xFFFFu), (int)wq.x >> 16, (int)(short)(wq.y & 0xFFFFu), (int)wq.y >> 16};
                    const uint32_t *src = row0 + (size_t)(ky * pitch + kx) * 16;
#pragma unroll
                    for (int j = 0; j < RUN; ++j) sep_mac4(acc[j], w, src[(size_t)j * s * 16]);
                }
        }
        // the dw layer's epilogue; the per-channel arrays are padded to whole chunks, so ch0 + 3 is always inside them
        const int ch0 = ch * 64 + 4 * cl;
        uint32_t packed[RUN];
        if (dpow2) {
            const int32_t *bp = a.dbias + ch0;
            const double *mp = a.dmprime + ch0;
            const bool sat = a.dstore == MI355_STORE_SATURATE;
            if (a.dact == MI355_ACT_LEAKY) {
                if (sat) sep_dw_group<MI355_ACT_LEAKY, true>(acc, bp, mp, a.zp_mid, packed);
                else sep_dw_group<MI355_ACT_LEAKY, false>(acc, bp, mp, a.zp_mid, packed);
            } else if (a.dact == MI355_ACT_RELU6) {
                if (sat) sep_dw_group<MI355_ACT_RELU6, true>(acc, bp, mp, a.zp_mid, packed);
                else sep_dw_group<MI355_ACT_RELU6, false>(acc, bp, mp, a.zp_mid, packed);
            } else {  // RELU is stored like LINEAR (ref src/convolutional_layer.c:740-742)
                if (sat) sep_dw_group<MI355_ACT_LINEAR, true>(acc, bp, mp, a.zp_mid, packed);
                else sep_dw_group<MI355_ACT_LINEAR, false>(acc, bp, mp, a.zp_mid, packed);
            }
        } else {
#pragma unroll
            for (int j = 0; j < RUN; ++j) packed[j] = 0x80808080u;
            // (channels >= c of the last chunk read the blob's zero padding, M = S = 0: integer 0 in, a finite byte out, masked off below)
#pragma unroll 1
            for (int c = 0; c < 4; ++c) {
                const int bias = a.dbias[ch0 + c];
                const double mv = a.dmval[ch0 + c], sv = a.dsval[ch0 + c];
#pragma unroll
                for (int j = 0; j < RUN; ++j) packed[j] ^= requant_u8(acc[j][c], bias, mv, sv, a.zp_mid, a.dact, a.dstore) << (8 * c);
            }
        }
        // channels >= c: biased 0
        const int nv = min(max(a.c - ch0, 0), 4);
        const uint32_t keep = nv == 4 ? 0xFFFFFFFFu : ((1u << (8 * nv)) - 1u);
        char *dst = T + (size_t)tb * SEP_TBYTES + (size_t)(run * RUN) * SEP_TPITCH + 4 * cl;
#pragma unroll
        for (int j = 0; j < RUN; ++j) *reinterpret_cast<uint32_t *>(dst + j * SEP_TPITCH) = packed[j] & keep;
    };

    // ---- pointwise stage
    const int mt0 = (fb * 4 + wave) * MS;              // first 32-filter tile of this wave
    const bool live = mt0 * 32 < a.n;                  // (wave-uniform) the wave has filters
    const int nst = GEN ? (a.c + 15) / 16 : (a.c + 31) / 32;  // K-steps of the layer
    auto load_a = [&](int q, int ms) -> v4i {
        v4i z = {0, 0, 0, 0};
        if (mt0 + ms >= a.mt32) return z;              // past the plane's rows (filters >= n there anyway)
        if constexpr (GEN) {
            return reinterpret_cast<const v4i *>(a.wk)[((size_t)(mt0 + ms) * a.ksteps + q) * 64 + lane];
        } else {
            const int blk = 2 * q + kh;                // 16-channel block of this lane half
            if (blk * 16 >= a.c) return z;
            const int g = blk >> a.cb_sh, u = blk & ((1 << a.cb_sh) - 1);
            const size_t mt16 = (size_t)(mt0 + ms) * 2 + (lj >> 4);
            return *reinterpret_cast<const v4i *>(a.wk + (mt16 * a.ksteps + g) * 1024 + u * 256 + (lj & 15) * 16);
        }
    };
    v16i acc[MS][NS];
#pragma unroll
    for (int ms = 0; ms < MS; ++ms)
#pragma unroll
        for (int ns = 0; ns < NS; ++ns)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[ms][ns][e] = 0;
    int sx[NS] = {};
    v4i an[MS];
    if (live) {
#pragma unroll
        for (int ms = 0; ms < MS; ++ms) an[ms] = load_a(0, ms);
    }
    const int ones = (GEN && kh) ? 0 : 0x01010101;     // generic plane: lane half 1 repeats half 0's channels against zero weights
    auto gemm = [&](int ch, int tb) {
        const char *Tb = T + (size_t)tb * SEP_TBYTES + (size_t)lj * SEP_TPITCH;
#pragma unroll
        for (int j = 0; j < SPC; ++j) {
            const int q = ch * SPC + j;
            if (q < nst) {
                v4i af[MS];
#pragma unroll
                for (int ms = 0; ms < MS; ++ms) af[ms] = an[ms];
                if (q + 1 < nst) {
#pragma unroll
                    for (int ms = 0; ms < MS; ++ms) an[ms] = load_a(q + 1, ms);
                }
                const int boff = 16 * (GEN ? j : 2 * j + kh);
                v4i bf[NS];
#pragma unroll
                for (int ns = 0; ns < NS; ++ns) {
                    bf[ns] = *reinterpret_cast<const v4i *>(Tb + (size_t)ns * 32 * SEP_TPITCH + boff);
                    int t = sx[ns];
#pragma unroll
                    for (int i = 0; i < 4; ++i) t = __builtin_amdgcn_sdot4(bf[ns][i], ones, t, false);
                    sx[ns] = t;
                }
#pragma unroll
                for (int ms = 0; ms < MS; ++ms)
#pragma unroll
                    for (int ns = 0; ns < NS; ++ns) acc[ms][ns] = __builtin_amdgcn_mfma_i32_32x32x32_i8(af[ms], bf[ns], acc[ms][ns], 0, 0, 0);
            }
        }
    };

    // ---- the chunk pipeline
    const int pb2 = a.pbufs == 2;
    stage(0, 0);
    __syncthreads();
    dw(0, 0, 0);
    if (nch > 1) {
        if (!pb2) __syncthreads();
        stage(1, pb2 ? 1 : 0);
    }
#pragma unroll 1
    for (int ch = 0; ch < nch; ++ch) {
        __syncthreads();  // T[ch & 1] is whole, chunk ch + 1's patch is staged, and T[(ch + 1) & 1] / the other patch buffer are read
        if (live) gemm(ch, ch & 1);
        if (ch + 1 < nch) {
            dw(ch + 1, pb2 ? ((ch + 1) & 1) : 0, (ch + 1) & 1);
            if (ch + 2 < nch) {
                if (!pb2) __syncthreads();
                stage(ch + 2, pb2 ? (ch & 1) : 0);
            }
        }
    }
    if (!live) return;

    // ---- pw epilogue: corrections, requantise (FP64 in the reference's order), stores.  Lane (lj, kh) holds pixel 32 ns + lj and
    //      accumulator rows 8 grp + 4 kh + r (the 32 x 32 MFMA's D layout); pixel p of the tile is output j = p % 8 of run p / 8
    const bool pow2 = a.hdr->pow2 == 1;
    const int OW1 = a.OW + 1, ohw = a.OH * a.OW;
#pragma unroll
    for (int ns = 0; ns < NS; ++ns) {
        const int sxt = sx[ns] + __shfl_xor(sx[ns], 32);
        const int p = ns * 32 + lj, prun = p >> 3;
        const int oy = oy0 + (prun & (RY - 1)), ox = ox0 + (prun >> a.ry_sh) * RUN + (p & 7);
        if (oy >= a.OH || ox >= a.OW) continue;
        const size_t pix = (size_t)oy * a.OW + ox;
        uint8_t *ycell = a.y ? a.y + ((size_t)a.out_lead + ((size_t)b * (a.OH + 1) + oy + 1) * OW1 + ox) * a.out_cs : nullptr;
#pragma unroll
        for (int ms = 0; ms < MS; ++ms)
#pragma unroll
            for (int grp = 0; grp < 4; ++grp) {
                const int row0 = (mt0 + ms) * 32 + 8 * grp + 4 * kh;
                if (row0 >= a.n) continue;
                uint32_t bytes[4] = {0, 0, 0, 0};
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int oc = row0 + r;
                    if (oc >= a.n) break;
                    const uint32_t acct = (uint32_t)acc[ms][ns][grp * 4 + r] + (uint32_t)a.dzp[oc] * (uint32_t)sxt + (uint32_t)a.cw[oc];
                    uint32_t u8;
                    if (pow2) u8 = sep_finish(requant_q_exact((int32_t)(acct + (uint32_t)a.bias[oc]), a.mprime[oc]), a.zp_act, a.act, a.store_mode);
                    else u8 = requant_u8((int32_t)acct, a.bias[oc], a.mval[oc], a.sval[oc], a.zp_act, a.act, a.store_mode);
                    bytes[r] = u8;
                    const size_t ridx = ((size_t)b * a.n + oc) * ohw + pix;
                    if (a.acc_out) a.acc_out[ridx] = (int32_t)acct;
                    if (a.y_f32) a.y_f32[ridx] = (float)((int)u8 - a.zp_act) * a.s_act;
                }
                if (ycell) {
                    uint8_t *dst = ycell + row0;
                    if (row0 + 3 < a.n) {
                        *reinterpret_cast<uint32_t *>(dst) = (bytes[0] | bytes[1] << 8 | bytes[2] << 16 | bytes[3] << 24) ^ 0x80808080u;
                    } else {
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            if (row0 + r < a.n) dst[r] = (uint8_t)(bytes[r] ^ 0x80u);
                    }
                }
            }
    }
}

// dynamic LDS above the 64 KiB default: raised per instantiation and device, only when a launch needs more (as dw_launch_one)
template <void (*kern)(const SepArgs)>
int sep_launch_one(const SepArgs &a, int grid, size_t lds, hipStream_t st)
{
    if (lds > 64 * 1024) {
        static size_t have[64] = {0};
        static std::mutex mu;
        int dev = 0;
        (void)hipGetDevice(&dev);
        std::lock_guard<std::mutex> lk(mu);
        size_t &h = have[dev & 63];
        if (lds > h) {
            if (hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
                return MI355_EHIP;
            h = lds;
        }
    }
    conv_launch_note(grid, SEP_THREADS, lds);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(SEP_THREADS), lds, st, a);
    return hipGetLastError() == hipSuccess ? MI355_OK : MI355_EHIP;
}

template <int KS, int S>
int sep_dispatch(const SepArgs &a, int ms, int grid, size_t lds, hipStream_t st)
{
    if (a.gen) return ms == 1 ? sep_launch_one<conv_sep_kernel<KS, S, true, 1>>(a, grid, lds, st)
                              : sep_launch_one<conv_sep_kernel<KS, S, true, 2>>(a, grid, lds, st);
    return ms == 1 ? sep_launch_one<conv_sep_kernel<KS, S, false, 1>>(a, grid, lds, st)
                   : sep_launch_one<conv_sep_kernel<KS, S, false, 2>>(a, grid, lds, st);
}

}  // namespace

// MI355_EINVAL when no tile fits LDS or the grid does not fit (nothing launched)
int conv_sep_launch(SepArgs &a, hipStream_t st)
{
    const int k = a.ksize, s = a.stride;
    const bool fixed = (k == 3 || k == 5) && (s == 1 || s == 2);
    a.nchunks = (a.c + 63) / 64;
    a.pieces16 = (a.c + 15) / 16;
    // a wave's slab is 32 filters up to 128 filters (every wave has work from n = 97 on), 64 above: filter blocks of 128 | 256
    const int ms = a.n <= SEP_FILTERS_MS1 ? 1 : 2;
    a.fblocks = (a.n + 128 * ms - 1) / (128 * ms);
    // conv_dw_launch's rule -- the tile with the fewest workgroups, under the throughput plan first within half a CU's LDS -- on this
    // kernel's LDS: two intermediate tiles and two patch buffers, one where two do not fit (or the layer is a single chunk)
    // (the 64-filter slab takes 288 registers, one wave a SIMD: a second workgroup never fits, so it keeps both patch buffers)
    const size_t limits[2] = {a.plan == MI355_PLAN_THROUGHPUT && ms == 1 ? SEP_LDS_SHARED : SEP_LDS_MAX, SEP_LDS_MAX};
    for (size_t limit : limits) {
        long best_tiles = 0;
        size_t best_lds = 0;
        for (int sh = 4; sh >= 2; --sh) {
            const int th = 1 << sh, tw = (16 >> sh) * DW_RUN;
            const long ph = (long)(th - 1) * s + k, pw = (long)(tw - 1) * s + k, pitch = pw | 1;
            const size_t pbytes = (size_t)(ph * pitch) * 64 + (fixed ? 0 : (size_t)k * k * 128);
            int pbufs = a.nchunks > 1 ? 2 : 1;
            if (2 * SEP_TBYTES + pbufs * pbytes > limit) pbufs = 1;
            const size_t lds = 2 * SEP_TBYTES + pbufs * pbytes;
            if (lds > limit) continue;
            const long tiles = (long)((a.OH + th - 1) / th) * ((a.OW + tw - 1) / tw);
            if (best_tiles && (tiles > best_tiles || (tiles == best_tiles && lds >= best_lds))) continue;
            best_tiles = tiles; best_lds = lds;
            a.ry_sh = sh; a.ph = (int)ph; a.pw = (int)pw; a.pitch = (int)pitch;
            a.pbytes = (int)pbytes; a.pbufs = pbufs;
            a.tiles_x = (a.OW + tw - 1) / tw; a.tiles_y = (a.OH + th - 1) / th;
        }
        if (!best_tiles) continue;
        a.fd_pw = fastdiv_make((uint32_t)a.pw);
        const long grid = best_tiles * a.B * a.fblocks;
        if (grid > 0x7FFFFFFF) return MI355_EINVAL;
        if (!fixed) return sep_dispatch<0, 0>(a, ms, (int)grid, best_lds, st);
        if (k == 3) return s == 1 ? sep_dispatch<3, 1>(a, ms, (int)grid, best_lds, st) : sep_dispatch<3, 2>(a, ms, (int)grid, best_lds, st);
        return s == 1 ? sep_dispatch<5, 1>(a, ms, (int)grid, best_lds, st) : sep_dispatch<5, 2>(a, ms, (int)grid, best_lds, st);
    }
    return MI355_EINVAL;
}
