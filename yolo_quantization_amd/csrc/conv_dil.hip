// conv_dil.hip -- the dilated (atrous) convolution: [convolutional] dilation=d, stride 1, any size 2..11, padding and channel count
// (DESIGN.md 7f).  With D = d (k - 1) + 1 and OH = H + 2 pad - D + 1:
//        acc[j][oy][ox] = sum_{ci, ky, kx} (w_u8[j][ci][ky][kx] - zp_w[j]) x_u8[ci][oy - pad + ky d][ox - pad + kx d]
// in exact int32 arithmetic, out-of-image taps the input zero point.
//
// Phases.  The taps of output (oy, ox) are d cells apart, so the outputs of one phase (qy, qx) = (oy % d, ox % d) read one
// d-subsampled copy of the input, and on it the layer is the DENSE k x k convolution: with (jy, jx) = (oy / d, ox / d), tap (ky, kx)
// is cell (jy + ky, jx + kx) of the grid of input cells (qy - pad + d r, qx - pad + d cc).  (In the words of space-to-batch: with
// qy - pad = ry + d ey, 0 <= ry < d, that is row jy + ey + ky of input phase image ry.)  Nothing is permuted in memory: the
// permutation is folded into the addresses of the staging loads and of the stores.
//
// Work split.  conv_dil_kernel is an implicit GEMM on V_MFMA_I32_32X32X32_I8: M = filters, N = 256 (or 64) output pixels, K =
// (channel chunk, tap, channel), the A fragments and the K order those of conv_kxk.hip (mi355_conv_pack's general-kernel
// fragments, read from global memory one K-step ahead).  A phase image is only ceil(OH / d) x ceil(OW / d) pixels, so the N
// pixels of a workgroup are G = N / (th tw) PHASE TILES of th x tw phase indices, consecutive entries of the image's list
// [phase (qy, qx)][tile (ty, tx)].  Per channel chunk the workgroup stages G patches of (th + k - 1) x (tw + k - 1) cells of `unit`
// bytes, gathered at cell stride d, out-of-image cells (and every cell of a slot past the list) the biased input zero point
// zp_in ^ 0x80; the pad ring is never read.  A lane's column origin is slot patch_cells + jy (tw + k - 1) + jx and every tap is
// the dense constant offset ky (tw + k - 1) + kx: the K loop is the dense layer's, on a patch of the dense layer's size, whatever d.
//
// Zero points: conv_kxk.hip's algebra over the true K = c k k,
//        sum_k (w_u8 - zp_w) x_u8 = sum_k w'x'  +  dz sum_k x'  +  [128 sum_k w' + 128 K dz]       w' = w - 128, x' = x - 128, dz = 128 - zp_w
// with sum_k x' from a V_DOT4 of every B fragment against a 0/1 byte mask of its true channels and taps.
#include "kargs.h"
#include <mutex>

namespace {

constexpr int DIL_THREADS = 256;
constexpr int DIL_MAX_SLOTS = 128;  // tap slots per chunk: 11 x 11 taps rounded up to whole K-steps, as conv_kxk.hip
constexpr size_t DIL_LDS_MAX = 160 * 1024;

__device__ __forceinline__ uint32_t dil_finish(int32_t q, int zp_act, int act, int store_mode)
{
    // requant_u8's second half (common.h): activation, zero point, store mode, uint8 wrap
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

// byte mask of the first `nb` bytes of a dword (nb clamped to 0..4), one 0x01 per valid byte
__device__ __forceinline__ int dil_ones_mask(int nb)
{
    nb = min(max(nb, 0), 4);
    return (int)(0x01010101u & (nb == 4 ? 0xFFFFFFFFu : ((1u << (8 * nb)) - 1u)));
}

// entry `tile` of an image's list of phase tiles: its phase (qy, qx) and first phase index (jy0, jx0)
struct DilTile { int qy, qx, jy0, jx0; };
__device__ __forceinline__ DilTile dil_tile(const DilArgs &a, int tile)
{
    const int phs = fd_div(tile, a.fd_tpp), r = tile - phs * a.tpp;
    const int ty = fd_div(r, a.fd_tx), tx = r - ty * a.tiles_x;
    DilTile t;
    t.qy = fd_div(phs, a.fd_nqx);
    t.qx = phs - t.qy * a.nqx;
    t.jy0 = ty << a.th_sh;
    t.jx0 = tx << a.tw_sh;
    return t;
}

// U: unit bytes per tap (4, 8, 16); MS: 32-row M sub-tiles per wave; WM: waves along M (4 / WM along N, 64 pixels each)
template <int U, int MS, int WM>
__global__ __launch_bounds__(DIL_THREADS) void conv_dil_kernel(const DilArgs a)
{
    constexpr int WN = 4 / WM, NS = 2, TPL = 16 / U;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int *tapoff = reinterpret_cast<int *>(smem);           // [DIL_MAX_SLOTS] cell offset of tap slot t in a patch
    char *P = smem + DIL_MAX_SLOTS * sizeof(int);          // [slots][ph][pw] cells of U bytes

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int kh = lane >> 5, lj = lane & 31;
    const int k = a.ksize, kk = k * k, d = a.dil, pw = a.pw;
    const int pc = a.ph * pw;                 // cells of one patch
    const int tsh = a.th_sh + a.tw_sh;        // a phase tile is 2^tsh pixels
    const int TW = 1 << a.tw_sh;

    const int mg = blockIdx.x % a.mgroups;
    const int nt = blockIdx.x / a.mgroups;
    const int b = nt / a.wpi;
    const int tile0 = (nt - b * a.wpi) * a.slots;  // first entry of the image's tile list this workgroup owns

    for (int t = tid; t < DIL_MAX_SLOTS; t += DIL_THREADS) tapoff[t] = t < kk ? (t / k) * pw + (t % k) : 0;

    // window origin (patch cell of tap (0, 0)) of this lane's columns
    int cbase[NS];
#pragma unroll
    for (int ns = 0; ns < NS; ++ns) {
        const int p = wn * 64 + ns * 32 + lj, q = p & ((1 << tsh) - 1);
        cbase[ns] = (p >> tsh) * pc + (q >> a.tw_sh) * pw + (q & (TW - 1));
    }
    const int mt0 = (mg * WM + wm) * MS;  // first 32-row M tile of this wave
    const v4i *wk = reinterpret_cast<const v4i *>(a.wk);
    const int W1 = a.W + 1;
    const uint32_t fill = (uint32_t)((a.zp_in ^ 0x80) & 0xFF) * 0x01010101u;
    const int ncells = a.slots * pc;

    v16i acc[MS][NS];
#pragma unroll
    for (int ms = 0; ms < MS; ++ms)
#pragma unroll
        for (int ns = 0; ns < NS; ++ns)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[ms][ns][e] = 0;
    int sx[NS] = {};

    v4i an[MS];
#pragma unroll
    for (int ms = 0; ms < MS; ++ms) an[ms] = wk[((size_t)(mt0 + ms) * a.ksteps) * 64 + lane];

#pragma unroll 1
    for (int ch = 0; ch < a.nchunks; ++ch) {
        __syncthreads();  // the previous chunk's fragments are read (and, first time round, the tap table is written)
        // ---- stage the chunk's patches: cell (r, cc) of a slot's patch is input (qy - pad + d (jy0 + r), qx - pad + d (jx0 + cc))
        const size_t coff = (size_t)ch * U;
        for (int i = tid; i < ncells; i += DIL_THREADS) {
            const int sl = fd_div(i, a.fd_pc), rem = i - sl * pc;
            const int r = fd_div(rem, a.fd_pw), cc = rem - r * pw;
            bool in = false;
            size_t src = 0;
            if (tile0 + sl < a.ntiles) {
                const DilTile t = dil_tile(a, tile0 + sl);
                const int iy = t.qy - a.pad + d * (t.jy0 + r), ix = t.qx - a.pad + d * (t.jx0 + cc);
                in = iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
                src = ((size_t)a.in_lead + ((size_t)b * (a.H + 1) + iy + 1) * W1 + ix) * a.in_cs + coff;
            }
            if constexpr (U == 16) {
                uint4 v = make_uint4(fill, fill, fill, fill);
                if (in) v = *reinterpret_cast<const uint4 *>(a.x + src);
                *reinterpret_cast<uint4 *>(P + (size_t)i * 16) = v;
            } else if constexpr (U == 8) {
                uint2 v = make_uint2(fill, fill);
                if (in) v = *reinterpret_cast<const uint2 *>(a.x + src);
                *reinterpret_cast<uint2 *>(P + (size_t)i * 8) = v;
            } else {
                uint32_t v = fill;
                if (in) v = *reinterpret_cast<const uint32_t *>(a.x + src);
                *reinterpret_cast<uint32_t *>(P + (size_t)i * 4) = v;
            }
        }
        __syncthreads();
        // channel mask of each fragment dword (valid channels of this chunk)
        const int cvalid = min(U, a.c - ch * U);
        int cm[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) cm[i] = dil_ones_mask(cvalid - (U == 16 ? 4 * i : (U == 8 ? 4 * (i & 1) : 0)));

#pragma unroll 1
        for (int st = 0; st < a.spc; ++st) {
            const int g = ch * a.spc + st;
            v4i af[MS];
#pragma unroll
            for (int ms = 0; ms < MS; ++ms) af[ms] = an[ms];
            if (g + 1 < a.ksteps) {
#pragma unroll
                for (int ms = 0; ms < MS; ++ms) an[ms] = wk[((size_t)(mt0 + ms) * a.ksteps + g + 1) * 64 + lane];
            }
            const int t0 = (2 * st + kh) * TPL;  // first tap slot of this lane half
            int toff[TPL], msk[4];
#pragma unroll
            for (int j = 0; j < TPL; ++j) toff[j] = tapoff[t0 + j];
#pragma unroll
            for (int i = 0; i < 4; ++i) msk[i] = (t0 + i / (4 / TPL) < kk) ? cm[i] : 0;
            v4i bf[NS];
#pragma unroll
            for (int ns = 0; ns < NS; ++ns) {
                if constexpr (U == 16) {
                    bf[ns] = *reinterpret_cast<const v4i *>(P + (size_t)(cbase[ns] + toff[0]) * 16);
                } else if constexpr (U == 8) {
                    const int2 lo = *reinterpret_cast<const int2 *>(P + (size_t)(cbase[ns] + toff[0]) * 8);
                    const int2 hi = *reinterpret_cast<const int2 *>(P + (size_t)(cbase[ns] + toff[1]) * 8);
                    bf[ns][0] = lo.x; bf[ns][1] = lo.y; bf[ns][2] = hi.x; bf[ns][3] = hi.y;
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) bf[ns][j] = *reinterpret_cast<const int *>(P + (size_t)(cbase[ns] + toff[j]) * 4);
                }
                int t = sx[ns];
#pragma unroll
                for (int i = 0; i < 4; ++i) t = __builtin_amdgcn_sdot4(bf[ns][i], msk[i], t, false);
                sx[ns] = t;
            }
#pragma unroll
            for (int ms = 0; ms < MS; ++ms)
#pragma unroll
                for (int ns = 0; ns < NS; ++ns) acc[ms][ns] = __builtin_amdgcn_mfma_i32_32x32x32_i8(af[ms], bf[ns], acc[ms][ns], 0, 0, 0);
        }
    }

    // ---- epilogue: corrections, requantise (FP64 in the reference's order), scattered stores.  Lane (lj, kh) holds column lj and
    //      accumulator rows 8 grp + 4 kh + r (the 32 x 32 MFMA's D layout)
    const bool pow2 = a.hdr->pow2 == 1;
    const int OW1 = a.OW + 1, ohw = a.OH * a.OW;
#pragma unroll
    for (int ns = 0; ns < NS; ++ns) {
        const int sxt = sx[ns] + __shfl_xor(sx[ns], 32);  // the two lane halves hold the two halves of every K-step
        const int p = wn * 64 + ns * 32 + lj, q = p & ((1 << tsh) - 1);
        const int tile = tile0 + (p >> tsh);
        if (tile >= a.ntiles) continue;  // a slot past the list computed on fill
        const DilTile t = dil_tile(a, tile);
        const int oy = t.qy + d * (t.jy0 + (q >> a.tw_sh)), ox = t.qx + d * (t.jx0 + (q & (TW - 1)));
        if (oy >= a.OH || ox >= a.OW) continue;  // past the phase's own extent
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
                    if (pow2) u8 = dil_finish(requant_q_exact((int32_t)(acct + (uint32_t)a.bias[oc]), a.mprime[oc]), a.zp_act, a.act, a.store_mode);
                    else u8 = requant_u8((int32_t)acct, a.bias[oc], a.mval[oc], a.sval[oc], a.zp_act, a.act, a.store_mode);
                    bytes[r] = u8;
                    const size_t ridx = ((size_t)b * a.n + oc) * ohw + pix;
                    if (a.acc_out) a.acc_out[ridx] = (int32_t)acct;
                    if (a.y_f32) a.y_f32[ridx] = (float)((int)u8 - a.zp_act) * a.s_act;
                }
                if (ycell) {
                    uint8_t *dst = ycell + row0;
                    if (row0 + 3 < a.n && ((uintptr_t)dst & 3) == 0) {
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

// dynamic LDS above the 64 KiB default: raised per instantiation and device, only when a launch needs more (kargs.h lds_limit_for)
template <void (*kern)(const DilArgs)>
int dil_launch_one(const DilArgs &a, int grid, size_t lds, hipStream_t st)
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
    conv_launch_note(grid, DIL_THREADS, lds);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(DIL_THREADS), lds, st, a);
    return hipGetLastError() == hipSuccess ? MI355_OK : MI355_EHIP;
}

template <int U>
int dil_dispatch(const DilArgs &a, int ms, int wm, int grid, size_t lds, hipStream_t st)
{
    if (wm == 4) return dil_launch_one<conv_dil_kernel<U, 1, 4>>(a, grid, lds, st);
    if (ms == 2) return dil_launch_one<conv_dil_kernel<U, 2, 1>>(a, grid, lds, st);
    return dil_launch_one<conv_dil_kernel<U, 1, 1>>(a, grid, lds, st);
}

int p2_shift(long v)  // log2 of the next power of two >= v
{
    int s = 0;
    while ((1L << s) < v) ++s;
    return s;
}

}  // namespace

// MI355_EINVAL when no tile fits (nothing launched)
int conv_dil_launch(DilArgs &a, hipStream_t st)
{
    const int U = a.unit, k = a.ksize, d = a.dil;
    if (k < 2 || k > 11 || d < 1 || a.OH < 1 || a.OW < 1) return MI355_EINVAL;
    if ((U != 4 && U != 8 && U != 16) || a.spc * 2 * (16 / U) > DIL_MAX_SLOTS) return MI355_EINVAL;
    if (a.in_cs % 16 || ((uintptr_t)a.x & 15)) return MI355_EINVAL;
    const int PH = (a.OH + d - 1) / d, PW = (a.OW + d - 1) / d;  // the largest phase image
    const int nqy = d < a.OH ? d : a.OH;
    a.nqx = d < a.OW ? d : a.OW;
    // 32 (n <= 32) or 64 filters x 256 pixels; when those patches do not fit in LDS, 128 filters x 64 pixels
    struct Cfg { int ms, wm; };
    const Cfg cfgs[2] = {{a.n <= 32 ? 1 : 2, 1}, {1, 4}};
    for (const Cfg &c : cfgs) {
        const int npx_sh = c.wm == 1 ? 8 : 6;
        a.tw_sh = p2_shift(PW) < 5 ? p2_shift(PW) : 5;
        a.th_sh = p2_shift(PH) < npx_sh - a.tw_sh ? p2_shift(PH) : npx_sh - a.tw_sh;
        a.slots = 1 << (npx_sh - a.th_sh - a.tw_sh);
        a.ph = (1 << a.th_sh) + k - 1; a.pw = (1 << a.tw_sh) + k - 1;
        const size_t lds = DIL_MAX_SLOTS * sizeof(int) + (size_t)a.slots * a.ph * a.pw * U;
        if (lds > DIL_LDS_MAX) continue;
        a.tiles_x = (PW + (1 << a.tw_sh) - 1) >> a.tw_sh;
        a.tpp = a.tiles_x * ((PH + (1 << a.th_sh) - 1) >> a.th_sh);
        const long ntiles = (long)nqy * a.nqx * a.tpp;
        const int mrows = 32 * c.ms * c.wm;
        a.mgroups = (a.n + mrows - 1) / mrows;
        const long wpi = (ntiles + a.slots - 1) / a.slots;
        const long grid = (long)a.mgroups * a.B * wpi;
        if (ntiles > 0x3FFFFFFF || grid > 0x7FFFFFFF) return MI355_EINVAL;
        a.ntiles = (int)ntiles; a.wpi = (int)wpi;
        a.fd_pc = fastdiv_make((uint32_t)(a.ph * a.pw)); a.fd_pw = fastdiv_make((uint32_t)a.pw);
        a.fd_tpp = fastdiv_make((uint32_t)a.tpp); a.fd_tx = fastdiv_make((uint32_t)a.tiles_x); a.fd_nqx = fastdiv_make((uint32_t)a.nqx);
        switch (U) {
        case 4: return dil_dispatch<4>(a, c.ms, c.wm, (int)grid, lds, st);
        case 8: return dil_dispatch<8>(a, c.ms, c.wm, (int)grid, lds, st);
        default: return dil_dispatch<16>(a, c.ms, c.wm, (int)grid, lds, st);
        }
    }
    return MI355_EINVAL;
}

