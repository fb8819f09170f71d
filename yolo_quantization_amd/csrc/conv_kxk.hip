// conv_kxk.hip -- convolutions of any size (1..11), stride, padding and channel count: the shapes the specialised kernels
// (conv_igemm / conv_ws3 / conv_small* / conv1x1 / conv_first*) do not serve.  Two kernels:
//
//  * conv_kxk_kernel: implicit GEMM on V_MFMA_I32_32X32X32_I8.  M = filters, N = output pixels of a TH x TW patch of one image,
//    K = (channel chunk, tap, channel).  Same result as the reference's im2col + GEMM (ref src/convolutional_layer.c:694-761,
//    src/im2col.c:26-50) in exact int32 arithmetic, with the zero-point algebra of conv_igemm.hip:
//        sum_k (w_u8 - zp_w) x_u8 = sum_k w'x'  +  d * sum_k x'  +  [128 sum_k w' + 128 K d]        w' = w - 128, x' = x - 128, d = 128 - zp_w
//    where the sums run over the layer's true K = c k k only.  Padding channels (>= c inside a cell) and padding taps (K-step tail)
//    carry weight 0 and are masked out of the receptive-field sum sum_k x' (V_DOT4 against a 0/1 byte mask).
//  * conv_ref_f32_general_kernel: the Makefile-default reference accumulation (fp32 adds, pass 1 with the weights, pass 2 with
//    -zp_w; ref src/gemm.c:279-299) for the same shapes: conv_aux.hip's conv_ref_f32_kernel with its own output map and stride.
//
// Halo rule.  The activation layout's one-cell pad ring covers a 3 x 3 window only, so the kernel never reads the ring: every tap
// (iy, ix) = (oy s + ky - pad, ox s + kx - pad) outside the image is the biased input zero point zp_in ^ 0x80 (im2col_get_pixel,
// ref src/im2col.c:10-11).  Per channel chunk a workgroup stages ((TH - 1) s + k) x ((TW - 1) s + k) cells of `unit` bytes in LDS,
// out-of-image cells filled with that value, and every tap is then a constant cell offset from a column's window origin.
//
// Dense K for few channels.  unit = channel bytes per tap: 4 (c <= 4: the RGB image's 4-byte cells, one zero-weight pad byte),
// 8 (c <= 8) or 16.  A lane's 16-byte fragment holds 16 / unit taps, a K-step (two lane halves) 32 / unit: the 7 x 7 stem on the
// image is 7 K-steps (K = 224) instead of 25 with a tap per 16 channels.  The packed weights are A fragments in lane order,
// [mpad / 32][ksteps][64 lanes][16 B] (shim.hip mi355_conv_pack), read straight from global memory one K-step ahead.
#include "kargs.h"
#include <mutex>

namespace {

constexpr int KXK_THREADS = 256;
constexpr int KXK_MAX_SLOTS = 128;  // tap slots per chunk: 11 x 11 taps rounded up to whole K-steps (unit 4: 16 x 8, unit 16: 61 x 2)

__device__ __forceinline__ uint32_t kxk_finish(int32_t q, int zp_act, int act, int store_mode)
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
__device__ __forceinline__ int ones_mask(int nb)
{
    nb = min(max(nb, 0), 4);
    return (int)(0x01010101u & (nb == 4 ? 0xFFFFFFFFu : ((1u << (8 * nb)) - 1u)));
}

// U: unit bytes per tap (4, 8, 16); MS: 32-row M sub-tiles per wave; WM: waves along M (4 / WM along N, 64 pixels each)
template <int U, int MS, int WM>
__global__ __launch_bounds__(KXK_THREADS) void conv_kxk_kernel(const KxkArgs a)
{
    constexpr int WN = 4 / WM, NS = 2, TPL = 16 / U;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int *tapoff = reinterpret_cast<int *>(smem);           // [KXK_MAX_SLOTS] cell offset of tap slot t in the patch
    char *P = smem + KXK_MAX_SLOTS * sizeof(int);          // [ph][pw] cells of U bytes

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int kh = lane >> 5, lj = lane & 31;
    const int k = a.ksize, kk = k * k, s = a.stride, pw = a.pw, ph = a.ph;
    const int TW = 1 << a.tw_sh, TH = (WN * 64) >> a.tw_sh;

    const int mg = blockIdx.x % a.mgroups;
    int nt = blockIdx.x / a.mgroups;
    const int tpi = a.tiles_x * a.tiles_y;
    const int b = nt / tpi;
    nt -= b * tpi;
    const int ty = nt / a.tiles_x, tx = nt - ty * a.tiles_x;
    const int oy0 = ty * TH, ox0 = tx * TW;
    const int iy0 = oy0 * s - a.pad, ix0 = ox0 * s - a.pad;

    for (int t = tid; t < KXK_MAX_SLOTS; t += KXK_THREADS) tapoff[t] = t < kk ? (t / k) * pw + (t % k) : 0;

    // window origin (patch cell of tap (0, 0)) of this lane's columns
    int cbase[NS];
#pragma unroll
    for (int ns = 0; ns < NS; ++ns) {
        const int p = wn * 64 + ns * 32 + lj;
        cbase[ns] = (p >> a.tw_sh) * s * pw + (p & (TW - 1)) * s;
    }
    const int mt0 = (mg * WM + wm) * MS;  // first 32-row M tile of this wave
    const v4i *wk = reinterpret_cast<const v4i *>(a.wk);
    const int W1 = a.W + 1;
    const uint32_t fill = (uint32_t)((a.zp_in ^ 0x80) & 0xFF) * 0x01010101u;
    const bool plain = a.in_cs == 4;  // the image's cells hold plain bytes: flipped into the biased domain when staged
    const int ncells = ph * pw;

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
        // ---- stage the chunk's patch: in-image cells from the tensor, the rest the biased input zero point
        const size_t coff = (size_t)ch * U;
        for (int i = tid; i < ncells; i += KXK_THREADS) {
            const int r = i / pw, cc = i - r * pw;
            const int iy = iy0 + r, ix = ix0 + cc;
            const bool in = iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
            const size_t src = (size_t)(a.in_lead + (b * (a.H + 1) + iy + 1) * W1 + ix) * a.in_cs + coff;
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
                if (in) v = *reinterpret_cast<const uint32_t *>(a.x + src) ^ (plain ? 0x80808080u : 0u);
                *reinterpret_cast<uint32_t *>(P + (size_t)i * 4) = v;
            }
        }
        __syncthreads();
        // channel mask of each fragment dword (valid channels of this chunk)
        const int cvalid = min(U, a.c - ch * U);
        int cm[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) cm[i] = ones_mask(cvalid - (U == 16 ? 4 * i : (U == 8 ? 4 * (i & 1) : 0)));

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

    // ---- epilogue: corrections, requantise (FP64 in the reference's order), stores.  Lane (lj, kh) holds column lj and
    //      accumulator rows 8 grp + 4 kh + r (the 32 x 32 MFMA's D layout)
    const bool pow2 = a.hdr->pow2 == 1;
    const int OW1 = a.OW + 1, ohw = a.OH * a.OW;
#pragma unroll
    for (int ns = 0; ns < NS; ++ns) {
        const int sxt = sx[ns] + __shfl_xor(sx[ns], 32);  // the two lane halves hold the two halves of every K-step
        const int p = wn * 64 + ns * 32 + lj;
        const int oy = oy0 + (p >> a.tw_sh), ox = ox0 + (p & (TW - 1));
        if (oy >= a.OH || ox >= a.OW) continue;
        const size_t pix = (size_t)oy * a.OW + ox;
        uint8_t *ycell = a.y ? a.y + (size_t)(a.out_lead + (b * (a.OH + 1) + oy + 1) * OW1 + ox) * a.out_cs : nullptr;
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
                    if (pow2) u8 = kxk_finish(requant_q_exact((int32_t)(acct + (uint32_t)a.bias[oc]), a.mprime[oc]), a.zp_act, a.act, a.store_mode);
                    else u8 = requant_u8((int32_t)acct, a.bias[oc], a.mval[oc], a.sval[oc], a.zp_act, a.act, a.store_mode);
                    bytes[r] = u8;
                    const size_t ridx = ((size_t)b * a.n + oc) * ohw + pix;
                    if (a.acc_out) a.acc_out[ridx] = (int32_t)acct;
                    if (a.y_f32) a.y_f32[ridx] = (float)((int)u8 - a.zp_act) * a.s_act;
                }
                if (ycell) {
                    const uint32_t flip = a.out_cs == 4 ? 0u : 0x80u;  // a 3-filter layer's 4-byte cells hold plain bytes like the image's
                    uint8_t *dst = ycell + row0;
                    if (row0 + 3 < a.n && ((uintptr_t)dst & 3) == 0) {
                        *reinterpret_cast<uint32_t *>(dst) = (bytes[0] | bytes[1] << 8 | bytes[2] << 16 | bytes[3] << 24) ^ (flip * 0x01010101u);
                    } else {
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            if (row0 + r < a.n) dst[r] = (uint8_t)(bytes[r] ^ flip);
                    }
                }
            }
    }
}

// One thread per output element, pixel fastest.  Same accumulation order as conv_aux.hip's conv_ref_f32_kernel (k = (ci, ky, kx),
// ref src/im2col.c:33-37), with its own output map and stride.
__global__ __launch_bounds__(256) void conv_ref_f32_general_kernel(const KxkArgs a)
{
    const int ohw = a.OH * a.OW;
    const long total = (long)a.B * a.n * ohw;
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int rem = (int)(idx % ohw);
    const int oc = (int)((idx / ohw) % a.n);
    const int b = (int)(idx / ((long)ohw * a.n));
    const int oy = rem / a.OW, ox = rem - oy * a.OW;
    const int W1 = a.W + 1, k = a.ksize;
    const int K = a.c * k * k;
    const uint8_t *wrow = a.w_u8 + (size_t)oc * K;
    const float zpw = (float)a.zp_w[oc];
    const bool plain = a.in_cs == 4;
    int32_t C = 0;
    for (int pass = 0; pass < 2; ++pass) {
        int kidx = 0;
        for (int ci = 0; ci < a.c; ++ci)
            for (int ky = 0; ky < k; ++ky)
                for (int kx = 0; kx < k; ++kx, ++kidx) {
                    const int iy = oy * a.stride + ky - a.pad, ix = ox * a.stride + kx - a.pad;
                    int xv;
                    if (iy < 0 || ix < 0 || iy >= a.H || ix >= a.W) {
                        xv = a.zp_in;  // ref src/im2col.c:10-11
                    } else {
                        const size_t cell = (size_t)a.in_lead + (size_t)(b * (a.H + 1) + (iy + 1)) * W1 + ix;
                        const uint8_t raw = a.x[cell * a.in_cs + ci];
                        xv = plain ? raw : (raw ^ 0x80);
                    }
                    // ref src/gemm.c:295  C[i*ldc+j] += ALPHA*A[i*lda+k]*B[k*ldb+j]  (float ALPHA = +1 / -1)
                    const float av = pass == 0 ? (float)wrow[kidx] : -zpw;
                    const float p = av * (float)xv;
                    C = (int32_t)((float)C + p);
                }
    }
    const uint32_t u8 = requant_u8(C, a.bias[oc], a.mval[oc], a.sval[oc], a.zp_act, a.act, a.store_mode);
    const size_t ridx = ((size_t)b * a.n + oc) * ohw + rem;
    if (a.acc_out) a.acc_out[ridx] = C;
    if (a.y_f32) a.y_f32[ridx] = (float)((int)u8 - a.zp_act) * a.s_act;
    if (a.y) {
        const size_t ocell = (size_t)a.out_lead + (size_t)(b * (a.OH + 1) + (oy + 1)) * (a.OW + 1) + ox;
        a.y[ocell * a.out_cs + oc] = (uint8_t)(a.out_cs == 4 ? u8 : (u8 ^ 0x80u));
    }
}

constexpr size_t KXK_LDS_MAX = 160 * 1024;

// dynamic LDS above the 64 KiB default: raised per instantiation and device, only when a launch needs more (kargs.h lds_limit_for)
template <void (*kern)(const KxkArgs)>
int kxk_launch_one(const KxkArgs &a, int grid, size_t lds, hipStream_t st)
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
    conv_launch_note(grid, KXK_THREADS, lds);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(KXK_THREADS), lds, st, a);
    return hipGetLastError() == hipSuccess ? MI355_OK : MI355_EHIP;
}

template <int U>
int kxk_dispatch(const KxkArgs &a, int ms, int wm, int grid, size_t lds, hipStream_t st)
{
    if (wm == 4) return kxk_launch_one<conv_kxk_kernel<U, 1, 4>>(a, grid, lds, st);
    if (ms == 2) return kxk_launch_one<conv_kxk_kernel<U, 2, 1>>(a, grid, lds, st);
    return kxk_launch_one<conv_kxk_kernel<U, 1, 1>>(a, grid, lds, st);
}

}  // namespace

// MI355_EINVAL when no tile fits (nothing launched)
int conv_kxk_launch(KxkArgs &a, hipStream_t st)
{
    const int U = a.unit;
    if (a.ksize < 1 || a.ksize > 11 || a.stride < 1 || a.OH < 1 || a.OW < 1) return MI355_EINVAL;
    if ((U != 4 && U != 8 && U != 16) || a.spc * 2 * (16 / U) > KXK_MAX_SLOTS) return MI355_EINVAL;
    if (a.in_cs != 4 && a.in_cs % 16) return MI355_EINVAL;
    if (((uintptr_t)a.x & (U - 1)) || (a.in_cs == 4 && U != 4)) return MI355_EINVAL;
    // tiles: 32 (n <= 32) or 64 filters x 256 pixels; when that patch does not fit in LDS (large strides), 128 filters x 64 pixels
    struct Cfg { int ms, wm; };
    const Cfg cfgs[2] = {{a.n <= 32 ? 1 : 2, 1}, {1, 4}};
    for (const Cfg &c : cfgs) {
        const int npx = (4 / c.wm) * 64;
        const int pref = a.OW <= 8 ? 8 : (a.OW <= 16 ? 16 : 32);
        const int tws[3] = {pref, 8, 16};
        for (int tw : tws) {
            if (tw > npx) continue;
            const int th = npx / tw;
            const long ph = (long)(th - 1) * a.stride + a.ksize, pw = (long)(tw - 1) * a.stride + a.ksize;
            const size_t lds = KXK_MAX_SLOTS * sizeof(int) + (size_t)(ph * pw) * U;
            if (lds > KXK_LDS_MAX) continue;
            a.tw_sh = tw == 8 ? 3 : (tw == 16 ? 4 : 5);
            a.ph = (int)ph; a.pw = (int)pw;
            a.tiles_x = (a.OW + tw - 1) / tw; a.tiles_y = (a.OH + th - 1) / th;
            const int mrows = 32 * c.ms * c.wm;
            a.mgroups = (a.n + mrows - 1) / mrows;
            const long grid = (long)a.mgroups * a.B * a.tiles_x * a.tiles_y;
            if (grid > 0x7FFFFFFF) return MI355_EINVAL;
            switch (U) {
            case 4: return kxk_dispatch<4>(a, c.ms, c.wm, (int)grid, lds, st);
            case 8: return kxk_dispatch<8>(a, c.ms, c.wm, (int)grid, lds, st);
            default: return kxk_dispatch<16>(a, c.ms, c.wm, (int)grid, lds, st);
            }
        }
    }
    return MI355_EINVAL;
}

int conv_ref_f32_general_launch(KxkArgs &a, hipStream_t st)
{
    const int bs = 256;
    const long total = (long)a.B * a.n * a.OH * a.OW;
    const long grid = (total + bs - 1) / bs;
    conv_launch_note(grid, bs, 0);
    hipLaunchKernelGGL(conv_ref_f32_general_kernel, dim3((unsigned)grid), dim3(bs), 0, st, a);
    return hipGetLastError() == hipSuccess ? MI355_OK : MI355_EHIP;
}
