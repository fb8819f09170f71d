// conv_tr.hip -- the transposed convolution ([deconvolutional]) on V_MFMA_I32_32X32X32_I8, split into its output phases.
//
// The layer is the dense stride-1 convolution of the zero-stuffed input x^ (x[iy][ix] at (iy s, ix s), every other cell zp_in) with
// the flipped weights.  Only a fraction 1 / s^2 of that convolution's taps meet a real sample: output (oy, ox) of phase
//     (ty, tx) = ((oy + pad) mod s, (ox + pad) mod s)          at quotient (qy, qx) = ((oy + pad) / s, (ox + pad) / s)
// reads x[qy - jy][qx - jx] through w[ci][f][ty + s jy][tx + s jx], jy < ceil((k - ty) / s), jx < ceil((k - tx) / s): each phase is
// a stride-1 implicit GEMM over its own taps, about c k k / s^2 of the twin's K.  Every other tap of the twin sees zp_in and adds
//     zp_in * sum_{taps outside the phase, ci} (w - zp_w),
// an int32 per (filter, phase) that the pack precomputes (TrBlobHeader.off_sw).  A phase without any tap (k < s) is that constant
// alone and is still requantised and stored.  The phase's own taps use the zero-point algebra of conv_igemm.hip / conv_kxk.hip:
//     sum (w_u8 - zp_w) x_u8 = sum w'x' + d sum x' + [128 sum w' + 128 K_phase d]       w' = w - 128, x' = x - 128, d = 128 - zp_w.
//
// Work split.  A workgroup (four waves) owns one image, a block of filters (32 or 64 on 256 quotients, or 128 on 64 quotients) and
// a TH x TW tile of QUOTIENT space.  All s^2 phases of that tile read the same input neighbourhood: rows qy0 - halo .. qy0 + TH - 1
// with halo = ceil(k / s) - 1.  The workgroup stages it once, every channel unit (16 bytes) as a plane [ph][pw] of 16-byte cells so
// that the 32 pixels of a B fragment read consecutive cells; out-of-image cells are the biased input zero point, channels >= c are 0
// (x' = 0 leaves both sums alone), so the MAC loop has neither bounds checks nor masks and the tensor's pad ring is never read.  It
// then walks the phases over the staged patch: accumulate, requantise (common.h requant_u8), store the phase's pixels at their
// interleaved (oy, ox) = (s qy + ty - pad, s qx + tx - pad).  When the channels of the smallest tile do not fit in LDS they are
// staged in chunks of an even number of units, per phase (nchunks > 1: s^2 times the staging traffic, large c at stride 1 only).
//
// K order (kargs.h): a K-step is 32 bytes, lane half kh = one channel unit of one tap.  Unit pairs first (step = pair * taps + tap,
// half kh = unit 2 pair + kh), then an odd last unit's taps in pairs (half kh = tap 2 tp + kh; a missing second tap reads a zero
// cell against zero weights).  A phase of one tap on 32 channels is one K-step, on 16 channels half of one.
#include "kargs.h"
#include <mutex>

namespace {

constexpr int TR_THREADS = 256;
constexpr size_t TR_LDS_MAX = 160 * 1024;

// 0xFF for each of the first nb bytes of a dword (nb clamped to 0..4)
__device__ __forceinline__ uint32_t keep_bytes(int nb)
{
    nb = min(max(nb, 0), 4);
    return nb == 4 ? 0xFFFFFFFFu : ((1u << (8 * nb)) - 1u);
}

// MS: 32-row M sub-tiles per wave; WM: waves along M (4 / WM along N, 64 quotients each)
template <int MS, int WM>
__global__ __launch_bounds__(TR_THREADS) void conv_tr_kernel(const TrArgs a)
{
    constexpr int WN = 4 / WM, NS = 2;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int *tapoff = reinterpret_cast<int *>(smem);  // [TR_MAX_TAPS] cell offset of tap t of the current phase from a pixel's base cell
    char *P = smem + TR_MAX_TAPS * sizeof(int);   // [cu][ph][pw] cells of 16 bytes, then one cell of zeros

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int kh = lane >> 5, lj = lane & 31;
    const int k = a.ksize, s = a.stride, pw = a.pw, ncells = a.ph * a.pw;
    const int TW = 1 << a.tw_sh, TH = (WN * 64) >> a.tw_sh;

    const int mg = blockIdx.x % a.mgroups;
    int nt = blockIdx.x / a.mgroups;
    const int tpi = a.tiles_x * a.tiles_y;
    const int b = nt / tpi;
    nt -= b * tpi;
    const int tyi = nt / a.tiles_x, txi = nt - tyi * a.tiles_x;
    const int qy0 = tyi * TH, qx0 = txi * TW;
    const int iy0 = qy0 - a.halo, ix0 = qx0 - a.halo;  // input cell of patch cell (0, 0)

    const int zcell = a.cu * ncells;
    if (tid == 0) *reinterpret_cast<uint4 *>(P + (size_t)zcell * 16) = make_uint4(0, 0, 0, 0);

    int cbase[NS];  // patch cell of (qy, qx) shifted by the halo: tap (jy, jx) is (halo - jy) * pw + (halo - jx) cells further
#pragma unroll
    for (int ns = 0; ns < NS; ++ns) {
        const int p = wn * 64 + ns * 32 + lj;
        cbase[ns] = (p >> a.tw_sh) * pw + (p & (TW - 1));
    }
    const int mt0 = (mg * WM + wm) * MS;  // first 32-row M tile of this wave
    const int mtiles = a.mpad / 32;
    const int W1 = a.W + 1;
    const uint32_t fill = (uint32_t)((a.zp_in ^ 0x80) & 0xFF) * 0x01010101u;
    const int OW1 = a.OW + 1, ohw = a.OH * a.OW;

#pragma unroll 1
    for (int phs = 0; phs < s * s; ++phs) {
        const int ty = phs / s, tx = phs - ty * s;
        const int jxn = tr_taps(k, s, tx), taps = tr_taps(k, s, ty) * jxn;
        const int G = tr_steps(a.nu, taps);
        __syncthreads();  // the previous phase has read its tap table (and, restaging, its patch)
        for (int t = tid; t < taps; t += TR_THREADS) tapoff[t] = (a.halo - t / jxn) * pw + (a.halo - t % jxn);

        v16i acc[MS][NS];
#pragma unroll
        for (int ms = 0; ms < MS; ++ms)
#pragma unroll
            for (int ns = 0; ns < NS; ++ns)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[ms][ns][e] = 0;
        int sx[NS] = {};

        // the phase's A fragments of this wave's M tiles, read straight from global memory one K-step ahead
        const v4i *wp = reinterpret_cast<const v4i *>(a.wk) + ((size_t)a.hdr->step0[phs] * mtiles + (size_t)mt0 * G) * 64 + lane;
        int g = 0;
        v4i an[MS];
#pragma unroll
        for (int ms = 0; ms < MS; ++ms) an[ms] = G > 0 ? wp[(size_t)ms * G * 64] : v4i{0, 0, 0, 0};

        // one K-step: this lane half's B cells are `off` past each pixel's base (valid), or the zero cell
        auto step = [&](int off, bool valid) {
            v4i af[MS];
#pragma unroll
            for (int ms = 0; ms < MS; ++ms) af[ms] = an[ms];
            ++g;
            if (g < G) {
#pragma unroll
                for (int ms = 0; ms < MS; ++ms) an[ms] = wp[((size_t)ms * G + g) * 64];
            }
            v4i bf[NS];
#pragma unroll
            for (int ns = 0; ns < NS; ++ns) {
                bf[ns] = *reinterpret_cast<const v4i *>(P + (size_t)(valid ? off + cbase[ns] : zcell) * 16);
                int t = sx[ns];
#pragma unroll
                for (int i = 0; i < 4; ++i) t = __builtin_amdgcn_sdot4(bf[ns][i], 0x01010101, t, false);
                sx[ns] = t;
            }
#pragma unroll
            for (int ms = 0; ms < MS; ++ms)
#pragma unroll
                for (int ns = 0; ns < NS; ++ns) acc[ms][ns] = __builtin_amdgcn_mfma_i32_32x32x32_i8(af[ms], bf[ns], acc[ms][ns], 0, 0, 0);
        };

#pragma unroll 1
        for (int ch = 0; ch < a.nchunks; ++ch) {
            const int u0 = ch * a.cu, ucur = min(a.cu, a.nu - u0);
            if (a.nchunks > 1 || phs == 0) {
                if (ch > 0) __syncthreads();  // the previous chunk's cells are read
                // ---- stage the chunk's patch: in-image cells from the tensor, the rest the biased input zero point; channels >= c zero
                for (int i = tid; i < ucur * ncells; i += TR_THREADS) {
                    const int u = i / ncells, cell = i - u * ncells;
                    const int r = cell / pw, cc = cell - r * pw;
                    const int iy = iy0 + r, ix = ix0 + cc;
                    uint4 v = make_uint4(fill, fill, fill, fill);
                    if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W)
                        v = *reinterpret_cast<const uint4 *>(a.x + (size_t)((long)a.in_lead + ((long)b * (a.H + 1) + iy + 1) * W1 + ix) * a.in_cs +
                                                             (size_t)(u0 + u) * 16);
                    const int nv = a.c - 16 * (u0 + u);
                    if (nv < 16) { v.x &= keep_bytes(nv); v.y &= keep_bytes(nv - 4); v.z &= keep_bytes(nv - 8); v.w &= keep_bytes(nv - 12); }
                    *reinterpret_cast<uint4 *>(P + (size_t)i * 16) = v;
                }
            }
            __syncthreads();
            if (taps == 0) continue;
#pragma unroll 1
            for (int up = 0; up < (ucur >> 1); ++up) {
                const int plane = (2 * up + kh) * ncells;
#pragma unroll 1
                for (int t = 0; t < taps; ++t) step(plane + tapoff[t], true);
            }
            if (ucur & 1) {  // the odd last unit: two taps per K-step
                const int plane = (ucur - 1) * ncells;
#pragma unroll 1
                for (int tp = 0; 2 * tp < taps; ++tp) {
                    const bool valid = 2 * tp + kh < taps;
                    step(plane + tapoff[valid ? 2 * tp + kh : 0], valid);
                }
            }
        }

        // ---- epilogue of the phase: corrections, requantise (FP64 in the reference's order), stores.  Lane (lj, kh) holds column lj
        //      and accumulator rows 8 grp + 4 kh + r (the 32 x 32 MFMA's D layout)
#pragma unroll
        for (int ns = 0; ns < NS; ++ns) {
            const int sxt = sx[ns] + __shfl_xor(sx[ns], 32);  // the two lane halves hold the two halves of every K-step
            const int p = wn * 64 + ns * 32 + lj;
            const int oy = (qy0 + (p >> a.tw_sh)) * s + ty - a.pad, ox = (qx0 + (p & (TW - 1))) * s + tx - a.pad;
            if (oy < 0 || oy >= a.OH || ox < 0 || ox >= a.OW) continue;
            const size_t pix = (size_t)oy * a.OW + ox;
            uint8_t *ycell = a.y ? a.y + (size_t)((long)a.out_lead + ((long)b * (a.OH + 1) + oy + 1) * OW1 + ox) * a.out_cs : nullptr;
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
                        const size_t pc = (size_t)phs * a.mpad + oc;
                        const uint32_t acct = (uint32_t)acc[ms][ns][grp * 4 + r] + (uint32_t)a.dzp[oc] * (uint32_t)sxt + (uint32_t)a.cw[pc] +
                                              (uint32_t)a.zp_in * (uint32_t)a.sw[pc];
                        const uint32_t u8 = requant_u8((int32_t)acct, a.bias[oc], a.mval[oc], a.sval[oc], a.zp_act, a.act, a.store_mode);
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
}

// dynamic LDS above the 64 KiB default: raised per instantiation and device, only when a launch needs more (kargs.h lds_limit_for)
template <void (*kern)(const TrArgs)>
int tr_launch_one(const TrArgs &a, int grid, size_t lds, hipStream_t st)
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
    conv_launch_note(grid, TR_THREADS, lds);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(TR_THREADS), lds, st, a);
    return hipGetLastError() == hipSuccess ? MI355_OK : MI355_EHIP;
}

size_t tr_lds(int units, int ncells) { return TR_MAX_TAPS * sizeof(int) + ((size_t)units * ncells + 1) * 16; }

}  // namespace

int conv_tr_launch(TrArgs &a, hipStream_t st)
{
    const int k = a.ksize, s = a.stride;
    if (k < 1 || k > 11 || s < 1 || s > TR_MAX_STRIDE || a.pad < 0 || a.pad > k - 1 || a.OH < 1 || a.OW < 1) return MI355_EINVAL;
    if (a.in_cs % 16 || a.in_cs < a.nu * 16 || ((uintptr_t)a.x & 15)) return MI355_EINVAL;
    a.halo = (k + s - 1) / s - 1;
    const int nqh = (a.OH - 1 + a.pad) / s + 1, nqw = (a.OW - 1 + a.pad) / s + 1;  // quotients that hold an output
    // tiles: 32 (n <= 32) or 64 filters x 256 quotients with every channel staged once; when that patch does not fit in LDS, 128 filters
    // x 64 quotients; when that does not either, the same tile on chunks of channels.  The throughput plan first looks for a tile of
    // which two workgroups fit a CU.
    struct Cfg { int ms, wm; };
    const Cfg cfgs[2] = {{a.n <= 32 ? 1 : 2, 1}, {1, 4}};
    const size_t caps[2] = {a.plan == MI355_PLAN_THROUGHPUT ? TR_LDS_MAX / 2 : TR_LDS_MAX, TR_LDS_MAX};
    for (int pass = 0; pass < 3; ++pass)
        for (const Cfg &c : cfgs) {
            if (pass == 2 && c.wm != 4) continue;
            const int npx = (4 / c.wm) * 64;
            const int tw = pass == 2 ? 8 : (nqw <= 8 ? 8 : (nqw <= 16 ? 16 : 32)), th = npx / tw;
            a.ph = th + a.halo; a.pw = tw + a.halo;
            const int ncells = a.ph * a.pw;
            a.cu = a.nu; a.nchunks = 1;
            if (pass < 2) {
                if (tr_lds(a.nu, ncells) > caps[pass]) continue;
            } else {
                a.cu = (int)(((TR_LDS_MAX - TR_MAX_TAPS * sizeof(int)) / 16 - 1) / ncells) & ~1;
                a.nchunks = (a.nu + a.cu - 1) / a.cu;
            }
            a.tw_sh = tw == 8 ? 3 : (tw == 16 ? 4 : 5);
            a.tiles_x = (nqw + tw - 1) / tw; a.tiles_y = (nqh + th - 1) / th;
            const int mrows = 32 * c.ms * c.wm;
            a.mgroups = (a.n + mrows - 1) / mrows;
            const long grid = (long)a.mgroups * a.B * a.tiles_x * a.tiles_y;
            if (grid > 0x7FFFFFFF) return MI355_EINVAL;
            const size_t lds = tr_lds(a.cu, ncells);
            if (c.wm == 4) return tr_launch_one<conv_tr_kernel<1, 4>>(a, (int)grid, lds, st);
            if (c.ms == 2) return tr_launch_one<conv_tr_kernel<2, 1>>(a, (int)grid, lds, st);
            return tr_launch_one<conv_tr_kernel<1, 1>>(a, (int)grid, lds, st);
        }
    return MI355_EINVAL;
}
