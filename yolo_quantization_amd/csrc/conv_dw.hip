// conv_dw.hip -- depthwise convolution (groups == c == n): size 1..11, any stride and padding, exact int32.
//
// Per filter j:  acc[j][p] = sum_taps (w_u8[j][tap] - zp_w[j]) * x_u8[j][tap(p)],  out-of-image taps = zp_in,
// then the dense layers' epilogue (ref src/convolutional_layer.c:726-760) with the channel's own constants.  One byte in, one byte
// out, k * k MACs per output and no reduction across channels: there is no GEMM here, so no MFMA.  The kernel is built around HBM
// traffic and LDS reuse instead.
//
// Work split.  A workgroup (256 threads) owns one image, one 64-byte channel chunk and a tile of TH x TW output pixels.  A lane owns
// four consecutive channels (one dword of a cell) and a run of DW_RUN = 8 output pixels along x; the 16 lanes of a run read the 16
// consecutive dwords of one cell, the four runs of a wave sit on four consecutive tile rows.  The 16 runs of a workgroup are
// 2^ry_sh rows by 16 >> ry_sh runs per row: tiles of 16 x 8, 8 x 16 or 4 x 32 pixels, chosen by the map (fewest tiles).  Workgroups
// are numbered (image, tile, chunk), chunk fastest: neighbours read the same cells, and small maps with many images still fill the chip.
//
// Data movement.  The input patch with its halo, ((TH - 1) s + k) x ((TW - 1) s + k) cells of 64 bytes, is staged once in LDS with
// 16-byte loads, un-biased (x_u8 = stored ^ 0x80) on the way; every out-of-image cell -- and every 16-byte piece beyond the layer's
// channels -- is written as zp_in, so the MAC loop has no bounds check for any padding and never reads the tensor's pad cells.  LDS
// rows are an odd number of cells apart: at odd strides the four runs of a wave then start in four different 64-byte bank groups.
// 3x3 and 5x5 at stride 1 | 2 hold the lane's (w - zp_w) in VGPRs (36 / 100) and walk the patch row by row: the lane reads the strip
// of (DW_RUN - 1) s + k dwords of a row once, extracts each byte once and feeds all DW_RUN outputs from registers (3.75 LDS reads per
// output for 3x3 stride 1; the sliding-window minimum is 3).  Every other size or stride takes the runtime-size path: the chunk's
// weights in LDS as int16, k * k LDS reads per output.
//
// Arithmetic.  v_mad_i32_i24 on (w - zp_w) in [-255, 255] and the unsigned input byte: exact, and |acc| <= 121 * 255 * 255 < 2^23.
// Epilogue.  common.h: requant_group (folded multiplier, integer LEAKY with its fallback) when every shift_value is a power of two,
// else requant_u8, the reference's operations one by one.  Four channels per stored dword, biased; channels >= n are not written.
#include "kargs.h"
#include <mutex>

namespace {

constexpr int DW_THREADS = 256;
constexpr size_t DW_LDS_MAX = 160 * 1024, DW_LDS_SHARED = 80 * 1024;

// one tap: four channels of one input dword (plain bytes) times the lane's four weights
__device__ __forceinline__ void dw_mac4(int (&acc)[4], const int (&w)[4], uint32_t d)
{
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[c] += __mul24(w[c], (int)((d >> (8 * c)) & 0xFFu));
}

// KS, S: compile-time size and stride (3 | 5, 1 | 2) or 0, 0 = both read from the arguments
template <int KS, int S, int ACT, bool SAT>
__global__ __launch_bounds__(DW_THREADS) void conv_dw_kernel(const DwArgs a)
{
    constexpr int RUN = DW_RUN;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint32_t *P = reinterpret_cast<uint32_t *>(smem);  // [ph][pitch] cells of 16 dwords

    const int tid = threadIdx.x, cl = tid & 15, run = tid >> 4;
    const int k = KS ? KS : a.ksize, s = KS ? S : a.stride, kk = k * k;
    const int pitch = a.pitch, pw = a.pw;
    int idx = blockIdx.x;
    const int chunk = idx % a.nchunks;
    idx /= a.nchunks;
    const int tpi = a.tiles_x * a.tiles_y;
    const int b = idx / tpi;
    idx -= b * tpi;
    const int ty = idx / a.tiles_x, tx = idx - ty * a.tiles_x;
    const int RY = 1 << a.ry_sh, TW = (16 >> a.ry_sh) * RUN;
    const int oy0 = ty * RY, ox0 = tx * TW;
    const int iy0 = oy0 * s - a.pad, ix0 = ox0 * s - a.pad;

    // ---- stage the patch: 16-byte pieces, plain bytes; outside the image or beyond the channels: the input zero point
    {
        const int vp = min(4, a.pieces16 - 4 * chunk);
        const uint32_t fill = (uint32_t)(a.zp_in & 0xFF) * 0x01010101u;
        const int npieces = a.ph * pw * 4;
        const size_t W1 = (size_t)a.W + 1;
        const uint8_t *xb = a.x + (size_t)chunk * 64;
        for (int i = tid; i < npieces; i += DW_THREADS) {
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
    }
    uint32_t *WL = P + (size_t)a.ph * pitch * 16;  // runtime-size path: [kk][64] int16 of this chunk
    const int16_t *wg = a.wd + (size_t)chunk * kk * 64;
    if constexpr (KS == 0) {
        const uint32_t *src = reinterpret_cast<const uint32_t *>(wg);
        for (int i = tid; i < kk * 32; i += DW_THREADS) WL[i] = src[i];
    }
    __syncthreads();

    const int ry = run & (RY - 1), rx = run >> a.ry_sh;
    const uint32_t *row0 = P + (size_t)(ry * s * pitch + rx * RUN * s) * 16 + cl;  // tap (0, 0) of the run's first output
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
                for (int kx = 0; kx < KS; ++kx) dw_mac4(acc[j], w[ky * KS + kx], st[j * S + kx]);
        }
    } else {
#pragma unroll 1
        for (int ky = 0; ky < k; ++ky)
#pragma unroll 1
            for (int kx = 0; kx < k; ++kx) {
                const uint2 wq = *reinterpret_cast<const uint2 *>(WL + (ky * k + kx) * 32 + 2 * cl);
                const int w[4] = {(int)(short)(wq.x & 0xFFFFu), (int)wq.x >> 16, (int)(short)(wq.y & 0xFFFFu), (int)wq.y >> 16};
                const uint32_t *src = row0 + (size_t)(ky * pitch + kx) * 16;
#pragma unroll
                for (int j = 0; j < RUN; ++j) dw_mac4(acc[j], w, src[(size_t)j * s * 16]);
            }
    }

    // ---- epilogue: requantise, stores
    const int ch0 = chunk * 64 + 4 * cl, oy = oy0 + ry;
    if (ch0 >= a.c || oy >= a.OH) return;
    const int n = a.c;
    const bool pow2 = a.hdr->pow2 == 1;
    uint32_t packed[RUN];
    if (pow2) {
        int32_t accb[4][RUN];
        double mp[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int bias = a.bias[ch0 + c];
            mp[c] = a.mprime[ch0 + c];
#pragma unroll
            for (int j = 0; j < RUN; ++j) accb[c][j] = acc[j][c] + bias;
        }
        requant_group<ACT, SAT, RUN>(accb, mp, a.zp_act, packed);
    } else {
#pragma unroll
        for (int j = 0; j < RUN; ++j) packed[j] = 0x80808080u;
#pragma unroll 1
        for (int c = 0; c < 4; ++c) {
            const int bias = a.bias[ch0 + c];
            const double mv = a.mval[ch0 + c], sv = a.sval[ch0 + c];
#pragma unroll
            for (int j = 0; j < RUN; ++j)
                packed[j] ^= requant_u8(acc[j][c], bias, mv, sv, a.zp_act, ACT, SAT ? MI355_STORE_SATURATE : MI355_STORE_WRAP) << (8 * c);
        }
    }
    const size_t ohw = (size_t)a.OH * a.OW;
    const int nv = min(4, n - ch0);  // channels of this dword that exist
#pragma unroll
    for (int j = 0; j < RUN; ++j) {
        const int ox = ox0 + rx * RUN + j;
        if (ox >= a.OW) break;
        const uint32_t plain = packed[j] ^ 0x80808080u;
        if (a.acc_out || a.y_f32) {
            for (int c = 0; c < nv; ++c) {
                const size_t ridx = ((size_t)b * n + ch0 + c) * ohw + (size_t)oy * a.OW + ox;
                if (a.acc_out) a.acc_out[ridx] = acc[j][c];
                if (a.y_f32) a.y_f32[ridx] = (float)((int)((plain >> (8 * c)) & 0xFFu) - a.zp_act) * a.s_act;
            }
        }
        if (a.y) {
            uint8_t *dst = a.y + ((size_t)a.out_lead + ((size_t)b * (a.OH + 1) + oy + 1) * ((size_t)a.OW + 1) + ox) * a.out_cs + ch0;
            if (nv == 4) {
                *reinterpret_cast<uint32_t *>(dst) = packed[j];
            } else {
                for (int c = 0; c < nv; ++c) dst[c] = (uint8_t)(packed[j] >> (8 * c));
            }
        }
    }
}

template <void (*kern)(const DwArgs)>
int dw_launch_one(const DwArgs &a, int grid, size_t lds, hipStream_t st)
{
    if (lds > 64 * 1024) {  // dynamic LDS above the default: raised per instantiation and device, only when a launch needs more
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
    conv_launch_note(grid, DW_THREADS, lds);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(DW_THREADS), lds, st, a);
    return hipGetLastError() == hipSuccess ? MI355_OK : MI355_EHIP;
}

template <int KS, int S>
int dw_dispatch(const DwArgs &a, int grid, size_t lds, hipStream_t st)
{
    const bool sat = a.store_mode == MI355_STORE_SATURATE;
    // RELU is stored like LINEAR (ref src/convolutional_layer.c:740-742)
    if (a.act == MI355_ACT_LEAKY)
        return sat ? dw_launch_one<conv_dw_kernel<KS, S, MI355_ACT_LEAKY, true>>(a, grid, lds, st)
                   : dw_launch_one<conv_dw_kernel<KS, S, MI355_ACT_LEAKY, false>>(a, grid, lds, st);
    if (a.act == MI355_ACT_RELU6)
        return sat ? dw_launch_one<conv_dw_kernel<KS, S, MI355_ACT_RELU6, true>>(a, grid, lds, st)
                   : dw_launch_one<conv_dw_kernel<KS, S, MI355_ACT_RELU6, false>>(a, grid, lds, st);
    return sat ? dw_launch_one<conv_dw_kernel<KS, S, MI355_ACT_LINEAR, true>>(a, grid, lds, st)
               : dw_launch_one<conv_dw_kernel<KS, S, MI355_ACT_LINEAR, false>>(a, grid, lds, st);
}

}  // namespace

int conv_dw_launch(DwArgs &a, hipStream_t st)
{
    const int k = a.ksize, s = a.stride;
    const bool fixed = (k == 3 || k == 5) && (s == 1 || s == 2);
    // The tile with the fewest workgroups whose patch fits: under the throughput plan first within half a CU's LDS, so that two
    // workgroups share a CU; a tie goes to the smaller patch.
    const size_t limits[2] = {a.plan == MI355_PLAN_THROUGHPUT ? DW_LDS_SHARED : DW_LDS_MAX, DW_LDS_MAX};
    for (size_t limit : limits) {
        long best_tiles = 0;
        size_t best_lds = 0;
        for (int sh = 4; sh >= 2; --sh) {
            const int th = 1 << sh, tw = (16 >> sh) * DW_RUN;
            const long ph = (long)(th - 1) * s + k, pw = (long)(tw - 1) * s + k, pitch = pw | 1;
            const size_t lds = (size_t)(ph * pitch) * 64 + (fixed ? 0 : (size_t)k * k * 128);
            if (lds > limit) continue;
            const long tiles = (long)((a.OH + th - 1) / th) * ((a.OW + tw - 1) / tw);
            if (best_tiles && (tiles > best_tiles || (tiles == best_tiles && lds >= best_lds))) continue;
            best_tiles = tiles; best_lds = lds;
            a.ry_sh = sh; a.ph = (int)ph; a.pw = (int)pw; a.pitch = (int)pitch;
            a.tiles_x = (a.OW + tw - 1) / tw; a.tiles_y = (a.OH + th - 1) / th;
        }
        if (!best_tiles) continue;
        a.nchunks = (a.c + 63) / 64;
        a.pieces16 = (a.c + 15) / 16;
        a.fd_pw = fastdiv_make((uint32_t)a.pw);
        const long grid = best_tiles * a.B * a.nchunks;
        if (grid > 0x7FFFFFFF) return MI355_EINVAL;
        if (!fixed) return dw_dispatch<0, 0>(a, (int)grid, best_lds, st);
        if (k == 3) return s == 1 ? dw_dispatch<3, 1>(a, (int)grid, best_lds, st) : dw_dispatch<3, 2>(a, (int)grid, best_lds, st);
        return s == 1 ? dw_dispatch<5, 1>(a, (int)grid, best_lds, st) : dw_dispatch<5, 2>(a, (int)grid, best_lds, st);
    }
    return MI355_EINVAL;
}
