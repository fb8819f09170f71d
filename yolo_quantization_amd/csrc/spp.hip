// spp.hip -- the SPP block's stride-1 "same" max pools (5 / 9 / 13 in yolov3-spp, yolov4, YOLO-Fastest) of one tensor in one launch.
//
// Semantics: y[i] = forward_maxpool_layer_quant(x, size = sizes[i], stride = 1, pad = sizes[i] - 1) (ref: src/maxpool_layer.c:109-172):
// the max over the in-image taps of the window centred on the cell, starting at uint8 0.  Bytes are stored biased (^ 0x80), so uint8 0
// is 0x80, the smallest signed byte, and the max is the signed byte max maxpool_u8_kernel (glue.hip) takes.
//
// Cascade.  A box max of size a of a box max of size b is the box max of size a + b - 1, so level i is computed
// from level i - 1 with the window d[i] = sizes[i] - sizes[i - 1] + 1 (5, 5, 5 for 5 / 9 / 13), and each box max is a row pass followed
// by a column pass: six passes of 4 taps instead of 25 + 81 + 169 taps.  Out-of-image positions hold 0x80 at level 0; an intermediate
// computed at an out-of-image position collects only taps that lie inside the larger window anyway, so the identity holds at the borders.
//
// Work split.  A workgroup (256 threads) owns one image, one 32-byte channel chunk (two 16-byte pieces, eight dwords) and one tile of
// TH x TW output pixels, 8 <= TH, TW <= 20: a map of up to 20 x 20 (the block's 13 x 13 and 19 x 19) is one tile, a larger one is cut
// into the fewest equal tiles.  Workgroups are numbered (image, tile, chunk), chunk fastest: neighbours read the rest of the same cells.
//
// Data movement.  The tile of x with a halo of R = (sizes[n - 1] - 1) / 2 cells is read from HBM once, 16 bytes per load, into LDS buffer
// P0; out-of-image cells and pieces beyond the channels are written as 0x80, so no pass has a bounds check and the tensor's pad cells
// are never read.  A second buffer P1 of the same shape takes the row passes: level i is row pass P0 -> P1, column pass P1 -> P0, then
// the centre TH x TW cells of P0 go to y[i] with 16-byte stores and P0 is the next level's input.  The valid region shrinks by
// (d[i] - 1) / 2 cells per level and ends at the tile.  LDS rows are an odd number of cells apart.
//
// A pass.  A lane owns one dword (four channels) of a line and a run of SPP_RUN = 8 consecutive positions along the pass direction: it
// reads the run's strip of 8 + d - 1 dwords once and slides the window in registers.  The eight lanes of a cell are consecutive, the
// eight runs of a wave lie on eight neighbouring lines: eight rows an odd number of cells apart in a row pass (eight different 32-byte
// bank groups), 64 consecutive dwords in a column pass.  A line whose length is no multiple of 8 has its last run moved back to end at
// the line's end (the overlap is written twice with the same bytes).  LDS reads per output dword of a pass: (8 + d - 1) / 8 = 1.5 for
// d = 5; over the shrinking regions of a 13 x 13 (19 x 19) tile with 5 / 9 / 13 that is 2.1 (1.7) dword reads per stored output byte, the
// 16-byte read of each store included (maxpool_u8_kernel: 275 global 16-byte loads per 16 output bytes).
//
// The max.  A byte compares like the signed halfword that holds it in its high byte, whatever the low byte holds.  A dword p is kept
// as two registers, o = p (bytes 1 and 3 in place) and e = p << 8 per halfword (bytes 0 and 2); a max of two dwords is then two
// v_pk_max_i16 and the dword is put together once per output: (e >> 8) | (o & 0xFF00FF00).  The window itself is built by doubling
// (windows of 2, 4, 8) and one last max of two overlapping windows: 2, 3, 3, 4, 4, 4 maxima per position for d = 3 .. 13.
#include "kargs.h"
#include <mutex>

namespace {

constexpr int SPP_THREADS = 256;
constexpr int SPP_CD = 8;  // dwords of a cell in LDS: the 32-byte chunk

template <int D>
__device__ __forceinline__ void spp_run(const uint32_t *src, uint32_t *dst, int stride)
{
    constexpr int L = SPP_RUN + D - 1;
    constexpr int W = D >= 8 ? 8 : (D >= 4 ? 4 : 2);  // the largest power of two <= D
    v2s o[L], e[L];
#pragma unroll
    for (int i = 0; i < L; ++i) {
        o[i] = __builtin_bit_cast(v2s, src[i * stride]);
        e[i] = o[i] << 8;
    }
#pragma unroll
    for (int w = 1; w < W; w *= 2)  // o[i], e[i]: the max over [i, i + 2w)
#pragma unroll
        for (int i = 0; i + 2 * w <= L; ++i) {
            o[i] = __builtin_elementwise_max(o[i], o[i + w]);
            e[i] = __builtin_elementwise_max(e[i], e[i + w]);
        }
#pragma unroll
    for (int j = 0; j < SPP_RUN; ++j) {  // [j, j + D) = [j, j + W) u [j + D - W, j + D)
        const v2s mo = __builtin_elementwise_max(o[j], o[j + D - W]), me = __builtin_elementwise_max(e[j], e[j + D - W]);
        dst[j * stride] = (__builtin_bit_cast(uint32_t, me) >> 8) | (__builtin_bit_cast(uint32_t, mo) & 0xFF00FF00u);
    }
}

// One pass over `nlines` lines of `len` outputs each.  base: dword index of line 0's first output, the same in both buffers; lines are
// lstride dwords apart, positions pstride.  The strip of an output starts (d - 1) / 2 positions before it.
__device__ __forceinline__ void spp_pass(const uint32_t *src, uint32_t *dst, int base, int d, int nlines, int lstride, int pstride, int len)
{
    const int c = threadIdx.x & (SPP_CD - 1);
    const int nruns = (len + SPP_RUN - 1) / SPP_RUN;
    for (int g = threadIdx.x / SPP_CD; g < nlines * nruns; g += SPP_THREADS / SPP_CD) {
        const int run = g / nlines, line = g - run * nlines;
        const int p0 = min(run * SPP_RUN, len - SPP_RUN);
        uint32_t *o = dst + base + line * lstride + p0 * pstride + c;
        const uint32_t *s = src + base + line * lstride + (p0 - (d - 1) / 2) * pstride + c;
        switch (d) {
        case 3: spp_run<3>(s, o, pstride); break;
        case 5: spp_run<5>(s, o, pstride); break;
        case 7: spp_run<7>(s, o, pstride); break;
        case 9: spp_run<9>(s, o, pstride); break;
        case 11: spp_run<11>(s, o, pstride); break;
        default: spp_run<13>(s, o, pstride); break;
        }
    }
}

__global__ __launch_bounds__(SPP_THREADS) void spp_u8_kernel(const SppArgs a)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int pitch = a.pitch, pw = a.pw, R = a.R, TH = a.TH, TW = a.TW;
    uint32_t *P0 = reinterpret_cast<uint32_t *>(smem);  // [ph][pitch] cells of SPP_CD dwords
    uint32_t *P1 = P0 + a.ph * pitch * SPP_CD;

    int idx = blockIdx.x;
    const int chunk = idx % a.nchunks;
    idx /= a.nchunks;
    const int tpi = a.tiles_x * a.tiles_y;
    const int b = idx / tpi;
    idx -= b * tpi;
    const int ty = idx / a.tiles_x, tx = idx - ty * a.tiles_x;
    const int oy0 = ty * TH, ox0 = tx * TW;
    const int vp = min(2, a.pieces16 - 2 * chunk);  // pieces of this chunk that hold channels
    const size_t W1 = (size_t)a.W + 1, row0 = (size_t)b * (a.H + 1) + 1;

    // ---- stage the patch: out of the image or beyond the channels: uint8 0
    for (int i = tid; i < a.ph * pw * 2; i += SPP_THREADS) {
        const int cell = i >> 1, q = i & 1;
        const int r = fd_div(cell, a.fd_pw), cc = cell - r * pw;
        const int iy = oy0 - R + r, ix = ox0 - R + cc;
        uint4 v = make_uint4(0x80808080u, 0x80808080u, 0x80808080u, 0x80808080u);
        if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W && q < vp)
            v = *reinterpret_cast<const uint4 *>(a.x + ((size_t)a.in_lead + (row0 + iy) * W1 + ix) * a.in_cs + chunk * 32 + q * 16);
        *reinterpret_cast<uint4 *>(P0 + (r * pitch + cc) * SPP_CD + q * 4) = v;
    }
    __syncthreads();

    const int cstride = SPP_CD, rstride = pitch * SPP_CD;
    int h = R;  // halo still valid around the tile
#pragma unroll 1
    for (int lv = 0; lv < a.n; ++lv) {
        const int d = a.d[lv], hp = h;
        h -= (d - 1) / 2;
        // rows of the previous level's region, columns of this level's
        spp_pass(P0, P1, ((R - hp) * pitch + R - h) * SPP_CD, d, TH + 2 * hp, rstride, cstride, TW + 2 * h);
        __syncthreads();
        // lines are this level's columns, positions its rows
        spp_pass(P1, P0, ((R - h) * pitch + R - h) * SPP_CD, d, TW + 2 * h, cstride, rstride, TH + 2 * h);
        __syncthreads();
        // the tile's in-image cells, whole 16-byte pieces (the next row pass only reads P0)
        uint8_t *y = a.y[lv] + chunk * 32;
        const int cs = a.out_cs[lv], lead = a.out_lead[lv];
        for (int i = tid; i < TH * TW * 2; i += SPP_THREADS) {
            const int cell = i >> 1, q = i & 1;
            const int ry = fd_div(cell, a.fd_tw), rx = cell - ry * TW;
            const int oy = oy0 + ry, ox = ox0 + rx;
            if (oy >= a.H || ox >= a.W || q >= vp) continue;
            const uint4 v = *reinterpret_cast<const uint4 *>(P0 + ((R + ry) * pitch + R + rx) * SPP_CD + q * 4);
            *reinterpret_cast<uint4 *>(y + ((size_t)lead + (row0 + oy) * W1 + ox) * cs + q * 16) = v;
        }
    }
}

}  // namespace

int spp_launch(SppArgs &a, hipStream_t st)
{
    int R = 0;
    for (int i = 0; i < a.n; ++i) R += (a.d[i] - 1) / 2;
    a.R = R;
    // the fewest equal tiles of at most SPP_TILE a side; a side is never below a run
    a.tiles_y = (a.H + SPP_TILE - 1) / SPP_TILE;
    a.tiles_x = (a.W + SPP_TILE - 1) / SPP_TILE;
    a.TH = (a.H + a.tiles_y - 1) / a.tiles_y;
    a.TW = (a.W + a.tiles_x - 1) / a.tiles_x;
    if (a.TH < SPP_RUN) a.TH = SPP_RUN;
    if (a.TW < SPP_RUN) a.TW = SPP_RUN;
    a.ph = a.TH + 2 * R;
    a.pw = a.TW + 2 * R;
    a.pitch = a.pw | 1;
    a.nchunks = (a.pieces16 + 1) / 2;
    a.fd_pw = fastdiv_make((uint32_t)a.pw);
    a.fd_tw = fastdiv_make((uint32_t)a.TW);
    const size_t lds = (size_t)a.ph * a.pitch * SPP_CD * 4 * 2;  // <= 67 584: under the 80 KB at which two workgroups share a CU
    const long grid = (long)a.B * a.tiles_x * a.tiles_y * a.nchunks;
    if (grid < 1 || grid > 0x7FFFFFFF) return MI355_EINVAL;
    if (lds > 64 * 1024) {  // dynamic LDS above the default: raised per device, only when a launch needs more
        static size_t have[64] = {0};
        static std::mutex mu;
        int dev = 0;
        (void)hipGetDevice(&dev);
        std::lock_guard<std::mutex> lk(mu);
        size_t &hv = have[dev & 63];
        if (lds > hv) {
            if (hipFuncSetAttribute(reinterpret_cast<const void *>(spp_u8_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
                return MI355_EHIP;
            hv = lds;
        }
    }
    hipLaunchKernelGGL(spp_u8_kernel, dim3((unsigned)grid), dim3(SPP_THREADS), lds, st, a);
    return hipGetLastError() == hipSuccess ? MI355_OK : MI355_EHIP;
}
