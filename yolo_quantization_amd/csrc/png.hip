// png.hip -- the device half of the PNG input path (mi355_png_unfilter, mi355_png_to_rgb): everything a PNG decoder does after the
// inflate, written to give the bytes stb_image v2.19 gives as the reference compiles it (ref: src/stb_image.h:4307-4931).  PNG is
// lossless and all of this is byte arithmetic, so "the same bytes" is exact.
#include "kargs.h"

// ---- scanline reconstruction -------------------------------------------------------------------------------------------------------
// Recon(x) = Filt(x) + predictor(a, b, c) mod 256 with a = Recon(x - bpp), b = the byte above, c = the byte above a, all zero outside
// the image (ref :4372-4431).  Sub, Average and Paeth are serial along a row, Up, Average and Paeth from row to row: the work is
// parallel across the bytes of a unit and along anti-diagonals only.  One wave takes a segment.  Lane r owns row y0 + r of a band of 64
// rows and works on unit x = t - r at step t: its b is what lane r - 1 produced one step earlier (one cross-lane move per step), its c
// is the b of the step before, its a its own last result.  Lanes of one wave hold rows of different filters, so the predictor is
// selected, not branched to.  Bands follow each other in the same wave; lane 0 takes its b from the last row of the band before, read
// back from the output.
//
// The bytes pass through the LDS in skewed tiles: tile k of a band covers steps k T .. k T + T - 1 (T = 192 / bpp units), that is
// units k T - r .. of row r, 192 bytes per row.  The wave loads a tile row by row (lane j the bytes j, j + 64, j + 128 of the row:
// coalesced), reconstructs it in place -- at a step every lane reads and writes the same byte offset of its own tile row, and rows are
// 49 dwords apart, so the 64 lanes fall on 64 different banks -- and stores it row by row.  Row 64 of the tile holds lane 0's b.
#define PNG_WAVES 4
#define PNG_TILE_BYTES 192
#define PNG_TILE_PITCH 196
#define PNG_TILE_ROWS 65

// LDS traffic of one wave is seen by the same wave in program order; this keeps the compiler from moving accesses across the point
// where lanes exchange data through the tile.  No other wave is waited for.
__device__ static inline void png_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ static inline uint32_t png_predict(uint32_t f, uint32_t a, uint32_t b, uint32_t c)
{
    const int pa = abs((int)b - (int)c), pb = abs((int)a - (int)c), pc = abs((int)a + (int)b - 2 * (int)c);
    const uint32_t paeth = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
    uint32_t p = 0;
    p = f == 1 ? a : p;
    p = f == 2 ? b : p;
    p = f == 3 ? (a + b) >> 1 : p;
    p = f == 4 ? paeth : p;
    return p;
}

template <int BPP>
__device__ static void png_unfilter_segment(const uint8_t *filtered, uint8_t *out, const int row_bytes, const int rows, uint8_t *tile, const int lane)
{
    constexpr int T = PNG_TILE_BYTES / BPP, NW = BPP > 4 ? 2 : 1;
    const int W = row_bytes / BPP;
    const size_t in_pitch = (size_t)row_bytes + 1;
    uint8_t *mine = tile + lane * PNG_TILE_PITCH, *above = tile + 64 * PNG_TILE_PITCH;
    for (int y0 = 0; y0 < rows; y0 += 64) {
        const int nr = rows - y0 < 64 ? rows - y0 : 64;
        const bool row_live = lane < nr;
        const uint32_t f = row_live ? filtered[(size_t)(y0 + lane) * in_pitch] : 0u;
        const uint8_t *prev = y0 ? out + (size_t)(y0 - 1) * (size_t)row_bytes : nullptr;
        uint32_t a[NW], c[NW], res[NW];
#pragma unroll
        for (int k = 0; k < NW; ++k) a[k] = c[k] = res[k] = 0;
        const int steps = W + nr - 1;
        for (int t0 = 0; t0 < steps; t0 += T) {
            const int tn = steps - t0 < T ? steps - t0 : T;
            // load: row r of the tile holds bytes (t0 - r) BPP .. of row y0 + r, zero outside the row
            for (int r = 0; r < nr; ++r) {
                const long base = ((long)t0 - r) * BPP;
                const uint8_t *row = filtered + (size_t)(y0 + r) * in_pitch + 1;
#pragma unroll
                for (int j = lane; j < PNG_TILE_BYTES; j += 64) {
                    const long at = base + j;
                    tile[r * PNG_TILE_PITCH + j] = (at >= 0 && at < row_bytes) ? row[at] : (uint8_t)0;
                }
            }
#pragma unroll
            for (int j = lane; j < PNG_TILE_BYTES; j += 64) {
                const long at = (long)t0 * BPP + j;
                above[j] = (prev && at < row_bytes) ? prev[at] : (uint8_t)0;
            }
            png_wave_sync();
            for (int s = 0; s < tn; ++s) {
                const int x = t0 + s - lane;
                const bool live = row_live && x >= 0 && x < W;
                uint32_t b[NW], raw[NW], now[NW];
#pragma unroll
                for (int k = 0; k < NW; ++k) {
                    b[k] = (uint32_t)__shfl_up((int)res[k], 1);
                    raw[k] = 0; now[k] = 0;
                }
#pragma unroll
                for (int k = 0; k < BPP; ++k) raw[k >> 2] |= (uint32_t)mine[s * BPP + k] << (8 * (k & 3));
                if (lane == 0) {
#pragma unroll
                    for (int k = 0; k < NW; ++k) b[k] = 0;
#pragma unroll
                    for (int k = 0; k < BPP; ++k) b[k >> 2] |= (uint32_t)above[s * BPP + k] << (8 * (k & 3));
                }
                if (x == 0) {
#pragma unroll
                    for (int k = 0; k < NW; ++k) a[k] = c[k] = 0;
                }
#pragma unroll
                for (int k = 0; k < BPP; ++k) {
                    const int sh = 8 * (k & 3);
                    const uint32_t v = ((raw[k >> 2] >> sh) + png_predict(f, (a[k >> 2] >> sh) & 255u, (b[k >> 2] >> sh) & 255u, (c[k >> 2] >> sh) & 255u)) & 255u;
                    now[k >> 2] |= v << sh;
                    if (live) mine[s * BPP + k] = (uint8_t)v;
                }
#pragma unroll
                for (int k = 0; k < NW; ++k) {
                    res[k] = live ? now[k] : 0u;
                    a[k] = res[k];
                    c[k] = b[k];
                }
            }
            png_wave_sync();
            // store: of row r, the bytes of the units this tile's steps reached
            for (int r = 0; r < nr; ++r) {
                const long base = ((long)t0 - r) * BPP;
                uint8_t *row = out + (size_t)(y0 + r) * (size_t)row_bytes;
#pragma unroll
                for (int j = lane; j < PNG_TILE_BYTES; j += 64) {
                    const long at = base + j;
                    if (j < tn * BPP && at >= 0 && at < row_bytes) row[at] = tile[r * PNG_TILE_PITCH + j];
                }
            }
            png_wave_sync();
        }
        // the next band reads this band's last row back from `out`
        if (y0 + 64 < rows) __threadfence();
    }
}

__global__ __launch_bounds__(64 * PNG_WAVES) void png_unfilter_kernel(const mi355_png_segment *table, int nsegments)
{
    __shared__ __attribute__((aligned(16))) uint8_t lds[PNG_WAVES][PNG_TILE_ROWS * PNG_TILE_PITCH];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int seg = blockIdx.x * PNG_WAVES + wave;
    if (seg >= nsegments) return;  // no workgroup barrier anywhere below: the waves are independent
    const mi355_png_segment sg = table[seg];
    const int row_bytes = __builtin_amdgcn_readfirstlane(sg.row_bytes), rows = __builtin_amdgcn_readfirstlane(sg.rows);
    uint8_t *tile = lds[wave];
    switch (__builtin_amdgcn_readfirstlane(sg.bpp)) {
    case 1: png_unfilter_segment<1>(sg.filtered, sg.out, row_bytes, rows, tile, lane); break;
    case 2: png_unfilter_segment<2>(sg.filtered, sg.out, row_bytes, rows, tile, lane); break;
    case 3: png_unfilter_segment<3>(sg.filtered, sg.out, row_bytes, rows, tile, lane); break;
    case 4: png_unfilter_segment<4>(sg.filtered, sg.out, row_bytes, rows, tile, lane); break;
    case 6: png_unfilter_segment<6>(sg.filtered, sg.out, row_bytes, rows, tile, lane); break;
    case 8: png_unfilter_segment<8>(sg.filtered, sg.out, row_bytes, rows, tile, lane); break;
    default: break;
    }
}

const char *png_unfilter_check(const mi355_png_segment *host, int nsegments)
{
    if (!host || nsegments < 1 || nsegments > 7 * 65535) return "png_unfilter: null table / need 1 <= nsegments <= 458745";
    for (int i = 0; i < nsegments; ++i) {
        const mi355_png_segment &s = host[i];
        if (!s.filtered || !s.out) return "png_unfilter: null segment pointer";
        if (s.bpp != 1 && s.bpp != 2 && s.bpp != 3 && s.bpp != 4 && s.bpp != 6 && s.bpp != 8) return "png_unfilter: bpp must be 1, 2, 3, 4, 6 or 8";
        if (s.rows < 1 || s.rows > 32768) return "png_unfilter: need 1 <= rows <= 32768";
        if (s.row_bytes < 1 || s.row_bytes > 8 * 32768) return "png_unfilter: need 1 <= row_bytes <= 262144";
        if (s.row_bytes % s.bpp) return "png_unfilter: row_bytes must be a multiple of bpp";
    }
    return nullptr;
}

int png_unfilter_launch(const mi355_png_segment *table_dev, int nsegments, hipStream_t st)
{
    hipLaunchKernelGGL(png_unfilter_kernel, dim3((unsigned)((nsegments + PNG_WAVES - 1) / PNG_WAVES)), dim3(64 * PNG_WAVES), 0, st, table_dev, nsegments);
    return hipGetLastError() == hipSuccess ? MI355_OK : MI355_EHIP;
}

// ---- de-interlacing, expansion, reduction to RGB -----------------------------------------------------------------------------------
__device__ static inline int png_channels(int color) { return color == 2 ? 3 : (color == 4 ? 2 : (color == 6 ? 4 : 1)); }

// grid: (workgroups of the largest image, B); one thread per pixel
__global__ __launch_bounds__(256) void png_to_rgb_kernel(const mi355_png_image *table)
{
    const mi355_png_image &im = table[blockIdx.y];
    const int w = im.w, h = im.h;
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long)w * h) return;
    const int y = (int)(t / w), x = (int)(t - (long)y * w);
    int p = 0, px = x, py = y, pw = w;
    if (im.interlace) {  // ref :4554-4557: xorig {0,4,0,2,0,1,0}, yorig {0,0,4,0,2,0,1}, xspc {8,8,4,4,2,2,1}, yspc {8,8,8,4,4,2,2}
        int xo, xs, ys;
        if (y & 1)      { p = 6; xo = 0; xs = 0; ys = 1; }
        else if (x & 1) { p = 5; xo = 1; xs = 1; ys = 1; }
        else if (y & 2) { p = 4; xo = 0; xs = 1; ys = 2; }
        else if (x & 2) { p = 3; xo = 2; xs = 2; ys = 2; }
        else if (y & 4) { p = 2; xo = 0; xs = 2; ys = 3; }
        else if (x & 4) { p = 1; xo = 4; xs = 3; ys = 3; }
        else            { p = 0; xo = 0; xs = 3; ys = 3; }
        px = x >> xs; py = y >> ys;
        pw = (w - xo + (1 << xs) - 1) >> xs;
    }
    const int depth = im.depth, color = im.color, n = png_channels(color);
    const size_t row_bytes = ((size_t)pw * (size_t)(n * depth) + 7) >> 3;
    const uint8_t *row = im.pass[p] + (size_t)py * row_bytes;
    uint32_t r, g, b;
    if (depth >= 8) {  // depth 16: the first byte of a sample is its high byte, which is what v >> 8 keeps (ref :1128, stbi__convert_16_to_8)
        const int step = depth >> 3;
        const uint8_t *s = row + (size_t)px * (size_t)(n * step);
        r = s[0];
        if (n >= 3) { g = s[step]; b = s[2 * step]; }  // colour types 2 and 6 only: type 3 has bit 1 set and one sample
        else g = b = r;
    } else {           // one sample per pixel, packed MSB first
        const int bit = px * depth;
        r = (row[bit >> 3] >> (8 - depth - (bit & 7))) & ((1u << depth) - 1u);
        if (color == 0) r *= depth == 1 ? 0xffu : (depth == 2 ? 0x55u : 0x11u);
        g = b = r;
    }
    if (color == 3) {
        const uint32_t i = r;
        if ((int)i < im.pal_len) { r = im.palette[3 * i]; g = im.palette[3 * i + 1]; b = im.palette[3 * i + 2]; }
        else r = g = b = 0;
    }
    uint8_t *o = im.rgb + (size_t)y * im.pitch + 3 * (size_t)x;
    o[0] = (uint8_t)r; o[1] = (uint8_t)g; o[2] = (uint8_t)b;
}

const char *png_to_rgb_check(const mi355_png_image *host, int B)
{
    if (!host || B < 1 || B > 65535) return "png_to_rgb: null table / need 1 <= B <= 65535";
    static const int xorig[7] = {0, 4, 0, 2, 0, 1, 0}, yorig[7] = {0, 0, 4, 0, 2, 0, 1};
    for (int b = 0; b < B; ++b) {
        const mi355_png_image &im = host[b];
        if (!im.rgb) return "png_to_rgb: null frame pointer";
        if (im.w < 1 || im.h < 1 || im.w > 32768 || im.h > 32768) return "png_to_rgb: need 1 <= w, h <= 32768 for every image";
        if (im.pitch < 3 * im.w) return "png_to_rgb: pitch < 3 * w";
        const int d = im.depth, c = im.color;
        const bool pair = (c == 0 && (d == 1 || d == 2 || d == 4 || d == 8 || d == 16)) || (c == 3 && (d == 1 || d == 2 || d == 4 || d == 8)) ||
                          ((c == 2 || c == 4 || c == 6) && (d == 8 || d == 16));
        if (!pair) return "png_to_rgb: unknown depth / colour pair";
        if (im.interlace != 0 && im.interlace != 1) return "png_to_rgb: interlace must be 0 or 1";
        if (c == 3 && (!im.palette || im.pal_len < 1 || im.pal_len > 256)) return "png_to_rgb: a palette image needs a palette of 1 .. 256 entries";
        for (int k = 0; k < (im.interlace ? 7 : 1); ++k)
            if (!im.pass[k] && (!im.interlace || (im.w > xorig[k] && im.h > yorig[k]))) return "png_to_rgb: null pass pointer";
    }
    return nullptr;
}

int png_to_rgb_launch(const mi355_png_image *table_dev, const mi355_png_image *table_host, int B, hipStream_t st)
{
    long most = 0;
    for (int b = 0; b < B; ++b) {
        const long threads = (long)table_host[b].h * table_host[b].w;
        if (threads > most) most = threads;
    }
    hipLaunchKernelGGL(png_to_rgb_kernel, dim3((unsigned)((most + 255) / 256), B), dim3(256), 0, st, table_dev);
    return hipGetLastError() == hipSuccess ? MI355_OK : MI355_EHIP;
}
