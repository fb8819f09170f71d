// jpeg.hip -- the device half of the JPEG input path (mi355_jpeg_idct, mi355_jpeg_to_rgb): everything a baseline JPEG decoder does
// after the entropy decode, written to give the bytes stb_image v2.19 gives as the reference compiles it (ref: src/stb_image.h).  All
// of it is integer arithmetic, so "the same bytes" is exact: dequantisation with stb's 16-bit store (:1969-1999), its two-pass 8x8
// inverse DCT (:2163-2261; columns first, the rounding between the passes makes the order part of the result), its resamplers as pure
// functions of the output pixel (:3173-3235, :3354-3363 with the row walk of :3611-3644) and its YCbCr -> RGB row (:3367-3391).
// Everything is computed in 32-bit wrapping arithmetic (uint32_t; an arithmetic shift where stb shifts an int), so hostile
// coefficients give some bytes and nothing undefined.
#include "kargs.h"

// ---- inverse DCT -------------------------------------------------------------------------------------------------------------------
// One 8-point pass on s[0..7] (the even part on s0, s2, s4, s6, the odd part on s1, s3, s5, s7): o[k] = e[k] + odd[k], o[7 - k] =
// e[k] - odd[k], with `bias` added to the even part first.  The multipliers are (int)(c * 4096 + 0.5) of the decimals stb lists.
__device__ static inline void idct8(const uint32_t s[8], uint32_t bias, uint32_t o[8])
{
    const uint32_t z = (s[2] + s[6]) * 2217u;
    const uint32_t e2 = z + s[6] * (uint32_t)-7567, e3 = z + s[2] * 3135u;
    const uint32_t e0 = (s[0] + s[4]) << 12, e1 = (s[0] - s[4]) << 12;
    const uint32_t x0 = e0 + e3 + bias, x3 = e0 - e3 + bias, x1 = e1 + e2 + bias, x2 = e1 - e2 + bias;
    uint32_t a = s[7], b = s[5], c = s[3], d = s[1];
    uint32_t p3 = a + c, p4 = b + d, p1 = a + d, p2 = b + c;
    const uint32_t p5 = (p3 + p4) * 4816u;
    a *= 1223u; b *= 8410u; c *= 12586u; d *= 6149u;
    p1 = p5 + p1 * (uint32_t)-3685;
    p2 = p5 + p2 * (uint32_t)-10497;
    p3 *= (uint32_t)-8034;
    p4 *= (uint32_t)-1597;
    d += p1 + p4; c += p2 + p3; b += p2 + p4; a += p1 + p3;
    o[0] = x0 + d; o[7] = x0 - d;
    o[1] = x1 + c; o[6] = x1 - c;
    o[2] = x2 + b; o[5] = x2 - b;
    o[3] = x3 + a; o[4] = x3 - a;
}

__device__ static inline uint32_t sar(uint32_t v, int n) { return (uint32_t)((int32_t)v >> n); }
__device__ static inline uint32_t clamp_byte(uint32_t v) { const int32_t i = (int32_t)v; return (uint32_t)(i < 0 ? 0 : (i > 255 ? 255 : i)); }
// The shifted value as the compiler cannot look through it.  hipcc (ROCm 7) folds clamp(a >> n) | clamp(b >> n) << 8 into one
// v_ashr_pk_u8_i32 and ORs the other two bytes onto its result as if the upper half of that register were zero; on the MI355X it is
// not (bytes 2 and 3 of every stored word came out with foreign bits), so the shift and the clamp are kept apart.
__device__ static inline uint32_t sar_opaque(uint32_t v, int n)
{
    uint32_t r = sar(v, n);
    asm volatile("" : "+v"(r));
    return r;
}

// LDS tile of one block: 8 rows of 8 dwords, 9 dwords apart, blocks 72 dwords apart.  ds_read_b32 / ds_write_b32 bank 32 dwords wide
// per 32-lane half (four blocks x eight lanes): dword 72 b + 9 r + k lies on bank (8 (b + r) + r + k) % 32, which is distinct over
// (b, r) at a fixed k -- the row accesses, lane r at column k -- and over (b, k) at a fixed r -- the column accesses, lane k at row r.
#define JPEG_TILE_ROW 9
#define JPEG_TILE_BLOCK 72

// Eight lanes per block, eight blocks per wave, 32 blocks per workgroup.  Lane r loads row r of its block's coefficients and of the
// quantiser (one 16-byte load each), dequantises, and the block is transposed through the LDS twice: lane c runs the column pass on
// column c, lane r the row pass on row r and stores the 8 bytes of output row r with one store.  stb's shortcut for a column whose
// seven AC values are zero (:2213) is the full formula's value ((4096 d + 512) >> 10 == 4 d), so there is no branch for it.
__global__ __launch_bounds__(256) void jpeg_idct_kernel(const mi355_jpeg_plane *table, int nplanes, int total)
{
    __shared__ uint32_t tile[32 * JPEG_TILE_BLOCK];
    const int r = threadIdx.x & 7, slot = threadIdx.x >> 3;
    const int g = blockIdx.x * 32 + slot;
    const bool live = g < total;
    uint32_t *t = tile + slot * JPEG_TILE_BLOCK;
    uint32_t v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint8_t *dst = nullptr;
    if (live) {
        int lo = 0, hi = nplanes - 1;  // the last plane whose first block is <= g
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (table[mid].first_block <= g) lo = mid;
            else hi = mid - 1;
        }
        const mi355_jpeg_plane pl = table[lo];
        const int local = g - pl.first_block, by = local / pl.blocks_w, bx = local - by * pl.blocks_w;
        const uint4 cw = *reinterpret_cast<const uint4 *>(pl.coef + (size_t)local * 64 + r * 8);
        const uint4 qw = *reinterpret_cast<const uint4 *>(pl.quant + r * 8);
        const uint32_t c4[4] = {cw.x, cw.y, cw.z, cw.w}, q4[4] = {qw.x, qw.y, qw.z, qw.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {  // (short)(coefficient * quantiser): the low 16 bits of the product, sign-extended
            v[2 * k] = (uint32_t)(int32_t)(int16_t)(uint16_t)((c4[k] & 0xffffu) * (q4[k] & 0xffffu));
            v[2 * k + 1] = (uint32_t)(int32_t)(int16_t)(uint16_t)((c4[k] >> 16) * (q4[k] >> 16));
        }
        dst = pl.out + ((size_t)by * 8 + r) * ((size_t)pl.blocks_w * 8) + (size_t)bx * 8;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) t[r * JPEG_TILE_ROW + k] = v[k];
    __syncthreads();
    uint32_t s[8], o[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) s[k] = t[k * JPEG_TILE_ROW + r];  // column r, top to bottom
    idct8(s, 512u, o);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 8; ++k) t[k * JPEG_TILE_ROW + r] = sar(o[k], 10);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 8; ++k) s[k] = t[r * JPEG_TILE_ROW + k];  // row r, left to right
    idct8(s, 65536u + (128u << 17), o);
    if (live) {
        uint2 out;
        out.x = clamp_byte(sar_opaque(o[0], 17)) | clamp_byte(sar_opaque(o[1], 17)) << 8 | clamp_byte(sar_opaque(o[2], 17)) << 16 | clamp_byte(sar_opaque(o[3], 17)) << 24;
        out.y = clamp_byte(sar_opaque(o[4], 17)) | clamp_byte(sar_opaque(o[5], 17)) << 8 | clamp_byte(sar_opaque(o[6], 17)) << 16 | clamp_byte(sar_opaque(o[7], 17)) << 24;
        *reinterpret_cast<uint2 *>(dst) = out;
    }
}

const char *jpeg_idct_check(const mi355_jpeg_plane *host, int nplanes)
{
    if (!host || nplanes < 1 || nplanes > 3 * 65535) return "jpeg_idct: null table / need 1 <= nplanes <= 196605";
    long total = 0;
    for (int i = 0; i < nplanes; ++i) {
        const mi355_jpeg_plane &p = host[i];
        if (!p.coef || !p.quant || !p.out) return "jpeg_idct: null plane pointer";
        if ((reinterpret_cast<size_t>(p.coef) & 15) || (reinterpret_cast<size_t>(p.quant) & 15) || (reinterpret_cast<size_t>(p.out) & 7))
            return "jpeg_idct: coef and quant must be 16-byte aligned, out 8-byte aligned";
        if (p.blocks_w < 1 || p.blocks_h < 1 || p.blocks_w > 32768 || p.blocks_h > 32768) return "jpeg_idct: need 1 <= blocks_w, blocks_h <= 32768";
        if (p.first_block != total) return "jpeg_idct: first_block must be the running count of the blocks of the planes before";
        total += (long)p.blocks_w * p.blocks_h;
        if (total >= (1L << 31) - 32) return "jpeg_idct: 2^31 blocks or more";
    }
    return nullptr;
}

int jpeg_idct_launch(const mi355_jpeg_plane *table_dev, const mi355_jpeg_plane *table_host, int nplanes, hipStream_t st)
{
    const mi355_jpeg_plane &last = table_host[nplanes - 1];
    const long total = last.first_block + (long)last.blocks_w * last.blocks_h;
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)((total + 31) / 32)), dim3(256), 0, st, table_dev, nplanes, (int)total);
    return hipGetLastError() == hipSuccess ? MI355_OK : MI355_EHIP;
}

// ---- upsampling + colour -----------------------------------------------------------------------------------------------------------
// The sample of component c at output pixel (x, y), w_lores = ceil(w / hs): stb's resampler of the component's (hs, vs) as a function
// of the pixel.  Its row walk (:3630-3644) reduces to: vs == 2 -> near = y >> 1, far = the row below for an odd y, above for an even
// one, clamped to the component's rows; nearest resampler -> row y / vs.
__device__ static inline int jpeg_sample(const mi355_jpeg_component &c, int w_lores, int x, int y)
{
    const uint8_t *base = c.plane;
    const size_t pitch = (size_t)c.pitch;
    if (c.hs == 1 && c.vs == 1) return base[y * pitch + x];
    if (c.vs == 2 && c.hs <= 2) {
        const int ny = y >> 1;
        int fy = (y & 1) ? ny + 1 : ny - 1;
        fy = fy < 0 ? 0 : (fy > c.rows - 1 ? c.rows - 1 : fy);
        const uint8_t *near = base + ny * pitch, *far = base + fy * pitch;
        if (c.hs == 1) return (3 * near[x] + far[x] + 2) >> 2;
        // (2, 2): t(i) = 3 near[i] + far[i], then 3 : 1 between neighbours; the row's first and last pixel take one sample
        const int w = w_lores;
        if (w == 1 || x == 0) return (3 * near[0] + far[0] + 2) >> 2;
        if (x == 2 * w - 1) return (3 * near[w - 1] + far[w - 1] + 2) >> 2;
        const int i = (x + 1) >> 1;  // the pair (i - 1, i) serves pixels 2 i - 1 and 2 i
        const int t0 = 3 * near[i - 1] + far[i - 1], t1 = 3 * near[i] + far[i];
        return (x & 1) ? (3 * t0 + t1 + 8) >> 4 : (3 * t1 + t0 + 8) >> 4;
    }
    if (c.hs == 2 && c.vs == 1) {
        const uint8_t *in = base + y * pitch;
        const int w = w_lores, i = x >> 1;
        if (w == 1 || x == 0) return in[0];
        if (x == 2 * w - 1) return in[w - 1];
        if (x == 2 * w - 2) return (3 * in[w - 2] + in[w - 1] + 2) >> 2;  // stb's last pair weighs the sample before the last (:3202)
        return (x & 1) ? (3 * in[i] + in[i + 1] + 2) >> 2 : (3 * in[i] + in[i - 1] + 2) >> 2;
    }
    return base[(size_t)(y / c.vs) * pitch + x / c.hs];
}

// grid: (workgroups of the largest image, B).  A thread owns four neighbouring x of one row: 12 bytes of interleaved RGB, three 4-byte
// stores where the position is 4-byte aligned and whole, single bytes otherwise.
__global__ __launch_bounds__(256) void jpeg_to_rgb_kernel(const mi355_jpeg_image *table)
{
    const mi355_jpeg_image &im = table[blockIdx.y];
    const int w = im.w, h = im.h, wq = (w + 3) >> 2;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= h * wq) return;
    const int y = t / wq, x0 = (t - y * wq) * 4;
    const int ncomp = im.mode == MI355_JPEG_GREY ? 1 : 3;
    int wl[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) wl[k] = k < ncomp ? (w + im.comp[k].hs - 1) / im.comp[k].hs : 0;
    uint8_t px[12];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int x = x0 + j < w ? x0 + j : w - 1;
        int s[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) s[k] = k < ncomp ? jpeg_sample(im.comp[k], wl[k], x, y) : 0;
        int rr, gg, bb;
        if (im.mode == MI355_JPEG_YCBCR) {  // (int)(c * 4096.0f + 0.5f) << 8 of 1.402, 0.71414, 0.34414, 1.772
            const int yf = (s[0] << 20) + (1 << 19), cb = s[1] - 128, cr = s[2] - 128;
            rr = (yf + cr * 1470208) >> 20;
            gg = (yf + cr * -748800 + (int)((uint32_t)(cb * -360960) & 0xffff0000u)) >> 20;
            bb = (yf + cb * 1858048) >> 20;
            rr = rr < 0 ? 0 : (rr > 255 ? 255 : rr);
            gg = gg < 0 ? 0 : (gg > 255 ? 255 : gg);
            bb = bb < 0 ? 0 : (bb > 255 ? 255 : bb);
        } else if (im.mode == MI355_JPEG_RGB) {
            rr = s[0]; gg = s[1]; bb = s[2];
        } else {
            rr = gg = bb = s[0];
        }
        px[3 * j] = (uint8_t)rr; px[3 * j + 1] = (uint8_t)gg; px[3 * j + 2] = (uint8_t)bb;
    }
    uint8_t *o = im.rgb + (size_t)y * im.pitch + 3 * (size_t)x0;
    if (x0 + 3 < w && (reinterpret_cast<size_t>(o) & 3) == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k)
            reinterpret_cast<uint32_t *>(o)[k] = px[4 * k] | (uint32_t)px[4 * k + 1] << 8 | (uint32_t)px[4 * k + 2] << 16 | (uint32_t)px[4 * k + 3] << 24;
    } else {
        const int n = 3 * (w - x0 < 4 ? w - x0 : 4);
        for (int k = 0; k < n; ++k) o[k] = px[k];
    }
}

const char *jpeg_to_rgb_check(const mi355_jpeg_image *host, int B)
{
    if (!host || B < 1 || B > 65535) return "jpeg_to_rgb: null table / need 1 <= B <= 65535";
    for (int b = 0; b < B; ++b) {
        const mi355_jpeg_image &im = host[b];
        if (!im.rgb) return "jpeg_to_rgb: null frame pointer";
        if (im.w < 1 || im.h < 1 || im.w > 32768 || im.h > 32768) return "jpeg_to_rgb: need 1 <= w, h <= 32768 for every image";
        if (im.pitch < 3 * im.w) return "jpeg_to_rgb: pitch < 3 * w";
        if (im.mode < MI355_JPEG_YCBCR || im.mode > MI355_JPEG_GREY) return "jpeg_to_rgb: unknown mode (MI355_JPEG_YCBCR .. _GREY)";
        for (int k = 0; k < (im.mode == MI355_JPEG_GREY ? 1 : 3); ++k) {
            const mi355_jpeg_component &c = im.comp[k];
            if (!c.plane) return "jpeg_to_rgb: null plane pointer";
            if (c.hs < 1 || c.hs > 4 || c.vs < 1 || c.vs > 4) return "jpeg_to_rgb: need 1 <= hs, vs <= 4";
            if (c.rows < (im.h + c.vs - 1) / c.vs) return "jpeg_to_rgb: a component has fewer than ceil(h / vs) rows";
            if (c.pitch < (im.w + c.hs - 1) / c.hs) return "jpeg_to_rgb: a component's pitch is below ceil(w / hs)";
        }
    }
    return nullptr;
}

int jpeg_to_rgb_launch(const mi355_jpeg_image *table_dev, const mi355_jpeg_image *table_host, int B, hipStream_t st)
{
    long most = 0;
    for (int b = 0; b < B; ++b) {
        const long threads = (long)table_host[b].h * ((table_host[b].w + 3) / 4);
        if (threads > most) most = threads;
    }
    hipLaunchKernelGGL(jpeg_to_rgb_kernel, dim3((unsigned)((most + 255) / 256), B), dim3(256), 0, st, table_dev);
    return hipGetLastError() == hipSuccess ? MI355_OK : MI355_EHIP;
}
