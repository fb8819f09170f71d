// frames.hip -- the batched input path for 8-bit interleaved frames (mi355_frames_u8_letterbox_minmax / _quantize): letterbox_image
// (ref: src/image.c:812-831) + the layer-0 quantiser (ref: src/blas.c:108-168) straight from the decoder's bytes, one launch per pass
// for the whole batch, no float image in memory.  Pass 1 reduces min / max of the letterboxed floats per image, the host derives
// (scale, zero point), pass 2 recomputes the same floats and stores the quantised planar bytes.
//
// Every float is the one letterbox_kernel (glue.hip) computes from load_image_color's planes (ref: src/image.c:1386, byte / 255.):
// the same expressions, each product and sum rounded on its own (-ffp-contract=off), the 0.5 fill, last column = the source's last
// column, last row = first term only.  The quantiser is image_quantize_per_image_kernel's expression, min / max reduce with
// image_minmax_batched_kernel's seeds, comparisons and atomics.
#include "kargs.h"

// letterbox_launch's geometry (glue.hip), shared by the host-side validation and the kernels: one function compiled for both sides, so
// the device walks exactly the rectangle the host checked.  false: the frame is refused.
struct FrameGeo {
    int new_w, new_h, ox, oy;
    float w_scale, h_scale;
};

__host__ __device__ static inline bool frame_geometry(int imw, int imh, int w, int h, FrameGeo &g)
{
    if (((float)w / imw) < ((float)h / imh)) { g.new_w = w; g.new_h = (imh * w) / imw; }
    else { g.new_h = h; g.new_w = (imw * h) / imh; }
    if (g.new_w < 2 || g.new_h < 2) return false;  // the reference divides by (w - 1), (h - 1)
    g.w_scale = (float)(imw - 1) / (g.new_w - 1);
    g.h_scale = (float)(imh - 1) / (g.new_h - 1);
    // (int)(r * h_scale) must stay a row of the source image (the reference asserts it), ix + 1 a column
    if ((int)((g.new_h - 1) * g.h_scale) > imh - 1 || (int)((g.new_h - 2) * g.h_scale) + 1 > imh - 1 ||
        (int)((g.new_w - 2) * g.w_scale) + 1 > imw - 1)
        return false;
    g.ox = (w - g.new_w) / 2;
    g.oy = (h - g.new_h) / 2;
    return true;
}

// byte -> float of load_image_color, one table per workgroup (256 threads, one entry each): (float)byte / 255.f
__device__ static inline void fill_byte_lut(float *lut)
{
    lut[threadIdx.x] = (float)threadIdx.x / 255.f;
    __syncthreads();
}

// the three letterboxed floats (planes 0, 1, 2) of output pixel (x, y)
__device__ static inline void letterbox_px3(const mi355_frame_u8 &f, const FrameGeo &g, const float *lut, int x, int y, float v[3])
{
    const int xx = x - g.ox, r = y - g.oy;
    if (xx < 0 || xx >= g.new_w || r < 0 || r >= g.new_h) {
        v[0] = v[1] = v[2] = .5f;
        return;
    }
    const bool last_x = xx == g.new_w - 1 || f.w == 1, last_y = r == g.new_h - 1 || f.h == 1;
    int ix = f.w - 1;
    float dx = 0.f;
    if (!last_x) {
        const float sx = xx * g.w_scale;
        ix = (int)sx;
        dx = sx - ix;
    }
    const float sy = r * g.h_scale;
    const int iy = (int)sy;
    const float dy = sy - iy;
    const uint8_t *row0 = f.data + (size_t)iy * f.pitch + 3 * (size_t)ix;
    const uint8_t *row1 = row0 + f.pitch;  // only read when !last_y
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int o = f.order == MI355_FRAME_BGR ? 2 - k : k;
        const float a = last_x ? lut[row0[o]] : (1 - dx) * lut[row0[o]] + dx * lut[row0[3 + o]];
        float val = (1 - dy) * a;
        if (!last_y) {
            const float b = last_x ? lut[row1[o]] : (1 - dx) * lut[row1[o]] + dx * lut[row1[3 + o]];
            val += dy * b;
        }
        v[k] = val;
    }
}

// grid: (workgroups per image, B).  mm[2 b] = max(x, +0), mm[2 b + 1] = min(x, -0) as in image_minmax_batched_kernel (seeded before)
__global__ __launch_bounds__(256) void frames_u8_letterbox_minmax_kernel(const mi355_frame_u8 *table, int w, int h, uint32_t *mm)
{
    __shared__ float lut[256];
    fill_byte_lut(lut);
    const mi355_frame_u8 f = table[blockIdx.y];
    uint32_t *mi = mm + 2 * (size_t)blockIdx.y;
    FrameGeo g;
    frame_geometry(f.w, f.h, w, h, g);  // checked by the launcher
    float mx = 0.0f, mn = 0.0f;
    const int hw = h * w;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < hw; i += gridDim.x * blockDim.x) {
        float v[3];
        letterbox_px3(f, g, lut, i % w, i / w, v);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            mx = v[k] > mx ? v[k] : mx;
            mn = v[k] < mn ? v[k] : mn;
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const float omx = __shfl_xor(mx, m), omn = __shfl_xor(mn, m);
        mx = omx > mx ? omx : mx;
        mn = omn < mn ? omn : mn;
    }
    if ((threadIdx.x & 63) == 0) {
        if (mx > 0.0f) atomicMax(reinterpret_cast<int *>(mi), __float_as_int(mx));
        if (mn < 0.0f) atomicMax(mi + 1, (uint32_t)__float_as_int(mn));
    }
}

// grid: (workgroups per image, B); a thread serves four neighbouring x of one row in all three planes: one 4-byte store per plane
// where the row position is 4-byte aligned, single bytes otherwise (w % 4 != 0: every other row, and the tail of each row)
__global__ __launch_bounds__(256) void frames_u8_letterbox_quantize_kernel(const mi355_frame_u8 *table, int w, int h,
                                                                           const float *scale_dev, const uint8_t *zp_dev, uint8_t *out)
{
    __shared__ float lut[256];
    fill_byte_lut(lut);
    const int wq = (w + 3) / 4;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < h * wq) {
        const mi355_frame_u8 f = table[blockIdx.y];
        FrameGeo g;
        frame_geometry(f.w, f.h, w, h, g);  // checked by the launcher
        const float scale = scale_dev[blockIdx.y];
        const int zp = zp_dev[blockIdx.y];
        const int y = t / wq, x0 = (t % wq) * 4;
        uint32_t packed[3] = {0, 0, 0};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (x0 + j >= w) break;
            float v[3];
            letterbox_px3(f, g, lut, x0 + j, y, v);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float q_f = (float)(round((double)(v[k] / scale)) + (double)zp);  // ref: src/blas.c:160-165
                const int q = (int)q_f;
                packed[k] |= (uint32_t)(q < 0 ? 0 : (q > 255 ? 255 : q)) << (8 * j);
            }
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            uint8_t *o = out + (((size_t)blockIdx.y * 3 + k) * h + y) * w + x0;
            if (x0 + 3 < w && (reinterpret_cast<size_t>(o) & 3) == 0) {
                *reinterpret_cast<uint32_t *>(o) = packed[k];
            } else {
                for (int j = 0; j < 4 && x0 + j < w; ++j) o[j] = (uint8_t)(packed[k] >> (8 * j));
            }
        }
    }
}

// Host-side check of the table's host mirror, before anything is launched: NULL when every frame can be served, else what is wrong.
const char *frames_u8_check(const mi355_frame_u8 *host, int B, int w, int h)
{
    if (!host || B <= 0 || B > 65535) return "frames_u8: null table / need 1 <= B <= 65535";
    if (w < 2 || h < 2 || w > 32768 || h > 32768) return "frames_u8: need 2 <= w, h <= 32768 for the network input";
    for (int b = 0; b < B; ++b) {
        const mi355_frame_u8 &f = host[b];
        if (!f.data) return "frames_u8: null frame pointer";
        if (f.w < 1 || f.h < 1 || f.w > 32768 || f.h > 32768) return "frames_u8: need 1 <= w, h <= 32768 for every frame";
        if (f.pitch < 3 * f.w) return "frames_u8: pitch < 3 * w";
        if (f.order != MI355_FRAME_RGB && f.order != MI355_FRAME_BGR) return "frames_u8: channel order must be MI355_FRAME_RGB or MI355_FRAME_BGR";
        FrameGeo g;
        if (!frame_geometry(f.w, f.h, w, h, g)) return "frames_u8: degenerate aspect (resized side < 2)";
    }
    return nullptr;
}

int frames_u8_letterbox_minmax_launch(const mi355_frame_u8 *table_dev, int B, int w, int h, uint32_t *mm, hipStream_t st)
{
    if (image_minmax_seed_launch(mm, B, st) != MI355_OK) return MI355_EHIP;
    const long want = ((long)h * w + 255) / 256;
    // about 2048 workgroups in all, at least one per image (image_minmax_batched_launch's sizing)
    const long cap = 2048 / B > 0 ? 2048 / B : 1;
    const int gx = (int)(want < cap ? want : cap);
    hipLaunchKernelGGL(frames_u8_letterbox_minmax_kernel, dim3(gx, B), dim3(256), 0, st, table_dev, w, h, mm);
    return hipGetLastError() == hipSuccess ? MI355_OK : MI355_EHIP;
}

int frames_u8_letterbox_quantize_launch(const mi355_frame_u8 *table_dev, int B, int w, int h, const float *scale_dev,
                                        const uint8_t *zp_dev, uint8_t *out, hipStream_t st)
{
    const long threads = (long)h * ((w + 3) / 4);
    hipLaunchKernelGGL(frames_u8_letterbox_quantize_kernel, dim3((unsigned)((threads + 255) / 256), B), dim3(256), 0, st, table_dev, w, h,
                       scale_dev, zp_dev, out);
    return hipGetLastError() == hipSuccess ? MI355_OK : MI355_EHIP;
}
