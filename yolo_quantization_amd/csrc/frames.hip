// frames.hip -- the batched input path for 8-bit frames: letterbox_image (ref: src/image.c:812-831) + the layer-0 quantiser (ref:
// src/blas.c:108-168) straight from the decoder's bytes, one launch per pass for the whole batch, no float image in memory.  Pass 1
// reduces min / max of the letterboxed floats per image, the host derives (scale, zero point), pass 2 recomputes the same floats and
// stores the quantised planar bytes.
//
// Every float is the one letterbox_kernel (glue.hip) computes from load_image_color's planes (ref: src/image.c:1386, byte / 255.):
// the same expressions, each product and sum rounded on its own (-ffp-contract=off), the 0.5 fill, last column = the source's last
// column, last row = first term only.  The quantiser is image_quantize_per_image_kernel's expression, min / max reduce with
// image_minmax_batched_kernel's seeds, comparisons and atomics.
//
// One path for every kind of frames.  A kind is a Source: it names its table entry of the C-ABI (Frame), its prefix in refusals (name),
// the refusals that are its own (check_pointers, check), and hands the kernels the bytes of a pixel's taps (taps).  The two kernels,
// the host-side check and the two launchers are templates over the Source, instantiated at the end of the file for
//   SourceU8      interleaved RGB / BGR (mi355_frames_u8_*): the bytes as they are;
//   SourceYUV     NV12 / NV21 (mi355_frames_yuv_*): the bytes of a source pixel are converted from (Y, U, V) in registers at every
//                 bilinear tap, with the integer formulas of the header (mi355_frame_yuv); no RGB frame is written anywhere;
//   SourcePlanar  three separate planes (mi355_frames_planar_*: I420, YV12, I422, I444, planar RGB / BGR): the YUV formats share the
//                 NV12 source's tap walk and arithmetic with their own chroma shifts, the RGB formats take their bytes as they are;
//   SourcePacked  one plane of four bytes per pixel (RGBA, BGRA, ARGB, ABGR) or per two pixels (YUYV, UYVY, YVYU)
//                 (mi355_frames_packed_*): the RGB formats pick three of a pixel's four bytes, the 4:2:2 formats are I422 with luma and
//                 chroma of a macropixel in one 4-byte group: one 4-byte load per row and macropixel the taps touch;
//   SourceP010    NV12 with 16-bit little-endian samples (mi355_frames_p010_*: P010, P012, P016): the high byte of every sample is
//                 the NV12 byte (truncation), loaded on its own;
//   SourceBayer   one plane of raw sensor samples (mi355_frames_bayer_*: 8-bit, 16-bit, CSI-2 RAW10 / RAW12; RGGB, BGGR, GRBG, GBRG or
//                 no mosaic): toned through the frame's optional tables and demosaiced bilinearly in registers at every tap.
// A slot may look at its frame through a view (mi355_frame_view: a rectangle under an EXIF orientation): Viewed<Source> wraps any of the
// six and is a Source itself (mi355_frames_*_view_*); its kernels, check and launchers are compiled from this file by frames_view.hip.
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
    // (int)(r * h_scale) must stay a row of the source image (the reference asserts it), and so must row iy + 1 and column ix + 1 where
    // letterbox_px3 reads them: a one-row / one-column frame never does (its f.h == 1 / f.w == 1 clauses, letterbox_launch's guards)
    if ((int)((g.new_h - 1) * g.h_scale) > imh - 1 || (imh > 1 && (int)((g.new_h - 2) * g.h_scale) + 1 > imh - 1) ||
        (imw > 1 && (int)((g.new_w - 2) * g.w_scale) + 1 > imw - 1))
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

// A source gives the kernels the bytes of the up to four taps of one output pixel: taps(ix, iy, two_x, two_y, p) fills p[dy][dx][k]
// with byte k (plane k) of source pixel (ix + dx, iy + dy); column 1 only when two_x, row 1 only when two_y (the launcher's geometry
// check keeps ix + 1 and iy + 1 inside the frame then).
struct SourceU8 {
    using Frame = mi355_frame_u8;
    static constexpr const char *name = "frames_u8";
    static const char *check_pointers(const Frame &f) { return f.data ? nullptr : "null frame pointer"; }
    static const char *check(const Frame &f)
    {
        if (f.pitch < 3 * f.w) return "pitch < 3 * w";
        if (f.order != MI355_FRAME_RGB && f.order != MI355_FRAME_BGR) return "channel order must be MI355_FRAME_RGB or MI355_FRAME_BGR";
        return nullptr;
    }
    const uint8_t *data;
    int w, h, pitch, o0, o2;  // byte offsets of planes 0 and 2 inside a pixel (plane 1 is byte 1 in both orders)
    __device__ explicit SourceU8(const mi355_frame_u8 &f)
        : data(f.data), w(f.w), h(f.h), pitch(f.pitch), o0(f.order == MI355_FRAME_BGR ? 2 : 0), o2(f.order == MI355_FRAME_BGR ? 0 : 2) {}
    __device__ void taps(int ix, int iy, bool two_x, bool two_y, uint8_t p[2][2][3]) const
    {
        const uint8_t *row = data + (size_t)iy * pitch + 3 * (size_t)ix;
#pragma unroll
        for (int r = 0; r < 2; ++r, row += pitch) {
            if (r == 1 && !two_y) break;
            p[r][0][0] = row[o0]; p[r][0][1] = row[1]; p[r][0][2] = row[o2];
            if (two_x) { p[r][1][0] = row[3 + o0]; p[r][1][1] = row[4]; p[r][1][2] = row[3 + o2]; }
        }
    }
};

// (yoff, cy, crv, cgu, cgv, cbu) of MI355_YUV_BT601, _BT601_FULL, _BT709, _BT709_FULL: round(x * 65536) of the standards' coefficients
static __constant__ int yuv_matrix[4][6] = {{16, 76309, 104597, 25675, 53279, 132201},
                                            {0, 65536, 91881, 22553, 46802, 116130},
                                            {16, 76309, 117489, 13975, 34925, 138438},
                                            {0, 65536, 103206, 12276, 30679, 121609}};

// The frame's matrix: uniform over the workgroup, read once from the constant table
struct YuvMatrix {
    int yoff, cy, crv, cgu, cgv, cbu;
    __device__ explicit YuvMatrix(int id)
    {
        const int *m = yuv_matrix[id];
        yoff = m[0]; cy = m[1]; crv = m[2]; cgu = m[3]; cgv = m[4]; cbu = m[5];
    }
};

__device__ static inline void copy3(int d[3], const int a[3]) { d[0] = a[0]; d[1] = a[1]; d[2] = a[2]; }
__device__ static inline uint8_t clamp8(int x) { return (uint8_t)(x < 0 ? 0 : (x > 255 ? 255 : x)); }

// the three chroma terms of one (U, V) sample: what R, G and B add to the luma term, the rounding constant included
__device__ static inline void yuv_chroma_terms(const YuvMatrix &m, int ub, int vb, int t[3])
{
    const int u = ub - 128, v = vb - 128;
    t[0] = m.crv * v + 32768;
    t[1] = 32768 - m.cgu * u - m.cgv * v;
    t[2] = m.cbu * u + 32768;
}

// int32 throughout, >> is the arithmetic shift; |luma term| < 2^25 and |chroma term| < 2^25: no overflow
__device__ static inline void yuv_rgb(const YuvMatrix &m, int luma, const int t[3], uint8_t out[3])
{
    const int yy = m.cy * (luma - m.yoff);
#pragma unroll
    for (int k = 0; k < 3; ++k) out[k] = clamp8((yy + t[k]) >> 16);
}

// The taps of a YUV source whose chroma sample of pixel (x, y) lies at (x >> sx, y >> sy), sx, sy in {0, 1}.  Columns ix, ix + 1 share
// a sample when sx = 1 and ix is even, rows iy, iy + 1 when sy = 1 and iy is even: a sample is loaded once; with a shift of 0 the
// neighbouring tap always has its own.  Src: m, pitch_y, luma_at(x, y), the address of the luma byte of pixel (x, y), luma_step, the
// bytes from there to the next pixel's, and chroma(cx, cy, t), the terms of the sample at (cx, cy).
template <class Src>
__device__ static inline void yuv_taps(const Src &s, int sx, int sy, int ix, int iy, bool two_x, bool two_y, uint8_t p[2][2][3])
{
    const bool next_cx = two_x && (ix & sx) == sx, next_cy = two_y && (iy & sy) == sy;
    const int cx = ix >> sx, cyy = iy >> sy;
    int t[2][2][3];
    s.chroma(cx, cyy, t[0][0]);
    if (next_cx) s.chroma(cx + 1, cyy, t[0][1]);
    else copy3(t[0][1], t[0][0]);
    if (next_cy) {
        s.chroma(cx, cyy + 1, t[1][0]);
        if (next_cx) s.chroma(cx + 1, cyy + 1, t[1][1]);
        else copy3(t[1][1], t[1][0]);
    } else {
        copy3(t[1][0], t[0][0]);
        copy3(t[1][1], t[0][1]);
    }
    const uint8_t *row = s.luma_at(ix, iy);
#pragma unroll
    for (int r = 0; r < 2; ++r, row += s.pitch_y) {
        if (r == 1 && !two_y) break;
        yuv_rgb(s.m, row[0], t[r][0], p[r][0]);
        if (two_x) yuv_rgb(s.m, row[Src::luma_step], t[r][1], p[r][1]);
    }
}

struct SourceYUV {
    using Frame = mi355_frame_yuv;
    static constexpr const char *name = "frames_yuv";
    static const char *check_pointers(const Frame &f) { return f.y && f.uv ? nullptr : "null plane pointer"; }
    static const char *check(const Frame &f)
    {
        if (f.pitch_y < f.w) return "pitch_y < w";
        if (f.pitch_uv < 2 * ((f.w + 1) / 2)) return "pitch_uv < 2 * ((w + 1) / 2)";
        if (f.layout != MI355_YUV_NV12 && f.layout != MI355_YUV_NV21) return "layout must be MI355_YUV_NV12 or MI355_YUV_NV21";
        if (f.matrix < MI355_YUV_BT601 || f.matrix > MI355_YUV_BT709_FULL) return "unknown matrix (MI355_YUV_BT601 .. _BT709_FULL)";
        return nullptr;
    }
    const uint8_t *y, *uv;
    int w, h, pitch_y, pitch_uv;
    int iu, iv;        // position of U and V inside a chroma pair: (0, 1) NV12, (1, 0) NV21
    bool pair_aligned; // every chroma pair starts at an even address: one 2-byte load serves it
    YuvMatrix m;
    __device__ explicit SourceYUV(const mi355_frame_yuv &f)
        : y(f.y), uv(f.uv), w(f.w), h(f.h), pitch_y(f.pitch_y), pitch_uv(f.pitch_uv), iu(f.layout == MI355_YUV_NV21 ? 1 : 0),
          iv(f.layout == MI355_YUV_NV21 ? 0 : 1), pair_aligned(((reinterpret_cast<size_t>(f.uv) | (size_t)f.pitch_uv) & 1) == 0),
          m(f.matrix) {}
    static constexpr int luma_step = 1;
    __device__ const uint8_t *luma_at(int x, int yy) const { return y + (size_t)yy * pitch_y + x; }
    // the chroma terms of the pair at (cx, cy)
    __device__ void chroma(int cx, int cyy, int t[3]) const
    {
        const uint8_t *p = uv + (size_t)cyy * pitch_uv + 2 * (size_t)cx;
        int b[2];
        if (pair_aligned) {
            const uint32_t two = *reinterpret_cast<const uint16_t *>(p);
            b[0] = (int)(two & 255); b[1] = (int)(two >> 8);
        } else {
            b[0] = p[0]; b[1] = p[1];
        }
        yuv_chroma_terms(m, b[iu], b[iv], t);
    }
    __device__ void taps(int ix, int iy, bool two_x, bool two_y, uint8_t p[2][2][3]) const { yuv_taps(*this, 1, 1, ix, iy, two_x, two_y, p); }
};

// Three separate planes (mi355_frame_planar).  YUV formats: y = plane Y, u / v the chroma planes whichever order the format names
// them in, sampled at (x >> sx, y >> sy).  RGB formats: y, u, v hold the planes of R, G, B and their bytes are the pixel's.  The
// format is uniform over the workgroup, so its branches do not diverge.
struct SourcePlanar {
    using Frame = mi355_frame_planar;
    static constexpr const char *name = "frames_planar";
    static const char *check_pointers(const Frame &f) { return f.plane[0] && f.plane[1] && f.plane[2] ? nullptr : "null plane pointer"; }
    static const char *check(const Frame &f)
    {
        if (f.format < MI355_PLANAR_I420 || f.format > MI355_PLANAR_BGR) return "unknown format (MI355_PLANAR_I420 .. _BGR)";
        if (f.matrix < MI355_YUV_BT601 || f.matrix > MI355_YUV_BT709_FULL) return "unknown matrix (MI355_YUV_BT601 .. _BT709_FULL)";
        const bool rgb = f.format == MI355_PLANAR_RGB || f.format == MI355_PLANAR_BGR;
        if (rgb && f.matrix != 0) return "matrix must be 0 with MI355_PLANAR_RGB / _BGR";
        const int cw = rgb || f.format == MI355_PLANAR_I444 ? f.w : (f.w + 1) / 2;  // the width of planes 1 and 2
        if (f.pitch[0] < f.w) return "pitch[0] < w";
        if (f.pitch[1] < cw || f.pitch[2] < cw) return "pitch[1] or pitch[2] below the width of its plane";
        return nullptr;
    }
    const uint8_t *y, *u, *v;
    int w, h, pitch_y, pitch_u, pitch_v;
    int sx, sy;
    bool rgb;
    YuvMatrix m;
    __device__ explicit SourcePlanar(const mi355_frame_planar &f)
        : w(f.w), h(f.h), sx(f.format == MI355_PLANAR_I420 || f.format == MI355_PLANAR_YV12 || f.format == MI355_PLANAR_I422 ? 1 : 0),
          sy(f.format == MI355_PLANAR_I420 || f.format == MI355_PLANAR_YV12 ? 1 : 0),
          rgb(f.format == MI355_PLANAR_RGB || f.format == MI355_PLANAR_BGR), m(f.matrix)
    {
        // the plane that serves (y | R), (u | G), (v | B): YV12 names V before U, BGR names B first
        const int iy = f.format == MI355_PLANAR_BGR ? 2 : 0, iv = f.format == MI355_PLANAR_YV12 ? 1 : (f.format == MI355_PLANAR_BGR ? 0 : 2);
        const int iu = 3 - iy - iv;
        y = f.plane[iy]; pitch_y = f.pitch[iy];
        u = f.plane[iu]; pitch_u = f.pitch[iu];
        v = f.plane[iv]; pitch_v = f.pitch[iv];
    }
    static constexpr int luma_step = 1;
    __device__ const uint8_t *luma_at(int x, int yy) const { return y + (size_t)yy * pitch_y + x; }
    // the chroma terms of the sample at (cx, cy): one byte from each chroma plane
    __device__ void chroma(int cx, int cyy, int t[3]) const
    {
        yuv_chroma_terms(m, u[(size_t)cyy * pitch_u + cx], v[(size_t)cyy * pitch_v + cx], t);
    }
    __device__ void taps(int ix, int iy, bool two_x, bool two_y, uint8_t p[2][2][3]) const
    {
        if (!rgb) {
            yuv_taps(*this, sx, sy, ix, iy, two_x, two_y, p);
            return;
        }
        const uint8_t *row[3] = {y + (size_t)iy * pitch_y + ix, u + (size_t)iy * pitch_u + ix, v + (size_t)iy * pitch_v + ix};
        const int pitch[3] = {pitch_y, pitch_u, pitch_v};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            p[0][0][k] = row[k][0];
            if (two_x) p[0][1][k] = row[k][1];
            if (two_y) {
                p[1][0][k] = row[k][pitch[k]];
                if (two_x) p[1][1][k] = row[k][pitch[k] + 1];
            }
        }
    }
};

// One plane of 4-byte groups (mi355_frame_packed): a group is a pixel of the RGB formats (planes 0, 1, 2 = R, G, B pick three of its
// bytes, the fourth is never looked at) and a macropixel of two pixels in the 4:2:2 formats, which are I422 (chroma at (x >> 1, y))
// with luma and chroma of a macropixel side by side.  A group is always one 4-byte load, whatever the frame's address and pitch: the
// load is declared unaligned and gfx950 serves unaligned global loads (hipcc merges four byte loads into this very instruction, so a
// byte-wise path for frames that are not 4-byte aligned would compile to the same code).  The format is uniform over the workgroup,
// so its branches do not diverge.
struct SourcePacked {
    using Frame = mi355_frame_packed;
    static constexpr const char *name = "frames_packed";
    static const char *check_pointers(const Frame &f) { return f.data ? nullptr : "null frame pointer"; }
    static const char *check(const Frame &f)
    {
        if (f.format < MI355_PACKED_RGBA || f.format > MI355_PACKED_YVYU) return "unknown format (MI355_PACKED_RGBA .. _YVYU)";
        if (f.matrix < MI355_YUV_BT601 || f.matrix > MI355_YUV_BT709_FULL) return "unknown matrix (MI355_YUV_BT601 .. _BT709_FULL)";
        const bool rgb = f.format <= MI355_PACKED_ABGR;
        if (rgb && f.matrix != 0) return "matrix must be 0 with MI355_PACKED_RGBA / _BGRA / _ARGB / _ABGR";
        if (rgb && f.pitch < 4 * f.w) return "pitch < 4 * w";
        if (!rgb && f.pitch < 4 * ((f.w + 1) / 2)) return "pitch < 4 * ((w + 1) / 2)";
        return nullptr;
    }
    const uint8_t *data;
    int w, h, pitch;
    int s0, s1, s2;  // bit positions inside a group (byte k in bits 8 k): of R, G, B, or of Y0, U, V (Y1 lies 16 bits above Y0)
    bool rgb;
    YuvMatrix m;
    __device__ explicit SourcePacked(const mi355_frame_packed &f)
        : data(f.data), w(f.w), h(f.h), pitch(f.pitch), rgb(f.format <= MI355_PACKED_ABGR), m(f.matrix)
    {
        // byte positions of (R, G, B) / (Y0, U, V) by format
        const int pos[7][3] = {{0, 1, 2}, {2, 1, 0}, {1, 2, 3}, {3, 2, 1}, {0, 1, 3}, {1, 0, 2}, {0, 3, 1}};
        s0 = 8 * pos[f.format][0]; s1 = 8 * pos[f.format][1]; s2 = 8 * pos[f.format][2];
    }
    // the four bytes of group gx of row yy, byte k in bits 8 k: one load at any alignment
    __device__ uint32_t group(int gx, int yy) const
    {
        uint32_t g;
        __builtin_memcpy(&g, data + (size_t)yy * pitch + 4 * (size_t)gx, 4);
        return g;
    }
    // 4:2:2: the RGB bytes of pixel x from its macropixel g (group x >> 1): Y[x & 1] and the macropixel's (U, V)
    __device__ void pixel422(uint32_t g, int x, uint8_t out[3]) const
    {
        int t[3];
        yuv_chroma_terms(m, (int)(g >> s1 & 255), (int)(g >> s2 & 255), t);
        yuv_rgb(m, (int)(g >> (s0 + 16 * (x & 1)) & 255), t, out);
    }
    __device__ void taps(int ix, int iy, bool two_x, bool two_y, uint8_t p[2][2][3]) const
    {
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            if (r == 1 && !two_y) break;
            if (rgb) {
                const uint32_t g = group(ix, iy + r);
                p[r][0][0] = (uint8_t)(g >> s0); p[r][0][1] = (uint8_t)(g >> s1); p[r][0][2] = (uint8_t)(g >> s2);
                if (two_x) {
                    const uint32_t g1 = group(ix + 1, iy + r);
                    p[r][1][0] = (uint8_t)(g1 >> s0); p[r][1][1] = (uint8_t)(g1 >> s1); p[r][1][2] = (uint8_t)(g1 >> s2);
                }
            } else {  // one load per row serves both taps of an even ix; an odd ix + 1 opens the next macropixel
                const uint32_t g = group(ix >> 1, iy + r);
                pixel422(g, ix, p[r][0]);
                if (two_x) pixel422((ix & 1) ? group((ix >> 1) + 1, iy + r) : g, ix + 1, p[r][1]);
            }
        }
    }
};

// NV12 with 16-bit little-endian samples, the significant bits at the top (mi355_frame_p010: P010, P012, P016).  The byte the NV12
// source would read is the sample's high byte -- truncation, not rounding --, a single byte load at any alignment; the low bytes are
// never loaded.
struct SourceP010 {
    using Frame = mi355_frame_p010;
    static constexpr const char *name = "frames_p010";
    static const char *check_pointers(const Frame &f) { return f.y && f.uv ? nullptr : "null plane pointer"; }
    static const char *check(const Frame &f)
    {
        if (f.pitch_y < 2 * f.w) return "pitch_y < 2 * w";
        if (f.pitch_uv < 4 * ((f.w + 1) / 2)) return "pitch_uv < 4 * ((w + 1) / 2)";
        if (f.layout != 0 || f.reserved[0] != 0 || f.reserved[1] != 0) return "layout and reserved must be 0";
        if (f.matrix < MI355_YUV_BT601 || f.matrix > MI355_YUV_BT709_FULL) return "unknown matrix (MI355_YUV_BT601 .. _BT709_FULL)";
        return nullptr;
    }
    const uint8_t *y, *uv;
    int w, h, pitch_y, pitch_uv;
    YuvMatrix m;
    __device__ explicit SourceP010(const mi355_frame_p010 &f)
        : y(f.y), uv(f.uv), w(f.w), h(f.h), pitch_y(f.pitch_y), pitch_uv(f.pitch_uv), m(f.matrix) {}
    static constexpr int luma_step = 2;
    __device__ const uint8_t *luma_at(int x, int yy) const { return y + (size_t)yy * pitch_y + 2 * (size_t)x + 1; }
    // the chroma terms of the pair at (cx, cy): the high bytes of its U and V samples
    __device__ void chroma(int cx, int cyy, int t[3]) const
    {
        const uint8_t *p = uv + (size_t)cyy * pitch_uv + 4 * (size_t)cx;
        yuv_chroma_terms(m, p[1], p[3], t);
    }
    __device__ void taps(int ix, int iy, bool two_x, bool two_y, uint8_t p[2][2][3]) const { yuv_taps(*this, 1, 1, ix, iy, two_x, two_y, p); }
};

// The tone tables of the workgroup's Bayer frame, [3][256] bytes.  Only the Bayer kernels name it, so only they carry it.
__shared__ __attribute__((aligned(4))) uint8_t bayer_tone_lds[768];

// Stages the frame's tone table, if it has one; the barrier of fill_byte_lut, which follows in both kernel bodies, publishes it.  The
// table may sit at any address: a dword load declared unaligned, as SourcePacked::group's.
__device__ static inline void bayer_stage_tone(const uint8_t *tone)
{
    if (tone && threadIdx.x < 192) {
        uint32_t four;
        __builtin_memcpy(&four, tone + 4 * threadIdx.x, 4);
        reinterpret_cast<uint32_t *>(bayer_tone_lds)[threadIdx.x] = four;
    }
}

// One plane of raw sensor samples behind a Bayer filter, or behind none (mi355_frame_bayer; the header defines D(frame), the RGB frame
// this source stands for).  The up to 2 x 2 taps of an output pixel are demosaiced from the 4 x 4 window of toned samples around them,
// (ix - 1 .. ix + 2, iy - 1 .. iy + 2) with coordinates outside the frame reflected: every sample of the window is loaded and toned
// once, then each tap picks its own sample and the averages of its neighbours by the colour of its site.  A site's colour is
// (a, b) = ((x ^ rx) & 1, (y ^ ry) & 1) with (rx, ry) the R site of the pattern: R at (0, 0), B at (1, 1), G elsewhere, so the
// tone table of a sample is a + b.  Pattern, sample layout and tone are uniform over the workgroup: no branch on them diverges;
// every array index is a constant after unrolling.
struct SourceBayer {
    using Frame = mi355_frame_bayer;
    static constexpr const char *name = "frames_bayer";
    static const char *check_pointers(const Frame &f) { return f.data ? nullptr : "null frame pointer"; }
    static const char *check(const Frame &f)
    {
        if (f.pattern < MI355_BAYER_RGGB || f.pattern > MI355_BAYER_MONO) return "unknown pattern (MI355_BAYER_RGGB .. _MONO)";
        if (f.sample < MI355_RAW_U8 || f.sample > MI355_RAW_MIPI12) return "unknown sample layout (MI355_RAW_U8 .. _MIPI12)";
        if (f.shift < 0 || f.shift > 8) return "shift outside 0..8";
        if (f.shift != 0 && f.sample != MI355_RAW_U16) return "shift must be 0 without MI355_RAW_U16";
        if (f.reserved[0] != 0 || f.reserved[1] != 0) return "reserved must be 0";
        if (f.sample == MI355_RAW_U8 && f.pitch < f.w) return "pitch < w";
        if (f.sample == MI355_RAW_U16 && f.pitch < 2 * f.w) return "pitch < 2 * w";
        if (f.sample == MI355_RAW_MIPI10 && f.pitch < 5 * ((f.w + 3) / 4)) return "pitch < 5 * ((w + 3) / 4)";
        if (f.sample == MI355_RAW_MIPI12 && f.pitch < 3 * ((f.w + 1) / 2)) return "pitch < 3 * ((w + 1) / 2)";
        if (f.pattern != MI355_BAYER_MONO && (f.w < 2 || f.h < 2)) return "a Bayer frame needs w, h >= 2";
        return nullptr;
    }
    const uint8_t *data;
    int w, h, pitch;
    int sample, shift;
    int rx, ry;  // the R site of the pattern
    bool mono, toned;
    __device__ explicit SourceBayer(const mi355_frame_bayer &f)
        : data(f.data), w(f.w), h(f.h), pitch(f.pitch), sample(f.sample), shift(f.shift),
          rx(f.pattern == MI355_BAYER_BGGR || f.pattern == MI355_BAYER_GRBG ? 1 : 0),
          ry(f.pattern == MI355_BAYER_BGGR || f.pattern == MI355_BAYER_GBRG ? 1 : 0), mono(f.pattern == MI355_BAYER_MONO),
          toned(f.tone != nullptr) {}
    // the byte offset of sample x inside its row
    __device__ int column(int x) const
    {
        if (sample == MI355_RAW_U16) return 2 * x;
        if (sample == MI355_RAW_MIPI10) return 5 * (x >> 2) + (x & 3);
        if (sample == MI355_RAW_MIPI12) return 3 * (x >> 1) + (x & 1);
        return x;
    }
    // raw8 of the sample at `at`
    __device__ int raw8(const uint8_t *at) const
    {
        if (sample != MI355_RAW_U16) return at[0];
        uint16_t v;
        __builtin_memcpy(&v, at, 2);
        const int r = (int)v >> shift;
        return r > 255 ? 255 : r;
    }
    // s of a sample of colour table t (0, 1, 2)
    __device__ int tone(int t, int raw) const
    {
        return toned ? bayer_tone_lds[256 * t + raw] : raw;
    }
    __device__ void taps(int ix, int iy, bool two_x, bool two_y, uint8_t p[2][2][3]) const
    {
        if (mono) {
            const uint8_t *row = data + (size_t)iy * pitch;
            const int c0 = column(ix), c1 = two_x ? column(ix + 1) : c0;
#pragma unroll
            for (int r = 0; r < 2; ++r, row += pitch) {
                if (r == 1 && !two_y) break;
                p[r][0][0] = p[r][0][1] = p[r][0][2] = (uint8_t)tone(0, raw8(row + c0));
                if (two_x) p[r][1][0] = p[r][1][1] = p[r][1][2] = (uint8_t)tone(0, raw8(row + c1));
            }
            return;
        }
        // the window's columns and rows, reflected (w, h >= 2; ix + 1 < w when two_x, iy + 1 < h when two_y); column 3 and row 3 serve
        // the second taps only
        const int x2 = ix + 1 < w ? ix + 1 : w - 2, y2 = iy + 1 < h ? iy + 1 : h - 2;
        const int xo[4] = {column(ix > 0 ? ix - 1 : 1), column(ix), column(x2), column(two_x && ix + 2 < w ? ix + 2 : w - 2)};
        const int yy[4] = {iy > 0 ? iy - 1 : 1, iy, y2, two_y && iy + 2 < h ? iy + 2 : h - 2};
        const int a0 = (ix ^ rx) & 1, b0 = (iy ^ ry) & 1;  // of window position [1][1], the first tap
        int s[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (i == 3 && !two_y) break;
            const uint8_t *row = data + (size_t)yy[i] * pitch;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (j == 3 && !two_x) break;
                s[i][j] = tone((a0 ^ ((j + 1) & 1)) + (b0 ^ ((i + 1) & 1)), raw8(row + xo[j]));
            }
        }
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            if (r == 1 && !two_y) break;
#pragma unroll
            for (int d = 0; d < 2; ++d) {
                if (d == 1 && !two_x) break;
                const int a = a0 ^ d, b = b0 ^ r, i = 1 + r, j = 1 + d;
                const int own = s[i][j], left_right = s[i][j - 1] + s[i][j + 1], up_down = s[i - 1][j] + s[i + 1][j];
                int red, green, blue;
                if (a != b) {  // a G site: its row neighbours are R in an R row (b == 0), B in a B row
                    const int hc = (left_right + 1) >> 1, vc = (up_down + 1) >> 1;
                    green = own;
                    red = b == 0 ? hc : vc;
                    blue = b == 0 ? vc : hc;
                } else {
                    const int diagonal = (s[i - 1][j - 1] + s[i - 1][j + 1] + s[i + 1][j - 1] + s[i + 1][j + 1] + 2) >> 2;
                    green = (left_right + up_down + 2) >> 2;
                    red = a == 0 ? own : diagonal;
                    blue = a == 0 ? diagonal : own;
                }
                p[r][d][0] = (uint8_t)red; p[r][d][1] = (uint8_t)green; p[r][d][2] = (uint8_t)blue;
            }
        }
    }
};

#ifdef FRAMES_VIEW_TU
// A view of a frame (mi355_frame_view): the rectangle [x0, x0 + w) x [y0, y0 + h) of the frame a Source stands for, turned or mirrored
// by an EXIF orientation; itself a Source.  w and h are the view's (sides swapped by the transposing orients 5..8), so that
// letterbox_px3's one-pixel clauses and frame_geometry see the view; the Source underneath is built from the whole frame, so chroma
// addressing, MIPI groups, the Bayer colour of a site and its reflection stay in frame coordinates.  View tap (u, v) is crop pixel
//   1 (u, v)   2 (cw-1-u, v)   3 (cw-1-u, ch-1-v)   4 (u, ch-1-v)   5 (v, u)   6 (v, ch-1-u)   7 (cw-1-v, ch-1-u)   8 (cw-1-v, u)
// (cw, ch the crop's sides) plus (x0, y0).  The up to 2 x 2 view taps are always a 2 x 2, 1 x 2, 2 x 1 or 1 x 1 cell of the frame: the
// Source's taps is called once, on the cell's low corner (two_x / two_y swapped by a transposing orient), so every kind keeps its shared
// loads, and the cell is permuted into p.  The view is uniform over the workgroup (blockIdx.y is the slot): no branch on it diverges.
template <class Source>
struct Viewed {
    using Frame = typename Source::Frame;
    Source src;
    int w, h;        // of the view
    int x0, y0;      // crop pixel (0, 0) in frame coordinates
    int ex, ey;      // the crop's last column and row: cw - 1, ch - 1
    bool swap, mx, my;  // the view's axes are the crop's swapped; the crop's x / y axis runs against the view axis it serves
    __device__ Viewed(const Frame &f, const mi355_frame_view &v)
        : src(f), w(v.orient >= 5 ? v.h : v.w), h(v.orient >= 5 ? v.w : v.h), x0(v.x0), y0(v.y0), ex(v.w - 1), ey(v.h - 1),
          swap(v.orient >= 5), mx(v.orient == 2 || v.orient == 3 || v.orient == 7 || v.orient == 8),
          my(v.orient == 3 || v.orient == 4 || v.orient == 6 || v.orient == 7) {}
    __device__ void taps(int ix, int iy, bool two_x, bool two_y, uint8_t p[2][2][3]) const
    {
        // along the crop's x axis runs view coordinate a, along its y axis view coordinate b
        const int a = swap ? iy : ix, b = swap ? ix : iy;
        const bool two_a = swap ? two_y : two_x, two_b = swap ? two_x : two_y;
        // the cell's low corner: a mirrored axis counts down, so its second tap is the lower coordinate
        const int cx = mx ? ex - a - (two_a ? 1 : 0) : a, cy = my ? ey - b - (two_b ? 1 : 0) : b;
        uint8_t c[2][2][3];
        src.taps(x0 + cx, y0 + cy, two_a, two_b, c);
        // the cell into view order: mirror it along the axes that run backwards, then transpose it.  Exchanges and selects at constant
        // indices only, so the cell stays in registers
        if (mx && two_a) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                if (i == 1 && !two_b) break;
#pragma unroll
                for (int k = 0; k < 3; ++k) { const uint8_t t = c[i][0][k]; c[i][0][k] = c[i][1][k]; c[i][1][k] = t; }
            }
        }
        if (my && two_b) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                if (j == 1 && !two_a) break;
#pragma unroll
                for (int k = 0; k < 3; ++k) { const uint8_t t = c[0][j][k]; c[0][j][k] = c[1][j][k]; c[1][j][k] = t; }
            }
        }
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            if (r == 1 && !two_y) break;
#pragma unroll
            for (int d = 0; d < 2; ++d) {
                if (d == 1 && !two_x) break;
#pragma unroll
                for (int k = 0; k < 3; ++k) p[r][d][k] = swap ? c[d][r][k] : c[r][d][k];
            }
        }
    }
};

#endif  // FRAMES_VIEW_TU

// the three letterboxed floats (planes 0, 1, 2) of output pixel (x, y)
template <class Source>
__device__ static inline void letterbox_px3(const Source &f, const FrameGeo &g, const float *lut, int x, int y, float v[3])
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
    uint8_t p[2][2][3];
    f.taps(ix, iy, !last_x, !last_y, p);  // row 1 is only read when !last_y, column 1 when !last_x
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float a = last_x ? lut[p[0][0][k]] : (1 - dx) * lut[p[0][0][k]] + dx * lut[p[0][1][k]];
        float val = (1 - dy) * a;
        if (!last_y) {
            const float b = last_x ? lut[p[1][0][k]] : (1 - dx) * lut[p[1][0][k]] + dx * lut[p[1][1][k]];
            val += dy * b;
        }
        v[k] = val;
    }
}

// grid: (workgroups per image, B).  mm[2 b] = max(x, +0), mm[2 b + 1] = min(x, -0) as in image_minmax_batched_kernel (seeded before).
// One body for every source; table[b]: what the Source of slot b is built from (a frame table, or ViewTable below); lut: the
// workgroup's 256-entry byte table.
template <class Source, class Table>
__device__ static inline void letterbox_minmax_body(Table table, int w, int h, uint32_t *mm, float *lut)
{
    fill_byte_lut(lut);
    const Source f(table[blockIdx.y]);
    uint32_t *mi = mm + 2 * (size_t)blockIdx.y;
    FrameGeo g;
    frame_geometry(f.w, f.h, w, h, g);  // checked by frames_check
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

#ifndef FRAMES_VIEW_TU
template <class Source>
__global__ __launch_bounds__(256) void frames_letterbox_minmax_kernel(const typename Source::Frame *table, int w, int h, uint32_t *mm)
{
    __shared__ float lut[256];
    letterbox_minmax_body<Source>(table, w, h, mm, lut);
}
#endif  // !FRAMES_VIEW_TU

// grid: (workgroups per image, B); a thread serves four neighbouring x of one row in all three planes: one 4-byte store per plane
// where the row position is 4-byte aligned, single bytes otherwise (w % 4 != 0: every other row, and the tail of each row)
template <class Source, class Table>
__device__ static inline void letterbox_quantize_body(Table table, int w, int h, const float *scale_dev, const uint8_t *zp_dev,
                                                      uint8_t *out, float *lut)
{
    fill_byte_lut(lut);
    const int wq = (w + 3) / 4;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < h * wq) {
        const Source f(table[blockIdx.y]);
        FrameGeo g;
        frame_geometry(f.w, f.h, w, h, g);  // checked by frames_check
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

#ifndef FRAMES_VIEW_TU
template <class Source>
__global__ __launch_bounds__(256) void frames_letterbox_quantize_kernel(const typename Source::Frame *table, int w, int h,
                                                                        const float *scale_dev, const uint8_t *zp_dev, uint8_t *out)
{
    __shared__ float lut[256];
    letterbox_quantize_body<Source>(table, w, h, scale_dev, zp_dev, out, lut);
}

// The Bayer kind's kernels: the shared bodies behind the staging of the frame's tone table, so that no other kind's kernel gains its LDS.
template <>
__global__ __launch_bounds__(256) void frames_letterbox_minmax_kernel<SourceBayer>(const mi355_frame_bayer *table, int w, int h, uint32_t *mm)
{
    __shared__ float lut[256];
    bayer_stage_tone(table[blockIdx.y].tone);
    letterbox_minmax_body<SourceBayer>(table, w, h, mm, lut);
}

template <>
__global__ __launch_bounds__(256) void frames_letterbox_quantize_kernel<SourceBayer>(const mi355_frame_bayer *table, int w, int h,
                                                                                     const float *scale_dev, const uint8_t *zp_dev,
                                                                                     uint8_t *out)
{
    __shared__ float lut[256];
    bayer_stage_tone(table[blockIdx.y].tone);
    letterbox_quantize_body<SourceBayer>(table, w, h, scale_dev, zp_dev, out, lut);
}

#else  // FRAMES_VIEW_TU
// The kernels of a view of every kind: the same bodies over Viewed<Source>, built from the slot's frame and view.  They are compiled in
// a translation unit of their own (frames_view.hip includes this file with FRAMES_VIEW_TU defined), so that the kernels above are
// compiled exactly as without them: a second caller of a source's taps in the same unit changes how it is inlined into them.
template <class Source>
struct ViewTable {
    const typename Source::Frame *frames;
    const mi355_frame_view *views;
    __device__ Viewed<Source> operator[](unsigned b) const { return Viewed<Source>(frames[b], views[b]); }
};

template <class Source>
__global__ __launch_bounds__(256) void frames_view_letterbox_minmax_kernel(const typename Source::Frame *table, const mi355_frame_view *views,
                                                                           int w, int h, uint32_t *mm)
{
    __shared__ float lut[256];
    letterbox_minmax_body<Viewed<Source>>(ViewTable<Source>{table, views}, w, h, mm, lut);
}

template <class Source>
__global__ __launch_bounds__(256) void frames_view_letterbox_quantize_kernel(const typename Source::Frame *table, const mi355_frame_view *views,
                                                                             int w, int h, const float *scale_dev, const uint8_t *zp_dev,
                                                                             uint8_t *out)
{
    __shared__ float lut[256];
    letterbox_quantize_body<Viewed<Source>>(ViewTable<Source>{table, views}, w, h, scale_dev, zp_dev, out, lut);
}

template <>
__global__ __launch_bounds__(256) void frames_view_letterbox_minmax_kernel<SourceBayer>(const mi355_frame_bayer *table,
                                                                                        const mi355_frame_view *views, int w, int h,
                                                                                        uint32_t *mm)
{
    __shared__ float lut[256];
    bayer_stage_tone(table[blockIdx.y].tone);
    letterbox_minmax_body<Viewed<SourceBayer>>(ViewTable<SourceBayer>{table, views}, w, h, mm, lut);
}

template <>
__global__ __launch_bounds__(256) void frames_view_letterbox_quantize_kernel<SourceBayer>(const mi355_frame_bayer *table,
                                                                                          const mi355_frame_view *views, int w, int h,
                                                                                          const float *scale_dev, const uint8_t *zp_dev,
                                                                                          uint8_t *out)
{
    __shared__ float lut[256];
    bayer_stage_tone(table[blockIdx.y].tone);
    letterbox_quantize_body<Viewed<SourceBayer>>(ViewTable<SourceBayer>{table, views}, w, h, scale_dev, zp_dev, out, lut);
}

#endif  // FRAMES_VIEW_TU

// Host-side check of the table's host mirror, before anything is launched: NULL when every frame can be served, else what is wrong
// ("<Source::name>: <reason>", in a buffer of the calling thread).  The conditions every kind shares are here, a kind's own in its
// Source::check_pointers and Source::check.
// The refusals that are a view's own, against the frame it looks at (already checked): NULL, or the reason.
static const char *view_check(const mi355_frame_view &v, int frame_w, int frame_h)
{
    if (v.orient < 1 || v.orient > 8) return "view: orient outside 1..8";
    if (v.reserved[0] != 0 || v.reserved[1] != 0 || v.reserved[2] != 0) return "view: reserved must be 0";
    if (v.w < 1 || v.h < 1) return "view: need w, h >= 1";
    // frame_w, frame_h <= 32768 and x0, y0 >= 0 where the differences are formed: no sum of the caller's numbers, no overflow
    if (v.x0 < 0 || v.y0 < 0 || v.w > frame_w - v.x0 || v.h > frame_h - v.y0) return "view: rectangle outside the frame";
    return nullptr;
}

// views: NULL (every slot is its whole frame as stored), or one view per slot: the frame is checked as ever, then the view, and the
// geometry is that of the view's oriented size.
template <class Source, class Frame>
static const char *frames_check_views(const Frame *host, const mi355_frame_view *views, int B, int w, int h)
{
    static thread_local char why[160];
    const char *bad = nullptr;
    if (!host || B <= 0 || B > 65535) bad = "null table / need 1 <= B <= 65535";
    else if (w < 2 || h < 2 || w > 32768 || h > 32768) bad = "need 2 <= w, h <= 32768 for the network input";
    for (int b = 0; b < B && !bad; ++b) {
        const Frame &f = host[b];
        FrameGeo g;
        bad = Source::check_pointers(f);  // in the order the refusals have always had
        if (!bad && (f.w < 1 || f.h < 1 || f.w > 32768 || f.h > 32768)) bad = "need 1 <= w, h <= 32768 for every frame";
        if (!bad) bad = Source::check(f);
        int vw = f.w, vh = f.h;
        if (!bad && views) {
            bad = view_check(views[b], f.w, f.h);
            vw = views[b].orient >= 5 ? views[b].h : views[b].w;
            vh = views[b].orient >= 5 ? views[b].w : views[b].h;
        }
        if (!bad && !frame_geometry(vw, vh, w, h, g)) bad = "degenerate aspect (resized side < 2)";
    }
    if (!bad) return nullptr;
    snprintf(why, sizeof(why), "%s: %s", Source::name, bad);
    return why;
}

#ifndef FRAMES_VIEW_TU
template <class Source, class Frame>
const char *frames_check(const Frame *host, int B, int w, int h)
{
    return frames_check_views<Source>(host, nullptr, B, w, h);
}
#else
template <class Source, class Frame>
const char *frames_view_check(const Frame *host, const mi355_frame_view *views_host, int B, int w, int h)
{
    return frames_check_views<Source>(host, views_host, B, w, h);
}
#endif

// about 2048 workgroups in all, at least one per image (image_minmax_batched_launch's sizing)
static int minmax_grid_x(int B, int w, int h)
{
    const long want = ((long)h * w + 255) / 256;
    const long cap = 2048 / B > 0 ? 2048 / B : 1;
    return (int)(want < cap ? want : cap);
}

static unsigned quantize_grid_x(int w, int h)
{
    const long threads = (long)h * ((w + 3) / 4);
    return (unsigned)((threads + 255) / 256);
}

#ifndef FRAMES_VIEW_TU
template <class Source, class Frame>
int frames_letterbox_minmax_launch(const Frame *table_dev, int B, int w, int h, uint32_t *mm, hipStream_t st)
{
    if (image_minmax_seed_launch(mm, B, st) != MI355_OK) return MI355_EHIP;
    hipLaunchKernelGGL(frames_letterbox_minmax_kernel<Source>, dim3(minmax_grid_x(B, w, h), B), dim3(256), 0, st, table_dev, w, h, mm);
    return hipGetLastError() == hipSuccess ? MI355_OK : MI355_EHIP;
}

template <class Source, class Frame>
int frames_letterbox_quantize_launch(const Frame *table_dev, int B, int w, int h, const float *scale_dev,
                                     const uint8_t *zp_dev, uint8_t *out, hipStream_t st)
{
    hipLaunchKernelGGL(frames_letterbox_quantize_kernel<Source>, dim3(quantize_grid_x(w, h), B), dim3(256), 0, st, table_dev, w, h,
                       scale_dev, zp_dev, out);
    return hipGetLastError() == hipSuccess ? MI355_OK : MI355_EHIP;
}

#else
// the same two launches for views: the grids depend on the network input alone
template <class Source, class Frame>
int frames_view_letterbox_minmax_launch(const Frame *table_dev, const mi355_frame_view *views_dev, int B, int w, int h, uint32_t *mm,
                                        hipStream_t st)
{
    if (image_minmax_seed_launch(mm, B, st) != MI355_OK) return MI355_EHIP;
    hipLaunchKernelGGL(frames_view_letterbox_minmax_kernel<Source>, dim3(minmax_grid_x(B, w, h), B), dim3(256), 0, st, table_dev, views_dev,
                       w, h, mm);
    return hipGetLastError() == hipSuccess ? MI355_OK : MI355_EHIP;
}

template <class Source, class Frame>
int frames_view_letterbox_quantize_launch(const Frame *table_dev, const mi355_frame_view *views_dev, int B, int w, int h,
                                          const float *scale_dev, const uint8_t *zp_dev, uint8_t *out, hipStream_t st)
{
    hipLaunchKernelGGL(frames_view_letterbox_quantize_kernel<Source>, dim3(quantize_grid_x(w, h), B), dim3(256), 0, st, table_dev,
                       views_dev, w, h, scale_dev, zp_dev, out);
    return hipGetLastError() == hipSuccess ? MI355_OK : MI355_EHIP;
}

#endif

// the six kinds behind the C-ABI (shim.hip)
#ifdef FRAMES_VIEW_TU
#define FRAMES_KIND(S)                                                                                                                \
    template const char *frames_view_check<S, S::Frame>(const S::Frame *, const mi355_frame_view *, int, int, int);                             \
    template int frames_view_letterbox_minmax_launch<S, S::Frame>(const S::Frame *, const mi355_frame_view *, int, int, int, uint32_t *,         \
                                                                  hipStream_t);                                                                \
    template int frames_view_letterbox_quantize_launch<S, S::Frame>(const S::Frame *, const mi355_frame_view *, int, int, int, const float *,   \
                                                                    const uint8_t *, uint8_t *, hipStream_t);
#else
#define FRAMES_KIND(S)                                                                                                                \
    template const char *frames_check<S, S::Frame>(const S::Frame *, int, int, int);                                                            \
    template int frames_letterbox_minmax_launch<S, S::Frame>(const S::Frame *, int, int, int, uint32_t *, hipStream_t);                         \
    template int frames_letterbox_quantize_launch<S, S::Frame>(const S::Frame *, int, int, int, const float *, const uint8_t *, uint8_t *, \
                                                               hipStream_t);
#endif
FRAMES_KIND(SourceU8)
FRAMES_KIND(SourceYUV)
FRAMES_KIND(SourcePlanar)
FRAMES_KIND(SourcePacked)
FRAMES_KIND(SourceP010)
FRAMES_KIND(SourceBayer)
