/*
 * input_frames.c -- frame input: raw frames in host or device memory in, the network's quantised input on the device out.
 *
 * Two launches for the whole batch (frames.hip): letterbox + min / max, then letterbox + quantise; the float image exists in registers
 * only.  The (scale, zero point) branches are the float path's (input_pair_shared, input_pairs_per_image).  Interleaved RGB / BGR
 * frames, NV12 / NV21 frames, frames of three separate planes, packed 4-byte frames (RGBA .. ABGR, YUYV .. YVYU), P010 frames and raw
 * Bayer / mono sensor frames differ in their table entries, the planes they describe and the pair of C-ABI calls; the table, the staging arena and everything else are
 * shared.
 */
#include <stdlib.h>
#include <string.h>
#include "host_internal.h"

enum { FR_U8, FR_YUV, FR_PLANAR, FR_PACKED, FR_P010, FR_BAYER }; /* the kind of frames an entry point feeds (net->fr_kind) */
static const size_t fr_entry_bytes[6] = {sizeof(mi355_frame_u8), sizeof(mi355_frame_yuv), sizeof(mi355_frame_planar),
                                         sizeof(mi355_frame_packed), sizeof(mi355_frame_p010), sizeof(mi355_frame_bayer)};

void fr_free(network *net)
{
    if (net->fr_arena_gpu) mi355_free(net->fr_arena_gpu);
    if (net->fr_table_gpu) mi355_free(net->fr_table_gpu);
    if (net->fr_mm_gpu) mi355_free(net->fr_mm_gpu);
    if (net->fr_pair_gpu) mi355_free(net->fr_pair_gpu);
    if (net->fr_views_gpu) mi355_free(net->fr_views_gpu);
    free(net->fr_table_host); free(net->fr_mm_host); free(net->fr_pair_host);
    net->fr_arena_gpu = NULL; net->fr_table_gpu = NULL; net->fr_table_host = NULL;
    net->fr_mm_gpu = net->fr_mm_host = NULL;
    net->fr_pair_gpu = net->fr_pair_host = NULL;
    net->fr_views_gpu = NULL;
    net->fr_arena_bytes = 0;
    net->fr_cap = 0;
}

/* Everything but the arena, sized by the batch; the one table holds entries of any kind (the planar entry is the largest). */
static void fr_alloc(network *net)
{
    const size_t B = (size_t)net->batch;
    if (net->fr_cap == net->batch) return;
    fr_free(net);
    check_mi355(mi355_alloc((void **)&net->fr_mm_gpu, 2 * sizeof(float) * B), "alloc minmax");
    check_mi355(mi355_alloc(&net->fr_pair_gpu, 5 * B), "alloc input pairs");
    check_mi355(mi355_alloc(&net->fr_table_gpu, sizeof(mi355_frame_planar) * B), "alloc frame table");
    check_mi355(mi355_alloc(&net->fr_views_gpu, sizeof(mi355_frame_view) * B), "alloc view table");
    net->fr_mm_host = calloc(2 * B, sizeof(float));
    net->fr_pair_host = calloc(5, B);
    net->fr_table_host = calloc(B, sizeof(mi355_frame_planar));
    net->fr_cap = net->batch;
}

/* The first touch of the device, after every refusal of an entry point.  Returns the host mirror of the table, [batch] entries of `kind`
 * for the entry point to fill. */
static void *fr_begin(network *net, int kind)
{
    check_mi355(mi355_init(net->gpu_index), "mi355_init");
    if (!net->stream && !net->on_default_stream) check_mi355(mi355_stream_acquire(&net->stream), "stream");
    fr_alloc(net);
    net->fr_kind = kind;
    return net->fr_table_host;
}

size_t fr_round(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

/* the staging arena holds at least `need` bytes */
static void fr_arena_reserve(network *net, size_t need)
{
    if (need <= net->fr_arena_bytes) return;
    net_wait(net); /* nothing in flight reads the arena that is freed */
    if (net->fr_arena_gpu) mi355_free(net->fr_arena_gpu);
    net->fr_arena_gpu = NULL; net->fr_arena_bytes = 0;
    check_mi355(mi355_alloc(&net->fr_arena_gpu, need), "alloc frame arena");
    net->fr_arena_bytes = need;
}

/* `bytes` host bytes go up as they are to the arena at *off, which moves on to the next 256-byte boundary */
static const uint8_t *fr_stage(network *net, const uint8_t *src, size_t bytes, size_t *off)
{
    uint8_t *dst = (uint8_t *)net->fr_arena_gpu + *off;
    check_mi355(mi355_h2d(dst, src, bytes, net->stream), "upload frame");
    *off += fr_round(bytes);
    return dst;
}

/* One plane of a frame in host memory, as it is: rows keep their pitch, the last row ends with its last sample. */
typedef struct {
    const uint8_t *host;
    size_t row_bytes, rows, pitch;
    const uint8_t **dev; /* the table entry's pointer to this plane: set to where the bytes went */
} fr_plane;

static size_t fr_plane_bytes(const fr_plane *p) { return (p->rows - 1) * p->pitch + p->row_bytes; }

/* Host frames go up to the arena: planes[b * np + k] is plane k of the frame in slot b.  Frame by frame, plane by plane, each at a
 * 256-byte boundary; one frame in several slots (`-batch B` of one image: the same pointers and geometry) goes up once.  The arena
 * is reserved with `extra` bytes behind the frames for what the caller stages after them; returns where those start. */
static size_t fr_stage_frames_and(network *net, const fr_plane *planes, int np, size_t extra)
{
    const int B = net->batch;
    size_t need = extra, off = 0;
    for (int i = 0; i < B * np; ++i) need += fr_round(fr_plane_bytes(&planes[i]));
    fr_arena_reserve(net, need);
    for (int b = 0; b < B; ++b) {
        const fr_plane *f = planes + (size_t)b * np, *same = NULL;
        for (int k = 0; k < b && !same; ++k) {
            const fr_plane *g = planes + (size_t)k * np;
            int eq = 1;
            for (int i = 0; i < np; ++i)
                eq &= g[i].host == f[i].host && g[i].row_bytes == f[i].row_bytes && g[i].rows == f[i].rows && g[i].pitch == f[i].pitch;
            if (eq) same = g;
        }
        for (int i = 0; i < np; ++i) *f[i].dev = same ? *same[i].dev : fr_stage(net, f[i].host, fr_plane_bytes(&f[i]), &off);
    }
    return off;
}

static void fr_stage_frames(network *net, const fr_plane *planes, int np) { (void)fr_stage_frames_and(net, planes, np, 0); }

/* The two launches of the table's kind; with views set (network_set_frame_views) the view pair of the same kind, which takes the view
 * table beside the frame table. */
static void fr_minmax(network *net)
{
    const int B = net->batch, kind = net->fr_kind, w = net->w, h = net->h;
    const void *tg = net->fr_table_gpu, *th = net->fr_table_host;
    const mi355_frame_view *vg = net->fr_views_gpu, *vh = net->fr_views;
    float *mm = net->fr_mm_gpu;
    void *st = net->stream;
    if (vh) {
        if (kind == FR_PLANAR) check_mi355(mi355_frames_planar_view_letterbox_minmax(tg, th, vg, vh, B, w, h, mm, st), "mi355_frames_planar_view_letterbox_minmax");
        else if (kind == FR_PACKED) check_mi355(mi355_frames_packed_view_letterbox_minmax(tg, th, vg, vh, B, w, h, mm, st), "mi355_frames_packed_view_letterbox_minmax");
        else if (kind == FR_P010) check_mi355(mi355_frames_p010_view_letterbox_minmax(tg, th, vg, vh, B, w, h, mm, st), "mi355_frames_p010_view_letterbox_minmax");
        else if (kind == FR_BAYER) check_mi355(mi355_frames_bayer_view_letterbox_minmax(tg, th, vg, vh, B, w, h, mm, st), "mi355_frames_bayer_view_letterbox_minmax");
        else if (kind == FR_YUV) check_mi355(mi355_frames_yuv_view_letterbox_minmax(tg, th, vg, vh, B, w, h, mm, st), "mi355_frames_yuv_view_letterbox_minmax");
        else check_mi355(mi355_frames_u8_view_letterbox_minmax(tg, th, vg, vh, B, w, h, mm, st), "mi355_frames_u8_view_letterbox_minmax");
        return;
    }
    if (kind == FR_PLANAR) check_mi355(mi355_frames_planar_letterbox_minmax(tg, th, B, w, h, mm, st), "mi355_frames_planar_letterbox_minmax");
    else if (kind == FR_PACKED) check_mi355(mi355_frames_packed_letterbox_minmax(tg, th, B, w, h, mm, st), "mi355_frames_packed_letterbox_minmax");
    else if (kind == FR_P010) check_mi355(mi355_frames_p010_letterbox_minmax(tg, th, B, w, h, mm, st), "mi355_frames_p010_letterbox_minmax");
    else if (kind == FR_BAYER) check_mi355(mi355_frames_bayer_letterbox_minmax(tg, th, B, w, h, mm, st), "mi355_frames_bayer_letterbox_minmax");
    else if (kind == FR_YUV) check_mi355(mi355_frames_yuv_letterbox_minmax(tg, th, B, w, h, mm, st), "mi355_frames_yuv_letterbox_minmax");
    else check_mi355(mi355_frames_u8_letterbox_minmax(tg, th, B, w, h, mm, st), "mi355_frames_u8_letterbox_minmax");
}

static void fr_quantize(network *net, const float *scale_dev, const uint8_t *zp_dev)
{
    const int B = net->batch, kind = net->fr_kind, w = net->w, h = net->h;
    const void *tg = net->fr_table_gpu, *th = net->fr_table_host;
    const mi355_frame_view *vg = net->fr_views_gpu, *vh = net->fr_views;
    uint8_t *out = net->input_uint8_gpu;
    void *st = net->stream;
    if (vh) {
        if (kind == FR_PLANAR) check_mi355(mi355_frames_planar_view_letterbox_quantize(tg, th, vg, vh, B, w, h, scale_dev, zp_dev, out, st), "mi355_frames_planar_view_letterbox_quantize");
        else if (kind == FR_PACKED) check_mi355(mi355_frames_packed_view_letterbox_quantize(tg, th, vg, vh, B, w, h, scale_dev, zp_dev, out, st), "mi355_frames_packed_view_letterbox_quantize");
        else if (kind == FR_P010) check_mi355(mi355_frames_p010_view_letterbox_quantize(tg, th, vg, vh, B, w, h, scale_dev, zp_dev, out, st), "mi355_frames_p010_view_letterbox_quantize");
        else if (kind == FR_BAYER) check_mi355(mi355_frames_bayer_view_letterbox_quantize(tg, th, vg, vh, B, w, h, scale_dev, zp_dev, out, st), "mi355_frames_bayer_view_letterbox_quantize");
        else if (kind == FR_YUV) check_mi355(mi355_frames_yuv_view_letterbox_quantize(tg, th, vg, vh, B, w, h, scale_dev, zp_dev, out, st), "mi355_frames_yuv_view_letterbox_quantize");
        else check_mi355(mi355_frames_u8_view_letterbox_quantize(tg, th, vg, vh, B, w, h, scale_dev, zp_dev, out, st), "mi355_frames_u8_view_letterbox_quantize");
        return;
    }
    if (kind == FR_PLANAR) check_mi355(mi355_frames_planar_letterbox_quantize(tg, th, B, w, h, scale_dev, zp_dev, out, st), "mi355_frames_planar_letterbox_quantize");
    else if (kind == FR_PACKED) check_mi355(mi355_frames_packed_letterbox_quantize(tg, th, B, w, h, scale_dev, zp_dev, out, st), "mi355_frames_packed_letterbox_quantize");
    else if (kind == FR_P010) check_mi355(mi355_frames_p010_letterbox_quantize(tg, th, B, w, h, scale_dev, zp_dev, out, st), "mi355_frames_p010_letterbox_quantize");
    else if (kind == FR_BAYER) check_mi355(mi355_frames_bayer_letterbox_quantize(tg, th, B, w, h, scale_dev, zp_dev, out, st), "mi355_frames_bayer_letterbox_quantize");
    else if (kind == FR_YUV) check_mi355(mi355_frames_yuv_letterbox_quantize(tg, th, B, w, h, scale_dev, zp_dev, out, st), "mi355_frames_yuv_letterbox_quantize");
    else check_mi355(mi355_frames_u8_letterbox_quantize(tg, th, B, w, h, scale_dev, zp_dev, out, st), "mi355_frames_u8_letterbox_quantize");
}

/* The common tail, the host mirror of the table filled with device pointers: table upload, min / max launch, the batch's one host
 * sync, the (scale, zero point) branch, quantiser launch, with the calls of the frames' kind. */
static void fr_finish(network *net)
{
    const int B = net->batch, kind = net->fr_kind;
    const void *th = net->fr_table_host;
    if (net->input_on_device) od_alloc(net);
    check_mi355(mi355_h2d(net->fr_table_gpu, th, fr_entry_bytes[kind] * (size_t)B, net->stream), "upload frame table");
    if (net->fr_views) check_mi355(mi355_h2d(net->fr_views_gpu, net->fr_views, sizeof(mi355_frame_view) * (size_t)B, net->stream), "upload view table");
    fr_minmax(net);
    const float *scale_dev;
    const uint8_t *zp_dev;
    if (net->input_on_device) { /* pairs and layer 0 follow on the stream: nothing comes back, nothing is waited for */
        od_pairs_and_entries(net, net->fr_mm_gpu);
        scale_dev = od_scale_dev(net);
        zp_dev = od_zp_dev(net);
    } else if (net->per_image) {
        check_mi355(mi355_d2h(net->fr_mm_host, net->fr_mm_gpu, 2 * sizeof(float) * (size_t)B, net->stream), "minmax d2h");
        net_wait(net); /* the batch's one host sync: every earlier upload is done too */
        input_pairs_per_image(net, net->fr_mm_host);
        scale_dev = (const float *)((const char *)net->pi_idx_gpu + 4 * (size_t)B);
        zp_dev = (const uint8_t *)net->pi_idx_gpu + 8 * (size_t)B;
    } else { /* image 0 defines the pair of the whole batch */
        check_mi355(mi355_d2h(net->fr_mm_host, net->fr_mm_gpu, 2 * sizeof(float) * (size_t)B, net->stream), "minmax d2h");
        net_wait(net); /* the batch's one host sync: every earlier upload is done too */
        float s; uint8_t zp;
        image_scale_zero_point(net->fr_mm_host[1] + 0.0f, net->fr_mm_host[0], &s, &zp);
        input_pair_shared(net, s, zp);
        float *sc = (float *)net->fr_pair_host;
        uint8_t *zq = (uint8_t *)net->fr_pair_host + 4 * (size_t)B;
        for (int b = 0; b < B; ++b) { sc[b] = s; zq[b] = zp; }
        check_mi355(mi355_h2d(net->fr_pair_gpu, net->fr_pair_host, 5 * (size_t)B, net->stream), "upload input pair");
        scale_dev = (const float *)net->fr_pair_gpu;
        zp_dev = (const uint8_t *)net->fr_pair_gpu + 4 * (size_t)B;
    }
    fr_quantize(net, scale_dev, zp_dev);
}

/* Every entry point: refuse what it must before the device is touched, fill its table entries with the caller's pointers, describe the
 * planes, stage them unless they are on the device already, fr_finish. */
void network_frames_u8_input_gpu(network *net, const uint8_t *const *frames, const int *w, const int *h, const int *pitch, int order,
                                 int frames_on_device)
{
    const int B = net->batch;
    if (!frames || !w || !h) error("network_frames_u8_input_gpu: null frames / sizes");
    if (net->c != 3) error("network_frames_u8_input_gpu: 8-bit frames feed 3-channel networks only");
    for (int b = 0; b < B; ++b) {
        if (!frames[b]) error("network_frames_u8_input_gpu: null frame");
        if (w[b] < 1 || h[b] < 1 || (pitch && pitch[b] < 3 * w[b])) error("network_frames_u8_input_gpu: need w, h >= 1 and pitch >= 3 * w for every frame");
    }
    mi355_frame_u8 *tab = fr_begin(net, FR_U8);
    fr_plane *planes = calloc((size_t)B, sizeof(fr_plane));
    for (int b = 0; b < B; ++b) {
        memset(&tab[b], 0, sizeof(tab[b]));
        tab[b].data = frames[b];
        tab[b].w = w[b]; tab[b].h = h[b]; tab[b].pitch = pitch ? pitch[b] : 3 * w[b]; tab[b].order = order;
        planes[b] = (fr_plane){frames[b], 3 * (size_t)w[b], (size_t)h[b], (size_t)tab[b].pitch, &tab[b].data};
    }
    if (!frames_on_device) fr_stage_frames(net, planes, 1);
    free(planes);
    fr_finish(net);
}

void network_frames_nv12_input_gpu(network *net, const uint8_t *const *y, const uint8_t *const *uv, const int *w, const int *h,
                                   const int *pitch_y, const int *pitch_uv, int layout, int matrix, int frames_on_device)
{
    const int B = net->batch;
    if (!y || !uv || !w || !h) error("network_frames_nv12_input_gpu: null planes / sizes");
    if (net->c != 3) error("network_frames_nv12_input_gpu: NV12 / NV21 frames feed 3-channel networks only");
    for (int b = 0; b < B; ++b) {
        if (!y[b] || !uv[b]) error("network_frames_nv12_input_gpu: null plane");
        if (w[b] < 1 || h[b] < 1) error("network_frames_nv12_input_gpu: need w, h >= 1 for every frame");
        if ((pitch_y && pitch_y[b] < w[b]) || (pitch_uv && pitch_uv[b] < 2 * ((w[b] + 1) / 2)))
            error("network_frames_nv12_input_gpu: need pitch_y >= w and pitch_uv >= 2 * ((w + 1) / 2) for every frame");
    }
    mi355_frame_yuv *tab = fr_begin(net, FR_YUV);
    fr_plane *planes = calloc(2 * (size_t)B, sizeof(fr_plane));
    for (int b = 0; b < B; ++b) {
        const int cw2 = 2 * ((w[b] + 1) / 2), ch = (h[b] + 1) / 2;
        memset(&tab[b], 0, sizeof(tab[b]));
        tab[b].y = y[b]; tab[b].uv = uv[b];
        tab[b].w = w[b]; tab[b].h = h[b]; tab[b].pitch_y = pitch_y ? pitch_y[b] : w[b]; tab[b].pitch_uv = pitch_uv ? pitch_uv[b] : cw2;
        tab[b].layout = layout; tab[b].matrix = matrix;
        planes[2 * b] = (fr_plane){y[b], (size_t)w[b], (size_t)h[b], (size_t)tab[b].pitch_y, &tab[b].y};
        planes[2 * b + 1] = (fr_plane){uv[b], (size_t)cw2, (size_t)ch, (size_t)tab[b].pitch_uv, &tab[b].uv};
    }
    if (!frames_on_device) fr_stage_frames(net, planes, 2);
    free(planes);
    fr_finish(net);
}

void network_frames_planar_input_gpu(network *net, const uint8_t *const *p0, const uint8_t *const *p1, const uint8_t *const *p2,
                                     const int *w, const int *h, const int *pitch0, const int *pitch1, const int *pitch2,
                                     int format, int matrix, int frames_on_device)
{
    const int B = net->batch;
    const uint8_t *const *const src[3] = {p0, p1, p2};
    const int *const pitches[3] = {pitch0, pitch1, pitch2};
    if (!p0 || !p1 || !p2 || !w || !h) error("network_frames_planar_input_gpu: null planes / sizes");
    if (format < MI355_PLANAR_I420 || format > MI355_PLANAR_BGR) error("network_frames_planar_input_gpu: unknown format (MI355_PLANAR_I420 .. _BGR)");
    if (matrix < MI355_YUV_BT601 || matrix > MI355_YUV_BT709_FULL) error("network_frames_planar_input_gpu: unknown matrix (MI355_YUV_BT601 .. _BT709_FULL)");
    const int rgb = format == MI355_PLANAR_RGB || format == MI355_PLANAR_BGR;
    if (rgb && matrix != 0) error("network_frames_planar_input_gpu: matrix must be 0 with MI355_PLANAR_RGB / _BGR");
    const int half_w = !rgb && format != MI355_PLANAR_I444, half_h = format == MI355_PLANAR_I420 || format == MI355_PLANAR_YV12;
    if (net->c != 3) error("network_frames_planar_input_gpu: planar frames feed 3-channel networks only");
    for (int b = 0; b < B; ++b) {
        if (!p0[b] || !p1[b] || !p2[b]) error("network_frames_planar_input_gpu: null plane");
        if (w[b] < 1 || h[b] < 1 || w[b] > 32768 || h[b] > 32768) error("network_frames_planar_input_gpu: need 1 <= w, h <= 32768 for every frame");
        for (int k = 0; k < 3; ++k)
            if (pitches[k] && pitches[k][b] < (k && half_w ? (w[b] + 1) / 2 : w[b]))
                error("network_frames_planar_input_gpu: need pitch >= the width of its plane for every plane");
    }
    mi355_frame_planar *tab = fr_begin(net, FR_PLANAR);
    fr_plane *planes = calloc(3 * (size_t)B, sizeof(fr_plane));
    for (int b = 0; b < B; ++b) {
        memset(&tab[b], 0, sizeof(tab[b]));
        tab[b].w = w[b]; tab[b].h = h[b]; tab[b].format = format; tab[b].matrix = matrix;
        for (int k = 0; k < 3; ++k) { /* plane 0 is w x h, planes 1 and 2 the format's chroma size */
            const int pw = k && half_w ? (w[b] + 1) / 2 : w[b], ph = k && half_h ? (h[b] + 1) / 2 : h[b];
            tab[b].plane[k] = src[k][b]; tab[b].pitch[k] = pitches[k] ? pitches[k][b] : pw;
            planes[3 * b + k] = (fr_plane){src[k][b], (size_t)pw, (size_t)ph, (size_t)tab[b].pitch[k], &tab[b].plane[k]};
        }
    }
    if (!frames_on_device) fr_stage_frames(net, planes, 3);
    free(planes);
    fr_finish(net);
}

void network_frames_packed_input_gpu(network *net, const uint8_t *const *frames, const int *w, const int *h, const int *pitch, int format,
                                     int matrix, int frames_on_device)
{
    const int B = net->batch;
    if (!frames || !w || !h) error("network_frames_packed_input_gpu: null frames / sizes");
    if (format < MI355_PACKED_RGBA || format > MI355_PACKED_YVYU) error("network_frames_packed_input_gpu: unknown format (MI355_PACKED_RGBA .. _YVYU)");
    if (matrix < MI355_YUV_BT601 || matrix > MI355_YUV_BT709_FULL) error("network_frames_packed_input_gpu: unknown matrix (MI355_YUV_BT601 .. _BT709_FULL)");
    const int rgb = format <= MI355_PACKED_ABGR;
    if (rgb && matrix != 0) error("network_frames_packed_input_gpu: matrix must be 0 with MI355_PACKED_RGBA / _BGRA / _ARGB / _ABGR");
    if (net->c != 3) error("network_frames_packed_input_gpu: packed frames feed 3-channel networks only");
    for (int b = 0; b < B; ++b) {
        if (!frames[b]) error("network_frames_packed_input_gpu: null frame");
        if (w[b] < 1 || h[b] < 1 || w[b] > 32768 || h[b] > 32768) error("network_frames_packed_input_gpu: need 1 <= w, h <= 32768 for every frame");
        if (pitch && pitch[b] < 4 * (rgb ? w[b] : (w[b] + 1) / 2))
            error("network_frames_packed_input_gpu: need pitch >= 4 * w (RGB formats) or 4 * ((w + 1) / 2) (4:2:2 formats) for every frame");
    }
    mi355_frame_packed *tab = fr_begin(net, FR_PACKED);
    fr_plane *planes = calloc((size_t)B, sizeof(fr_plane));
    for (int b = 0; b < B; ++b) {
        const int row = 4 * (rgb ? w[b] : (w[b] + 1) / 2); /* whole groups: a pixel, or a macropixel of two */
        memset(&tab[b], 0, sizeof(tab[b]));
        tab[b].data = frames[b];
        tab[b].w = w[b]; tab[b].h = h[b]; tab[b].pitch = pitch ? pitch[b] : row; tab[b].format = format; tab[b].matrix = matrix;
        planes[b] = (fr_plane){frames[b], (size_t)row, (size_t)h[b], (size_t)tab[b].pitch, &tab[b].data};
    }
    if (!frames_on_device) fr_stage_frames(net, planes, 1);
    free(planes);
    fr_finish(net);
}

void network_frames_p010_input_gpu(network *net, const uint8_t *const *y, const uint8_t *const *uv, const int *w, const int *h,
                                   const int *pitch_y, const int *pitch_uv, int matrix, int frames_on_device)
{
    const int B = net->batch;
    if (!y || !uv || !w || !h) error("network_frames_p010_input_gpu: null planes / sizes");
    if (matrix < MI355_YUV_BT601 || matrix > MI355_YUV_BT709_FULL) error("network_frames_p010_input_gpu: unknown matrix (MI355_YUV_BT601 .. _BT709_FULL)");
    if (net->c != 3) error("network_frames_p010_input_gpu: P010 frames feed 3-channel networks only");
    for (int b = 0; b < B; ++b) {
        if (!y[b] || !uv[b]) error("network_frames_p010_input_gpu: null plane");
        if (w[b] < 1 || h[b] < 1 || w[b] > 32768 || h[b] > 32768) error("network_frames_p010_input_gpu: need 1 <= w, h <= 32768 for every frame");
        if ((pitch_y && pitch_y[b] < 2 * w[b]) || (pitch_uv && pitch_uv[b] < 4 * ((w[b] + 1) / 2)))
            error("network_frames_p010_input_gpu: need pitch_y >= 2 * w and pitch_uv >= 4 * ((w + 1) / 2) for every frame");
    }
    mi355_frame_p010 *tab = fr_begin(net, FR_P010);
    fr_plane *planes = calloc(2 * (size_t)B, sizeof(fr_plane));
    for (int b = 0; b < B; ++b) {
        const int cw4 = 4 * ((w[b] + 1) / 2), ch = (h[b] + 1) / 2; /* bytes of a row of (U, V) pairs of 16-bit samples */
        memset(&tab[b], 0, sizeof(tab[b]));
        tab[b].y = y[b]; tab[b].uv = uv[b];
        tab[b].w = w[b]; tab[b].h = h[b]; tab[b].pitch_y = pitch_y ? pitch_y[b] : 2 * w[b]; tab[b].pitch_uv = pitch_uv ? pitch_uv[b] : cw4;
        tab[b].matrix = matrix;
        planes[2 * b] = (fr_plane){y[b], 2 * (size_t)w[b], (size_t)h[b], (size_t)tab[b].pitch_y, &tab[b].y};
        planes[2 * b + 1] = (fr_plane){uv[b], (size_t)cw4, (size_t)ch, (size_t)tab[b].pitch_uv, &tab[b].uv};
    }
    if (!frames_on_device) fr_stage_frames(net, planes, 2);
    free(planes);
    fr_finish(net);
}

/* the bytes of a tightly packed row of w raw samples, by layout */
static int bayer_row_bytes(int sample, int w)
{
    return sample == MI355_RAW_U16 ? 2 * w : sample == MI355_RAW_MIPI10 ? 5 * ((w + 3) / 4) : sample == MI355_RAW_MIPI12 ? 3 * ((w + 1) / 2) : w;
}

void network_frames_bayer_input_gpu(network *net, const uint8_t *const *frames, const int *w, const int *h, const int *pitch, int pattern,
                                    int sample, int shift, const uint8_t *const *tone, int frames_on_device)
{
    const int B = net->batch;
    if (!frames || !w || !h) error("network_frames_bayer_input_gpu: null frames / sizes");
    if (pattern < MI355_BAYER_RGGB || pattern > MI355_BAYER_MONO) error("network_frames_bayer_input_gpu: unknown pattern (MI355_BAYER_RGGB .. _MONO)");
    if (sample < MI355_RAW_U8 || sample > MI355_RAW_MIPI12) error("network_frames_bayer_input_gpu: unknown sample layout (MI355_RAW_U8 .. _MIPI12)");
    if (shift < 0 || shift > 8) error("network_frames_bayer_input_gpu: shift outside 0..8");
    if (shift != 0 && sample != MI355_RAW_U16) error("network_frames_bayer_input_gpu: shift must be 0 without MI355_RAW_U16");
    if (net->c != 3) error("network_frames_bayer_input_gpu: raw sensor frames feed 3-channel networks only");
    for (int b = 0; b < B; ++b) {
        if (!frames[b]) error("network_frames_bayer_input_gpu: null frame");
        if (w[b] < 1 || h[b] < 1 || w[b] > 32768 || h[b] > 32768) error("network_frames_bayer_input_gpu: need 1 <= w, h <= 32768 for every frame");
        if (pattern != MI355_BAYER_MONO && (w[b] < 2 || h[b] < 2)) error("network_frames_bayer_input_gpu: a Bayer frame needs w, h >= 2");
        if (pitch && pitch[b] < bayer_row_bytes(sample, w[b]))
            error("network_frames_bayer_input_gpu: need pitch >= w (U8), 2 * w (U16), 5 * ((w + 3) / 4) (MIPI10) or 3 * ((w + 1) / 2) (MIPI12) "
                  "for every frame");
    }
    mi355_frame_bayer *tab = fr_begin(net, FR_BAYER);
    fr_plane *planes = calloc((size_t)B, sizeof(fr_plane));
    size_t tone_bytes = 0;
    for (int b = 0; b < B; ++b) {
        const int row = bayer_row_bytes(sample, w[b]);
        memset(&tab[b], 0, sizeof(tab[b]));
        tab[b].data = frames[b];
        tab[b].tone = tone ? tone[b] : NULL;
        tab[b].w = w[b]; tab[b].h = h[b]; tab[b].pitch = pitch ? pitch[b] : row;
        tab[b].pattern = pattern; tab[b].sample = sample; tab[b].shift = shift;
        planes[b] = (fr_plane){frames[b], (size_t)row, (size_t)h[b], (size_t)tab[b].pitch, &tab[b].data};
        if (tab[b].tone) tone_bytes += fr_round(768);
    }
    if (!frames_on_device) { /* the tone tables go up behind the frames; a table several slots share goes up once */
        size_t off = fr_stage_frames_and(net, planes, 1, tone_bytes);
        for (int b = 0; b < B; ++b) {
            if (!tone || !tone[b]) continue;
            int same = -1;
            for (int k = 0; k < b && same < 0; ++k)
                if (tone[k] == tone[b]) same = k;
            tab[b].tone = same >= 0 ? tab[same].tone : fr_stage(net, tone[b], 768, &off);
        }
    }
    free(planes);
    fr_finish(net);
}
