/*
 * darknet.c -- `./darknet detector test <data> <cfg> <weights> <image> [flags]`, the drop-in entry point
 * (ref: examples/darknet.c:220 main -> examples/detector.c:952 run_detector -> :878 test_detector), INT8 path only.
 *
 * The flow is test_detector's (examples/detector.c:878-950):
 *   read_data_cfg(<data>) `names=`, get_labels            :880-882
 *   load_network, set_batch_network                        :885-886
 *   load image -> letterbox_image(net->w, net->h)          :903-904   (here: on the device, mi355_letterbox_forward)
 *   quantization_weights_and_activations (layer-0 quantiser on the float image) :918   (here: on the device)
 *   network_predict, "Predicted in"                        :922-924
 *   get_network_boxes(im.w, im.h, thresh, hier, 0, 1)      :926       (here: box decode on the device)
 *   do_nms_sort(nms = .45)                                 :930
 *   draw_detections -> prints "<name>: <p>%"               :931 (src/image.c:255); drawing / saving the image is not built
 *
 * Flags of the reference kept: -i <gpu>, -thresh <t>, -hier <t>, -gpus a,b,c (ref :954-986), -close_quantization
 * (rejected: float path not built).  Added: -batch <B> (replicates the image), -accum exact|ref-f32,
 * -parity wrap|saturate, -dump <dir> (per-layer tensors in the reference layout), -graph (hipGraph replay), -n <iters>,
 * -save_packed <file> / -packed <file>, -boxes (one machine-readable line per kept box), -bcast (with
 * -gpus: replica 0 reads the weights file, the others receive the packed blobs by one RCCL broadcast over xGMI),
 * -inflight <N> (with -n <iters>: after the timed passes, the same passes dealt round-robin to N executors of the prepared
 * model -- network_replica: own activations and stream, shared packed weights; the 4th on the default stream -- and their rate).
 * -list <file> (instead of <image>: one image path per line, dealt into batches of -batch, every image quantised with its own scale /
 * zero point -- set_input_quantization_per_image -- and reported with the block `detector test` prints for it alone).
 * -frames u8 (the sources go to the device as the 8-bit interleaved bytes they are, the whole batch through one
 * network_frames_u8_input_gpu call: no float conversion on the host, no float image on the device; same output).
 * -frames nv12 | nv21 [-matrix bt601|bt601f|bt709|bt709f] (every source is a raw video frame in a file named <anything>_<W>x<H>.nv12:
 * W * H luma bytes, then the interleaved half-resolution chroma plane; both planes go up as they are and are converted inside the
 * letterbox, network_frames_nv12_input_gpu; the output is that of -frames u8 on the converted RGB frame).
 * -frames i420 | yv12 | i422 | i444 [-matrix ...] (the same for raw frames of three tightly packed planes, as software decoders write
 * them, in files named <anything>_<W>x<H>.<format>; network_frames_planar_input_gpu).
 * -frames rgba | bgra | argb | abgr (raw frames of four bytes a pixel, as display surfaces and screen capture deliver them, 4 * W * H
 * bytes; no -matrix) and -frames yuyv | uyvy | yvyu [-matrix ...] (raw packed 4:2:2 frames as cameras deliver them,
 * 4 * ((W + 1) / 2) * H bytes), in files named <anything>_<W>x<H>.<format>; network_frames_packed_input_gpu.
 * -frames p010 [-matrix ...] (raw P010 frames as hardware decoders deliver 10-bit video, NV12's shape with 16-bit little-endian
 * samples, in files named <anything>_<W>x<H>.p010; network_frames_p010_input_gpu).
 * -frames rggb | bggr | grbg | gbrg | mono [-raw u8|u16|mipi10|mipi12] [-raw_shift N] [-tone file] (raw sensor frames, one sample per
 * pixel behind a Bayer filter or none, in files named <anything>_<W>x<H>.<pattern>: W * H bytes (u8, the default), 2 * W * H (u16,
 * little-endian, reduced to min(v >> N, 255)), CSI-2 RAW10 or RAW12 rows; -tone: a file of 768 bytes, the [3][256] tables every sample
 * goes through by the colour of its site; network_frames_bayer_input_gpu; no -matrix; the output is that of -frames u8 on the
 * demosaiced RGB frame mi355_yolo_int8.h defines).
 * -input_device (detector test: the input scales and layer 0's constants are derived on the device, no copy back and no wait inside
 * the input step -- set_input_quantization_on_device; the output is unchanged).
 * -jpeg_device (JPEG sources: their scans are entropy-decoded on the device too -- set_jpeg_entropy_on_device; the output is unchanged).
 * -png_device (PNG sources: their IDAT streams are inflated on the device too -- set_png_inflate_on_device; the output is unchanged).
 *
 * Image input: a baseline JPEG of ANY size -- any file that starts FF D8, whatever its name: entropy decode on the host, inverse DCT,
 * upsampling and colour conversion on the device (network_frames_jpeg_input_gpu), the pixels stb_image gives the reference, byte for
 * byte; a JPEG source always takes the byte path on the device, so `-frames u8` is implied --, a binary PPM (P6) of ANY size
 * (letterboxed like the reference does), a raw `.u8` file holding [c][h][w] bytes at network size, or `synthetic:<seed>`.  A PNG of
 * ANY size, colour type and bit depth, interlaced or not -- any file whose first 16 bytes are the PNG signature and the head of an IHDR
 * chunk, whatever its name: chunk parse and inflate on the host, scanline reconstruction, de-interlacing and expansion to RGB on the
 * device (network_frames_png_input_gpu), stb_image's pixels again, `-frames u8` implied like for a JPEG.  A -list may mix PNG, JPEG
 * and PPM files of different sizes.  Progressive and CMYK JPEGs, BMP, GIF and the other formats of the reference's stb_image are not
 * built and are refused with a message (which still lists PNG: a file with the PNG signature but no IHDR behind it gets it).
 * -view x,y,w,h | -orient N | -orient exif | -tiles CxR[,overlap] (with -frames, one image, one device: every slot looks at a
 * rectangle of the frame under an EXIF orientation -- network_set_frame_views --; `exif` reads a JPEG file's own, other files get 1;
 * -tiles fills C * R slots with network_tile_views' tiles and prints ONE block, network_detections_views' boxes in the image's
 * coordinates after one NMS).
 */
#include <math.h>
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "darknet_q.h"
#include "raw_frame_file.h"

static int find_arg(int argc, char **argv, const char *arg)
{
    for (int i = 0; i < argc; ++i)
        if (argv[i] && 0 == strcmp(argv[i], arg)) { argv[i] = 0; return 1; }
    return 0;
}
static const char *find_char_arg(int argc, char **argv, const char *arg, const char *def)
{
    for (int i = 0; i < argc - 1; ++i)
        if (argv[i] && 0 == strcmp(argv[i], arg)) { def = argv[i + 1]; argv[i] = 0; argv[i + 1] = 0; break; }
    return def;
}

typedef struct { int w, h, c; float *data; } image; /* planar float [c][h][w] in 0..1, like the reference's `image` */

/* the bytes of a PPM / raw / synthetic source: interleaved RGB [h][w][3] (PPM, *planar = 0) or planes [c][h][w] at network size */
static uint8_t *load_bytes_any(const char *path, int netc, int neth, int netw, int *w, int *h, int *c, int *planar)
{
    if (0 == strncmp(path, "synthetic", 9) || (strlen(path) > 3 && 0 == strcmp(path + strlen(path) - 3, ".u8"))) {
        const size_t n = (size_t)netc * neth * netw;
        uint8_t *raw = malloc(n);
        if (0 == strncmp(path, "synthetic", 9)) {
            unsigned long long s = 88172645463325252ULL;
            const char *colon = strchr(path, ':');
            if (colon) s ^= strtoull(colon + 1, NULL, 10) * 0x9E3779B97F4A7C15ULL;
            for (size_t i = 0; i < n; ++i) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; raw[i] = (uint8_t)(s >> 32); }
            raw[0] = 0; raw[1] = 255; /* full range: the reference's dynamic quantiser is then the identity */
        } else {
            FILE *f = fopen(path, "rb");
            if (!f) { fprintf(stderr, "Cannot load image \"%s\"\n", path); exit(0); }
            if (fread(raw, 1, n, f) != n) error("raw .u8 image has the wrong size");
            fclose(f);
        }
        *w = netw; *h = neth; *c = netc; *planar = 1;
        return raw;
    }
    FILE *f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "Cannot load image \"%s\"\n", path); exit(0); }
    char magic[3] = {0};
    int iw = 0, ih = 0, maxv = 0;
    if (fscanf(f, "%2s %d %d %d", magic, &iw, &ih, &maxv) != 4 || strcmp(magic, "P6") || maxv != 255 || iw < 1 || ih < 1)
        error("image must be a baseline JPEG, a binary PPM (P6, maxval 255), a raw .u8 file or synthetic:<seed>; PNG, BMP, GIF and the "
              "other formats of stb_image are not built");
    fgetc(f);
    if (netc != 3) error("PPM input needs a 3-channel network");
    uint8_t *rgb = malloc((size_t)3 * iw * ih);
    if (fread(rgb, 1, (size_t)3 * iw * ih, f) != (size_t)3 * iw * ih) error("PPM truncated");
    fclose(f);
    *w = iw; *h = ih; *c = 3; *planar = 0;
    return rgb;
}

/* A file that starts FF D8 is a JPEG, whatever its name. */
static int is_jpeg_file(const char *path)
{
    if (!path || 0 == strncmp(path, "synthetic", 9)) return 0;
    FILE *f = fopen(path, "rb");
    if (!f) return 0; /* the loaders report a missing file */
    unsigned char two[2] = {0, 0};
    const size_t got = fread(two, 1, 2, f);
    fclose(f);
    return got == 2 && two[0] == 0xFF && two[1] == 0xD8;
}

/* A file whose first 16 bytes are the PNG signature and the length and type of an IHDR chunk is a PNG, whatever its name. */
static int is_png_file(const char *path)
{
    static const unsigned char head[16] = {137, 80, 78, 71, 13, 10, 26, 10, 0, 0, 0, 13, 'I', 'H', 'D', 'R'};
    if (!path || 0 == strncmp(path, "synthetic", 9)) return 0;
    FILE *f = fopen(path, "rb");
    if (!f) return 0;
    unsigned char got[16];
    const size_t n = fread(got, 1, 16, f);
    fclose(f);
    return n == 16 && 0 == memcmp(got, head, 16);
}

/* the files decoded on the device: 0 none of them, CODED_JPEG, CODED_PNG */
enum { CODED_NONE = 0, CODED_JPEG = 1, CODED_PNG = 2 };
static int coded_kind(const char *path) { return is_jpeg_file(path) ? CODED_JPEG : is_png_file(path) ? CODED_PNG : CODED_NONE; }

static uint8_t *read_file(const char *path, size_t *bytes)
{
    FILE *f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "Cannot load image \"%s\"\n", path); exit(0); }
    fseek(f, 0, SEEK_END);
    const long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    uint8_t *data = malloc(n > 0 ? (size_t)n : 1);
    if (n < 0 || fread(data, 1, (size_t)n, f) != (size_t)n) file_error((char *)path);
    fclose(f);
    *bytes = (size_t)n;
    return data;
}

/* load_image_color's contract (ref: src/image.c:1361-1395: bytes / 255., planar) for PPM / raw / synthetic sources */
static image load_image_any(const char *path, int netc, int neth, int netw)
{
    image im = {0, 0, 0, NULL};
    int planar = 0;
    uint8_t *raw = load_bytes_any(path, netc, neth, netw, &im.w, &im.h, &im.c, &planar);
    const size_t hw = (size_t)im.w * im.h;
    im.data = malloc(hw * im.c * sizeof(float));
    if (planar) {
        for (size_t i = 0; i < hw * im.c; ++i) im.data[i] = (float)raw[i] / 255.0f;
    } else {
        for (int k = 0; k < 3; ++k)
            for (size_t i = 0; i < hw; ++i) im.data[(size_t)k * hw + i] = (float)raw[3 * i + k] / 255.f; /* ref :1386 */
    }
    free(raw);
    return im;
}

/* -frames u8: the same sources as interleaved RGB bytes [h][w][3], no float conversion (planar sources are interleaved) */
static uint8_t *load_frame_u8(const char *path, int netc, int neth, int netw, int *w, int *h)
{
    int c = 0, planar = 0;
    uint8_t *raw = load_bytes_any(path, netc, neth, netw, w, h, &c, &planar);
    if (c != 3) error("-frames u8 needs a 3-channel network");
    if (!planar) return raw;
    const size_t hw = (size_t)*w * *h;
    uint8_t *rgb = malloc(3 * hw);
    for (int k = 0; k < 3; ++k)
        for (size_t i = 0; i < hw; ++i) rgb[3 * i + k] = raw[(size_t)k * hw + i];
    free(raw);
    return rgb;
}

static void dump_layer(const char *dir, network *net, int i)
{
    layer *l = &net->layers[i];
    pull_layer_output(net, i);
    char path[512];
    const size_t cnt = (size_t)net->batch * l->outputs;
    if (l->type != YOLO) {
        snprintf(path, sizeof(path), "%s/L%02d_u8.bin", dir, i);
        FILE *f = fopen(path, "wb"); if (!f) file_error(path);
        fwrite(l->output_uint8_final, 1, cnt, f); fclose(f);
    }
    if (l->output_int32_gpu) {
        snprintf(path, sizeof(path), "%s/L%02d_int32.bin", dir, i);
        FILE *f = fopen(path, "wb"); if (!f) file_error(path);
        fwrite(l->output_int32, sizeof(int32_t), cnt, f); fclose(f);
    }
    if (l->output_gpu) {
        snprintf(path, sizeof(path), "%s/L%02d_f32.bin", dir, i);
        FILE *f = fopen(path, "wb"); if (!f) file_error(path);
        fwrite(l->output, sizeof(float), cnt, f); fclose(f);
    }
}

/* -frames u8: the sources go up as interleaved bytes (network_frames_u8_input_gpu), no host float conversion; nv12 | nv21: they are raw
 * _<W>x<H>.nv12 files (network_frames_nv12_input_gpu); i420 | yv12 | i422 | i444: raw _<W>x<H>.<format> files
 * (network_frames_planar_input_gpu); rgba | bgra | argb | abgr | yuyv | uyvy | yvyu: raw _<W>x<H>.<format> files of one packed plane
 * (network_frames_packed_input_gpu); p010: raw _<W>x<H>.p010 files (network_frames_p010_input_gpu); rggb | bggr | grbg | gbrg | mono:
 * raw _<W>x<H>.<pattern> files of sensor samples (network_frames_bayer_input_gpu) */
enum { FRAMES_NONE, FRAMES_U8, FRAMES_NV12, FRAMES_PLANAR, FRAMES_PACKED, FRAMES_P010, FRAMES_BAYER };

typedef struct {
    const char *datacfg, *cfgfile, *weightfile, *filename, *dumpdir, *packed_in, *packed_out;
    const char *listfile;  /* -list: image paths, one per line, per-image input quantisation */
    int frames;            /* -frames: FRAMES_NONE, or how the sources go to the device (feed_frames) */
    int yuv_layout, yuv_matrix; /* MI355_YUV_NV12 / _NV21, MI355_YUV_BT601 .. _BT709_FULL (-matrix) */
    int planar_format;     /* MI355_PLANAR_I420 .. MI355_PLANAR_I444 */
    int packed_format;     /* MI355_PACKED_RGBA .. MI355_PACKED_YVYU */
    int bayer_pattern, raw_sample, raw_shift; /* MI355_BAYER_RGGB .. _MONO, MI355_RAW_U8 .. _MIPI12 (-raw), 0..8 (-raw_shift) */
    const uint8_t *tone;   /* -tone: the file's 768 bytes, or NULL */
    float thresh, hier_thresh;
    int batch, accum, store, use_graph, iters, gpu, boxes, quiet, inflight;
    int jpeg_device;       /* -jpeg_device: JPEG scans are entropy-decoded on the device (set_jpeg_entropy_on_device) */
    int png_device;        /* -png_device: PNG streams are inflated on the device (set_png_inflate_on_device) */
    int view_set, view[4]; /* -view x,y,w,h: the rectangle of the frame every slot looks at */
    int orient;            /* -orient N: 1..8; -orient exif: -1, the file's EXIF orientation (JPEG files; other files 1); 0: not given */
    int tiles, tile_cols, tile_rows, tile_overlap; /* -tiles CxR[,overlap]: the image's tiles fill the batch's C * R slots */
    int input_device;      /* -input_device: scales and layer-0 constants are derived on the device (set_input_quantization_on_device) */
    int rank, nranks;      /* -gpus with -bcast: this replica's rank; rank 0 reads the weights file, the others receive blobs */
    const void *comm_id;   /* shared 128-byte RCCL unique id (NULL: every replica reads the file) */
    double seconds; /* out: per forward pass */
} detect_job;

/* Boxes of the whole batch (slot b's source image is imw[b] x imh[b]) from one decode, NMS applied (ref :892, :927): dets[b], num[b].
 * Returns the class count, 0 for a network without a yolo layer (nothing to print). */
static int batch_detections(const detect_job *job, network *net, const int *imw, const int *imh, detection **dets, int *num)
{
    int classes = 0;
    for (int i = 0; i < net->n; ++i)
        if (net->layers[i].type == YOLO) classes = net->layers[i].classes; /* ref: `l = net->layers[net->n-1]` (:910) */
    for (int b = 0; b < net->batch; ++b) { dets[b] = NULL; num[b] = 0; }
    if (!classes) return 0;
    const float nms = .45f; /* ref :892 */
    if (network_detections_batch(net, imw, imh, job->thresh, 1, nms, 0, dets, num)) error("detector: the network's yolo layers cannot be decoded together");
    return classes;
}

/* -orient exif: the EXIF orientation of a JPEG file, 1 for every other file */
static int file_orientation(const char *path)
{
    if (!is_jpeg_file(path)) return 1;
    FILE *f = fopen(path, "rb");
    if (!f) file_error(path);
    static uint8_t head[1 << 16]; /* APP1 lies in front of the tables and the scan */
    const size_t n = fread(head, 1, sizeof(head), f);
    fclose(f);
    return jpeg_exif_orientation_host(head, n);
}

/* -view, -orient, -tiles: the views of the batch's slots on the one fw x fh frame they all hold */
static void set_job_views(const detect_job *job, network *net, int fw, int fh)
{
    const int B = net->batch;
    const int orient = job->orient < 0 ? file_orientation(job->filename) : job->orient ? job->orient : 1;
    mi355_frame_view *views = calloc((size_t)B, sizeof(mi355_frame_view));
    if (job->tiles) {
        if (network_tile_views(fw, fh, job->tile_cols, job->tile_rows, job->tile_overlap, orient, views) != B)
            error("-tiles: the tiles do not fit the image (a tile larger than the image, or an overlap at or above the tile size)");
    } else {
        for (int b = 0; b < B; ++b) {
            views[b].x0 = job->view_set ? job->view[0] : 0; views[b].y0 = job->view_set ? job->view[1] : 0;
            views[b].w = job->view_set ? job->view[2] : fw; views[b].h = job->view_set ? job->view[3] : fh;
            views[b].orient = orient;
        }
    }
    network_set_frame_views(net, views);
    free(views);
}

/* draw_detections' console output for one slot of batch_detections' result */
static void print_detections(const detect_job *job, int classes, const detection *dets, int nboxes, char **names, int nnames)
{
    if (!classes) return;
    printf("%d\n", nboxes);
    printf("-----------------------\n");
    for (int i = 0; i < nboxes; ++i) /* draw_detections' console output (src/image.c:246-257) */
        for (int j = 0; j < classes; ++j)
            if (dets[i].prob[j] > job->thresh) {
                if (names && j < nnames) printf("%s: %.0f%%\n", names[j], dets[i].prob[j] * 100);
                else printf("class %d: %.0f%%\n", j, dets[i].prob[j] * 100);
                if (job->boxes)
                    printf("box: class %d prob %.9g x %.9g y %.9g w %.9g h %.9g\n", j, dets[i].prob[j], dets[i].bbox.x,
                           dets[i].bbox.y, dets[i].bbox.w, dets[i].bbox.h);
            }
}

/* A JPEG or PNG slot failed: the library's message names the slot of the call it was given, which held the slots of that kind only */
static void coded_slot_error(int kind, char *const *paths, const int *slot_of, int n)
{
    const char *why = kind == CODED_PNG ? network_png_last_error() : network_jpeg_last_error();
    int k = -1;
    if (sscanf(why, kind == CODED_PNG ? "png slot %d:" : "jpeg slot %d:", &k) == 1 && k >= 0 && k < n) {
        const char *colon = strchr(why, ':');
        fprintf(stderr, "slot %d (%s):%s\n", slot_of[k], paths[slot_of[k]], colon ? colon + 1 : why);
    } else {
        fprintf(stderr, "%s\n", why);
    }
    error(kind == CODED_PNG ? "cannot decode a PNG source" : "cannot decode a JPEG source");
}

/* -frames u8 with JPEG or PNG files among the sources: every such slot is decoded into a frame on the device (one
 * network_jpeg_decode_gpu call for all the JPEGs and one network_png_decode_gpu call for all the PNGs; with nothing but JPEGs or nothing
 * but PNGs, network_frames_jpeg_input_gpu / network_frames_png_input_gpu does the whole input step), the other sources go up as the
 * bytes they are, and one network_frames_u8_input_gpu call takes the batch's frames where they lie. */
static void feed_frames_coded(network *net, char *const *paths, int *imw, int *imh)
{
    const int B = net->batch;
    uint8_t **file = calloc((size_t)B, sizeof(uint8_t *)); /* per slot: the coded file's bytes, or the decoded PPM / raw frame */
    size_t *bytes = calloc((size_t)B, sizeof(size_t));
    int *kind = calloc((size_t)B, sizeof(int));
    int *slot_of[3] = {NULL, calloc((size_t)B, sizeof(int)), calloc((size_t)B, sizeof(int))};
    const uint8_t **cdata[3] = {NULL, calloc((size_t)B, sizeof(uint8_t *)), calloc((size_t)B, sizeof(uint8_t *))};
    size_t *cbytes[3] = {NULL, calloc((size_t)B, sizeof(size_t)), calloc((size_t)B, sizeof(size_t))};
    int nc[3] = {0, 0, 0};
    for (int b = 0; b < B; ++b) {
        if (b && paths[b] == paths[b - 1]) { /* the same source again: the same bytes, decoded and uploaded once */
            file[b] = file[b - 1]; bytes[b] = bytes[b - 1]; kind[b] = kind[b - 1];
            imw[b] = imw[b - 1]; imh[b] = imh[b - 1];
        } else if ((kind[b] = coded_kind(paths[b]))) {
            file[b] = read_file(paths[b], &bytes[b]);
        } else {
            file[b] = load_frame_u8(paths[b], net->c, net->h, net->w, &imw[b], &imh[b]);
            bytes[b] = (size_t)3 * imw[b] * imh[b];
        }
        const int k = kind[b];
        if (k) { cdata[k][nc[k]] = file[b]; cbytes[k][nc[k]] = bytes[b]; slot_of[k][nc[k]++] = b; }
    }
    if (nc[CODED_JPEG] == B) {
        if (network_frames_jpeg_input_gpu(net, cdata[CODED_JPEG], cbytes[CODED_JPEG], imw, imh)) coded_slot_error(CODED_JPEG, paths, slot_of[CODED_JPEG], B);
    } else if (nc[CODED_PNG] == B) {
        if (network_frames_png_input_gpu(net, cdata[CODED_PNG], cbytes[CODED_PNG], imw, imh)) coded_slot_error(CODED_PNG, paths, slot_of[CODED_PNG], B);
    } else {
        uint8_t **crgb = calloc((size_t)B, sizeof(uint8_t *));
        int *cw = calloc((size_t)B, sizeof(int)), *ch = calloc((size_t)B, sizeof(int)), *cp = calloc((size_t)B, sizeof(int));
        const uint8_t **frame = calloc((size_t)B, sizeof(uint8_t *));
        int *pitch = calloc((size_t)B, sizeof(int));
        void **up = calloc((size_t)B, sizeof(void *));
        for (int k = CODED_JPEG; k <= CODED_PNG; ++k) {
            if (!nc[k]) continue;
            const int rc = k == CODED_PNG ? network_png_decode_gpu(net, cdata[k], cbytes[k], nc[k], crgb, cw, ch, cp)
                                          : network_jpeg_decode_gpu(net, cdata[k], cbytes[k], nc[k], crgb, cw, ch, cp);
            if (rc) coded_slot_error(k, paths, slot_of[k], nc[k]);
            for (int i = 0; i < nc[k]; ++i) {
                const int b = slot_of[k][i];
                frame[b] = crgb[i]; imw[b] = cw[i]; imh[b] = ch[i]; pitch[b] = cp[i];
            }
        }
        for (int b = 0; b < B; ++b) {
            if (kind[b]) continue;
            pitch[b] = 3 * imw[b];
            if (b && file[b] == file[b - 1]) { frame[b] = frame[b - 1]; continue; }
            if (mi355_alloc(&up[b], bytes[b]) || mi355_h2d(up[b], file[b], bytes[b], net->stream)) {
                fprintf(stderr, "MI355: %s\n", mi355_last_error());
                error("cannot stage the image on the device");
            }
            frame[b] = up[b];
        }
        network_frames_u8_input_gpu(net, frame, imw, imh, pitch, MI355_FRAME_RGB, 1);
        if (mi355_stream_sync(net->stream)) error("sync"); /* the uploaded frames are freed below */
        for (int b = 0; b < B; ++b) if (up[b]) mi355_free(up[b]);
        free(crgb); free(cw); free(ch); free(cp); free(frame); free(pitch); free(up);
    }
    /* on the device nothing waits for the uploads: the sources are freed below */
    if (net->input_on_device && mi355_stream_sync(net->stream)) error("sync");
    for (int b = 0; b < B; ++b) if (!b || file[b] != file[b - 1]) free(file[b]);
    free(file); free(bytes); free(kind);
    for (int k = CODED_JPEG; k <= CODED_PNG; ++k) { free(slot_of[k]); free(cdata[k]); free(cbytes[k]); }
}

/* -frames: the batch's sources, one path per slot, through the entry point of the kind that is set: one call for the whole input step.
 * A slot whose path is the slot's before it (one image in every slot, the free slots of a short last batch) shares its bytes, which
 * then go up once.  imw, imh: the sources' sizes. */
static void feed_frames(const detect_job *job, network *net, char *const *paths, int *imw, int *imh)
{
    const int B = net->batch;
    if (job->frames == FRAMES_U8)
        for (int b = 0; b < B; ++b)
            if ((!b || paths[b] != paths[b - 1]) && coded_kind(paths[b])) { feed_frames_coded(net, paths, imw, imh); return; }
    uint8_t **raw = calloc((size_t)B, sizeof(uint8_t *));
    const uint8_t **pl[3];
    for (int k = 0; k < 3; ++k) pl[k] = calloc((size_t)B, sizeof(uint8_t *));
    for (int b = 0; b < B; ++b) {
        if (b && paths[b] == paths[b - 1]) {
            for (int k = 0; k < 3; ++k) pl[k][b] = pl[k][b - 1];
            imw[b] = imw[b - 1]; imh[b] = imh[b - 1];
        } else if (job->frames == FRAMES_U8) {
            pl[0][b] = raw[b] = load_frame_u8(paths[b], net->c, net->h, net->w, &imw[b], &imh[b]);
        } else { /* the file's planes one after the other */
            char why[1024];
            size_t bytes[2];
            const int kind = job->frames == FRAMES_NV12 ? RAW_FRAME_NV12 : job->frames == FRAMES_P010 ? RAW_FRAME_P010
                           : job->frames == FRAMES_PACKED ? RAW_FRAME_RGBA + job->packed_format
                           : job->frames == FRAMES_BAYER ? RAW_FRAME_SENSOR + 8 * job->raw_sample + job->bayer_pattern : job->planar_format;
            raw[b] = load_raw_frame_file(paths[b], kind, &imw[b], &imh[b], bytes, why, sizeof(why));
            if (!raw[b]) error(why);
            pl[0][b] = raw[b]; pl[1][b] = raw[b] + bytes[0]; pl[2][b] = pl[1][b] + bytes[1];
        }
    }
    if (job->frames == FRAMES_PLANAR)
        network_frames_planar_input_gpu(net, pl[0], pl[1], pl[2], imw, imh, NULL, NULL, NULL, job->planar_format, job->yuv_matrix, 0);
    else if (job->frames == FRAMES_NV12)
        network_frames_nv12_input_gpu(net, pl[0], pl[1], imw, imh, NULL, NULL, job->yuv_layout, job->yuv_matrix, 0);
    else if (job->frames == FRAMES_PACKED)
        network_frames_packed_input_gpu(net, pl[0], imw, imh, NULL, job->packed_format, job->yuv_matrix, 0);
    else if (job->frames == FRAMES_P010)
        network_frames_p010_input_gpu(net, pl[0], pl[1], imw, imh, NULL, NULL, job->yuv_matrix, 0);
    else if (job->frames == FRAMES_BAYER) {
        for (int b = 0; b < B; ++b) pl[1][b] = job->tone; /* one table for every slot: it goes up once */
        network_frames_bayer_input_gpu(net, pl[0], imw, imh, NULL, job->bayer_pattern, job->raw_sample, job->raw_shift,
                                       job->tone ? pl[1] : NULL, 0);
    } else
        network_frames_u8_input_gpu(net, pl[0], imw, imh, NULL, MI355_FRAME_RGB, 0);
    /* on the device nothing waits for the uploads: the sources are freed below */
    if (net->input_on_device && mi355_stream_sync(net->stream)) error("sync");
    for (int b = 0; b < B; ++b) free(raw[b]);
    for (int k = 0; k < 3; ++k) free(pl[k]);
    free(raw);
}

/* -list <file>: one image path per line (the reference's valid= lists), dealt into batches of -batch with every image quantised on
 * its own (set_input_quantization_per_image).  Each image prints the block `detector test` prints for it alone.  The slots a short
 * last batch leaves free repeat its last image (they are not printed). */
static void test_detector_list(detect_job *job, network *net, char **names, int nnames)
{
    FILE *f = fopen(job->listfile, "r");
    if (!f) file_error(job->listfile);
    char **paths = NULL;
    int np = 0;
    char line[4096];
    while (fgets(line, sizeof(line), f)) {
        size_t n = strlen(line);
        while (n && (line[n - 1] == '\n' || line[n - 1] == '\r' || line[n - 1] == ' ')) line[--n] = 0;
        if (!n) continue;
        paths = realloc(paths, sizeof(char *) * (size_t)(np + 1));
        paths[np] = malloc(n + 1);
        memcpy(paths[np++], line, n + 1);
    }
    fclose(f);
    for (int i = 0; i < np; ++i)
        if (coded_kind(paths[i])) { /* a JPEG or PNG source takes the byte path on the device: -frames u8 is implied for the whole list */
            if (job->frames != FRAMES_NONE && job->frames != FRAMES_U8)
                error(is_jpeg_file(paths[i]) ? "-list: a JPEG file does not go with raw -frames formats" : "-list: a PNG file does not go with raw -frames formats");
            job->frames = FRAMES_U8;
            break;
        }
    if (set_input_quantization_per_image(net, 1)) error("-list: layer 0 cannot quantise every image on its own");
    const int B = net->batch;
    int *imw = calloc((size_t)B, sizeof(int)), *imh = calloc((size_t)B, sizeof(int));
    detection **dets = calloc((size_t)B, sizeof(detection *));
    int *num = calloc((size_t)B, sizeof(int));
    for (int first = 0; first < np; first += B) {
        const int cnt = np - first < B ? np - first : B;
        if (job->frames) {
            char **slot = calloc((size_t)B, sizeof(char *));
            for (int b = 0; b < B; ++b) slot[b] = paths[first + (b < cnt ? b : cnt - 1)];
            feed_frames(job, net, slot, imw, imh);
            free(slot);
        } else {
            for (int b = 0; b < B; ++b) {
                const char *path = paths[first + (b < cnt ? b : cnt - 1)];
                image im = load_image_any(path, net->c, net->h, net->w);
                float *im_gpu = NULL;
                const size_t imbytes = (size_t)im.c * im.h * im.w * sizeof(float);
                if (mi355_alloc((void **)&im_gpu, imbytes) || mi355_h2d(im_gpu, im.data, imbytes, net->stream)) {
                    fprintf(stderr, "MI355: %s\n", mi355_last_error());
                    error("cannot stage the image on the device");
                }
                network_letterbox_input_gpu(net, b, im_gpu, im.w, im.h);
                if (mi355_stream_sync(net->stream)) error("sync");
                mi355_free(im_gpu);
                imw[b] = im.w; imh[b] = im.h;
                free(im.data);
            }
            network_quantize_input_gpu(net);
        }
        const double t0 = what_time_is_it_now();
        network_predict(net, net->input);
        const double dt = what_time_is_it_now() - t0;
        const int classes = batch_detections(job, net, imw, imh, dets, num); /* one decode per forward pass, every slot's block from it */
        for (int b = 0; b < cnt; ++b) {
            printf("%s: Predicted in %f seconds. (batch %d, %.1f images/s, gpu %d, accum=%s, parity=%s)\n", paths[first + b], dt, B,
                   B / dt, job->gpu, job->accum == MI355_ACC_EXACT ? "exact" : "ref-f32", job->store == MI355_STORE_WRAP ? "wrap" : "saturate");
            print_detections(job, classes, dets[b], num[b], names, nnames);
        }
        free_detections_batch(dets, num, B);
    }
    free(imw); free(imh); free(dets); free(num);
    for (int i = 0; i < np; ++i) free(paths[i]);
    free(paths);
}

/* one network on one device: load, input path, predict, boxes, NMS, print */
static void test_detector(detect_job *job)
{
    char **names = NULL;
    int nnames = 0;
    if (job->datacfg) {
        char *name_list = data_cfg_find(job->datacfg, "names");
        if (name_list) { names = get_labels(name_list, &nnames); free(name_list); }
        else fprintf(stderr, "%s has no names= entry: classes are printed by index\n", job->datacfg);
    }
    network *net;
    if (job->packed_in || (job->comm_id && job->rank != 0)) { /* deployed model / broadcast receiver: cfg only, blobs arrive packed */
        net = parse_network_cfg((char *)job->cfgfile, 0);
    } else {
        net = load_network((char *)job->cfgfile, (char *)job->weightfile, 0);
    }
    net->gpu_index = job->gpu;
    net->accum_mode = job->accum;
    net->store_mode = job->store;
    net->dump_int32 = job->dumpdir != NULL;
    net->use_graph = job->use_graph;
    set_batch_network(net, job->batch);
    if (job->packed_in) network_load_packed(net, (char *)job->packed_in);
    if (job->comm_id) { /* one-shot RCCL broadcast of the packed weights from replica 0 (xGMI), ~9 MB for yolov3-tiny */
        void *comm = NULL;
        if (mi355_init(job->gpu) || mi355_comm_init(&comm, job->nranks, job->comm_id, job->rank)) {
            fprintf(stderr, "RCCL: %s %s\n", mi355_last_error(), mi355_comm_last_error());
            error("mi355_comm_init");
        }
        if (job->rank == 0 && !job->packed_in) quantization_prep_host(net, 1.0f / 255.0f, 0);
        network_bcast_packed(net, comm, job->rank, 0);
        mi355_comm_destroy(comm);
    }

    if (job->jpeg_device) set_jpeg_entropy_on_device(net, 1);
    if (job->png_device) set_png_inflate_on_device(net, 1);
    if (job->input_device) {
        if (job->inflight > 1) error("-input_device does not go with -inflight: a replica's bank is filled by its own input step");
        if (set_input_quantization_on_device(net, 1)) error("-input_device: layer 0 cannot run on constants derived on the device");
    }
    if (job->listfile) {
        if (mi355_init(job->gpu)) error("mi355_init");
        test_detector_list(job, net, names, nnames);
        for (int i = 0; i < nnames; ++i) free(names[i]);
        free(names);
        free_network(net);
        return;
    }
    image im = {0, 0, 0, NULL};
    float *im_gpu = NULL;
    if (job->frames) { /* the source in every batch slot (it goes up once) */
        if (mi355_init(job->gpu)) { fprintf(stderr, "MI355: %s\n", mi355_last_error()); error("mi355_init (this build has no CPU data path)"); }
        char **slot = calloc((size_t)job->batch, sizeof(char *));
        int *fw = calloc((size_t)job->batch, sizeof(int)), *fh = calloc((size_t)job->batch, sizeof(int));
        for (int b = 0; b < job->batch; ++b) slot[b] = (char *)job->filename;
        feed_frames(job, net, slot, fw, fh);
        im.w = fw[0]; im.h = fh[0];
        if (job->view_set || job->orient || job->tiles) { /* the first pass told the frame's size: once more, through the views */
            set_job_views(job, net, im.w, im.h);
            feed_frames(job, net, slot, fw, fh);
        }
        free(slot); free(fw); free(fh);
    } else {
        im = load_image_any(job->filename, net->c, net->h, net->w);
        /* input path on the device: the float image goes up once, letterbox_image + the layer-0 quantiser run in HBM */
        const size_t imbytes = (size_t)im.c * im.h * im.w * sizeof(float);
        if (mi355_init(job->gpu) || mi355_alloc((void **)&im_gpu, imbytes) || mi355_h2d(im_gpu, im.data, imbytes, NULL) || mi355_stream_sync(NULL)) {
            fprintf(stderr, "MI355: %s\n", mi355_last_error());
            error("cannot stage the image on the device (this build has no CPU data path)");
        }
        for (int b = 0; b < job->batch; ++b) network_letterbox_input_gpu(net, b, im_gpu, im.w, im.h);
        network_quantize_input_gpu(net); /* == quantization_weights_and_activations on the letterboxed floats (ref :918) */
    }
    if (job->packed_out) network_save_packed(net, (char *)job->packed_out);

    double t0 = what_time_is_it_now();
    for (int it = 0; it < job->iters; ++it) network_predict(net, net->input);
    job->seconds = (what_time_is_it_now() - t0) / job->iters;
    if (!job->quiet)
        printf("%s: Predicted in %f seconds. (batch %d, %.1f images/s, gpu %d, accum=%s, parity=%s)\n", job->filename, job->seconds,
               job->batch, job->batch / job->seconds, job->gpu, job->accum == MI355_ACC_EXACT ? "exact" : "ref-f32",
               job->store == MI355_STORE_WRAP ? "wrap" : "saturate");

    if (job->inflight > 1 && job->accum == MI355_ACC_EXACT && !job->dumpdir) { /* several batches in flight (darknet_q.h network_replica) */
        const int n = job->inflight > 8 ? 8 : job->inflight;
        network *ex[8] = {net};
        for (int k = 1; k < n; ++k) {
            net->replica_default_stream = (k == 3 && !job->use_graph); /* the fourth hardware queue belongs to the default stream */
            ex[k] = network_replica(net);
            if (mi355_d2d(ex[k]->input_uint8_gpu, net->input_uint8_gpu, (size_t)net->batch * net->inputs, ex[k]->stream) ||
                mi355_stream_sync(ex[k]->stream)) error("replica input");
        }
        const int passes = job->iters * n;
        for (int k = 0; k < n; ++k) forward_network_gpu(ex[k]); /* the throughput plan's kernels: first launch outside the timing */
        for (int k = 0; k < n; ++k) if (mi355_stream_sync(ex[k]->stream)) error("sync");
        const double t1 = what_time_is_it_now();
        for (int it = 0; it < passes; ++it) forward_network_gpu(ex[it % n]);
        for (int k = 0; k < n; ++k) if (mi355_stream_sync(ex[k]->stream)) error("sync");
        const double dt = (what_time_is_it_now() - t1) / passes;
        if (!job->quiet)
            printf("%d batches in flight: %f seconds per pass (batch %d, %.1f images/s, gpu %d)\n", n, dt, job->batch, job->batch / dt, job->gpu);
        job->seconds = dt;
        for (int k = n - 1; k >= 1; --k) free_network(ex[k]);
    }

    if (!job->quiet) { /* every slot holds the one image */
        const int B = net->batch;
        int *imw = calloc((size_t)B, sizeof(int)), *imh = calloc((size_t)B, sizeof(int)), *num = calloc((size_t)B, sizeof(int));
        detection **dets = calloc((size_t)B, sizeof(detection *));
        for (int b = 0; b < B; ++b) { imw[b] = im.w; imh[b] = im.h; }
        if (net->fr_views) { /* one block for the image: every slot's boxes in the frame's coordinates, one NMS over them */
            int classes = 0, *frame_of_slot = calloc((size_t)B, sizeof(int)); /* every slot looks at frame 0 */
            for (int i = 0; i < net->n; ++i)
                if (net->layers[i].type == YOLO) classes = net->layers[i].classes;
            if (classes && network_detections_views(net, imw, imh, frame_of_slot, job->thresh, .45f, 0, dets, num))
                error("detector: the network's yolo layers cannot be decoded together");
            print_detections(job, classes, dets[0], num[0], names, nnames);
            free(frame_of_slot);
        } else {
            const int classes = batch_detections(job, net, imw, imh, dets, num);
            print_detections(job, classes, dets[0], num[0], names, nnames);
        }
        free_detections_batch(dets, num, B);
        free(imw); free(imh); free(num); free(dets);
    }
    if (job->dumpdir) for (int i = 0; i < net->n; ++i) dump_layer(job->dumpdir, net, i);
    if (im_gpu) mi355_free(im_gpu);
    free(im.data);
    for (int i = 0; i < nnames; ++i) free(names[i]);
    free(names);
    free_network(net);
}

static void *detector_thread(void *p)
{
    test_detector((detect_job *)p);
    return NULL;
}

int main(int argc, char **argv)
{
    if (argc < 2) {
        fprintf(stderr, "usage: %s detector test <data> <cfg> <weights> <image> [-thresh t] [-i gpu | -gpus a,b,..] [-batch B] "
                        "[-accum exact|ref-f32] [-parity wrap|saturate] [-dump dir] [-graph] [-n iters] [-boxes] "
                        "[-save_packed file] [-packed file] [-bcast] [-inflight N] [-list file] [-frames u8|nv12|nv21|i420|yv12|i422|i444|rgba|bgra|argb|abgr|yuyv|uyvy|yvyu|p010|rggb|bggr|grbg|gbrg|mono] [-matrix bt601|bt601f|bt709|bt709f] [-raw u8|u16|mipi10|mipi12] [-raw_shift N] [-tone file] [-view x,y,w,h] [-orient 1..8|exif] [-tiles CxR[,overlap]] [-input_device] [-jpeg_device] [-png_device]\n", argv[0]);
        return 0;
    }
    detect_job job;
    memset(&job, 0, sizeof(job));
    job.gpu = atoi(find_char_arg(argc, argv, "-i", "0"));
    const char *gpu_list = find_char_arg(argc, argv, "-gpus", NULL);
    if (find_arg(argc, argv, "-nogpu")) error("-nogpu: this build has no CPU data path");
    if (find_arg(argc, argv, "-close_quantization")) error("-close_quantization: the float path is not built");
    job.thresh = (float)atof(find_char_arg(argc, argv, "-thresh", ".5"));
    job.hier_thresh = (float)atof(find_char_arg(argc, argv, "-hier", ".5"));
    job.batch = atoi(find_char_arg(argc, argv, "-batch", "1"));
    const char *accum_s = find_char_arg(argc, argv, "-accum", "exact");
    const char *parity_s = find_char_arg(argc, argv, "-parity", "wrap");
    job.dumpdir = find_char_arg(argc, argv, "-dump", NULL);
    job.packed_in = find_char_arg(argc, argv, "-packed", NULL);
    job.packed_out = find_char_arg(argc, argv, "-save_packed", NULL);
    job.use_graph = find_arg(argc, argv, "-graph");
    job.boxes = find_arg(argc, argv, "-boxes");
    job.input_device = find_arg(argc, argv, "-input_device");
    job.jpeg_device = find_arg(argc, argv, "-jpeg_device");
    job.png_device = find_arg(argc, argv, "-png_device");
    const int bcast = find_arg(argc, argv, "-bcast");
    job.iters = atoi(find_char_arg(argc, argv, "-n", "1"));
    job.inflight = atoi(find_char_arg(argc, argv, "-inflight", "1"));
    job.listfile = find_char_arg(argc, argv, "-list", NULL);
    const char *frames_s = find_char_arg(argc, argv, "-frames", NULL);
    const char *matrix_s = find_char_arg(argc, argv, "-matrix", NULL);
    static const char *const planar_known[4] = {"i420", "yv12", "i422", "i444"}; /* MI355_PLANAR_I420 .. MI355_PLANAR_I444 */
    job.frames = FRAMES_NONE;
    job.planar_format = MI355_PLANAR_I420;
    if (frames_s && 0 == strcmp(frames_s, "u8")) job.frames = FRAMES_U8;
    if (frames_s && (0 == strcmp(frames_s, "nv12") || 0 == strcmp(frames_s, "nv21"))) job.frames = FRAMES_NV12;
    for (int k = 0; k < 4; ++k)
        if (frames_s && 0 == strcmp(frames_s, planar_known[k])) { job.frames = FRAMES_PLANAR; job.planar_format = k; }
    static const char *const packed_known[7] = {"rgba", "bgra", "argb", "abgr", "yuyv", "uyvy", "yvyu"}; /* MI355_PACKED_RGBA .. _YVYU */
    for (int k = 0; k < 7; ++k)
        if (frames_s && 0 == strcmp(frames_s, packed_known[k])) { job.frames = FRAMES_PACKED; job.packed_format = k; }
    if (frames_s && 0 == strcmp(frames_s, "p010")) job.frames = FRAMES_P010;
    static const char *const bayer_known[5] = {"rggb", "bggr", "grbg", "gbrg", "mono"}; /* MI355_BAYER_RGGB .. _MONO */
    for (int k = 0; k < 5; ++k)
        if (frames_s && 0 == strcmp(frames_s, bayer_known[k])) { job.frames = FRAMES_BAYER; job.bayer_pattern = k; }
    if (frames_s && !job.frames)
        error("-frames: `u8` (8-bit interleaved frames), `nv12` and `nv21` (raw video frames, files named _<W>x<H>.nv12), `i420`, `yv12`, "
              "`i422` and `i444` (raw planar frames, files named _<W>x<H>.<format>), `rgba`, `bgra`, `argb`, `abgr`, `yuyv`, `uyvy` and "
              "`yvyu` (raw packed frames, files named _<W>x<H>.<format>) and `p010` (raw 10-bit video frames, files named _<W>x<H>.p010) "
              "are known, and `rggb`, `bggr`, `grbg`, `gbrg` and `mono` (raw sensor frames, files named _<W>x<H>.<pattern>; -raw names "
              "their sample layout)");
    job.yuv_layout = frames_s && 0 == strcmp(frames_s, "nv21") ? MI355_YUV_NV21 : MI355_YUV_NV12;
    job.yuv_matrix = MI355_YUV_BT601;
    if (matrix_s) {
        static const char *const known[4] = {"bt601", "bt601f", "bt709", "bt709f"}; /* MI355_YUV_BT601 .. MI355_YUV_BT709_FULL */
        int m = -1;
        for (int k = 0; k < 4; ++k) if (0 == strcmp(matrix_s, known[k])) m = k;
        if (m < 0) error("-matrix: bt601 (the default), bt601f, bt709 and bt709f are known");
        if (job.frames == FRAMES_PACKED && job.packed_format <= MI355_PACKED_ABGR)
            error("-matrix does not go with -frames rgba | bgra | argb | abgr: their bytes are RGB already");
        if (job.frames != FRAMES_NV12 && job.frames != FRAMES_PLANAR && job.frames != FRAMES_PACKED && job.frames != FRAMES_P010)
            error("-matrix goes with -frames nv12 | nv21 | i420 | yv12 | i422 | i444 | yuyv | uyvy | yvyu | p010");
        job.yuv_matrix = m;
    }
    const char *raw_s = find_char_arg(argc, argv, "-raw", NULL), *shift_s = find_char_arg(argc, argv, "-raw_shift", NULL);
    const char *tone_s = find_char_arg(argc, argv, "-tone", NULL);
    job.raw_sample = MI355_RAW_U8; job.raw_shift = 0; job.tone = NULL;
    if ((raw_s || shift_s || tone_s) && job.frames != FRAMES_BAYER) error("-raw, -raw_shift and -tone go with -frames rggb | bggr | grbg | gbrg | mono");
    if (raw_s) {
        static const char *const known[4] = {"u8", "u16", "mipi10", "mipi12"}; /* MI355_RAW_U8 .. MI355_RAW_MIPI12 */
        int r = -1;
        for (int k = 0; k < 4; ++k) if (0 == strcmp(raw_s, known[k])) r = k;
        if (r < 0) error("-raw: u8 (the default), u16, mipi10 and mipi12 are known");
        job.raw_sample = r;
    }
    if (shift_s) {
        if (strlen(shift_s) != 1 || shift_s[0] < '0' || shift_s[0] > '8') error("-raw_shift: 0 .. 8");
        job.raw_shift = shift_s[0] - '0';
        if (job.raw_shift && job.raw_sample != MI355_RAW_U16) error("-raw_shift goes with -raw u16");
    }
    if (tone_s) { /* exactly 768 bytes: [3][256] */
        static uint8_t table[769];
        FILE *tf = fopen(tone_s, "rb");
        if (!tf) file_error(tone_s);
        const size_t got = fread(table, 1, sizeof(table), tf);
        fclose(tf);
        if (got != 768) error("-tone: the file must hold exactly 768 bytes, the [3][256] tables of R, G and B");
        job.tone = table;
    }
    if (job.iters < 1) job.iters = 1;
    if (job.batch < 1) job.batch = 1;
    const char *view_s = find_char_arg(argc, argv, "-view", NULL), *orient_s = find_char_arg(argc, argv, "-orient", NULL);
    const char *tiles_s = find_char_arg(argc, argv, "-tiles", NULL);
    job.view_set = job.orient = job.tiles = job.tile_overlap = 0;
    if (view_s) {
        char tail;
        if (sscanf(view_s, "%d,%d,%d,%d%c", &job.view[0], &job.view[1], &job.view[2], &job.view[3], &tail) != 4) error("-view: x,y,w,h");
        job.view_set = 1;
    }
    if (orient_s) {
        if (0 == strcmp(orient_s, "exif")) job.orient = -1;
        else if (strlen(orient_s) == 1 && orient_s[0] >= '1' && orient_s[0] <= '8') job.orient = orient_s[0] - '0';
        else error("-orient: 1 .. 8 (the EXIF numbering) or `exif` (a JPEG file's own; other files 1)");
    }
    if (tiles_s) {
        char tail;
        const int got = sscanf(tiles_s, "%dx%d,%d%c", &job.tile_cols, &job.tile_rows, &job.tile_overlap, &tail);
        if ((got != 2 && got != 3) || job.tile_cols < 1 || job.tile_rows < 1 || job.tile_cols * (long)job.tile_rows > 4096 || job.tile_overlap < 0)
            error("-tiles: CxR[,overlap]");
        if (view_s) error("-tiles does not go with -view: the tiles are the views");
        job.tiles = 1;
        job.batch = job.tile_cols * job.tile_rows; /* one image fills the batch */
    }
    if ((view_s || orient_s || tiles_s) && (job.listfile || gpu_list || job.inflight > 1))
        error("-view, -orient and -tiles run one image on one device, without -list, -gpus and -inflight");
    job.accum = 0 == strcmp(accum_s, "ref-f32") ? MI355_ACC_REF_F32 : MI355_ACC_EXACT;
    job.store = 0 == strcmp(parity_s, "saturate") ? MI355_STORE_SATURATE : MI355_STORE_WRAP;
    if (strcmp(argv[1], "detector")) {
        fprintf(stderr, "Not an option: %s\n", argv[1]);
        return 0;
    }
    if (job.listfile && (gpu_list || job.dumpdir || job.inflight > 1 || job.packed_in || job.packed_out))
        error("-list runs on one device (-i) without -dump, -inflight, -packed or -save_packed");
    if (job.listfile && argc >= 6 && argv[2] && !strcmp(argv[2], "test") && argv[3] && argv[4] && argv[5] && (argc < 7 || !argv[6])) {
        job.datacfg = argv[3]; job.cfgfile = argv[4]; job.weightfile = argv[5]; job.filename = NULL;
        test_detector(&job);
        return 0;
    }
    if (argc < 7 || !argv[2] || strcmp(argv[2], "test") || !argv[3] || !argv[4] || !argv[5] || !argv[6]) {
        fprintf(stderr, "only `detector test <data> <cfg> <weights> <image>` is part of the INT8 inference path (train/valid/recall: SURVEY.md 2 rows 12,22)\n");
        return 0;
    }
    job.datacfg = argv[3]; job.cfgfile = argv[4]; job.weightfile = argv[5]; job.filename = argv[6];
    if (coded_kind(job.filename)) { /* a JPEG or PNG source takes the byte path on the device: -frames u8 is implied */
        if (job.frames != FRAMES_NONE && job.frames != FRAMES_U8)
            error(is_jpeg_file(job.filename) ? "a JPEG image does not go with raw -frames formats" : "a PNG image does not go with raw -frames formats");
        job.frames = FRAMES_U8;
    }
    if ((job.view_set || job.orient || job.tiles) && !job.frames) error("-view, -orient and -tiles go with -frames (a JPEG or PNG file implies -frames u8)");
    if (!gpu_list) {
        test_detector(&job);
        return 0;
    }
    /* -gpus a,b,c (ref: examples/detector.c:954-977 parses the same list for training): one host thread per device, each
     * with its own network replica and its own `-batch` images -- images shard embarrassingly, no steady-state traffic.
     * Weights reach every device from the file, or with -bcast from replica 0 by one RCCL broadcast (mi355_bcast_blob). */
    int gpus[64], ngpus = 0;
    char *list = malloc(strlen(gpu_list) + 1);
    strcpy(list, gpu_list);
    for (char *tok = strtok(list, ","); tok && ngpus < 64; tok = strtok(NULL, ",")) gpus[ngpus++] = atoi(tok);
    if (ngpus < 1) error("-gpus: empty list");
    if (mi355_device_count() < 1) error("no HIP device visible (this build has no CPU data path)");
    static char comm_id[128];
    if (bcast && mi355_comm_unique_id(comm_id)) {
        fprintf(stderr, "RCCL: %s\n", mi355_comm_last_error());
        error("-bcast needs librccl");
    }
    detect_job *jobs = calloc((size_t)ngpus, sizeof(detect_job));
    pthread_t *th = calloc((size_t)ngpus, sizeof(pthread_t));
    for (int g = 0; g < ngpus; ++g) {
        jobs[g] = job;
        jobs[g].gpu = gpus[g];
        jobs[g].rank = g; jobs[g].nranks = ngpus;
        jobs[g].comm_id = bcast ? comm_id : NULL;
        jobs[g].quiet = g != 0; /* device 0 of the list prints the detections */
        jobs[g].dumpdir = g == 0 ? job.dumpdir : NULL;
        jobs[g].packed_out = g == 0 ? job.packed_out : NULL;
        if (pthread_create(&th[g], NULL, detector_thread, &jobs[g])) error("pthread_create");
    }
    double slowest = 0;
    for (int g = 0; g < ngpus; ++g) {
        pthread_join(th[g], NULL);
        if (jobs[g].seconds > slowest) slowest = jobs[g].seconds;
    }
    printf("%d GPUs x batch %d: %.1f images/s (slowest replica %f s per pass)\n", ngpus, job.batch, ngpus * job.batch / slowest, slowest);
    free(jobs); free(th); free(list);
    return 0;
}
