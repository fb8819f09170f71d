/*
 * input_coded.c -- coded-image input: JPEG and PNG files in host memory in, interleaved RGB frames in device memory out, for the 8-bit
 * frame path (input_frames.c).
 *
 * Every format goes the same way.  The host half decodes every slot as far as the host goes (jpeg.c, jpeg_scan.c, png.c); a slot that
 * names the bytes of an earlier slot shares its decode and its frame, and a slot the host refuses ends the call before the device is
 * touched.  Then one staging block -- the format's tables, then the bytes the device reads, laid out exactly like its device copy --
 * goes up in one copy, and two launches make the frames.  The buffers are a coded_bufs of the network: they grow when a call needs
 * more, after a wait (nothing in flight reads what is freed), and the staging block is rewritten only after the upload that read it
 * last has completed.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "host_internal.h"
#include "jpeg.h"
#include "jpeg_scan.h"
#include "png.h"
#include "png_scan.h"

enum { CODED_ERR_LEN = 320 };

/* What a format brings to the slot pass; an item is its host decode of one image. */
typedef struct {
    const char *name; /* "jpeg", "png": how its messages start */
    char *err;        /* its buffer of the calling thread, CODED_ERR_LEN bytes */
    size_t item_bytes;
    int (*decode)(const uint8_t *data, size_t bytes, void *item, char *why, size_t whylen);
    void (*release)(void *item); /* also of an item that is all zero */
} coded_format;

typedef struct { size_t at; int w, h, pitch; } coded_frame; /* an RGB frame, `at` bytes into the frames' buffer */

typedef struct {
    int n, nu;         /* slots; distinct images among them */
    int *first;        /* [n] the first slot that names slot b's bytes */
    int *frame;        /* [n] of a first slot: its image's index among the nu */
    char *items;       /* [n] items, those of the first slots filled */
    coded_frame *out;  /* [nu] where the images' frames go */
} coded_slots;

static int coded_refuse(char *err, const char *why)
{
    snprintf(err, CODED_ERR_LEN, "%s", why);
    return MI355_EINVAL;
}

static void coded_slots_free(const coded_format *f, coded_slots *s)
{
    for (int b = 0; b < s->n; ++b) f->release(s->items + f->item_bytes * (size_t)b);
    free(s->items); free(s->first); free(s->frame); free(s->out);
}

/* The host half.  MI355_EINVAL: f->err names the first slot that was refused, everything is freed again and nothing has touched the
 * device. */
static int coded_slots_decode(const coded_format *f, const uint8_t *const *data, const size_t *bytes, int n, coded_slots *s, const char *oom)
{
    *s = (coded_slots){n, 0, calloc((size_t)n, sizeof(int)), calloc((size_t)n, sizeof(int)), calloc((size_t)n, f->item_bytes),
                       calloc((size_t)n, sizeof(coded_frame))};
    if (!s->first || !s->frame || !s->items || !s->out) error(oom);
    for (int b = 0; b < n; ++b) {
        s->first[b] = b;
        for (int k = 0; k < b && s->first[b] == b; ++k)
            if (data[k] == data[b] && bytes[k] == bytes[b]) s->first[b] = k;
        if (s->first[b] != b) continue;
        char why[256];
        if (!data[b]) snprintf(f->err, CODED_ERR_LEN, "%s slot %d: null data", f->name, b);
        else if (f->decode(data[b], bytes[b], s->items + f->item_bytes * (size_t)b, why, sizeof(why)))
            snprintf(f->err, CODED_ERR_LEN, "%s slot %d: %s", f->name, b, why);
        else { s->frame[b] = s->nu++; continue; }
        coded_slots_free(f, s);
        return MI355_EINVAL;
    }
    return MI355_OK;
}

/* a bump cursor: `bytes` at *at, which moves on to the next 256-byte boundary */
static size_t take(size_t *at, size_t bytes)
{
    const size_t here = *at;
    *at += fr_round(bytes);
    return here;
}

static coded_frame coded_frame_take(size_t *at, int w, int h)
{
    const int pitch = (3 * w + 3) & ~3;
    return (coded_frame){take(at, (size_t)h * (size_t)pitch), w, h, pitch};
}

/* every slot's frame, then the host half is freed */
static void coded_slots_finish(const coded_format *f, coded_slots *s, void *rgb_gpu, uint8_t **rgb_dev, int *w, int *h, int *pitch)
{
    for (int b = 0; b < s->n; ++b) {
        const coded_frame *o = &s->out[s->frame[s->first[b]]];
        rgb_dev[b] = (uint8_t *)rgb_gpu + o->at; w[b] = o->w; h[b] = o->h; pitch[b] = o->pitch;
    }
    coded_slots_free(f, s);
}

/* ------------------------------------------------------------------------------------------------- the buffer set */
static void coded_bufs_free(coded_bufs *cb)
{
    if (cb->in_gpu) mi355_free(cb->in_gpu);
    if (cb->work_gpu) mi355_free(cb->work_gpu);
    if (cb->rgb_gpu) mi355_free(cb->rgb_gpu);
    free(cb->stage_host);
    memset(cb, 0, sizeof(*cb));
}

void coded_free(network *net)
{
    coded_bufs_free(&net->jpg);
    coded_bufs_free(&net->png);
    if (net->jpg_coef_gpu) mi355_free(net->jpg_coef_gpu);
    if (net->jpg_status_gpu) mi355_free(net->jpg_status_gpu);
    free(net->jpg_status_host);
    net->jpg_coef_gpu = net->jpg_status_gpu = NULL;
    net->jpg_status_host = NULL;
    net->jpg_coef_bytes = net->jpg_status_bytes = 0;
    if (net->png_filt_gpu) mi355_free(net->png_filt_gpu);
    if (net->png_status_gpu) mi355_free(net->png_status_gpu);
    free(net->png_status_host);
    net->png_filt_gpu = net->png_status_gpu = NULL;
    net->png_status_host = NULL;
    net->png_filt_bytes = net->png_status_bytes = 0;
}

typedef struct { void **buf; size_t *have, need; const char *what; } coded_want; /* a device buffer that holds at least `need` bytes */

/* The first touch of the device, after every refusal: the device buffers are reserved with at most one wait (nothing in flight reads
 * what is freed), the upload that read the staging block last has completed, and the block holds stage_bytes.  Returns the block. */
static uint8_t *coded_begin(network *net, coded_bufs *cb, const coded_want *want, int nwant, size_t stage_bytes, const char *oom)
{
    check_mi355(mi355_init(net->gpu_index), "mi355_init");
    if (!net->stream && !net->on_default_stream) check_mi355(mi355_stream_acquire(&net->stream), "stream");
    int waited = 0;
    for (const coded_want *q = want; q < want + nwant; ++q) {
        if (q->need <= *q->have) continue;
        if (!waited) { net_wait(net); waited = 1; }
        if (*q->buf) mi355_free(*q->buf);
        *q->buf = NULL; *q->have = 0;
        check_mi355(mi355_alloc(q->buf, q->need), q->what);
        *q->have = q->need;
    }
    if (cb->upload_pending && !waited) net_wait(net);
    cb->upload_pending = 0;
    if (cb->stage_bytes < stage_bytes) {
        free(cb->stage_host);
        cb->stage_host = malloc(stage_bytes);
        if (!cb->stage_host) error(oom);
        cb->stage_bytes = stage_bytes;
    }
    return cb->stage_host;
}

/* network_frames_jpeg_input_gpu, network_frames_png_input_gpu: the format's decode for net->batch images, then the 8-bit frame path on
 * those device frames */
typedef int coded_decode_gpu(network *net, const uint8_t *const *data, const size_t *bytes, int n, uint8_t **rgb_dev, int *w, int *h, int *pitch);

static int coded_frames_input(network *net, const uint8_t *const *data, const size_t *bytes, int *w, int *h, coded_decode_gpu *decode, char *err,
                              const char *null_argument, const char *not_3_channels)
{
    if (!net || !w || !h) return coded_refuse(err, null_argument);
    if (net->c != 3) return coded_refuse(err, not_3_channels);
    const int B = net->batch;
    uint8_t **rgb = calloc((size_t)B, sizeof(uint8_t *));
    int *pitch = calloc((size_t)B, sizeof(int));
    const int rc = decode(net, data, bytes, B, rgb, w, h, pitch);
    if (rc == MI355_OK) network_frames_u8_input_gpu(net, (const uint8_t *const *)rgb, w, h, pitch, MI355_FRAME_RGB, 1);
    free(rgb); free(pitch);
    return rc;
}

/* ------------------------------------------------------------------------------------------------- JPEG input
 * The host decodes the entropy-coded streams (jpeg.c), the device does the rest (jpeg.hip): the staging block -- plane table, image
 * table, quantiser tables, coefficients -- goes up, then mi355_jpeg_idct over every block of the batch and mi355_jpeg_to_rgb over every
 * image.
 *
 * With set_jpeg_entropy_on_device the host only finds the scans (jpeg_scan.c).  Behind the three tables the staging block then holds the
 * segment table, the Huffman tables and the unstuffed bytes of every segment; the coefficient planes are zeroed on the device,
 * mi355_jpeg_entropy fills them, the status words come back (the call's one wait of its own), and the two launches follow on the same
 * planes. */
static _Thread_local char jpg_err[CODED_ERR_LEN];
const char *network_jpeg_last_error(void) { return jpg_err; }

void set_jpeg_entropy_on_device(network *net, int on) { net->jpg_entropy_on_device = on != 0; }

void set_jpeg_entropy_subseq_bits(network *net, int bits)
{
    if (bits < 32 || bits > 8192 || (bits & 31)) error("set_jpeg_entropy_subseq_bits: a multiple of 32 in 32 .. 8192");
    net->jpg_subseq_bits = bits;
}

static const char *jpg_entropy_reason(int code)
{
    return code == MI355_JPEG_EHUFF ? "bad huffman code" : code == MI355_JPEG_EDC ? "bad DC category" :
           code == MI355_JPEG_EINDEX ? "coefficient index past the end of the block" : "unknown status";
}

typedef struct { dnq_jpeg im; dnq_jpeg_scan_list sl; } jpg_item; /* sl: with the entropy decode on the device only */

static int jpg_item_decode(const uint8_t *data, size_t bytes, void *item, char *why, size_t whylen)
{
    return jpeg_decode_host(data, bytes, &((jpg_item *)item)->im, why, whylen);
}

static int jpg_item_scan(const uint8_t *data, size_t bytes, void *item, char *why, size_t whylen)
{
    return jpeg_scan_host(data, bytes, &((jpg_item *)item)->im, &((jpg_item *)item)->sl, why, whylen);
}

static void jpg_item_release(void *item)
{
    jpeg_free(&((jpg_item *)item)->im);
    jpeg_scan_free(&((jpg_item *)item)->sl);
}

typedef struct {
    int entropy; /* the entropy decode runs on the device; without it nsegs, nhuff and stream_bytes are 0 */
    int nplanes, nsegs, nhuff;
    size_t stream_bytes;
    size_t off_images, off_quant, off_segs, off_huff, off_bits; /* into the staging block; the plane table is at 0 */
    size_t in, coef, work, rgb;                                 /* what the call needs of every buffer */
} jpg_layout;

/* The layout of the staging block (= of its device copy), of the coefficient planes, of the component planes and of the frames, in one
 * walk that serves twice: with stage == NULL it only sizes (L->in, coef, work, rgb), with the staging block it fills the plane table,
 * the image table and the quantiser tables with the addresses the same steps give.  Plane pi's coefficients live in the staging
 * block behind the tables and are copied there (coef_gpu == NULL: the host decoded them), or in coef_gpu, where the device puts them. */
static void jpg_walk(const coded_slots *s, jpg_layout *L, uint8_t *stage, const coded_bufs *cb, uint8_t *coef_gpu)
{
    const jpg_item *items = (const jpg_item *)s->items;
    size_t in = 0, coef = 0, work = 0, rgb = 0;
    take(&in, sizeof(mi355_jpeg_plane) * (size_t)L->nplanes);
    L->off_images = take(&in, sizeof(mi355_jpeg_image) * (size_t)s->nu);
    L->off_quant = take(&in, 128 * (size_t)L->nplanes);
    L->off_segs = take(&in, sizeof(mi355_jpeg_segment) * (size_t)L->nsegs);
    if (stage) memset(stage, 0, in); /* the tables */
    L->off_huff = take(&in, sizeof(mi355_jpeg_huff) * (size_t)L->nhuff);
    L->off_bits = take(&in, L->stream_bytes);
    mi355_jpeg_plane *planes = (mi355_jpeg_plane *)stage;
    int pi = 0, blocks_before = 0;
    for (int b = 0; b < s->n; ++b) {
        if (s->first[b] != b) continue;
        const dnq_jpeg *im = &items[b].im;
        const int i = s->frame[b];
        mi355_jpeg_image *g = stage ? (mi355_jpeg_image *)(stage + L->off_images) + i : NULL;
        const coded_frame o = s->out[i] = coded_frame_take(&rgb, im->w, im->h);
        if (stage) { g->rgb = (uint8_t *)cb->rgb_gpu + o.at; g->w = o.w; g->h = o.h; g->pitch = o.pitch; g->mode = im->mode; }
        for (int k = 0; k < im->ncomp; ++k, ++pi) {
            const dnq_jpeg_comp *c = &im->comp[k];
            const size_t blocks = (size_t)c->blocks_w * c->blocks_h;
            const size_t coef_at = take(L->entropy ? &coef : &in, 128 * blocks), out_at = take(&work, 64 * blocks);
            const int first_block = blocks_before;
            blocks_before += (int)blocks;
            if (!stage) continue;
            memcpy(stage + L->off_quant + 128 * (size_t)pi, c->quant, 128);
            if (!coef_gpu) memcpy(stage + coef_at, c->coef, 128 * blocks);
            planes[pi].coef = (const int16_t *)((coef_gpu ? coef_gpu : (uint8_t *)cb->in_gpu) + coef_at);
            planes[pi].quant = (const uint16_t *)((uint8_t *)cb->in_gpu + L->off_quant + 128 * (size_t)pi);
            planes[pi].out = (uint8_t *)cb->work_gpu + out_at;
            planes[pi].blocks_w = c->blocks_w; planes[pi].blocks_h = c->blocks_h; planes[pi].first_block = first_block;
            g->comp[k].plane = planes[pi].out; g->comp[k].pitch = 8 * c->blocks_w; g->comp[k].rows = c->rows;
            g->comp[k].hs = c->hs; g->comp[k].vs = c->vs;
        }
    }
    L->in = in; L->coef = coef; L->work = work; L->rgb = rgb;
}

/* What the entropy decode on the device adds to the staging block: segment table, Huffman tables, the segments' bytes.
 * slot_of_seg[q]: the slot segment q came with. */
static void jpg_fill_segments(const coded_slots *s, const jpg_layout *L, uint8_t *stage, const uint8_t *in_gpu, int *slot_of_seg)
{
    const jpg_item *items = (const jpg_item *)s->items;
    const mi355_jpeg_plane *planes = (const mi355_jpeg_plane *)stage;
    mi355_jpeg_segment *segs = (mi355_jpeg_segment *)(stage + L->off_segs);
    size_t bits_at = L->off_bits;
    int pi = 0, si = 0, hi = 0;
    for (int b = 0; b < s->n; ++b) {
        if (s->first[b] != b) continue;
        const dnq_jpeg *im = &items[b].im;
        const dnq_jpeg_scan_list *sl = &items[b].sl;
        memcpy(stage + L->off_huff + sizeof(mi355_jpeg_huff) * (size_t)hi, sl->huff, sizeof(mi355_jpeg_huff) * (size_t)sl->nhuff);
        memcpy(stage + bits_at, sl->bytes, sl->nbytes);
        for (int q = 0; q < sl->nsegs; ++q, ++si) {
            const dnq_jpeg_scan_seg *z = &sl->segs[q];
            mi355_jpeg_segment *t = &segs[si];
            slot_of_seg[si] = b;
            t->bits = (const uint32_t *)(in_gpu + bits_at + z->offset);
            t->huff = (const mi355_jpeg_huff *)(in_gpu + L->off_huff);
            t->nhuff = L->nhuff;
            t->nbytes = z->nbytes;
            t->ncomp = z->ncomp;
            for (int c = 0; c < z->ncomp; ++c) {
                const dnq_jpeg_comp *k = &im->comp[z->comp[c]];
                t->coef[c] = (int16_t *)planes[pi + z->comp[c]].coef;
                t->bh[c] = z->bh[c]; t->bv[c] = z->bv[c];
                t->blocks_w[c] = k->blocks_w; t->blocks_h[c] = k->blocks_h;
                t->dc[c] = hi + z->dc[c]; t->ac[c] = hi + z->ac[c];
            }
            t->units_x = z->units_x; t->units_y = z->units_y; t->first_unit = z->first_unit; t->nunits = z->nunits;
        }
        pi += im->ncomp;
        hi += sl->nhuff;
        bits_at += sl->nbytes; /* a multiple of 4: every segment is padded to one */
    }
}

int network_jpeg_decode_gpu(network *net, const uint8_t *const *data, const size_t *bytes, int n, uint8_t **rgb_dev, int *w, int *h, int *pitch)
{
    static const char oom[] = "network_jpeg_decode_gpu: out of memory";
    if (!net || !data || !bytes || !rgb_dev || !w || !h || !pitch || n < 1 || n > 65535)
        return coded_refuse(jpg_err, "network_jpeg_decode_gpu: null argument / need 1 <= n <= 65535");
    const int entropy = net->jpg_entropy_on_device;
    coded_bufs *cb = &net->jpg;
    const coded_format f = {"jpeg", jpg_err, sizeof(jpg_item), entropy ? jpg_item_scan : jpg_item_decode, jpg_item_release};
    coded_slots s;
    if (coded_slots_decode(&f, data, bytes, n, &s, oom)) return MI355_EINVAL;
    jpg_layout L = {.entropy = entropy};
    for (int b = 0; b < n; ++b) { /* the items of the other slots are empty */
        const jpg_item *it = (const jpg_item *)s.items + b;
        L.nplanes += it->im.ncomp; L.nsegs += it->sl.nsegs; L.nhuff += it->sl.nhuff; L.stream_bytes += it->sl.nbytes;
    }
    jpg_walk(&s, &L, NULL, cb, NULL);
    const size_t status_bytes = sizeof(int) * (size_t)L.nsegs;
    if (net->jpg_status_bytes < status_bytes) {
        free(net->jpg_status_host);
        net->jpg_status_host = malloc(status_bytes);
        if (!net->jpg_status_host) error(oom);
    }
    const coded_want want[] = {{&cb->in_gpu, &cb->in_bytes, L.in, entropy ? "alloc jpeg streams" : "alloc jpeg coefficients"},
                               {&net->jpg_coef_gpu, &net->jpg_coef_bytes, L.coef, "alloc jpeg coefficients"},
                               {&cb->work_gpu, &cb->work_bytes, L.work, "alloc jpeg planes"},
                               {&cb->rgb_gpu, &cb->rgb_bytes, L.rgb, "alloc jpeg frames"},
                               {&net->jpg_status_gpu, &net->jpg_status_bytes, status_bytes, "alloc jpeg status"}};
    uint8_t *stage = coded_begin(net, cb, want, 5, L.in, oom), *in_gpu = cb->in_gpu;
    jpg_walk(&s, &L, stage, cb, entropy ? net->jpg_coef_gpu : NULL);
    int *slot_of_seg = entropy ? calloc((size_t)L.nsegs, sizeof(int)) : NULL;
    if (entropy) jpg_fill_segments(&s, &L, stage, in_gpu, slot_of_seg);
    coded_slots_finish(&f, &s, cb->rgb_gpu, rgb_dev, w, h, pitch);
    /* one copy; then, for the entropy decode, its launch and the one wait of its own (for its status words); then two launches */
    check_mi355(mi355_h2d(in_gpu, stage, L.in, net->stream), entropy ? "upload jpeg streams" : "upload jpeg coefficients");
    if (entropy) {
        check_mi355(mi355_memset(net->jpg_coef_gpu, 0, L.coef, net->stream), "zero jpeg coefficients");
        check_mi355(mi355_jpeg_entropy((const mi355_jpeg_segment *)(in_gpu + L.off_segs), (const mi355_jpeg_segment *)(stage + L.off_segs), L.nsegs,
                                       net->jpg_subseq_bits ? net->jpg_subseq_bits : 1024, (int *)net->jpg_status_gpu, net->stream), "mi355_jpeg_entropy");
        check_mi355(mi355_d2h(net->jpg_status_host, net->jpg_status_gpu, status_bytes, net->stream), "read jpeg status");
        net_wait(net); /* the upload has completed with it: nothing is left pending */
        int bad = 0;
        while (bad < L.nsegs && !net->jpg_status_host[bad]) ++bad;
        if (bad < L.nsegs) snprintf(jpg_err, sizeof(jpg_err), "jpeg slot %d: %s (device)", slot_of_seg[bad], jpg_entropy_reason(net->jpg_status_host[bad]));
        free(slot_of_seg);
        if (bad < L.nsegs) return MI355_EINVAL;
    } else
        cb->upload_pending = 1;
    check_mi355(mi355_jpeg_idct((const mi355_jpeg_plane *)in_gpu, (const mi355_jpeg_plane *)stage, L.nplanes, net->stream), "mi355_jpeg_idct");
    check_mi355(mi355_jpeg_to_rgb((const mi355_jpeg_image *)(in_gpu + L.off_images), (const mi355_jpeg_image *)(stage + L.off_images), s.nu, net->stream),
                "mi355_jpeg_to_rgb");
    return MI355_OK;
}

int network_frames_jpeg_input_gpu(network *net, const uint8_t *const *data, const size_t *bytes, int *w, int *h)
{
    return coded_frames_input(net, data, bytes, w, h, network_jpeg_decode_gpu, jpg_err, "network_frames_jpeg_input_gpu: null argument",
                              "network_frames_jpeg_input_gpu: JPEG images feed 3-channel networks only");
}

/* ------------------------------------------------------------------------------------------------- PNG input
 * The host parses the chunks and inflates (png.c), the device does the rest (png.hip): the staging block -- segment table, image table,
 * palettes, filtered bytes -- goes up, then mi355_png_unfilter over every pass of every image and mi355_png_to_rgb over every image.
 *
 * With set_png_inflate_on_device the host only finds the deflate streams (png_scan.c).  The staging block then holds segment table,
 * image table, palettes, stream table and the compressed bytes; the filtered bytes get a device buffer of their own, which
 * mi355_png_inflate fills; its status words come back (the call's one wait of its own), and the two launches follow on those bytes. */
static _Thread_local char png_err[CODED_ERR_LEN];
const char *network_png_last_error(void) { return png_err; }

void set_png_inflate_on_device(network *net, int on) { net->png_inflate_on_device = on != 0; }

typedef dnq_png_scan png_item; /* z: with the inflate on the device only */

static int png_item_decode(const uint8_t *data, size_t bytes, void *item, char *why, size_t whylen)
{
    return png_decode_host(data, bytes, &((png_item *)item)->im, why, whylen);
}

static int png_item_scan(const uint8_t *data, size_t bytes, void *item, char *why, size_t whylen)
{
    png_item *it = item;
    if (png_scan_host(data, bytes, it, why, whylen)) return -1;
    const char *big = it->im.filtered_bytes >= ((size_t)1 << 31) ? "2^31 or more filtered bytes: inflate this image on the host" :
                      it->nbytes > ((size_t)1 << 28) ? "more than 2^28 compressed bytes: inflate this image on the host" : NULL;
    if (!big) return 0;
    snprintf(why, whylen, "%s", big);
    png_scan_free(it);
    memset(it, 0, sizeof(*it));
    return -1;
}

static void png_item_release(void *item)
{
    png_free(&((png_item *)item)->im);
    png_scan_free(item);
}

typedef struct {
    int inflate; /* the inflate runs on the device; without it the staging block has no stream table and filt is 0 */
    int nsegs;
    size_t off_images, off_pal, off_streams; /* into the staging block; the segment table is at 0 */
    size_t in, filt, work, rgb;              /* what the call needs of every buffer */
} png_layout;

/* The layout of the staging block (= of its device copy), of the filtered bytes on the device (inflate), of the reconstructed passes
 * and of the frames, in one walk that serves twice like jpg_walk: with stage == NULL it only sizes, with the staging block it fills
 * the segment table, the image table, the palettes and the stream table and copies the filtered bytes, or the compressed ones.
 * slot_of_stream[i] (inflate): the slot stream i came with. */
static void png_walk(const coded_slots *s, png_layout *L, uint8_t *stage, const coded_bufs *cb, uint8_t *filt_gpu, int *slot_of_stream)
{
    const png_item *items = (const png_item *)s->items;
    size_t in = 0, filt = 0, work = 0, rgb = 0;
    take(&in, sizeof(mi355_png_segment) * (size_t)L->nsegs);
    L->off_images = take(&in, sizeof(mi355_png_image) * (size_t)s->nu);
    L->off_pal = take(&in, 768 * (size_t)s->nu);
    L->off_streams = take(&in, L->inflate ? sizeof(mi355_png_stream) * (size_t)s->nu : 0);
    if (stage) memset(stage, 0, in); /* the tables */
    mi355_png_segment *segs = (mi355_png_segment *)stage;
    uint8_t *in_gpu = cb->in_gpu;
    int si = 0;
    for (int b = 0; b < s->n; ++b) {
        if (s->first[b] != b) continue;
        const dnq_png *p = &items[b].im;
        const int i = s->frame[b];
        mi355_png_image *g = stage ? (mi355_png_image *)(stage + L->off_images) + i : NULL;
        const coded_frame o = s->out[i] = coded_frame_take(&rgb, p->w, p->h);
        const size_t bytes_at = L->inflate ? take(&in, items[b].zcap) : take(&in, p->filtered_bytes);
        const size_t filt_at = L->inflate ? take(&filt, p->filtered_bytes) : 0;
        const uint8_t *filtered = L->inflate ? filt_gpu + filt_at : in_gpu + bytes_at;
        if (stage) {
            g->rgb = (uint8_t *)cb->rgb_gpu + o.at; g->w = o.w; g->h = o.h; g->pitch = o.pitch;
            g->depth = p->depth; g->color = p->color; g->interlace = p->interlace; g->pal_len = p->pal_len;
            if (p->color == 3) {
                memcpy(stage + L->off_pal + 768 * (size_t)i, p->palette, 768);
                g->palette = in_gpu + L->off_pal + 768 * (size_t)i;
            }
            if (L->inflate) {
                mi355_png_stream *t = (mi355_png_stream *)(stage + L->off_streams) + i;
                memcpy(stage + bytes_at, items[b].z, items[b].zcap); /* the zero bytes behind the stream included */
                t->z = (const uint32_t *)(in_gpu + bytes_at); t->nbytes = (uint32_t)items[b].nbytes;
                t->out = filt_gpu + filt_at; t->cap = (uint32_t)p->filtered_bytes;
                t->npasses = p->npasses;
                for (int k = 0; k < p->npasses; ++k) { t->rows[k] = p->pass[k].rows; t->row_bytes[k] = p->pass[k].row_bytes; }
                slot_of_stream[i] = b;
            } else
                memcpy(stage + bytes_at, p->filtered, p->filtered_bytes);
        }
        for (int k = 0; k < p->npasses; ++k, ++si) {
            const dnq_png_pass *q = &p->pass[k];
            const size_t rows_at = take(&work, (size_t)q->rows * (size_t)q->row_bytes);
            if (!stage) continue;
            segs[si].filtered = filtered + q->offset;
            segs[si].out = (uint8_t *)cb->work_gpu + rows_at;
            segs[si].row_bytes = q->row_bytes; segs[si].rows = q->rows; segs[si].bpp = p->bpp;
            g->pass[q->index] = segs[si].out;
        }
    }
    L->in = in; L->filt = filt; L->work = work; L->rgb = rgb;
}

int network_png_decode_gpu(network *net, const uint8_t *const *data, const size_t *bytes, int n, uint8_t **rgb_dev, int *w, int *h, int *pitch)
{
    static const char oom[] = "network_png_decode_gpu: out of memory";
    if (!net || !data || !bytes || !rgb_dev || !w || !h || !pitch || n < 1 || n > 65535)
        return coded_refuse(png_err, "network_png_decode_gpu: null argument / need 1 <= n <= 65535");
    const int inflate = net->png_inflate_on_device;
    const coded_format f = {"png", png_err, sizeof(png_item), inflate ? png_item_scan : png_item_decode, png_item_release};
    coded_slots s;
    if (coded_slots_decode(&f, data, bytes, n, &s, oom)) return MI355_EINVAL;
    png_layout L = {.inflate = inflate};
    for (int b = 0; b < n; ++b) L.nsegs += ((const png_item *)s.items)[b].im.npasses; /* the items of the other slots are empty */
    coded_bufs *cb = &net->png;
    png_walk(&s, &L, NULL, cb, NULL, NULL);
    const int nstreams = inflate ? s.nu : 0;
    const size_t status_bytes = sizeof(int) * (size_t)nstreams;
    if (net->png_status_bytes < status_bytes) {
        free(net->png_status_host);
        net->png_status_host = malloc(status_bytes);
        if (!net->png_status_host) error(oom);
    }
    const coded_want want[] = {{&cb->in_gpu, &cb->in_bytes, L.in, inflate ? "alloc png streams" : "alloc png scanlines"},
                               {&net->png_filt_gpu, &net->png_filt_bytes, L.filt, "alloc png scanlines"},
                               {&cb->work_gpu, &cb->work_bytes, L.work, "alloc png passes"},
                               {&cb->rgb_gpu, &cb->rgb_bytes, L.rgb, "alloc png frames"},
                               {&net->png_status_gpu, &net->png_status_bytes, status_bytes, "alloc png status"}};
    uint8_t *stage = coded_begin(net, cb, want, 5, L.in, oom), *in_gpu = cb->in_gpu;
    int *slot_of_stream = inflate ? calloc((size_t)nstreams, sizeof(int)) : NULL;
    if (inflate && !slot_of_stream) error(oom);
    png_walk(&s, &L, stage, cb, net->png_filt_gpu, slot_of_stream);
    coded_slots_finish(&f, &s, cb->rgb_gpu, rgb_dev, w, h, pitch);
    /* one copy; then, for the inflate, its launch and the one wait of its own (for its status words); then two launches */
    check_mi355(mi355_h2d(in_gpu, stage, L.in, net->stream), inflate ? "upload png streams" : "upload png scanlines");
    if (inflate) {
        check_mi355(mi355_png_inflate((const mi355_png_stream *)(in_gpu + L.off_streams), (const mi355_png_stream *)(stage + L.off_streams), nstreams,
                                      (int *)net->png_status_gpu, net->stream), "mi355_png_inflate");
        check_mi355(mi355_d2h(net->png_status_host, net->png_status_gpu, status_bytes, net->stream), "read png status");
        net_wait(net); /* the upload has completed with it: nothing is left pending */
        int bad = 0;
        while (bad < nstreams && !net->png_status_host[bad]) ++bad;
        if (bad < nstreams) snprintf(png_err, sizeof(png_err), "png slot %d: %s (device)", slot_of_stream[bad], png_inflate_reason(net->png_status_host[bad]));
        free(slot_of_stream);
        if (bad < nstreams) return MI355_EINVAL;
    } else
        cb->upload_pending = 1;
    check_mi355(mi355_png_unfilter((const mi355_png_segment *)in_gpu, (const mi355_png_segment *)stage, L.nsegs, net->stream), "mi355_png_unfilter");
    check_mi355(mi355_png_to_rgb((const mi355_png_image *)(in_gpu + L.off_images), (const mi355_png_image *)(stage + L.off_images), s.nu, net->stream),
                "mi355_png_to_rgb");
    return MI355_OK;
}

int network_frames_png_input_gpu(network *net, const uint8_t *const *data, const size_t *bytes, int *w, int *h)
{
    return coded_frames_input(net, data, bytes, w, h, network_png_decode_gpu, png_err, "network_frames_png_input_gpu: null argument",
                              "network_frames_png_input_gpu: PNG images feed 3-channel networks only");
}
