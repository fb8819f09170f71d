/*
 * darknet_q.h -- plain-C host side of the MI355X INT8 path (libdarknet_q.so, ./darknet).
 *
 * Mirrors the reference's host interface for the quantized inference path only, with the same names, argument
 * meaning and error behaviour (die via error(), ref: src/utils.c:232-237), so a darknet user finds what they know:
 *
 *   struct layer { forward, forward_gpu, ... quant fields }   ref: include/darknet.h:154-226, 471-491
 *   struct network                                            ref: include/darknet.h:562-639
 *   parse_network_cfg / load_weights / load_network           ref: src/parser.c:682-815, 1201-1305; src/network.c:49
 *   set_batch_network                                         ref: src/network.c:383-397
 *   quantization_weights_and_activations                      ref: src/blas.c:259-346
 *   forward_network / forward_network_gpu / network_predict   ref: src/network.c:229-261, 835-861, 570-581
 *
 * What differs, on purpose:
 *   * `forward` (the CPU function pointer) is not a compute path here: it is set to a function that dies with a
 *     message.  This build has exactly one data path, `forward_gpu` -> libmi355yolo.so (HIP, gfx950).
 *   * the network carries a device uint8 activation pointer (the reference's GPU executor only threads floats,
 *     ref: src/network.c:835-861) and batch > 1 means "the batch-1 function applied per image" (the reference's
 *     epilogue handles image 0 only, ref: src/convolutional_layer.c:726-751).
 *   * quantization_weights_and_activations() is idempotent (the reference's accumulates weights_sum_int and
 *     re-folds batch-norm on every call, ref: src/blas.c:285-286,309 -- valid for the first call only, which is the
 *     behaviour reproduced).
 */
#ifndef DARKNET_Q_H
#define DARKNET_Q_H
#include <stddef.h>
#include <stdint.h>
#include "mi355_yolo_int8.h"

#ifdef __cplusplus
extern "C" {
#endif

/* same enumerator values as the reference (include/darknet.h:87-89, 99-130) */
typedef enum { LOGISTIC = 0, RELU = 1, LINEAR = 3, RELU6 = 8, LEAKY = 9 } ACTIVATION;
typedef enum { CONVOLUTIONAL = 0, MAXPOOL = 3, ROUTE = 8, SHORTCUT = 13, YOLO = 23, UPSAMPLE = 26 } LAYER_TYPE;

/* layer.fuse_next: the layer after a conv that runs inside the conv's kernel.  The type of that layer decides the kind */
enum { FUSE_NONE = 0, FUSE_POOL, FUSE_UPSAMPLE, FUSE_SHORTCUT, FUSE_YOLO };

#define QUANT_POSITIVE_LIMIT 255
#define QUANT_NEGATIVE_LIMIT 0

struct network;
typedef struct network network;
struct layer;
typedef struct layer layer;

struct layer {
    LAYER_TYPE type;
    ACTIVATION activation;
    void (*forward)(struct layer, struct network);     /* dies: no CPU data path in this build */
    void (*forward_gpu)(struct layer, struct network); /* HIP path */

    int batch, h, w, c, out_h, out_w, out_c;
    int n, size, stride, pad, groups;
    int inputs, outputs, nweights, batch_normalize;
    int count; /* layer index */

    /* quantization fields, same names as the reference */
    int close_quantization, layer_quant_flag, quant_stop_flag, fisrt_time_train_fag;
    float *input_data_uint8_scales, *activ_data_uint8_scales, *weight_data_uint8_scales;
    uint8_t *input_data_uint8_zero_point, *activ_data_uint8_zero_point, *weight_data_uint8_zero_point;
    int32_t *weights_sum_int;
    uint32_t *mult_zero_point;
    float *M;
    int32_t *M0;
    int *M0_right_shift;
    double *M_value, *M0_right_shift_value;
    uint8_t *weights_uint8;
    int32_t *biases_int32;
    float *biases, *scales, *rolling_mean, *rolling_variance;

    /* route */
    int *input_layers, *input_sizes;
    /* shortcut (quantized residual add, builder-specified: mi355_shortcut_forward): `index` = the layer added to the
     * previous layer's output (ref field name, src/shortcut_layer.c:28), the two 16.16 multipliers of the prep */
    int index;
    int32_t shortcut_Ka, shortcut_Kb;
    /* yolo */
    int classes, total;
    int *mask;
    float *anchors; /* the reference calls this l.biases for yolo layers */
    float *anchors_gpu, *det_recs_gpu; /* on-device box decode (network_yolo_detections_gpu): anchors, records, counts */
    int *mask_gpu, *det_counts_gpu, det_cap;
    int *det_sizes_gpu; /* [2][batch] source widths, heights (network_yolo_detections_gpu_sizes) */

    /* host mirrors of the outputs, reference layout (filled by pull_layer_output) */
    float *output;               /* [batch][outputs] float (quant_stop convs, yolo) */
    int32_t *output_int32;       /* [batch][outputs] pre-requant accumulators (conv) */
    uint8_t *output_uint8_final; /* [batch][outputs] */

    /* device side */
    mi355_tensor out_t;            /* PHWC uint8 activations */
    int out_view;                  /* out_t.data is a channel window of a later route layer's buffer (not owned) */
    int route_elided;              /* route: every input already writes into out_t (see plan_views) -- no copy at run time */
    void *blob_gpu;                /* packed weights + per-channel params (mi355_conv_pack) */
    int blob_shared;               /* 1: blob_gpu belongs to the network this one is a replica of (network_replica): never freed / re-uploaded here */
    size_t blob_bytes;
    void *blob_host;
    uint8_t *weights_uint8_gpu;    /* raw weights / zero points for the ref-f32 verification mode */
    uint8_t *weight_zero_point_gpu;
    int32_t *output_int32_gpu;     /* reference layout; allocated only when net->dump_int32 */
    float *output_gpu;             /* reference layout float (quant_stop convs, yolo) */
    uint8_t *output_uint8_nchw_gpu; /* scratch for pull_layer_output */
    int input_direct;   /* layer 0 only.  1: it is fed the network's input_nchw_t, no conversion pass; its forward_gpu clears it on the
                           first MI355_EINVAL */
    int fuse_next;      /* FUSE_*: the planner's candidate (plan_fusion); a launcher's refusal sets it back to FUSE_NONE.
                           POOL: this conv and the 2x2 maxpool (stride 2, or stride 1 behind a 128 / 256-channel conv) after it run as
                           one kernel.  UPSAMPLE: it stores its pixels straight into the upsample layer's tensor.  SHORTCUT: its epilogue
                           also does the quantized residual add of the [shortcut].  YOLO: this quant_stop head conv also writes the yolo
                           layer's activations */
    int fuse_pool_keep; /* FUSE_POOL which also stores the conv's own tensor: a route reads it */
    int conv_kernel;    /* kernel family that served this conv's last forward (mi355_last_conv_kernel) */
    int prepared;
};

/* The buffers of one coded-image input path (JPEG, PNG): lazily allocated, grown when needed, freed with the network. */
typedef struct coded_bufs {
    void *stage_host;           /* host staging block: the format's tables, then the bytes the device reads */
    size_t stage_bytes;
    void *in_gpu;               /* its device copy, the same layout */
    size_t in_bytes;
    void *work_gpu;             /* what the first launch writes for the second: component planes (JPEG), reconstructed passes (PNG) */
    size_t work_bytes;
    void *rgb_gpu;              /* the RGB frames of the last call */
    size_t rgb_bytes;
    int upload_pending;         /* an upload from the staging block may be in flight: wait before rewriting it */
} coded_bufs;

struct network {
    int n, batch;
    layer *layers;
    int h, w, c, inputs, outputs;
    size_t *seen;
    float *input;         /* host float CHW image(s) (layer-0 quantiser input) */
    uint8_t *input_uint8; /* host [batch][c][h][w] */
    float *output;
    int train, index;
    int close_quantization;

    /* device side */
    int gpu_index;
    void *stream;
    uint8_t *input_uint8_gpu; /* reference layout on the device */
    float *quant_mm_gpu;      /* device scratch of the layer-0 quantiser: max, min of the float image */
    float *input_gpu;         /* batch x inputs floats on the device: the letterboxed images of the device input path */
    mi355_tensor input_t;     /* cs==4 image tensor */
    mi355_tensor input_nchw_t; /* input_uint8_gpu described as it is (planar): layer 0 reads it in place where its kernel can */
    int input_direct_off;     /* user knob (dnq_net_set "input_direct" 0): never feed the planes directly, whatever is re-allocated */
    const mi355_tensor *cur_t; /* uint8 hand-off: the reference's `net.input_uint8 = l.output_uint8_final` */
    const float *cur_f32_gpu;  /* float hand-off: `net.input = l.output` */

    /* knobs (CLI: -accum exact|ref-f32, -parity wrap|saturate) */
    int accum_mode, store_mode;
    int dump_int32; /* keep int32 accumulators of every conv (parity runs) */
    int keep_head_float; /* 0 (default): a head conv fused with its yolo layer does not store its own float tensor (l.output: an
                            intermediate only the yolo layer reads); 1: it does (per-layer parity dumps) */
    int fuse_maxpool; /* 1 (default): all four fused forms are on: a conv runs the maxpool / upsample / [shortcut] / yolo layer after it
                         in its own kernel where plan_fusion marks it (layer.fuse_next); a fused conv's own tensor is not stored unless
                         something else reads it.  0: every layer writes its own tensor like the reference (per-layer parity dumps) */
    int verbose;
    int prepared;
    int range_lo, range_hi; /* diagnostic (tools/layer_flood.py): forward_network_gpu runs layers [range_lo, range_hi) only, on the tensors the
                               last full pass left behind; 0, 0 = the whole network */
    int on_default_stream; /* this executor launches on the device's default (NULL) stream and owns no stream of its own */
    int replica_default_stream; /* set before network_replica(): the NEXT replica runs on the default stream.  HIP keeps one of the
                                   device's four hardware queues for that stream and maps every created stream onto the other three:
                                   a fourth batch in flight only runs beside the other three from there (bench: 0.2719 -> 0.2671 ms
                                   per step; a fourth created stream shares a queue with the first: 0.2719 -> 0.30).  Only for hosts
                                   that put nothing else on the default stream. */
    int plan;             /* MI355_PLAN_*: handed to every conv launch; network_replica switches parent and replica to the throughput plan
                             (change it with network_set_plan, which also re-derives the fusion plan and drops a captured graph) */
    int plan_user;        /* the plan the caller asked for (network_set_plan); a parent returns to it when its last replica is freed */
    int has_host_weights; /* load_weights ran: raw weights_uint8 / biases / scales of every layer are on the host */
    int has_l0_weights;   /* imported from a packed exchange: blobs only, plus layer 0's raw record (re-prep on a new input scale) */
    char *cfg_path;       /* the cfg this network was parsed from (network_replica parses it again) */
    struct network *replica_of; /* non-NULL: a replica (network_replica): packed weights on the device are the parent's */
    int n_replicas;             /* live replicas of this network: it cannot be freed, re-batched or re-prepared while > 0 */
    uint64_t *selfcheck_gpu; /* [passes] checksums of the pending self-check */
    int selfcheck_passes;
    void *graph; /* hipGraph of the layer loop, built lazily when use_graph */
    int use_graph;
    /* per-layer HIP-event timing on net->stream (replaces the commented what_time_is_it_now() probes of
     * ref: src/network.c:244-246) */
    void **prof_ev;      /* [prof_cap][n+2] events */
    int prof_cap, prof_used;
    int prof_stride, prof_calls; /* events are recorded on every prof_stride-th forward (they cost ~2.4 us per layer) ... */
    int prof_phase;              /* ... the ones with call index % prof_stride == prof_phase */
    /* per-image input quantisation (set_input_quantization_per_image): layer 0 runs on a bank of blobs, one per distinct
     * (scale, zero point) of the batch; the bank's slots are a cache keyed by (scale bits, zero point).  A replica owns its own. */
    int per_image;
    void *pi_bank_gpu, *pi_bank_host; /* [pi_cap] layer-0 blobs, pi_entry_bytes apart (host: staging of the uploads) */
    size_t pi_entry_bytes;
    int pi_cap;
    uint32_t *pi_key_scale;     /* [pi_cap] float bits of the slot's input scale */
    int *pi_key_zp;             /* [pi_cap] its zero point, -1: empty */
    long *pi_stamp;             /* [pi_cap] last batch that used the slot */
    long pi_tick;
    void *pi_idx_gpu, *pi_idx_host; /* [B] int32 entry | [B] float scale | [B] uint8 zero point */
    float *pi_mm_gpu, *pi_mm_host;  /* [B][2] max, min */
    int pi_packed;              /* bank entries packed by the last batch (the others came from the cache) */
    /* Frame input (network_frames_u8 / _nv12 / _planar / _packed / _p010 / _bayer_input_gpu): lazily allocated, sized by the batch, freed with the network and on
     * re-batch.  A replica owns its own. */
    void *fr_arena_gpu;         /* staging of host frames: the bytes as they came, rows at their pitch, 256-byte aligned planes */
    size_t fr_arena_bytes;
    void *fr_table_gpu, *fr_table_host; /* [fr_cap] entries of the kind last fed (mi355_frame_u8 | _yuv | _planar | _packed | _p010 | _bayer) and their host mirror:
                                           one table for every kind, sized for the largest entry */
    int fr_kind;                /* the kind of frames in the table */
    float *fr_mm_gpu, *fr_mm_host; /* [fr_cap][2] max, min */
    void *fr_pair_gpu, *fr_pair_host; /* shared-scale mode: [fr_cap] float scale | [fr_cap] uint8 zero point, image 0's in every slot */
    int fr_cap;
    mi355_frame_view *fr_views; /* network_set_frame_views: [batch] views, the network's copy; NULL: every slot is its whole frame as stored.  Cleared on re-batch */
    void *fr_views_gpu;         /* [fr_cap] mi355_frame_view, uploaded beside the frame table while views are set */
    /* JPEG input (network_jpeg_decode_gpu).  The staging block holds plane table | image table | quantiser tables | coefficients, the
     * work buffer the component planes the inverse DCT writes.  A replica owns its own. */
    coded_bufs jpg;
    /* set_jpeg_entropy_on_device: the staging block then holds plane table | image table | quantiser tables | segment table | Huffman
     * tables | unstuffed scan bytes, and the coefficients exist on the device only */
    int jpg_entropy_on_device;
    int jpg_subseq_bits;        /* bits a lane decodes per round (mi355_jpeg_entropy); 0: the default, 1024 */
    void *jpg_coef_gpu;         /* the coefficient planes mi355_jpeg_entropy fills */
    size_t jpg_coef_bytes;
    void *jpg_status_gpu;       /* one status word per segment of the last call */
    int *jpg_status_host;       /* their host copy */
    size_t jpg_status_bytes;
    /* PNG input (network_png_decode_gpu).  The staging block holds segment table | image table | palettes | filtered bytes, the work
     * buffer the reconstructed passes mi355_png_unfilter writes.  A replica owns its own. */
    coded_bufs png;
    /* set_png_inflate_on_device: the staging block then holds segment table | image table | palettes | stream table | compressed bytes,
     * and the filtered bytes exist on the device only */
    int png_inflate_on_device;
    void *png_filt_gpu;         /* the filtered bytes mi355_png_inflate writes */
    size_t png_filt_bytes;
    void *png_status_gpu;       /* one status word per stream of the last call */
    int *png_status_host;       /* their host copy */
    size_t png_status_bytes;
    /* Batched box decode (network_yolo_detections_batch_gpu): lazily allocated, grown when needed, freed with the network and on
     * re-batch.  A replica owns its own. */
    int *detb_ints_gpu, *detb_ints_host; /* [2][batch] source sizes | counts [batch][nheads] | offsets [batch + 1] */
    int *detb_work_gpu;                  /* mi355_yolo_detections_batch's scratch */
    float *detb_recs_gpu;                /* packed records of the batch */
    int detb_batch, detb_nheads;         /* what detb_ints_* are sized for */
    long detb_work_ints;
    size_t detb_recs_cap;                /* records detb_recs_gpu holds */
    /* Input quantisation on the device (set_input_quantization_on_device): pairs and layer-0 bank entries are derived in HBM
     * (mi355_input_pairs, mi355_l0_derive), one slot per image, each initialised with the prepared layer-0 blob.  Lazily allocated,
     * sized by the batch, freed with the network and on re-batch.  A replica owns its own, its copy of the constant table included. */
    int input_on_device;
    void *od_bank_gpu;                   /* [od_cap] layer-0 blobs, pi_entry_bytes apart */
    int od_cap;
    void *od_idx_gpu;                    /* [B] int32 entry | [B] float scale | [B] uint8 zero point (pi_idx_gpu's layout) */
    void *od_kept_gpu;                   /* [B] float scale | [B] uint8 zero point: the pair every image's entry stands for */
    uint32_t *od_status_gpu;             /* [B] MI355_INPUT_* bits of the last batch */
    float *od_mm_gpu;                    /* [B][2] max, min of the float path */
    void *od_const_gpu, *od_const_host;  /* mi355_l0_consts + n mi355_l0_channel */
    long host_waits;                     /* times the host library waited for the device on this network's behalf (network_host_waits) */
};

/* ---- construction / IO ------------------------------------------------------------------------------------ */
network *parse_network_cfg(char *filename, int close_quantization);
void load_weights(network *net, char *filename);
network *load_network(char *cfg, char *weights, int clear);
void set_batch_network(network *net, int b);
void free_network(network *net);

/* ---- host prep (M0/shift/biases_int32, packing, upload, device buffers) ------------------------------------ */
void quant_multi_smaller_than_one_to_scale_and_shift(float real_multiplier, int32_t *quantized_multiplier,
                                                     int *right_shift);
void quant_image_with_min_max(int count, const float *input, uint8_t *out, float *scale, uint8_t *zero_point);
void quantization_weights_and_activations(network *net);
/* same, but with the layer-0 input scale / zero point given instead of derived from net->input (serving mode:
 * uint8 images arrive already quantised) */
void quantization_weights_and_activations_fixed_input(network *net, float in_scale, uint8_t in_zp);
/* the layer-0 quantiser (ref: src/blas.c:279 -> :108-168) on float images already in HBM: device min / max + quantise,
 * layer 0 re-derived only when scale / zero point change */
void quantization_weights_and_activations_gpu(network *net, const float *input_gpu);
/* Input path on the device: letterbox_image (ref: src/image.c:812-831) of a planar float image in HBM
 * into batch slot `slot` of the network's float input, then the layer-0 quantiser over the whole batch. */
void network_letterbox_input_gpu(network *net, int slot, const float *im_gpu, int imw, int imh);
void network_quantize_input_gpu(network *net);
/* The whole input step for a batch of 8-bit interleaved frames as a decoder delivers them, without a float image anywhere: frames[b] holds
 * h[b] rows of w[b] pixels, three bytes each in `order` (MI355_FRAME_RGB / MI355_FRAME_BGR), rows pitch[b] bytes apart (pitch == NULL:
 * 3 * w[b]); one entry per batch slot, sizes may differ.  frames_on_device == 0: host pointers, the bytes go up as they are into a
 * staging arena the network owns (grown lazily, reused); != 0: device pointers, used in place (they must stay valid until the network's
 * stream has run the call).  Then: frame table upload, letterbox + min / max of the batch in one launch
 * (mi355_frames_u8_letterbox_minmax), the batch's one d2h + host sync, (scale, zero point) per image with the reference's expressions;
 * with per-image quantisation on, the layer-0 bank is updated, otherwise image 0's pair serves every slot and layer 0 is re-derived when
 * the pair changed (the branches, and errors, of quantization_weights_and_activations_gpu); last the quantiser launch
 * (mi355_frames_u8_letterbox_quantize) into the network's uint8 input.  Bytes, scales and zero points equal
 * network_letterbox_input_gpu on every frame's planes (byte / 255.f) + network_quantize_input_gpu, bit for bit.  3-channel networks only;
 * a frame the letterbox cannot serve, a pitch below 3 * w or a null pointer die via error() before anything is launched. */
void network_frames_u8_input_gpu(network *net, const uint8_t *const *frames, const int *w, const int *h, const int *pitch, int order,
                                 int frames_on_device);
/* The same step for NV12 / NV21 frames as video decoders and camera stacks deliver them (layout: MI355_YUV_NV12 / MI355_YUV_NV21):
 * y[b] holds h[b] rows of w[b] luma bytes pitch_y[b] bytes apart, uv[b] (h[b] + 1) / 2 rows of (w[b] + 1) / 2 chroma pairs pitch_uv[b]
 * bytes apart (a null pitch array: tightly packed planes).  Both planes go up as they are -- half the bytes of the RGB frame -- and are
 * converted in registers with the integer formulas and the `matrix` (MI355_YUV_BT601 .. MI355_YUV_BT709_FULL) of mi355_frame_yuv
 * (mi355_yolo_int8.h); no RGB frame exists anywhere.  The result is, bit for bit, network_frames_u8_input_gpu's on the RGB frame those
 * formulas give; arena, min / max and pair buffers, the one host sync and both (scale, zero point) branches are that function's.
 * frames_on_device != 0: the plane pointers are device pointers (a decoder's surfaces), used in place. */
void network_frames_nv12_input_gpu(network *net, const uint8_t *const *y, const uint8_t *const *uv, const int *w, const int *h,
                                   const int *pitch_y, const int *pitch_uv, int layout, int matrix, int frames_on_device);
/* The same step for frames of three separate planes, as software decoders (yuv420p), JPEG decoders and [3][h][w] tensors deliver them
 * (format: MI355_PLANAR_I420, _YV12, _I422, _I444, _RGB, _BGR of mi355_frame_planar, mi355_yolo_int8.h).  p0[b], p1[b], p2[b] are
 * frame b's planes in the order the format names them: p0 holds h[b] rows of w[b] bytes, p1 and p2 the format's chroma size
 * ((w + 1) / 2 wide in I420 / YV12 / I422, (h + 1) / 2 high in I420 / YV12, else w and h), rows pitch0[b], pitch1[b], pitch2[b] bytes
 * apart (a null pitch array: that plane is tightly packed).  The three planes go up as they are and the YUV formats are converted in
 * registers with `matrix` (MI355_YUV_BT601 .. MI355_YUV_BT709_FULL; 0 with the RGB formats), chroma at [y >> sy][x >> sx]: I420 gives,
 * bit for bit, network_frames_nv12_input_gpu's result on the interleaved chroma planes, every format network_frames_u8_input_gpu's
 * on the interleaved RGB frame of the same pixels.  Arena, min / max and pair buffers, the one host sync and both (scale, zero point)
 * branches are that function's.  frames_on_device != 0: the plane pointers are device pointers, used in place. */
void network_frames_planar_input_gpu(network *net, const uint8_t *const *p0, const uint8_t *const *p1, const uint8_t *const *p2,
                                     const int *w, const int *h, const int *pitch0, const int *pitch1, const int *pitch2,
                                     int format, int matrix, int frames_on_device);
/* The same step for frames of one packed plane of 4-byte groups (format: MI355_PACKED_* of mi355_frame_packed, mi355_yolo_int8.h):
 * RGBA, BGRA, ARGB, ABGR -- a pixel is four bytes, the fourth is never looked at, pitch[b] >= 4 * w[b], matrix must be 0 -- as display
 * surfaces, screen capture and decoder post-processing deliver them, and YUYV (YUY2), UYVY, YVYU -- a macropixel of two pixels is
 * four bytes, pitch[b] >= 4 * ((w[b] + 1) / 2), converted in registers with `matrix` (MI355_YUV_BT601 .. MI355_YUV_BT709_FULL) and chroma
 * at [y][x >> 1] -- as USB / V4L2 cameras deliver them.  frames[b] holds h[b] rows pitch[b] bytes apart (a null pitch array: tightly
 * packed rows of whole groups); the bytes go up as they are.  The result is, bit for bit, network_frames_u8_input_gpu's on the RGB
 * frame of the same pixels, and for the 4:2:2 formats network_frames_planar_input_gpu's on the MI355_PLANAR_I422 frame of the
 * de-interleaved samples.  Arena, min / max and pair buffers, the one host sync and both (scale, zero point) branches are that
 * function's.  frames_on_device != 0: device pointers, used in place.  3-channel networks only; an unknown format or matrix, a matrix
 * with an RGB format, a null pointer, w or h outside 1..32768 or a pitch below its minimum die via error() before the device is
 * touched. */
void network_frames_packed_input_gpu(network *net, const uint8_t *const *frames, const int *w, const int *h, const int *pitch, int format,
                                     int matrix, int frames_on_device);
/* The same step for P010 / P012 / P016 frames as hardware decoders deliver 10-bit streams: NV12's two planes with 16-bit little-endian
 * samples, the significant bits at the top.  y[b] holds h[b] rows of w[b] samples pitch_y[b] BYTES apart (>= 2 * w[b]), uv[b]
 * (h[b] + 1) / 2 rows of (w[b] + 1) / 2 (U, V) pairs pitch_uv[b] bytes apart (>= 4 * ((w[b] + 1) / 2)); a null pitch array: tightly
 * packed.  Both planes go up as they are; the device reads the high byte of every sample (truncation, not rounding) and goes on as
 * the NV12 source with `matrix`: the result is, bit for bit, network_frames_nv12_input_gpu's on the MI355_YUV_NV12 frame
 * (y >> 8, uv >> 8).  frames_on_device != 0: device pointers, used in place.  Refusals as above. */
void network_frames_p010_input_gpu(network *net, const uint8_t *const *y, const uint8_t *const *uv, const int *w, const int *h,
                                   const int *pitch_y, const int *pitch_uv, int matrix, int frames_on_device);
/* JPEG images.  The host half (yolo_quantization_amd/host/jpeg.h: jpeg_decode_host, jpeg_info_host, jpeg_free; no device needed) parses
 * a baseline JPEG and decodes its entropy-coded streams into quantised coefficients; the device does the rest -- dequantisation, inverse
 * DCT, chroma upsampling, YCbCr -> RGB (mi355_jpeg_idct, mi355_jpeg_to_rgb) -- and leaves the pixels stbi_load(file, .., 3) returns in
 * the reference (ref: src/image.c:1293-1315), byte for byte, as interleaved RGB frames in device memory.
 *
 * network_jpeg_decode_gpu: data[b], bytes[b] are the n images' files in host memory (slots that name the same bytes are decoded
 * once and share a frame).  All n are entropy-decoded first; if one fails the call returns MI355_EINVAL, network_jpeg_last_error()
 * (a buffer of the calling thread) names the slot and the reason ("jpeg slot 2: progressive JPEG (SOF2) is not supported") and nothing
 * has been launched or uploaded.  Otherwise coefficients and tables go up from one staging block in one copy on the network's stream,
 * the two launches follow, and rgb_dev[b], w[b], h[b], pitch[b] describe image b's frame: device memory the network owns, valid until
 * the next call (on the network's stream: the call only enqueues).  The staging block is not rewritten before the upload that read it
 * has completed (the next call waits for the stream if need be).  Device errors die via error() like everywhere else.
 *
 * network_frames_jpeg_input_gpu: the above for net->batch images, then network_frames_u8_input_gpu on those device frames: both scale
 * modes, set_input_quantization_on_device, replicas and graph replay are that function's.  w[b], h[b] receive every image's size, for
 * the detection calls.  Returns 0, or MI355_EINVAL with network_jpeg_last_error() as above (a frame the letterbox cannot serve still
 * dies in network_frames_u8_input_gpu). */
typedef struct dnq_jpeg dnq_jpeg;
int jpeg_decode_host(const uint8_t *data, size_t bytes, dnq_jpeg *out, char *err, size_t errlen);
int jpeg_info_host(const uint8_t *data, size_t bytes, dnq_jpeg *out, char *err, size_t errlen);
void jpeg_free(dnq_jpeg *j);
int network_jpeg_decode_gpu(network *net, const uint8_t *const *data, const size_t *bytes, int n, uint8_t **rgb_dev, int *w, int *h,
                            int *pitch);
int network_frames_jpeg_input_gpu(network *net, const uint8_t *const *data, const size_t *bytes, int *w, int *h);
const char *network_jpeg_last_error(void);
/* Entropy decoding on the device, opt-in (off: every call above does what it always did).  On: network_jpeg_decode_gpu only FINDS the
 * scans on the host (yolo_quantization_amd/host/jpeg_scan.h: the same headers and the same refusals, which still launch nothing) and
 * uploads their unstuffed bytes and Huffman tables instead of coefficients; mi355_jpeg_entropy decodes every restart interval of every
 * scan of the batch in one launch into planes zeroed on the device, and mi355_jpeg_idct / mi355_jpeg_to_rgb follow as before.  For a
 * file the host decoder accepts and decodes in full the coefficients, and so the frames, are the host path's, bit for bit.  The call
 * reads the segments' status words back and WAITS for them once (it shows in network_host_waits(), also with
 * set_input_quantization_on_device, whose input step is otherwise wait-free): a symbol that decodes to nothing returns MI355_EINVAL
 * with "jpeg slot 2: bad huffman code (device)" (or "bad DC category", "coefficient index past the end of the block"), the frames
 * are not produced and network_frames_jpeg_input_gpu does not go on.  What the host decoder makes of truncated or corrupt data is
 * not reproduced: such a file gives a status or some image, never an access outside the buffers.  A replica made afterwards inherits
 * the mode.  set_jpeg_entropy_subseq_bits: the bits a lane decodes per round, a multiple of 32 in 32 .. 8192 (default 1024). */
void set_jpeg_entropy_on_device(network *net, int on);
void set_jpeg_entropy_subseq_bits(network *net, int bits);
struct dnq_jpeg_scan_list;
int jpeg_scan_host(const uint8_t *data, size_t bytes, dnq_jpeg *out, struct dnq_jpeg_scan_list *scans, char *err, size_t errlen);
void jpeg_scan_free(struct dnq_jpeg_scan_list *scans);
/* PNG images, the mirror of the JPEG calls above.  The host half (yolo_quantization_amd/host/png.h: png_decode_host, png_info_host,
 * png_free; no device needed) parses the chunks and inflates; the device does the rest -- scanline reconstruction, de-interlacing,
 * bit-depth and palette expansion, the reduction to RGB (mi355_png_unfilter, mi355_png_to_rgb) -- and leaves the pixels
 * stbi_load(file, .., 3) returns in the reference, byte for byte, for every colour type, bit depth, filter and for Adam7, as
 * interleaved RGB frames in device memory.
 *
 * network_png_decode_gpu: data[b], bytes[b] are the n images' files in host memory (slots that name the same bytes are decoded once
 * and share a frame).  All n are parsed and inflated first; if one fails the call returns MI355_EINVAL, network_png_last_error() (a
 * buffer of the calling thread) names the slot and the reason ("png slot 2: invalid filter") and nothing has been launched or
 * uploaded.  Otherwise the segment table, the image table, the palettes and the filtered bytes go up from one staging block in one
 * copy on the network's stream, the two launches follow, and rgb_dev[b], w[b], h[b], pitch[b] describe image b's frame: device memory
 * the network owns, valid until the next call (on the network's stream: the call only enqueues and waits for nothing -- "invalid
 * filter" is found on the host).  The staging block is not rewritten before the upload that read it has completed.
 *
 * network_frames_png_input_gpu: the above for net->batch images, then network_frames_u8_input_gpu on those device frames: both scale
 * modes, set_input_quantization_on_device, replicas and graph replay are that function's.  3-channel networks only. */
typedef struct dnq_png dnq_png;
int png_decode_host(const uint8_t *data, size_t bytes, dnq_png *out, char *err, size_t errlen);
int png_info_host(const uint8_t *data, size_t bytes, dnq_png *out, char *err, size_t errlen);
void png_free(dnq_png *p);
int network_png_decode_gpu(network *net, const uint8_t *const *data, const size_t *bytes, int n, uint8_t **rgb_dev, int *w, int *h,
                           int *pitch);
int network_frames_png_input_gpu(network *net, const uint8_t *const *data, const size_t *bytes, int *w, int *h);
const char *network_png_last_error(void);
/* set_png_inflate_on_device(net, 1): network_png_decode_gpu (and network_frames_png_input_gpu) only finds the deflate streams on the host
 * (yolo_quantization_amd/host/png_scan.h: the same headers and the same refusals, which still launch nothing) and uploads the compressed
 * bytes instead of the filtered ones; mi355_png_inflate inflates every image of the batch in one launch, one wave each, into a device
 * buffer of the network, and the two launches follow unchanged.  The frames, and so the network's input, are byte for byte the ones
 * of the host inflate.  A stream the device refuses returns MI355_EINVAL with "png slot <b>: <reason> (device)" -- the host decoder's
 * reason -- after the inflate and before anything else is launched: the call waits once for the status words (network_host_waits()
 * counts it), in this mode only.  An image with 2^31 or more filtered bytes, or more than 2^28 compressed ones, is refused in this
 * mode; the host mode takes it.  Off by default; a replica inherits the mode. */
void set_png_inflate_on_device(network *net, int on);
struct dnq_png_scan;
int png_scan_host(const uint8_t *data, size_t bytes, struct dnq_png_scan *out, char *err, size_t errlen);
void png_scan_free(struct dnq_png_scan *s);
/* The same step for raw sensor frames: one plane with one sample per pixel behind a Bayer colour filter (pattern: MI355_BAYER_RGGB,
 * _BGGR, _GRBG, _GBRG) or none (MI355_BAYER_MONO), as machine-vision cameras (BayerRG8 .., Mono8 .. Mono16) and MIPI CSI-2 sensors
 * without an ISP (RAW10, RAW12) deliver them.  sample: MI355_RAW_U8 (pitch[b] >= w[b]), MI355_RAW_U16 (little-endian, reduced to
 * min(v >> shift, 255), shift 0..8; pitch[b] >= 2 * w[b]), MI355_RAW_MIPI10 (pitch[b] >= 5 * ((w[b] + 3) / 4)) or MI355_RAW_MIPI12
 * (pitch[b] >= 3 * ((w[b] + 1) / 2)); shift must be 0 with the others.  tone: NULL, or [batch] pointers each NULL (identity) or 768
 * bytes, the [3][256] tables (R, G, B) every sample of that frame goes through by the colour of its site before anything is averaged
 * (MONO: table 0).  frames[b] holds h[b] rows pitch[b] bytes apart (a null pitch array: tightly packed); the bytes go up as they are,
 * a frame or a tone table that several slots share goes up once, and the frame is demosaiced bilinearly in registers inside the
 * letterbox: the result is, bit for bit, network_frames_u8_input_gpu's on the RGB frame D(frame) that mi355_yolo_int8.h defines at
 * mi355_frame_bayer.  Arena, min / max and pair buffers, the one host sync and both (scale, zero point) branches are that function's.
 * frames_on_device != 0: frames[b] and tone[b] are device pointers, used in place.  3-channel networks only; an unknown pattern or
 * sample layout, a shift outside 0..8 or without MI355_RAW_U16, a null frame, w or h outside 1..32768, a Bayer frame below 2 x 2 or
 * a pitch below its minimum die via error() before the device is touched. */
void network_frames_bayer_input_gpu(network *net, const uint8_t *const *frames, const int *w, const int *h,
                                    const int *pitch /* NULL: tight */, int pattern, int sample, int shift,
                                    const uint8_t *const *tone /* NULL, or [batch] of NULL | 768 bytes */,
                                    int frames_on_device);
/* Per-image input quantisation, opt-in (off: image 0 defines the scale of the whole batch, as before).  On: every image of a batch is
 * quantised with its own min / max, scale and zero point, and layer 0 runs with that image's constants (mi355_conv_forward_per_image):
 * slot b of every layer equals the batch-1 run on image b.  The quantisers above honour it.  Returns 0, or MI355_EINVAL with a message
 * when layer 0 is not a 3 -> n 3x3 stride-1 convolution (the general kernel is not served per image) or the network holds no raw
 * layer-0 weights to derive the constants from.  A replica made afterwards inherits the mode and keeps its own bank. */
int set_input_quantization_per_image(network *net, int on);
/* layer 0's blob for input scale s / zero point zp into dst (mi355_conv_pack_size bytes): one bank entry, derived by the host prep
 * exactly as the per-image quantisers derive it; the network's layer-0 record is unchanged afterwards.  Host only (no device). */
void network_layer0_entry(network *net, float s, uint8_t zp, void *dst);
/* layer 0's constant table for mi355_l0_derive (mi355_yolo_int8.h: a mi355_l0_consts and one mi355_l0_channel per filter: the folded
 * float bias, weight scale, weight zero point and plain weight sum) into dst; returns its size in bytes, with dst == NULL the size
 * alone.  Host only. */
size_t network_layer0_consts(network *net, void *dst);
/* the (scale, zero point) of every image of the last per-image batch: scale[batch], zp[batch] (with the input quantisation on the
 * device: of the last batch in either scale mode, after waiting for the network's stream) */
void network_input_quantization(network *net, float *scale, uint8_t *zp);
/* Input quantisation on the device, opt-in (off: every call behaves as described above).  On: every device input path --
 * quantization_weights_and_activations_gpu, network_quantize_input_gpu and the five network_frames_*_input_gpu calls -- runs min / max,
 * the (scale, zero point) of every image (mi355_input_pairs), layer 0's constants for them (mi355_l0_derive) and the quantiser as one
 * chain of launches on the network's stream: no copy back, no wait, no host arithmetic, no upload of layer-0 data.  With device frames
 * (frames_on_device != 0) the whole call only enqueues work; host frames are still staged by the call, and since nothing waits for
 * those uploads any more the caller keeps them valid until the network's stream has run the call.  Layer 0 always runs on the
 * network's bank, one slot per image: with per-image quantisation every image has its own pair and entry, without it image 0's pair
 * and entry 0 serve every slot.  Bytes, pairs and bank entries equal the synchronous path's, bit for bit.  A captured graph stays valid
 * whatever the pairs are, in both scale modes.  A network that is not prepared yet is prepared with (1 / 255, 0) by the first call;
 * that, the one-time allocations and a growing staging arena may wait for the device, a steady-state call does not.
 * What kills the synchronous path (an all-zero image, a layer-0 multiplier outside (0, 1), ...) cannot be reported by a call that does
 * not wait: the image's slot keeps the pair and the entry of its previous batch and network_input_status() names the reason.
 * Returns 0, or MI355_EINVAL with a message under set_input_quantization_per_image's conditions.  Switching drops a captured graph.
 * A replica made afterwards inherits the mode. */
int set_input_quantization_on_device(network *net, int on);
/* status[batch] of the last on-device input step: MI355_INPUT_* bits (mi355_yolo_int8.h), 0 = the image was quantised with its own
 * pair.  Waits for the network's stream.  Returns the number of non-zero entries (0, and zeros, with the mode off). */
int network_input_status(network *net, uint32_t *status /* [batch] */);
/* image b's layer-0 bank entry as the device holds it (dnq_net_pi_entry_bytes bytes) into dst.  Waits for the network's stream. */
void network_input_bank_entry(network *net, int b, void *dst);
/* how often this library has waited for the device on this network's behalf so far (every stream synchronisation, every blocking
 * copy back): the difference over a sequence of calls is the number of host round trips it made */
long network_host_waits(network *net);
/* the host half of the prep only (per-channel integers + packed blobs, no device needed) */
void quantization_prep_host(network *net, float in_scale, uint8_t in_zp);

/* Batches in flight (serving throughput): a replica is a second executor of the SAME prepared model on the same device --
 * its own activation tensors, network input and HIP stream, the parent's packed weights in HBM (read-only in every kernel).
 * forward_network_gpu on parent and replicas in turn puts independent batches on separate streams, so that the device
 * overlaps one batch's launch gaps, pipeline fills and VALU-bound layers with another batch's MFMA-bound layers
 * (measured: DESIGN.md 4.3).  The parent must be prepared and must outlive its replicas; a replica cannot re-derive
 * layer 0 for another input scale, serve MI355_ACC_REF_F32 or be re-batched (error()). */
network *network_replica(network *parent);
/* the same with the stream choice as a parameter instead of the one-shot field: default_stream != 0 -> the replica launches on the
 * device's default (NULL) stream -- HIP's fourth hardware queue -- and owns no stream of its own */
network *network_replica_ex(network *parent, int default_stream);
/* MI355_PLAN_LATENCY / MI355_PLAN_THROUGHPUT for every conv launch of this executor from the next pass on.  Waits for the executor's
 * stream, drops a captured hipGraph (it holds the other plan's kernels) and re-derives the conv + pool / upsample / yolo / residual
 * fusion flags: a launcher that declined a fused call under one plan (flag cleared at run time) is asked again under the other. */
void network_set_plan(network *net, int plan);

/* ---- execution ----------------------------------------------------------------------------------------------- */
void forward_network(network *net);     /* == forward_network_gpu; dies if no device */
void forward_network_gpu(network *net); /* input: net->input_uint8_gpu already holds [batch][c][h][w] uint8 */
float *network_predict(network *net, float *input);
/* upload net->input_uint8 (host) -> device */
void push_network_input_uint8(network *net, const uint8_t *host_nchw);
/* device -> host mirrors of layer i in the reference layout */
void pull_layer_output(network *net, int i);
/* get_yolo_detections + correct_yolo_boxes (ref: src/yolo_layer.c:246-277,316-345, as called by get_network_boxes,
 * src/network.c:583-640) of yolo layer i for the whole batch on the device; only the detections are copied back.
 * recs: [batch][max_recs][6 + classes] floats {rank, x, y, w, h, objectness, prob[classes]} sorted by rank (the order of
 * the reference's loop), counts: [batch] detections found (records beyond max_recs are dropped). */
void network_yolo_detections_gpu(network *net, int i, int imw, int imh, float thresh, int relative, float *recs,
                                 int max_recs, int *counts);
/* the same with one source image size per batch slot (imw[b], imh[b]: host arrays) for correct_yolo_boxes */
void network_yolo_detections_gpu_sizes(network *net, int i, const int *imw, const int *imh, float thresh, int relative, float *recs,
                                       int max_recs, int *counts);

/* The same decode for ALL yolo layers and the whole batch in one call (mi355_yolo_detections_batch): image b's records, packed back to
 * back, are recs[offsets[b] .. offsets[b + 1]) -- records of 6 + classes floats as above, in the reference's order without a host sort:
 * yolo layers in network order, rank ascending inside a layer (rank = cell * n + anchor within the record's own layer).
 *   imw, imh        [batch] source sizes (host)
 *   max_per_image   an image keeps its FIRST max_per_image records of that order; <= 0: every candidate, which never truncates
 *   recs            host, room for batch * min(max_per_image, candidates) records, candidates = sum of n * h * w over the yolo layers
 *                   (network_detections_batch_shape) -- with max_per_image <= 0 that is batch * candidates * (6 + classes) floats,
 *                   56 MB for yolov3-tiny at 416, batch 64, 80 classes; the device buffer kept on the network has the same size
 *   counts          host [batch][nheads]: detections FOUND per image and yolo layer (found may exceed kept)
 *   offsets         host [batch + 1]
 * Per call: one upload (the sizes), three launches, one download of counts + offsets, one download of offsets[batch] records, two
 * synchronisations of net->stream (one when nothing was found), whatever the batch and the number of yolo layers.
 * Returns 0, or MI355_EINVAL with a message on stderr and nothing launched: no yolo layer, more than MI355_YOLO_MAX_HEADS of them, yolo
 * layers with differing `classes`, a size < 1. */
int network_yolo_detections_batch_gpu(network *net, const int *imw, const int *imh, float thresh, int relative, int max_per_image,
                                      float *recs, int *counts, int *offsets);
/* number of yolo layers, their common `classes`, candidates per image; 0 or MI355_EINVAL as above.  Host only. */
int network_detections_batch_shape(network *net, int *nheads, int *classes, int *candidates);

/* ---- detections (what `detector test` does after network_predict; ref: include/darknet.h:658-669) -------------------- */
typedef struct { float x, y, w, h; } box;
typedef struct detection {
    box bbox;
    int classes;
    float *prob;
    float *mask;
    float objectness;
    int sort_class;
} detection;
/* ref: src/network.c:583-640 -- yolo layers in network order, image 0 of the batch (get_network_boxes_batch: image b) */
detection *get_network_boxes(network *net, int w, int h, float thresh, float hier, int *map, int relative, int *num);
detection *get_network_boxes_batch(network *net, int b, int w, int h, float thresh, float hier, int *map, int relative, int *num);
void free_detections(detection *dets, int n);
/* get_network_boxes_batch for every image of the batch from ONE decode: dets[b] (num[b] entries; dets, num: [batch], the caller's) is
 * the array get_network_boxes_batch(net, b, imw[b], imh[b], thresh, ., ., relative, .) returns, with do_nms_sort(dets[b], num[b], classes,
 * nms) applied when nms > 0.  max_per_image as in network_yolo_detections_batch_gpu (<= 0: every candidate; the host copy holds only the
 * records that exist).  Returns 0 or MI355_EINVAL like that call (dets[b] = NULL, num[b] = 0 then). */
int network_detections_batch(network *net, const int *imw, const int *imh, float thresh, int relative, float nms, int max_per_image,
                             detection **dets, int *num);
void free_detections_batch(detection **dets, int *num, int batch); /* frees every dets[b], not the two arrays */
/* The device-free half of it: packed records (B images, offsets [B + 1]) -> detection arrays -> NMS. */
void detections_from_records(const float *recs, const int *offsets, int B, int classes, float nms, detection **dets, int *num);
/* flat copies of a detection array for FFI callers: boxes [n][4], objectness [n], probs [n][classes], in the array's order */
void detections_to_arrays(const detection *dets, int n, int classes, float *boxes, float *objectness, float *probs);
void do_nms_sort(detection *dets, int total, int classes, float thresh); /* ref: src/box.c:58-89 */
void do_nms_sort_arrays(const float *boxes, float *probs, const float *objectness, int n, int classes, float thresh);
float box_iou(box a, box b);
/* ---- frame views: a batch slot looks at a rectangle of its frame, mirrored or turned (mi355_frame_view, mi355_yolo_int8.h) ----------
 * network_set_frame_views: views holds net->batch entries, which are copied; NULL clears.  While views are set, every
 * network_frames_*_input_gpu call (and the JPEG and PNG inputs, which feed the u8 one) uploads the view table beside the frame table and
 * letterboxes slot b's view of its frame: the result is, bit for bit, network_frames_u8_input_gpu's on the view materialised as an RGB
 * frame.  w[b], h[b] of those calls stay the FRAME's sizes, and slots that name the same frame with different views upload it once.
 * Both scale modes, set_input_quantization_on_device and graph replay are the shared tail's.  A view the shim refuses dies via error()
 * as a frame the letterbox cannot serve does.  A replica owns its own views (none when made); re-batching clears them. */
void network_set_frame_views(network *net, const mi355_frame_view *views);
/* cols * rows views that cover a frame_w x frame_h frame, row by row (out[r * cols + c]), all with `orient`.  A tile is
 * ceil((frame_w + (cols - 1) * overlap) / cols) wide, tile c starts at c * (tile_w - overlap), and the last one is moved left so that it
 * ends on the frame's edge; rows likewise.  Returns cols * rows, or MI355_EINVAL (nothing written): a count or frame side below 1, a
 * negative overlap, an orient outside 1..8, a tile larger than the frame, an overlap at or above the tile size.  Host only. */
int network_tile_views(int frame_w, int frame_h, int cols, int rows, int overlap, int orient, mi355_frame_view *out);
/* A box relative to the view -- what the decode returns with relative = 1 when imw[b], imh[b] are the view's ORIENTED size (h x w for
 * orients 5..8) -- becomes a box relative to the frame.  In double: (u, t) = (b.x * vw, b.y * vh) and the sizes in view pixels; the
 * orient undone on continuous coordinates (a mirrored axis is c - u, a transposing orient swaps the axes and the two sizes); plus
 * (x0, y0); divided by the frame's size; stored as float.  Host only. */
void network_view_box_to_frame(const mi355_frame_view *v, int frame_w, int frame_h, box *b);
/* Detections of a batch of views, per FRAME.  frame_w[b], frame_h[b]: the size of the frame slot b looks at (the arrays given to the
 * input call); frame_of_slot[b] in 0 .. batch - 1 names that frame.  Runs network_detections_batch with the views' oriented sizes,
 * relative boxes and no NMS, maps every box to its frame (network_view_box_to_frame), concatenates the slots of a frame in slot order
 * and applies do_nms_sort once per frame when nms > 0, so that an object two overlapping tiles report is kept once.  dets[f], num[f]
 * (both [batch], the caller's; free_detections_batch frees them) are frame f's; a frame no slot names gets NULL, 0.  Without views set
 * every slot is its whole frame.  Returns 0, or MI355_EINVAL (a frame_of_slot outside the batch, or network_detections_batch's). */
int network_detections_views(network *net, const int *frame_w, const int *frame_h, const int *frame_of_slot, float thresh, float nms,
                             int max_per_image, detection **dets, int *num);
/* The device-free half: slot_dets[b] (slot_num[b] entries, relative to slot b's view) are consumed -- their boxes mapped, their entries
 * moved into dets[frame_of_slot[b]], the arrays freed --, then the NMS.  views == NULL: whole frames. */
int detections_views_merge(detection **slot_dets, int *slot_num, int B, const mi355_frame_view *views, const int *frame_w,
                           const int *frame_h, const int *frame_of_slot, int classes, float nms, detection **dets, int *num);
/* The EXIF orientation (IFD0 tag 0x0112, SHORT, count 1) of a JPEG file in memory: 1..8, and 1 for anything absent, malformed or out
 * of range.  Never fails, never reads outside [data, data + bytes).  The decode path ignores EXIF, as the reference's stb_image does:
 * the caller puts the value into a view.  Host only. */
int jpeg_exif_orientation_host(const uint8_t *data, size_t bytes);
char *data_cfg_find(const char *datacfg, const char *key); /* `key = value` of a .data file, or NULL */
char **get_labels(char *filename, int *count);

/* per-layer profiling: record HIP events around every layer for the next `max_steps` forward passes (eager
 * launches only), then read the per-layer sums in ms: out[0] = input layout conversion, out[1+i] = layer i. */
void network_profile_begin(network *net, int max_steps);
void network_profile_set_stride(network *net, int stride);
/* Determinism self-check (a race detector for the hand-scheduled kernels: counted waits, in-place register reuse): `passes` forward
 * passes over the input that is on the device, a device-side checksum of every yolo layer's output after each; nothing is synchronised.
 * network_selfcheck_result() waits, reads the checksums back and returns the number of passes that differ from the first (0 = all
 * identical, -1 = no self-check pending). */
void network_selfcheck(network *net, int passes);
int network_selfcheck_result(network *net);
void network_profile_set_phase(network *net, int phase);
int network_profile_read(network *net, float *ms_sum /* [n+1] */);

/* packed-weight exchange for multi-GPU start-up: rank 0 exports, the bytes travel by RCCL broadcast, the other
 * ranks import into a network parsed from the same cfg (no weights file needed there). */
size_t network_packed_size(network *net);
void network_export_packed(network *net, void *buf);
void network_import_packed(network *net, const void *buf, size_t bytes);
void network_import_packed_host(network *net, const void *buf, size_t bytes); /* host half only (no device) */
/* same exchange with the buffer already on the device (what bench.py hands over after torch.distributed.broadcast) */
void network_import_packed_gpu(network *net, const void *dev_buf, size_t bytes);
/* the whole start-up exchange behind the C ABI: root exports + uploads, one mi355_bcast_blob (RCCL over xGMI), the other
 * ranks import from HBM.  comm: mi355_comm_init handle of the calling rank. */
void network_bcast_packed(network *net, void *comm, int rank, int root);
/* the same bytes as a file: written once after load_weights + prep, read back with one fread */
void network_save_packed(network *net, char *filename);
void network_load_packed(network *net, char *filename);

/* what the planner decided for layer i, as it stands now (after the launchers had their say at run time): out[0..7] = route_elided,
 * out_view, byte offset of the layer's tensor inside the buffer that owns it, fuse_next_pool, fuse_next_upsample, fuse_next_shortcut,
 * fuse_next_yolo, fuse_pool_keep.  Returns 0, or -1 for a bad index.  Read-only: tests and tools look at the plan through it. */
int dnq_layer_plan(network *net, int i, int *out);

/* misc */
void error(const char *s);
void file_error(const char *s);
double what_time_is_it_now(void);
const char *get_layer_string(LAYER_TYPE t);

#ifdef __cplusplus
}
#endif
#endif
