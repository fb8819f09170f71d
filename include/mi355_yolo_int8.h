/*
 * mi355_yolo_int8.h -- C-ABI of libmi355yolo.so: the MI355X (gfx950) INT8 quantized-convolution inference
 * kernels for the darknet uint8-quantization fork ArtyZe/yolo_quantization.
 *
 * This is the drop-in boundary: plain C, raw device pointers and sizes, no HIP / torch types.  A darknet host
 * (ours: yolo_quantization_amd/host, or the reference itself -- see INTEGRATION.md) binds these from the
 * `layer.forward_gpu` function pointers (reference include/darknet.h:158-163).  Every entry point returns 0 on
 * success or a negative MI355_E* code; nothing aborts, nothing falls back to the CPU.
 *
 * Paths cited as `ref:` are relative to the reference repository root.
 *
 * Device activation layout ("PHWC"): a tensor of B images x H x W pixels x C channels is an array of *cells*
 * of `cs` bytes (cs >= C, cs % 16 == 0, or cs == 4 for the 3-channel network input):
 *
 *     cell(b, y, x) = lead + (b*(H+1) + (y+1))*(W+1) + x          0 <= y < H, 0 <= x < W
 *
 * Row 0 of every image block and column W of every row are *pad cells* shared between neighbours (the right pad
 * of row y is the left pad of row y+1; the bottom pad row of image b is the top pad row of image b+1), so a 3x3
 * tap is the constant cell offset dy*(W+1)+dx everywhere.  Pad cells hold the consumer's input zero point
 * (ref: src/convolutional_layer.c:703-705,715 -- im2col pads with the input zero point).  Bytes are stored
 * *biased*: stored = uint8 ^ 0x80, i.e. the signed value (uint8 - 128) that V_MFMA_I32_*_I8 consumes directly.
 */
#ifndef MI355_YOLO_INT8_H
#define MI355_YOLO_INT8_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- error codes ---------------------------------------------------------------------------------------- */
#define MI355_OK 0
#define MI355_EINVAL (-22)   /* bad argument / unsupported shape */
#define MI355_ENOMEM (-12)   /* device allocation failed */
#define MI355_EHIP (-5)      /* HIP runtime error: mi355_last_error() has the text */
#define MI355_ENODEV (-19)   /* no gfx950 device */

/* ACTIVATION enum values of the reference (ref: include/darknet.h:87-89) */
#define MI355_ACT_RELU 1
#define MI355_ACT_LINEAR 3
#define MI355_ACT_RELU6 8
#define MI355_ACT_LEAKY 9

/* uint8 store behaviour of the requantise epilogue */
#define MI355_STORE_WRAP 0      /* ref default path: stored before clamp -> wraps mod 256 (convolutional_layer.c:737-749) */
#define MI355_STORE_SATURATE 1  /* builder-defined: the default path's formulas with clamp(0,255) BEFORE the store.  Equals the MKL
                                   flavour's epilogue (convolutional_layer.c:572-596) for LEAKY / LINEAR / RELU6 on every int32
                                   (proved exhaustively, tests/test_host_cpu.py), differs for RELU (:591 adds no zero point);
                                   that flavour cannot be built here, so this mode is NOT pinned against a reference output */

/* accumulation semantics */
#define MI355_ACC_EXACT 0    /* exact int32 on V_MFMA_I32_*_I8: the integers the reference's formula defines; equals the default build
                                wherever its fp32 accumulation is exact (pinned: tests/test_gpu_refpin.py) and the MKL flavour's
                                accumulators: that flavour cannot be built here, but the MKL entry point it calls is in the image --
                                cblas_gemm_s16s16s32 with the argument lists of ref :557-569 returns exactly these integers beyond 2^24
                                as well (tests/test_mkl_pin.py: the GEMM half pinned against the real library, the epilogue not) */
#define MI355_ACC_REF_F32 1  /* bit-faithful emulation of ref src/gemm.c:279-299 (fp32 step-wise accumulate,
                                two passes); slow verification kernel, never on the throughput path */

/* ---- runtime (replaces ref src/cuda.c: cuda_set_device :9, cuda_make_array :90-104, cuda_push/pull_array
 *      :151-167, cuda_free :144-149, check_error :27-49) ---------------------------------------------------- */
/* ABI version of this header.  Structs that cross the boundary (mi355_conv_desc, mi355_tensor) carry no size field: a field is only ever
 * APPENDED, and every append bumps this number (6: mi355_conv_desc.epilogue_packed).  A caller compares MI355_ABI_VERSION (what it was built
 * against) with mi355_abi_version() (what it loaded) once at start-up -- the darknet host, integration/mi355_glue.c and the Python binding
 * all do -- so that a caller built against an older, shorter struct fails loudly instead of having the shim read past its end. */
#define MI355_ABI_VERSION 6
int mi355_abi_version(void);
int mi355_init(int device);                       /* select device, verify gfx950 */
const char *mi355_last_error(void);
int mi355_device_count(void);
int mi355_alloc(void **dptr, size_t bytes);
int mi355_free(void *dptr);
int mi355_memset(void *dptr, int byte, size_t bytes, void *stream);
int mi355_h2d(void *dst, const void *src, size_t bytes, void *stream);
int mi355_d2h(void *dst, const void *src, size_t bytes, void *stream);
int mi355_d2d(void *dst, const void *src, size_t bytes, void *stream);
int mi355_stream_create(void **stream);
int mi355_stream_destroy(void *stream);
/* A stream that was MEASURED to run side by side with the default stream and with every other acquired stream of the device
 * (HIP deals created streams round-robin onto the device's four hardware queues, the default stream owns one; streams on one
 * queue serialise, and which created stream shares whose queue depends on every stream the process created before).  The first
 * three acquisitions per device come from the measured pool, later ones are plain streams.  Release instead of destroy. */
int mi355_stream_acquire(void **stream);
int mi355_stream_release(void *stream);
int mi355_stream_sync(void *stream);              /* stream == NULL: device synchronize */
/* HIP events on the launch stream (bench.py times kernels with these, not with torch.cuda.Event) */
int mi355_event_create(void **ev);
int mi355_event_destroy(void *ev);
int mi355_event_record(void *ev, void *stream);
int mi355_event_elapsed_ms(void *start, void *stop, float *ms); /* synchronises on `stop` */
/* hipGraph capture of a layer sequence (launch-bound tail of the net) */
int mi355_graph_begin(void *stream);
int mi355_graph_end(void *stream, void **graph_exec);
int mi355_graph_launch(void *graph_exec, void *stream);
int mi355_graph_destroy(void *graph_exec);

/* ---- the path's one collective: one-shot RCCL broadcast of the packed weights over xGMI -----------------
 * The reference has no inference-time communication (its multi-GPU code is host-staged weight averaging for training,
 * ref: src/network.c:1100-1194); images shard by rank and every device holds a replica of the packed blobs.  librccl is
 * bound with dlopen at the first call (MI355_ENODEV when absent).  One communicator rank per device: call mi355_init(dev)
 * on the thread first.  id128: the 128-byte ncclUniqueId, created on one rank and handed to the others by the launcher
 * (a shared variable between host threads, the process launcher's store between processes). */
int mi355_comm_unique_id(void *id128);
int mi355_comm_init(void **comm, int nranks, const void *id128, int rank);
int mi355_bcast_blob(void *comm, void *dev_buf, size_t bytes, int root, void *stream); /* in place, asynchronous on `stream` */
int mi355_comm_destroy(void *comm);
const char *mi355_comm_last_error(void);

/* ---- tensors ----------------------------------------------------------------------------------------------- */
typedef struct mi355_tensor {
    void *data;   /* device pointer to cell 0 */
    int B, H, W;  /* images, rows, columns */
    int C;        /* logical channels */
    int cs;       /* bytes per cell */
    int lead;     /* pad cells in front of image 0 */
    int tail;     /* pad cells behind the last image */
} mi355_tensor;

/* Fill in cs/lead/tail for (B,H,W,C) and return the byte size of the buffer (0 on bad dims). data untouched. */
size_t mi355_tensor_describe(mi355_tensor *t, int B, int H, int W, int C);
/* The reference's own input layout as a tensor descriptor: [B][C][H][W] uint8 planes, plain bytes, no pad cells (cs = 1,
 * lead = tail = 0) -- `net.input_uint8` as it is (ref: src/network.c:248).  Accepted as `x` by mi355_conv_forward /
 * mi355_conv_pool_forward for the 3-channel first layer only (exact mode, 16 or 32 filters, even map, W % 4 == 0): the kernel
 * reads the three colour planes in place and pads with desc.zp_in, so the network input needs no layout conversion pass.
 * Other shapes return MI355_EINVAL: convert with mi355_nchw_to_tensor then.  Returns the byte size. */
size_t mi355_tensor_describe_nchw(mi355_tensor *t, int B, int H, int W, int C);
/* Set every byte of the buffer (pads included) to the biased zero point (zp ^ 0x80). */
int mi355_tensor_fill(const mi355_tensor *t, uint8_t zero_point, void *stream);
/* Reference layout <-> device layout.  nchw is the reference's `net.input_uint8` / `l.output_uint8_final`
 * layout [B][C][H][W] uint8 (ref: src/network.c:248-250), resident on the device. */
int mi355_nchw_to_tensor(const uint8_t *nchw, const mi355_tensor *t, void *stream);
int mi355_tensor_to_nchw(const mi355_tensor *t, uint8_t *nchw, void *stream);

/* ---- quantized convolution ----------------------------------------------------------------------------- */
/* Host-side packing of one conv layer's weights (replaces the per-forward operand prep of the reference: the
 * `zero_point_uint8` table ref: src/blas.c:290-300 and GEMM pass 2 ref: src/convolutional_layer.c:721 are
 * folded into per-channel constants).  weights_uint8: [n][c*k*k] in the reference's (ci,ky,kx) order
 * (ref: src/parser.c:1146), zp_w: [n].  Returns the packed blob size; writes it when `blob` != NULL.
 * The blob is position independent (offsets only) so it can be broadcast to other GPUs as bytes.
 * Accepted shapes: n >= 1, c >= 1, 1 <= ksize <= 11 (0 / MI355_EINVAL otherwise).  3x3 layers on c % 16 == 0 or on the
 * 3-channel image and 1x1 layers on c % 16 == 0 get the specialised kernels' packing; every other shape the general
 * kernel's (conv_kxk.hip), whose layout depends on (n, c, ksize) only, not on stride or padding. */
size_t mi355_conv_pack_size(int n, int c, int ksize);
int mi355_conv_pack(int n, int c, int ksize, const uint8_t *weights_uint8, const uint8_t *zp_w,
                    const int32_t *biases_int32, const double *M_value, const double *shift_value, void *blob);
/* Optional second packing step, on the same HOST blob before it is uploaded: the per-channel constants of the requantise
 * epilogue (ref: src/convolutional_layer.c:726-751) that the fused conv + maxpool kernels need for ONE (activation, zero
 * point) -- the range of accumulators whose stored byte cannot wrap (:737-749, where max-pooling commutes with the
 * requantisation) and the integer form M0 / shift of M_value (ref: src/blas.c:387-418).  Without it (or when a launch's
 * activation / zp_act differ from the packed ones, or the store saturates) every workgroup derives them itself: same bytes,
 * a quarter to a third of the first layer's run time.  RELU is stored as LINEAR (the reference's integer
 * path treats them alike, :740-742). */
int mi355_conv_pack_epilogue(int n, int c, int ksize, int activation, int zp_act, void *blob);

typedef struct mi355_conv_desc {
    int n, c, ksize, stride, pad; /* filters, input channels, kernel size 1..11, stride >= 1, padding >= 0 (the cfg's pad=1 means
                                   * ksize/2).  The specialised 3x3 / 1x1 shapes (see mi355_conv_pack) run at stride 1 | 2 with
                                   * pad = ksize/2 in exact mode (stride 2: 3x3, c % 16 == 0) and at any stride / padding in
                                   * ref-f32 mode; every other shape at any stride and padding in both modes.  1x1 layers:
                                   * stride 1, pad 0 only (the reference's 1x1 path is not a convolution otherwise). */
    int activation;               /* MI355_ACT_* */
    int store_mode;               /* MI355_STORE_* */
    int accum_mode;               /* MI355_ACC_* */
    uint8_t zp_in, zp_act;        /* input / activation zero points */
    float s_act;                  /* activation scale (only for y_f32) */
    int plan;                     /* MI355_PLAN_*: which kernel / tile the launcher should prefer (results are identical) */
    int epilogue_packed;          /* 1: the caller finished `blob` with mi355_conv_pack_epilogue(activation, zp_act) of THIS desc.  A hint for the
                                   * kernel choice only (results are identical): kernels that live off the table (conv + maxpool with 16 / 32
                                   * input channels on 16 x 16 x 64 tiles) are picked when it is set; a blob that does not carry the promised
                                   * table still yields the right bytes, slowly (every window takes the reference's order) */
} mi355_conv_desc;
/* MI355_PLAN_LATENCY (0, default): one batch at a time -- every launch is sized to fill the whole chip on its own (one big
 * workgroup per CU: 128 x 384 row-image tiles, the weights-stationary 3x3 kernel with up to 160 KB of LDS).
 * MI355_PLAN_THROUGHPUT: several independent batches are in flight on separate streams (darknet_q.h network_replica) --
 * prefer kernels of which TWO workgroups fit a CU (<= 80 KB of LDS, 4 waves), so that a workgroup of another batch's
 * layer can move in next to it: a launch that needs an empty CU waits until every small workgroup of the other streams
 * has drained from one.  Measured in DESIGN.md 4.3. */
#define MI355_PLAN_LATENCY 0
#define MI355_PLAN_THROUGHPUT 1

/* forward_convolutional_layer_quant_inputi_outputi (ref: src/convolutional_layer.c:694-761) for a whole batch,
 * "apply the batch-1 function independently per image".
 *   x        input tensor (C == desc.c).  desc.c == 3 selects the first-layer kernel and x.cs must be 4.
 *   blob     device copy of the mi355_conv_pack blob
 *   w_u8     device copy of the raw weights_uint8 / zp_w (only read when accum_mode == MI355_ACC_REF_F32)
 *   y        output tensor (C == desc.n), nullable
 *   acc_out  nullable: pre-requant int32 accumulators, reference layout [B][n][H*W] == l.output_int32
 *   y_f32    nullable: quant_stop tail (ref :752-760), reference layout [B][n][H*W] float == l.output */
int mi355_conv_forward(const mi355_conv_desc *desc, const mi355_tensor *x, const void *blob, const uint8_t *w_u8,
                       const uint8_t *zp_w, const mi355_tensor *y, int32_t *acc_out, float *y_f32, void *stream);

/* The same convolution fused with the size-2 / stride-2 maxpool that follows it (ref: forward_maxpool_layer_quant,
 * src/maxpool_layer.c:109-172, window offset 0 on even maps): writes ypool (B, H/2, W/2, n) directly and, when y is
 * non-NULL, the pre-pool tensor as well.  3x3 convs on even H, W only, exact accumulation mode; returns MI355_EINVAL
 * otherwise and the caller runs the two layers separately.  Results are identical to conv_forward + maxpool_forward. */
int mi355_conv_pool_forward(const mi355_conv_desc *desc, const mi355_tensor *x, const void *blob, const mi355_tensor *y,
                            const mi355_tensor *ypool, void *stream);

/* A quant_stop head convolution fused with the yolo layer that follows it (ref: forward_yolo_layer, src/yolo_layer.c:132-146):
 * writes y (uint8), y_f32 (== l.output of the conv, ref :752-760) and yolo_out (== l.output of the yolo layer: logistic on
 * x, y, objectness and class scores of every anchor) from one kernel.  desc.n must be a multiple of classes + 5; exact
 * accumulation mode.  Results are identical to mi355_conv_forward + mi355_yolo_forward.  y_f32 may be NULL (the conv's own float
 * tensor is an intermediate only the yolo layer reads): the 1x1 heads then write yolo_out alone -- MI355_EINVAL where the kernel
 * that serves the shape cannot (pass the buffer then). */
int mi355_conv_yolo_forward(const mi355_conv_desc *desc, const mi355_tensor *x, const void *blob, const mi355_tensor *y,
                            float *y_f32, float *yolo_out, int classes, void *stream);

/* A convolution fused with the nearest-neighbour upsample layer that follows it (ref: forward_upsample_layer_quant,
 * src/upsample_layer.c:96-113): y_up is the (stride*H) x (stride*W) tensor, every output pixel is stored stride x stride
 * times; the conv's own tensor is not stored.  Layers with c % 64 == 0, exact mode.  Identical to conv_forward + upsample_forward. */
int mi355_conv_upsample_forward(const mi355_conv_desc *desc, const mi355_tensor *x, const void *blob, const mi355_tensor *y_up,
                                int stride, void *stream);

/* A convolution fused with the quantized residual add that follows it (`[shortcut] quantized=1`, mi355_shortcut_forward below):
 * every requantised byte a of the convolution (zero point desc.zp_act) is combined with the byte b of `from` at the same
 * pixel and channel, y_sum = clamp(zp_out + ((Ka*(a - zp_act) + Kb*(b - zp_from) + 2^15) >> 16)); the convolution's own
 * tensor is not stored.  Stride-1 exact-mode 3x3 layers with 128 / 256 input channels (conv_ws3.hip: 16 of YOLOv3's 23 residual
 * blocks); MI355_EINVAL otherwise and the caller runs the two layers separately (measured faster for the other kernels).  Bytes are identical to
 * mi355_conv_forward + mi355_shortcut_forward. */
int mi355_conv_shortcut_forward(const mi355_conv_desc *desc, const mi355_tensor *x, const void *blob, const mi355_tensor *from,
                                const mi355_tensor *y_sum, int32_t Ka, int32_t Kb, uint8_t zp_from, uint8_t zp_out, void *stream);

/* Layer 0 with one input scale / zero point PER IMAGE.  Only layer 0 depends on the input scale (ref: src/blas.c:300-333), so each image
 * needs its own layer-0 constants: a BANK is E blobs of this layer at a fixed byte stride entry_bytes (a multiple of 16, at least
 * mi355_conv_pack_size), each the mi355_conv_pack (+ mi355_conv_pack_epilogue) output for one (s_in, zp_in) -- same weights, zero
 * points and activation in every entry.  Image b uses entry entry_of_image[b] (int32, device) and pads with zp_in_of_image[b] (uint8,
 * device); desc.zp_in is ignored.  Images with equal (s_in, zp_in) may share an entry.  Every slot's bytes equal the shared-scale call
 * at batch 1 on that image with that image's blob.  Because the kernel arguments point at the bank and the index arrays, a captured
 * graph stays valid when their contents change.  Served by the first-layer kernels only: 3 -> n, 3x3, stride 1, pad 1 (exact mode:
 * the MFMA kernels for 16 / 32 filters on even maps, the VALU kernels otherwise; ref-f32 mode: the emulation kernel); any other
 * shape returns MI355_EINVAL up front.  Pad cells of a cs == 4 tensor are never read by these calls (the bottom pad row of image b
 * is the top pad row of image b + 1, which cannot hold two zero points): out-of-image taps take the image's zero point in registers. */
int mi355_conv_forward_per_image(const mi355_conv_desc *desc, const mi355_tensor *x, const void *bank, size_t entry_bytes,
                                 const int32_t *entry_of_image, const uint8_t *zp_in_of_image, const uint8_t *w_u8,
                                 const uint8_t *zp_w, const mi355_tensor *y, int32_t *acc_out, float *y_f32, void *stream);
int mi355_conv_pool_forward_per_image(const mi355_conv_desc *desc, const mi355_tensor *x, const void *bank, size_t entry_bytes,
                                      const int32_t *entry_of_image, const uint8_t *zp_in_of_image, const mi355_tensor *y,
                                      const mi355_tensor *ypool, void *stream);

/* Tile configuration override for benchmarking (0 = auto). */
int mi355_conv_set_tile(int bm, int bn);
/* Development switches.  Bits 0..8 are timing ablations of the K loop (no DMA / no s_barrier / no MFMA / ...), compiled
 * in only with -DMI355_ABLATE: results are WRONG when set; tools/conv_microbench.py --ablate only.  Two bits select
 * among equivalent kernels and leave results unchanged (tests use them to cross-check): 512 = conv_rows.hip walks the
 * channel chunks unrotated, 1024 = fused conv+maxpool never uses conv_small.hip / the first-layer MFMA kernel, 8192 = 1x1
 * layers never use conv1x1.hip, 4096 = 32 -> 64 conv + maxpool on conv_small32.hip (round 6: eight waves per workgroup, measured slower; conv_small.hip without the bit), 16384 = 3x3 layers never use conv_ws3.hip, 2^20 = the row-image 3x3 kernel on the 32x32x32 MFMA
 * (conv_rows.hip) instead of the 16x16x64 one (conv_rows16.hip), 2^21 = mi355_conv_pool_forward refuses the 128 / 256-channel
 * layers (the host then runs conv and maxpool separately), 2048 = plain tile walk in the first-layer kernels, 131072 = no raised
 * priority around the MFMA chains of the conv+pool kernels, 65536 (2^16) = 1x1 layers with fewer than 32 filters (the detection heads)
 * keep conv1x1.hip's eight-wave workgroups and per-wave V_DOT4 channel sums instead of the sum-row form sized to its groups. */
int mi355_debug_flags(int flags);
/* Which kernel family served the calling thread's most recent mi355_conv_*forward call (tests assert that a shape reaches
 * the kernel it is meant to exercise): 0 none yet, 1 first layer (conv_aux.hip), 2 conv_small.hip (few-channel / 64-channel
 * conv + maxpool), 3 conv1x1.hip, 4 conv_ws3.hip, 5 conv_igemm.hip / conv_rows.hip / conv_rows16.hip, 6 fp32-accumulate emulation,
 * 7 conv_pool16.hip (16 -> 32 + maxpool with the packed epilogue table), 8 conv_small32.hip (32 -> 64 + maxpool). */
int mi355_last_conv_kernel(void);
/* Geometry of the calling thread's most recent convolution kernel launch (any mi355_conv_*forward call): workgroups in the grid,
 * threads per workgroup, bytes of dynamic LDS, as the launcher chose them for the plan, batch and tile count.  Each pointer may be
 * NULL.  Recorded host-side when the kernel is launched, so a call that was refused before any launch leaves the previous launch's
 * values.  Returns MI355_EINVAL (and zeros) before the thread's first launch.  Tests assert with it which tiling branch a shape
 * reaches. */
int mi355_last_conv_launch(int *grid, int *threads, int *lds_bytes);

/* ---- glue layers ---------------------------------------------------------------------------------------- */
/* forward_maxpool_layer_quant (ref: src/maxpool_layer.c:109-172): window offset -pad/2, OOB taps = uint8 0.  y must be
 * (x.H + pad - size) / stride + 1 rows by (x.W + pad - size) / stride + 1 columns, C's truncating division (ref :31-32).
 * Refused with MI355_EINVAL before anything is launched, mi355_last_error() then reads "invalid argument: " and one of:
 *     "maxpool: null"                                          x, y or one of their data pointers is NULL
 *     "maxpool: layout"                                        a cell size that is no multiple of 16 (the cs == 4 image), x.C != y.C, x.B != y.B
 *     "maxpool: need size >= 1, stride >= 1 and pad >= 0"      checked before the division above
 *     "maxpool: output dims"                                   y.H / y.W are not the sizes above, or those are below 1 */
int mi355_maxpool_forward(const mi355_tensor *x, const mi355_tensor *y, int size, int stride, int pad, void *stream);
/* forward_upsample_layer_quant (ref: src/upsample_layer.c:96-113, src/blas.c:781-803), nearest x stride */
int mi355_upsample_forward(const mi355_tensor *x, const mi355_tensor *y, int stride, void *stream);
/* forward_route_layer_quant (ref: src/route_layer.c:107-130): channel concat of n inputs, no rescale */
int mi355_route_forward(const mi355_tensor *const *xs, int n, const mi355_tensor *y, void *stream);
/* quant_stop tail of a glue layer (ref: src/maxpool_layer.c:163-171, src/upsample_layer.c:104-112, src/route_layer.c:121-129):
 * out_f32[b][out_c0 + c][pix] = (int)(x[b][pix][c0 + c] - zero_point) * scale for c < nc; out_f32 is the reference's
 * `l.output` layout [B][out_C][H*W].  A route with quant_stop calls it once per input with that input's own scale / zero
 * point (ref :125: `net.layers[index].activ_data_uint8_*`). */
int mi355_dequant_forward(const mi355_tensor *x, int c0, int nc, uint8_t zero_point, float scale, float *out_f32, int out_C,
                          int out_c0, void *stream);
/* Quantized residual add, `[shortcut] quantized=1`.  The reference has NO integer shortcut (src/shortcut_layer.c:62-75 and
 * src/blas.c:490-514 are float only), so this op is builder-specified (parity status: unpinned, the
 * oracle is oracle.c:orc_shortcut_u8):
 *     K = round((float)(s_in / s_out) * 2^16)                          mi355_shortcut_multiplier, 1 <= K < 2^21
 *     q = zp_out + ((Ka*(a - zp_a) + Kb*(b - zp_b) + 2^15) >> 16)      arithmetic shift: round half up
 *     y = clamp(q, 0, 255)                                             linear activation only
 * a = the previous layer's tensor, b = the tensor of layer `from`; same batch / map / channels (YOLOv3's residual blocks). */
int mi355_shortcut_multiplier(float s_in, float s_out, int32_t *K);
int mi355_shortcut_forward(const mi355_tensor *a, const mi355_tensor *b, const mi355_tensor *y, int32_t Ka, int32_t Kb,
                           uint8_t zp_a, uint8_t zp_b, uint8_t zp_out, void *stream);
/* letterbox_image (ref: src/image.c:812-831; bilinear resize_image :1199-1242, embed_image :428-439, fill 0.5): planar
 * float image [c][imh][imw] in device memory -> [c][h][w], aspect ratio kept, centred.  Bit-identical floats. */
int mi355_letterbox_forward(const float *im_f32, int imw, int imh, int c, float *out_f32, int w, int h, void *stream);
/* Layer-0 input quantiser (ref: quant_weights_with_min_max_channel with one channel, src/blas.c:108-168, called on the
 * float image at src/blas.c:279), both halves on device memory.  mi355_image_minmax: minmax[0] = max(x, 0.0f),
 * minmax[1] = min(x, 0.0f) (-0.0f when no element is negative) over `count` floats, the reference's seeds and
 * comparisons (NaNs are skipped).  mi355_image_quantize: out[k] = clamp((int)(float)(round((double)(x[k] / scale)) +
 * (double)zero_point), 0, 255), the reference's evaluation order (:160-165). */
int mi355_image_minmax(const float *x_f32, long count, float *minmax, void *stream);
int mi355_image_quantize(const float *x_f32, long count, float scale, int zero_point, uint8_t *out_u8, void *stream);
/* Per-image input quantisation (opt-in; the calls above keep "image 0 defines the scale"): B images of count_per_image floats each.
 * mi355_image_minmax_batched: minmax[2 b], minmax[2 b + 1] = mi355_image_minmax of image b (same seeds, NaN handling, comparisons), one
 * launch.  mi355_image_quantize_per_image: image b quantised with scale_dev[b], zp_dev[b] -- read from DEVICE memory, so that a captured
 * graph stays valid for the next batch's scales -- in mi355_image_quantize's evaluation order.  B <= 65535. */
int mi355_image_minmax_batched(const float *x_f32, int B, long count_per_image, float *minmax, void *stream);
int mi355_image_quantize_per_image(const float *x_f32, int B, long count_per_image, const float *scale_dev, const uint8_t *zp_dev,
                                   uint8_t *out_u8, void *stream);
/* The rest of the input step on the device, so that nothing comes back to the host between the min / max and the quantiser: the
 * (scale, zero point) of every image from the batch's min / max, and layer 0's bank entries (mi355_conv_forward_per_image) from those
 * pairs.  Both are stream-ordered launches; every value they write is bit for bit what the host computes from the same inputs.
 *
 * mi355_input_pairs: minmax_dev is [B][2] max, min as the min / max calls above leave them.  Image b gets the reference's scale and zero
 * point (ref: src/blas.c:125-150: scale = (max - min) * (1.0f / 255.0f), zero point = clamp(round(0.0f - min / scale), 0, 255), the
 * division in float, clamp and round in double) into scale_dev[b], zp_dev[b]; shared != 0: image 0's pair into all B slots.
 * entry_dev[b] (may be NULL) = b, or 0 with shared: the bank entry of image b.  status_dev[b] = 0, or the MI355_INPUT_* bit of what
 * the reference asserts against (an all-zero image, a zero scale); such a slot keeps the pair it held before the call, so the arrays
 * must hold valid pairs when the first call runs.
 *
 * mi355_l0_derive: one workgroup per entry rewrites, in a bank whose slots were initialised with this layer's packed blob
 * (mi355_conv_pack + mi355_conv_pack_epilogue for any input pair), everything that depends on the pair: entry e for (scale_dev[e],
 * zp_dev[e]), B entries, or entry 0 alone with shared != 0.  The layer's constants come from consts_dev: a mi355_l0_consts followed by
 * n mi355_l0_channel (consts_host: the same bytes on the host, read for the shape and the activation).  Per channel: the requantisation
 * multiplier M = s_in * w_scale / s_act in float, its (M0, shift) decomposition (ref: src/blas.c:387-418), biases_int32 =
 * (int32)(bias / (s_in * w_scale) + (float)weights_sum_int) (ref :333), then the blob's bias, cw + bias, M_value, shift_value, their
 * product, shift, the header's pow2 and the whole epilogue table (entries, flags, key, byte table, the first layer's per-lane records).
 * Where the host prep dies or mi355_conv_pack refuses, the MI355_INPUT_* bit is ORed into status_dev of the entry's images, the slot
 * is left as it was and the images' pairs are set back to kept_scale_dev / kept_zp_dev; otherwise the pair is copied there.  So the
 * kept arrays always hold the pair each image's entry stands for; they must be initialised with the pair of the blob the slots were
 * initialised with.  3 -> n 3x3 first layers only; entry_bytes a multiple of 16 and at least mi355_conv_pack_size(n, 3, 3).
 * New structs and new calls: MI355_ABI_VERSION is unchanged. */
#define MI355_INPUT_ALL_ZERO   1u   /* max == min == 0 */
#define MI355_INPUT_ZERO_SCALE 2u   /* (max - min) / 255 underflows to 0 */
#define MI355_INPUT_M_RANGE    4u   /* some channel's M is outside (0, 1) */
#define MI355_INPUT_NEG_SHIFT  8u   /* ... or decomposes with a negative shift */
#define MI355_INPUT_PACK_RANGE 16u  /* ... or fails mi355_conv_pack's 0 < M_value < 1, 0 < shift_value <= 1 */
#define MI355_INPUT_BIAS_RANGE 32u  /* ... or its float bias sum is outside int32 */
#define MI355_INPUT_BAD_SLOT   64u  /* the slot does not hold a first-layer blob of this shape */
typedef struct mi355_l0_channel {
    float bias;        /* the float bias, batch norm folded in (b of the host prep) */
    float w_scale;     /* weight_data_uint8_scales */
    int32_t w_zp;      /* weight_data_uint8_zero_point */
    int32_t wsum;      /* plain sum of the channel's K uint8 weights */
} mi355_l0_channel;
typedef struct mi355_l0_consts {
    int32_t n, K;      /* filters, c * size * size (27) */
    int32_t zp_act, activation; /* MI355_ACT_* */
    float s_act;
    int32_t reserved[3];
} mi355_l0_consts;     /* followed by n mi355_l0_channel */
int mi355_input_pairs(const float *minmax_dev, int B, int shared, int32_t *entry_dev, float *scale_dev, uint8_t *zp_dev,
                      uint32_t *status_dev, void *stream);
int mi355_l0_derive(const mi355_l0_consts *consts_dev, const mi355_l0_consts *consts_host, void *bank, size_t entry_bytes, int B,
                    int shared, float *scale_dev, uint8_t *zp_dev, float *kept_scale_dev, uint8_t *kept_zp_dev, uint32_t *status_dev,
                    void *stream);
/* The same input step for a whole batch of 8-bit interleaved frames as a decoder delivers them (RGB or BGR, three bytes per pixel, rows
 * `pitch` bytes apart), in two launches and without a float image in memory.  A source sample is (float)byte / 255.f -- load_image_color's
 * planes (ref: src/image.c:1386) -- and every letterboxed float is the one mi355_letterbox_forward computes from those planes; min / max
 * and the quantised bytes equal mi355_image_minmax_batched / mi355_image_quantize_per_image on that float image, bit for bit.
 * One table entry per batch slot; frames may differ in size.  A new struct and new calls: MI355_ABI_VERSION is unchanged. */
#define MI355_FRAME_RGB 0   /* plane k reads byte k of a pixel */
#define MI355_FRAME_BGR 1   /* plane k reads byte 2 - k */
typedef struct mi355_frame_u8 {
    const uint8_t *data; /* DEVICE pointer to the first byte of row 0 */
    int w, h;            /* pixels */
    int pitch;           /* bytes from one row to the next, >= 3 * w */
    int order;           /* MI355_FRAME_* */
    int reserved[2];     /* explicit padding to 32 bytes, zero */
} mi355_frame_u8;
/* table_dev: B entries in device memory, read by the kernels.  table_host: the caller's host copy of the same B entries; the
 * launcher validates THAT before anything is launched (the conditions of mi355_letterbox_forward per frame -- resized sides >= 2, every
 * source row / column the resize touches inside the frame --, pitch >= 3 * w, non-null data, a known order) and returns MI355_EINVAL
 * with a message when any frame fails; the two copies must agree.  (w, h): the network input size, B <= 65535.
 * mi355_frames_u8_letterbox_minmax: minmax[2 b], minmax[2 b + 1] = max / min of frame b's letterboxed floats against the 0.0f seeds
 * (device memory), nothing else is stored.  mi355_frames_u8_letterbox_quantize: the same floats quantised with scale_dev[b], zp_dev[b]
 * (device memory) into out_u8[B][3][h][w] planar bytes, the layout of the network's uint8 input. */
int mi355_frames_u8_letterbox_minmax(const mi355_frame_u8 *table_dev, const mi355_frame_u8 *table_host, int B, int w, int h,
                                     float *minmax, void *stream);
int mi355_frames_u8_letterbox_quantize(const mi355_frame_u8 *table_dev, const mi355_frame_u8 *table_host, int B, int w, int h,
                                       const float *scale_dev, const uint8_t *zp_dev, uint8_t *out_u8, void *stream);
/* The same two calls for NV12 / NV21 frames as video decoders and camera stacks deliver them: a Y plane of h rows of w bytes, pitch_y
 * bytes apart, and a chroma plane of (h + 1) / 2 rows of (w + 1) / 2 byte pairs, pitch_uv bytes apart; a pair is (U, V) in NV12 and
 * (V, U) in NV21.  Odd w and h are legal.  Pixel (x, y) takes Y[y][x] and the pair at [y / 2][x / 2] (nearest sampling: no chroma
 * interpolation, no siting offset).  Its 8-bit RGB is computed in int32 with an arithmetic (floor) right shift and a clamp to 0..255:
 *     yy = cy * (Y - yoff)
 *     R = clamp((yy + crv * (V - 128)                   + 32768) >> 16)
 *     G = clamp((yy - cgu * (U - 128) - cgv * (V - 128) + 32768) >> 16)
 *     B = clamp((yy + cbu * (U - 128)                   + 32768) >> 16)
 * with (yoff, cy, crv, cgu, cgv, cbu), round(x * 65536) of the standards' real coefficients:
 *     MI355_YUV_BT601       (limited range)  16, 76309, 104597, 25675, 53279, 132201
 *     MI355_YUV_BT601_FULL                    0, 65536,  91881, 22553, 46802, 116130
 *     MI355_YUV_BT709       (limited range)  16, 76309, 117489, 13975, 34925, 138438
 *     MI355_YUV_BT709_FULL                    0, 65536, 103206, 12276, 30679, 121609
 * The conversion happens in registers at every bilinear tap; from those bytes on nothing is new: min / max and the quantised bytes are,
 * bit for bit, what the u8 calls above give for the interleaved RGB frame these formulas make.  A new struct and new calls:
 * MI355_ABI_VERSION is unchanged. */
#define MI355_YUV_NV12 0   /* chroma pair = (U, V) */
#define MI355_YUV_NV21 1   /* chroma pair = (V, U) */
#define MI355_YUV_BT601 0
#define MI355_YUV_BT601_FULL 1
#define MI355_YUV_BT709 2
#define MI355_YUV_BT709_FULL 3
typedef struct mi355_frame_yuv {
    const uint8_t *y, *uv; /* DEVICE pointers to the first byte of row 0 of each plane */
    int w, h;              /* pixels (of the Y plane) */
    int pitch_y;           /* bytes from one Y row to the next, >= w */
    int pitch_uv;          /* bytes from one chroma row to the next, >= 2 * ((w + 1) / 2) */
    int layout;            /* MI355_YUV_NV12 / MI355_YUV_NV21 */
    int matrix;            /* MI355_YUV_BT601 .. MI355_YUV_BT709_FULL */
    int reserved[2];       /* explicit padding to 48 bytes, zero */
} mi355_frame_yuv;
/* The contract of the u8 calls: table_host is validated before anything is launched; a null plane, w or h outside 1..32768, a pitch
 * below its minimum, an unknown layout or matrix, or a frame the letterbox geometry refuses return MI355_EINVAL with a message that
 * starts "frames_yuv:", and nothing is written.  B <= 65535. */
int mi355_frames_yuv_letterbox_minmax(const mi355_frame_yuv *table_dev, const mi355_frame_yuv *table_host, int B, int w, int h,
                                      float *minmax, void *stream);
int mi355_frames_yuv_letterbox_quantize(const mi355_frame_yuv *table_dev, const mi355_frame_yuv *table_host, int B, int w, int h,
                                        const float *scale_dev, const uint8_t *zp_dev, uint8_t *out_u8, void *stream);
/* The same two calls for frames of three separate planes, as software decoders (libav's yuv420p), JPEG decoders and [3][h][w] tensors
 * deliver them.  plane[0] always holds h rows of w bytes; the other two hold ch rows of cw bytes each, by format:
 *     MI355_PLANAR_I420, _YV12   cw = (w + 1) / 2, ch = (h + 1) / 2     (4:2:0)
 *     MI355_PLANAR_I422          cw = (w + 1) / 2, ch = h               (4:2:2)
 *     MI355_PLANAR_I444          cw = w,           ch = h               (4:4:4)
 *     MI355_PLANAR_RGB, _BGR     cw = w,           ch = h
 * Rows of plane k lie pitch[k] bytes apart, pitch[0] >= w and pitch[1], pitch[2] >= cw; the three pitches are independent and odd
 * w and h are legal.  In the YUV formats pixel (x, y) takes Y[y][x], U[y >> sy][x >> sx] and V[y >> sy][x >> sx], where sx = 1 when
 * the chroma planes are half as wide and sy = 1 when they are half as high, else 0 (nearest sampling: no chroma interpolation, no
 * siting offset -- the NV12 rule, generalised), and its RGB bytes come from the int32 formulas and the `matrix` rows of
 * mi355_frame_yuv above, in registers at every bilinear tap.  In the two RGB formats byte k of a pixel is the byte of the plane that
 * holds channel k (R, G, B); no formula is applied and `matrix` must be 0.  From those bytes on nothing is new: min / max and the
 * quantised bytes are, bit for bit, what the u8 calls give for the interleaved RGB frame of the same pixels, and I420 gives what the
 * _yuv_ calls give for the NV12 frame with the interleaved chroma planes.  A new struct and new calls: MI355_ABI_VERSION is unchanged. */
#define MI355_PLANAR_I420 0  /* planes Y, U, V; chroma (w+1)/2 x (h+1)/2 */
#define MI355_PLANAR_YV12 1  /* planes Y, V, U; same sizes */
#define MI355_PLANAR_I422 2  /* planes Y, U, V; chroma (w+1)/2 x h */
#define MI355_PLANAR_I444 3  /* planes Y, U, V; chroma w x h */
#define MI355_PLANAR_RGB  4  /* planes R, G, B, all w x h; matrix must be 0 */
#define MI355_PLANAR_BGR  5  /* planes B, G, R */
typedef struct mi355_frame_planar {   /* 64 bytes */
    const uint8_t *plane[3];          /* DEVICE pointers, in the order the format names */
    int w, h;                         /* pixels (of plane 0) */
    int pitch[3];                     /* bytes from one row of plane k to the next */
    int format, matrix;               /* MI355_PLANAR_*; matrix: MI355_YUV_BT601 .. _BT709_FULL */
    int reserved[3];                  /* zero */
} mi355_frame_planar;
/* The contract of the _yuv_ calls: table_host is validated before anything is launched; a null plane, w or h outside 1..32768,
 * pitch[0] < w, a chroma pitch below that plane's width, an unknown format or matrix, a non-zero matrix with MI355_PLANAR_RGB / _BGR,
 * or a frame the letterbox geometry refuses return MI355_EINVAL with a message that starts "frames_planar:", and nothing is written.
 * B <= 65535. */
int mi355_frames_planar_letterbox_minmax(const mi355_frame_planar *table_dev, const mi355_frame_planar *table_host,
                                         int B, int w, int h, float *minmax, void *stream);
int mi355_frames_planar_letterbox_quantize(const mi355_frame_planar *table_dev, const mi355_frame_planar *table_host,
                                           int B, int w, int h, const float *scale_dev, const uint8_t *zp_dev,
                                           uint8_t *out_u8, void *stream);
/* The same two calls for frames of one packed plane, four bytes per pixel or per pair of pixels, as display surfaces, screen capture,
 * decoder post-processing (RGBA / BGRA) and USB / V4L2 cameras (YUYV = YUY2, UYVY) deliver them.  Rows lie `pitch` bytes apart.
 *   MI355_PACKED_RGBA, _BGRA, _ARGB, _ABGR: pixel (x, y) is the four bytes at data + y * pitch + 4 * x; plane k (R, G, B) reads byte
 *     {0, 1, 2}, {2, 1, 0}, {1, 2, 3}, {3, 2, 1} of them.  The fourth byte (alpha or padding) has no influence on any result.
 *     pitch >= 4 * w, `matrix` must be 0, no formula is applied.
 *   MI355_PACKED_YUYV, _UYVY, _YVYU (4:2:2): a macropixel of two neighbouring pixels is the four bytes at
 *     data + y * pitch + 4 * (x >> 1): Y0 U Y1 V, U Y0 V Y1 or Y0 V Y1 U.  Pixel x takes Y[x & 1] and the macropixel's (U, V) -- chroma
 *     at [y][x >> 1], MI355_PLANAR_I422's rule --, and its RGB bytes come from the int32 formulas and the `matrix` rows of
 *     mi355_frame_yuv above, in registers at every bilinear tap.  A row holds (w + 1) / 2 macropixels: pitch >= 4 * ((w + 1) / 2); with
 *     an odd w the second luma byte of a row's last macropixel is never used.
 * A pixel / macropixel is one 4-byte load, which the device serves at any alignment: any address and pitch are legal, multiples of 4
 * are the natural and the aligned case.  From the RGB bytes on nothing is new: min / max and the quantised bytes are, bit for bit, what the u8 calls give for the
 * interleaved RGB frame of the same pixels, and what the planar calls give for the MI355_PLANAR_I422 frame with the de-interleaved
 * samples.  A new struct and new calls: MI355_ABI_VERSION is unchanged. */
#define MI355_PACKED_RGBA 0  /* bytes R G B x */
#define MI355_PACKED_BGRA 1  /* bytes B G R x */
#define MI355_PACKED_ARGB 2  /* bytes x R G B */
#define MI355_PACKED_ABGR 3  /* bytes x B G R */
#define MI355_PACKED_YUYV 4  /* bytes Y0 U Y1 V (YUY2) */
#define MI355_PACKED_UYVY 5  /* bytes U Y0 V Y1 */
#define MI355_PACKED_YVYU 6  /* bytes Y0 V Y1 U */
typedef struct mi355_frame_packed {   /* 32 bytes */
    const uint8_t *data;              /* DEVICE pointer to the first byte of row 0 */
    int w, h;                         /* pixels */
    int pitch;                        /* bytes from one row to the next */
    int format, matrix;               /* MI355_PACKED_*; matrix: MI355_YUV_BT601 .. _BT709_FULL, 0 with the four RGB formats */
    int reserved;                     /* zero */
} mi355_frame_packed;
/* The contract of the _yuv_ calls: table_host is validated before anything is launched; a null pointer, w or h outside 1..32768, a
 * pitch below its minimum, an unknown format or matrix, a non-zero matrix with one of the four RGB formats, or a frame the letterbox
 * geometry refuses return MI355_EINVAL with a message that starts "frames_packed:", and nothing is written.  B <= 65535. */
int mi355_frames_packed_letterbox_minmax(const mi355_frame_packed *table_dev, const mi355_frame_packed *table_host,
                                         int B, int w, int h, float *minmax, void *stream);
int mi355_frames_packed_letterbox_quantize(const mi355_frame_packed *table_dev, const mi355_frame_packed *table_host,
                                           int B, int w, int h, const float *scale_dev, const uint8_t *zp_dev,
                                           uint8_t *out_u8, void *stream);
/* The same two calls for P010 / P012 / P016 frames, as hardware decoders deliver HEVC / AV1 Main10 streams: NV12's two planes with
 * 16-bit little-endian samples whose significant bits are at the top.  y holds h rows of w samples, uv (h + 1) / 2 rows of (w + 1) / 2
 * pairs (U, V) of samples; pitches are in BYTES, pitch_y >= 2 * w and pitch_uv >= 4 * ((w + 1) / 2).  The 8-bit sample is the HIGH BYTE
 * of the 16-bit one -- a truncation (sample >> 8), NOT a rounding, and so the same for P010, P012 and P016 --:
 *     Y8[y][x] = y[y * pitch_y + 2 * x + 1]
 *     U8 = uv[cy * pitch_uv + 4 * cx + 1],  V8 = uv[cy * pitch_uv + 4 * cx + 3]     with cx = x >> 1, cy = y >> 1
 * Single bytes are loaded: no alignment is required of the planes or pitches, and the low bytes have no influence on any result.  From
 * these bytes on it is the NV12 source: the results are, bit for bit, what the _yuv_ calls give for the MI355_YUV_NV12 frame
 * (y >> 8, uv >> 8).  The entry has mi355_frame_yuv's field layout; `layout` is reserved.  A new struct and new calls:
 * MI355_ABI_VERSION is unchanged. */
typedef struct mi355_frame_p010 {   /* 48 bytes */
    const uint8_t *y, *uv; /* DEVICE pointers to the first byte of row 0 of each plane */
    int w, h;              /* pixels (of the Y plane) */
    int pitch_y;           /* bytes from one Y row to the next, >= 2 * w */
    int pitch_uv;          /* bytes from one chroma row to the next, >= 4 * ((w + 1) / 2) */
    int layout;            /* reserved, zero */
    int matrix;            /* MI355_YUV_BT601 .. MI355_YUV_BT709_FULL */
    int reserved[2];       /* zero */
} mi355_frame_p010;
/* The contract of the _yuv_ calls: a null plane, w or h outside 1..32768, a pitch below its minimum, an unknown matrix, a non-zero
 * `layout` or `reserved`, or a frame the letterbox geometry refuses return MI355_EINVAL with a message that starts "frames_p010:",
 * and nothing is written.  B <= 65535. */
int mi355_frames_p010_letterbox_minmax(const mi355_frame_p010 *table_dev, const mi355_frame_p010 *table_host, int B, int w, int h,
                                       float *minmax, void *stream);
int mi355_frames_p010_letterbox_quantize(const mi355_frame_p010 *table_dev, const mi355_frame_p010 *table_host, int B, int w, int h,
                                         const float *scale_dev, const uint8_t *zp_dev, uint8_t *out_u8, void *stream);
/* The same two calls for raw sensor frames: one sample per pixel behind a Bayer colour filter (machine-vision cameras: BayerRG8 and its
 * kin; MIPI CSI-2 sensors without an ISP: RAW10 / RAW12) or no filter at all (Mono8 .. Mono16).  The frame is demosaiced in registers
 * at the taps of the letterbox; no RGB frame is written.  D(frame), the interleaved RGB frame the calls stand for, is defined here, all
 * arithmetic in int32:
 *   raw8(x, y), the 8-bit sample, by `sample`:
 *     MI355_RAW_U8      the byte data[y * pitch + x];
 *     MI355_RAW_U16     min(v >> shift, 255) of the little-endian 16-bit value v at data[y * pitch + 2 * x], any address parity,
 *                       shift in 0..8: 2, 4, 6 serve LSB-aligned 10-, 12-, 14-bit samples, 8 MSB-aligned or 16-bit ones.  A truncation
 *                       as in the P010 kind, and a saturation where a sample exceeds its nominal range;
 *     MI355_RAW_MIPI10  CSI-2 RAW10, four pixels in five bytes: data[y * pitch + 5 * (x >> 2) + (x & 3)]; the fifth byte of a group
 *                       holds the low bits and is never read;
 *     MI355_RAW_MIPI12  CSI-2 RAW12, two pixels in three bytes: data[y * pitch + 3 * (x >> 1) + (x & 1)]; the third byte is never read.
 *   c(x, y), the colour of site (x, y): P[y & 1][x & 1] of `pattern` P = MI355_BAYER_RGGB (R G / G B), _BGGR (B G / G R), _GRBG
 *     (G R / B G), _GBRG (G B / R G); MI355_BAYER_MONO: no mosaic.
 *   s(x, y) = tone[c(x, y)][raw8(x, y)], the toned sample: `tone` is a table of 3 x 256 bytes (R, G, B) of this frame, or NULL for the
 *     identity.  It carries black level, white-balance gain and the transfer curve in one lookup, and is applied to samples, before
 *     any averaging.  MONO uses table 0.
 *   Neighbour coordinates outside the frame are reflected without repeating the edge, -1 -> 1 and w -> w - 2, rows likewise, which
 *     keeps the colour phase: Bayer frames need w, h >= 2, MONO frames w, h >= 1.
 *   Bilinear demosaic, >> on non-negative sums.  At an R or B site with own colour A and opposite colour C:
 *       out[A] = s(x, y)
 *       out[G] = (s(x-1, y) + s(x+1, y) + s(x, y-1) + s(x, y+1) + 2) >> 2
 *       out[C] = (s(x-1, y-1) + s(x+1, y-1) + s(x-1, y+1) + s(x+1, y+1) + 2) >> 2
 *     at a G site with Hc = c(x ^ 1, y) and Vc the other of R and B:
 *       out[G] = s(x, y),  out[Hc] = (s(x-1, y) + s(x+1, y) + 1) >> 1,  out[Vc] = (s(x, y-1) + s(x, y+1) + 1) >> 1
 *     MONO: out = (s, s, s).
 * Min / max and the quantised bytes are, bit for bit, what the u8 calls give for the interleaved RGB frame D(frame).  No equality with
 * any other demosaic (OpenCV, camera SDKs) is claimed: their filters and border rules differ.  16-bit samples and MIPI groups are read
 * with byte-granular loads: any address and pitch are legal.  A new struct and new calls: MI355_ABI_VERSION is unchanged. */
#define MI355_BAYER_RGGB 0  /* R G / G B */
#define MI355_BAYER_BGGR 1  /* B G / G R */
#define MI355_BAYER_GRBG 2  /* G R / B G */
#define MI355_BAYER_GBRG 3  /* G B / R G */
#define MI355_BAYER_MONO 4  /* no mosaic: R = G = B = the sample */
#define MI355_RAW_U8 0      /* one byte a sample */
#define MI355_RAW_U16 1     /* two bytes a sample, little-endian, reduced by `shift` */
#define MI355_RAW_MIPI10 2  /* CSI-2 RAW10 */
#define MI355_RAW_MIPI12 3  /* CSI-2 RAW12 */
typedef struct mi355_frame_bayer {   /* 48 bytes */
    const uint8_t *data;             /* DEVICE pointer to the first byte of row 0 */
    const uint8_t *tone;             /* DEVICE pointer to [3][256] bytes, or NULL: identity */
    int w, h;                        /* pixels */
    int pitch;                       /* bytes from one row to the next */
    int pattern;                     /* MI355_BAYER_* */
    int sample;                      /* MI355_RAW_* */
    int shift;                       /* 0..8 with MI355_RAW_U16, else 0 */
    int reserved[2];                 /* zero */
} mi355_frame_bayer;
/* The contract of the _yuv_ calls: table_host is validated before anything is launched, and each of these returns MI355_EINVAL with a
 * message of its own behind "frames_bayer: ", nothing written: a null data pointer; w or h outside 1..32768; an unknown pattern; an
 * unknown sample layout; a shift outside 0..8; a non-zero shift without MI355_RAW_U16; a non-zero `reserved`; pitch < w (U8),
 * < 2 * w (U16), < 5 * ((w + 3) / 4) (MIPI10) or < 3 * ((w + 1) / 2) (MIPI12); a Bayer frame below 2 x 2; a frame the letterbox
 * geometry refuses.  B <= 65535. */
int mi355_frames_bayer_letterbox_minmax(const mi355_frame_bayer *table_dev, const mi355_frame_bayer *table_host, int B, int w, int h,
                                        float *minmax, void *stream);
int mi355_frames_bayer_letterbox_quantize(const mi355_frame_bayer *table_dev, const mi355_frame_bayer *table_host, int B, int w, int h,
                                          const float *scale_dev, const uint8_t *zp_dev, uint8_t *out_u8, void *stream);
/* Frame views: a batch slot looks at a rectangle of its frame, mirrored or turned.  For every kind above, the two calls with a table of
 * views beside the table of frames, one view per slot (views_dev in device memory, views_host its host mirror).
 *
 * Let RGB(frame) be the interleaved RGB frame the kind's entry stands for: the bytes themselves (u8, packed and planar RGB), the int32
 * formulas above with the kind's chroma rule (every YUV kind), D(frame) (Bayer and mono).  The view of a frame is
 *     V = O_orient(a),  a = RGB(frame)[y0 : y0 + h, x0 : x0 + w]                    (a is [h][w][3])
 * with O the EXIF orientations, the transforms that make a file carrying that value upright (numpy notation):
 *     1  a                      2  a[:, ::-1]              3  a[::-1, ::-1]                       4  a[::-1]
 *     5  a.transpose(1, 0, 2)   6  rot90(a, -1)            7  a[::-1, ::-1].transpose(1, 0, 2)    8  rot90(a, 1)
 * Orients 5..8 give a view of h x w pixels.  The crop is a crop of the CONVERTED frame: the chroma of view pixel (x0 + i, y0 + j) is the
 * full frame's sample at ((x0 + i) >> sx, (y0 + j) >> sy), so odd offsets are legal in every subsampled kind, 4:2:2 macropixels and MIPI
 * groups may be cut anywhere, a Bayer site keeps the colour its frame coordinates give it, and Bayer neighbours outside the view but
 * inside the frame are the real samples (reflection happens at the frame's border only).
 *
 * The claim, and the only one: min / max and the quantised bytes are, bit for bit, what the mi355_frames_u8_* calls give for V
 * materialised as an interleaved RGB frame.
 *
 * Refusals (MI355_EINVAL, nothing launched or written), per slot in this order: the kind's own refusals of the FRAME, in their order and
 * words; then behind the kind's prefix "view: orient outside 1..8", "view: reserved must be 0", "view: need w, h >= 1",
 * "view: rectangle outside the frame" (x0 < 0, y0 < 0, x0 + w > the frame's w or y0 + h > the frame's h); then the letterbox geometry of
 * the view's oriented size ("degenerate aspect (resized side < 2)").  New structs and new calls: MI355_ABI_VERSION is unchanged. */
typedef struct mi355_frame_view {   /* 32 bytes */
    int x0, y0, w, h;               /* the rectangle [x0, x0 + w) x [y0, y0 + h) of the stored frame */
    int orient;                     /* 1..8, the EXIF numbering */
    int reserved[3];                /* zero */
} mi355_frame_view;
int mi355_frames_u8_view_letterbox_minmax(const mi355_frame_u8 *table_dev, const mi355_frame_u8 *table_host, const mi355_frame_view *views_dev,
    const mi355_frame_view *views_host, int B, int w, int h, float *minmax, void *stream);
int mi355_frames_u8_view_letterbox_quantize(const mi355_frame_u8 *table_dev, const mi355_frame_u8 *table_host, const mi355_frame_view *views_dev,
    const mi355_frame_view *views_host, int B, int w, int h, const float *scale_dev, const uint8_t *zp_dev, uint8_t *out_u8, void *stream);
int mi355_frames_yuv_view_letterbox_minmax(const mi355_frame_yuv *table_dev, const mi355_frame_yuv *table_host, const mi355_frame_view *views_dev,
    const mi355_frame_view *views_host, int B, int w, int h, float *minmax, void *stream);
int mi355_frames_yuv_view_letterbox_quantize(const mi355_frame_yuv *table_dev, const mi355_frame_yuv *table_host, const mi355_frame_view *views_dev,
    const mi355_frame_view *views_host, int B, int w, int h, const float *scale_dev, const uint8_t *zp_dev, uint8_t *out_u8, void *stream);
int mi355_frames_planar_view_letterbox_minmax(const mi355_frame_planar *table_dev, const mi355_frame_planar *table_host, const mi355_frame_view *views_dev,
    const mi355_frame_view *views_host, int B, int w, int h, float *minmax, void *stream);
int mi355_frames_planar_view_letterbox_quantize(const mi355_frame_planar *table_dev, const mi355_frame_planar *table_host, const mi355_frame_view *views_dev,
    const mi355_frame_view *views_host, int B, int w, int h, const float *scale_dev, const uint8_t *zp_dev, uint8_t *out_u8, void *stream);
int mi355_frames_packed_view_letterbox_minmax(const mi355_frame_packed *table_dev, const mi355_frame_packed *table_host, const mi355_frame_view *views_dev,
    const mi355_frame_view *views_host, int B, int w, int h, float *minmax, void *stream);
int mi355_frames_packed_view_letterbox_quantize(const mi355_frame_packed *table_dev, const mi355_frame_packed *table_host, const mi355_frame_view *views_dev,
    const mi355_frame_view *views_host, int B, int w, int h, const float *scale_dev, const uint8_t *zp_dev, uint8_t *out_u8, void *stream);
int mi355_frames_p010_view_letterbox_minmax(const mi355_frame_p010 *table_dev, const mi355_frame_p010 *table_host, const mi355_frame_view *views_dev,
    const mi355_frame_view *views_host, int B, int w, int h, float *minmax, void *stream);
int mi355_frames_p010_view_letterbox_quantize(const mi355_frame_p010 *table_dev, const mi355_frame_p010 *table_host, const mi355_frame_view *views_dev,
    const mi355_frame_view *views_host, int B, int w, int h, const float *scale_dev, const uint8_t *zp_dev, uint8_t *out_u8, void *stream);
int mi355_frames_bayer_view_letterbox_minmax(const mi355_frame_bayer *table_dev, const mi355_frame_bayer *table_host, const mi355_frame_view *views_dev,
    const mi355_frame_view *views_host, int B, int w, int h, float *minmax, void *stream);
int mi355_frames_bayer_view_letterbox_quantize(const mi355_frame_bayer *table_dev, const mi355_frame_bayer *table_host, const mi355_frame_view *views_dev,
    const mi355_frame_view *views_host, int B, int w, int h, const float *scale_dev, const uint8_t *zp_dev, uint8_t *out_u8, void *stream);
/* The device half of a baseline JPEG decoder: everything after the entropy decode, for a whole batch in two launches, leaving interleaved
 * RGB frames in device memory that the u8 calls above take as they are.  The bytes are the ones stb_image v2.19 returns as the reference
 * compiles it (ref: src/stb_image.h; load_image_color -> stbi_load(.., 3), src/image.c:1293-1315): all of this is integer arithmetic in
 * stb, and every step is restated exactly, computed in 32-bit wrapping arithmetic so that no input is undefined.
 *
 * mi355_jpeg_idct: one launch for every 8x8 block of every component plane of every image.  A plane is blocks_w x blocks_h blocks;
 * block (bx, by) reads coef[(by * blocks_w + bx) * 64 ..], 64 quantised coefficients in natural (row-major, de-zigzagged) order, and
 * the plane's 64 quantiser values, and writes an 8 x 8 byte tile at out[(8 by + r) * 8 * blocks_w + 8 bx ..] (the plane's pitch is
 * 8 * blocks_w).  Per block, in this order: d = (int16_t)(coefficient * quantiser), the low 16 bits of the product (ref :1969-1999);
 * the column pass, +512, >> 10; the row pass, +65536 + (128 << 17), >> 17, clamp to 0..255 (ref :2163-2261).  first_block is the
 * running count of the blocks of the planes before (plane 0: 0).  coef and quant 16-byte aligned, out 8-byte aligned.
 *
 * mi355_jpeg_to_rgb: one launch for the batch; image b is w x h pixels, rows `pitch` >= 3 * w bytes apart at `rgb` (any alignment).
 * Component k of pixel (x, y) is read from comp[k] through stb's resampler for the component's (hs, vs), as a pure function of (x, y)
 * with w_lores = ceil(w / hs) and `rows` the component's real row count:
 *     (1, 1)  plane[y][x]                                   (1, 2)  (3 near[x] + far[x] + 2) >> 2
 *     (2, 1)  ref :3183-3209: 3 : 1 between horizontal neighbours, the first and last pixel of a row take one sample, the pixel before
 *             the last weighs sample w_lores - 2 three times (stb's own asymmetry), w_lores == 1: the sample
 *     (2, 2)  ref :3213-3235: t(i) = 3 near[i] + far[i], then (3 t + t' + 8) >> 4 between neighbours, (t + 2) >> 2 at both ends
 *     other   plane[y / vs][x / hs]
 * near = row y >> 1, far = row (y >> 1) + 1 for an odd y and (y >> 1) - 1 for an even one, clamped to 0 .. rows - 1 (ref :3630-3644).
 * mode: MI355_JPEG_YCBCR converts with ref :3367-3391 (20-bit fixed point, the Cb term of G masked with 0xffff0000, clamp),
 * MI355_JPEG_RGB stores the three samples as they are, MI355_JPEG_GREY replicates comp[0].
 *
 * The contract of the frame calls: table_host mirrors table_dev and is validated before anything is launched (null pointers, alignment,
 * sizes outside 1..32768, a running count that does not add up, hs / vs outside 1..4, rows < ceil(h / vs), a component pitch below
 * ceil(w / hs), pitch < 3 * w, an unknown mode): MI355_EINVAL with a message that starts "jpeg_idct:" / "jpeg_to_rgb:", nothing is
 * written.  New structs and new calls: MI355_ABI_VERSION is unchanged. */
#define MI355_JPEG_YCBCR 0
#define MI355_JPEG_RGB   1
#define MI355_JPEG_GREY  2
typedef struct mi355_jpeg_plane {     /* 48 bytes */
    const int16_t *coef;              /* DEVICE: [blocks_h * blocks_w][64] */
    const uint16_t *quant;            /* DEVICE: [64], natural order */
    uint8_t *out;                     /* DEVICE: 8 * blocks_h rows of 8 * blocks_w bytes */
    int blocks_w, blocks_h;
    int first_block;                  /* blocks of the planes before this one in the table */
    int reserved[3];                  /* zero */
} mi355_jpeg_plane;
typedef struct mi355_jpeg_component { /* 24 bytes */
    const uint8_t *plane;             /* DEVICE: the component's samples (mi355_jpeg_plane.out) */
    int pitch;                        /* bytes from one row to the next */
    int rows;                         /* the component's real row count, >= ceil(h / vs) */
    int hs, vs;                       /* upsampling factors, 1..4 */
} mi355_jpeg_component;
typedef struct mi355_jpeg_image {     /* 96 bytes */
    uint8_t *rgb;                     /* DEVICE: h rows of w interleaved RGB pixels */
    int w, h, pitch;
    int mode;                         /* MI355_JPEG_* */
    mi355_jpeg_component comp[3];     /* MI355_JPEG_GREY reads comp[0] only */
} mi355_jpeg_image;
int mi355_jpeg_idct(const mi355_jpeg_plane *table_dev, const mi355_jpeg_plane *table_host, int nplanes, void *stream);
int mi355_jpeg_to_rgb(const mi355_jpeg_image *table_dev, const mi355_jpeg_image *table_host, int B, void *stream);
/* Entropy decoding of baseline JPEG scans on the device: the step in front of mi355_jpeg_idct.  The host finds the scans and copies
 * their bytes out unstuffed (yolo_quantization_amd/host/jpeg_scan.h); a SEGMENT is one restart interval of a scan, or the whole scan
 * where there is none, and decodes on its own: the DC predictions start at zero.  mi355_jpeg_entropy is one launch for every segment
 * of a batch, one 256-thread workgroup per segment with the segment's Huffman tables in LDS.  The segment's bits are cut into
 * subsequences of subseq_bits bits (a multiple of 32 in 32..8192) that the lanes decode speculatively and re-decode until every
 * lane's entry state (bit position, block slot inside the unit, zigzag index) is its predecessor's exit state; then every lane stores
 * the non-zero coefficients of its blocks at coef[c][block * 64 + natural position].  THE PLANES MUST BE ZERO BEFORE THE LAUNCH.
 *
 * A unit is what the scan interleaves: bh[c] x bv[c] blocks of each of its ncomp components in turn, unit u at column u % units_x and
 * row u / units_x of the unit grid; block (x, y) of component c of that unit is block (ux * bh[c] + x, uy * bv[c] + y) of a plane
 * blocks_w[c] blocks wide.  A one-component scan has bh = bv = 1 and the grid of the component's real size.  The segment holds units
 * first_unit .. first_unit + nunits - 1 and nothing is stored for a block beyond them.  `bits`: nbytes bytes of unstuffed data, 4-byte
 * aligned, followed by zero bytes up to at least ((nbytes + 3) & ~3) + 8.  huff[dc[c]], huff[ac[c]]: the tables of component c.
 * status_dev[s]: 0, or the MI355_JPEG_E* of the first symbol of segment s that decodes to nothing (what was stored before it stays).
 *
 * table_host mirrors table_dev and is validated before anything is launched (null or misaligned pointers, ncomp outside 1..3, bh / bv
 * outside 1..4, a unit grid larger than a plane, units outside the grid, a table index outside 0..nhuff - 1, nbytes above 2^28,
 * subseq_bits): MI355_EINVAL with a message that starts "jpeg_entropy:", nothing is launched.  What the tables at `huff` hold cannot
 * be checked from the host: they decide what is decoded, never where it is stored, and every loop is bounded by the bits of the
 * segment.  New structs and a new call: MI355_ABI_VERSION is unchanged. */
#define MI355_JPEG_EHUFF 1            /* no code of the table matches */
#define MI355_JPEG_EDC   2            /* DC category above 15 */
#define MI355_JPEG_EINDEX 3           /* coefficient index past 63 */
typedef struct mi355_jpeg_huff {      /* 976 bytes: one Huffman table, canonical codes (T.81 C.2) */
    uint16_t look[256];               /* by the next 8 bits: (length << 8) | symbol of a code of <= 8 bits, 0: a longer code */
    int32_t maxcode[17], mincode[17], first[17]; /* per code length 1..16: largest code + 1, smallest code, index of its first symbol */
    int32_t nvalues;
    uint8_t values[256];
} mi355_jpeg_huff;
typedef struct mi355_jpeg_segment {   /* 144 bytes */
    const uint32_t *bits;             /* DEVICE */
    const mi355_jpeg_huff *huff;      /* DEVICE: [nhuff] */
    int16_t *coef[3];                 /* DEVICE: the plane of scan component c, [blocks_h[c] * blocks_w[c]][64] */
    uint32_t nbytes;
    int ncomp;
    int bh[3], bv[3];
    int blocks_w[3], blocks_h[3];
    int dc[3], ac[3];
    int units_x, units_y;
    int first_unit, nunits;
    int nhuff;
    int reserved;                     /* zero */
} mi355_jpeg_segment;
int mi355_jpeg_entropy(const mi355_jpeg_segment *table_dev, const mi355_jpeg_segment *table_host, int nsegments, int subseq_bits,
                       int *status_dev, void *stream);
/* The device half of a PNG decoder: everything after the inflate, for a whole batch in two launches, leaving interleaved RGB frames in
 * device memory that the u8 calls above take as they are.  The bytes are the ones stb_image v2.19 returns as the reference compiles it
 * (ref: src/stb_image.h:4307-4931; load_image_color -> stbi_load(.., 3)); PNG is lossless, so this holds for every colour type, bit
 * depth, filter and for Adam7.  The host parses the chunks and inflates (yolo_quantization_amd/host/png.h).
 *
 * mi355_png_unfilter: one launch for every SEGMENT of a batch; a segment is one pass of one image (a file that is not interlaced is one
 * segment).  `filtered`: rows rows of 1 + row_bytes bytes, each led by its filter byte 0..4 (None, Sub, Up, Average, Paeth; the host
 * has refused anything else, a larger value reconstructs as None); `out`: the reconstructed rows, row_bytes apart.  bpp is the filter
 * unit: channels * depth / 8 for depths 8 and 16, 1 for depths 1, 2 and 4, where the filters run over the packed bytes (ref :4364-4367);
 * row_bytes is a multiple of it.  The row above the first row is zero (ref :4372, first_row_filter).  One wave per segment, four
 * segments per workgroup: lane r owns row y0 + r of a band of 64 rows and is r units behind the lane above it, so that `up` arrives
 * from that lane by one cross-lane move per step; see DESIGN.md.  Any alignment of filtered and out.
 *
 * mi355_png_to_rgb: one launch for the batch, one thread per output pixel.  Image b is w x h pixels, rows `pitch` >= 3 * w bytes apart
 * at `rgb` (any alignment).  The pixel's pass and position in it follow stb's xorig / yorig / xspc / yspc (ref :4554-4557); pass[k] is
 * the reconstructed pass k (0..6; a plain image reads pass[0]; a pass without pixels may be null), its rows ceil(pw * channels * depth
 * / 8) bytes apart with pw the pass's width.  Depths 1 / 2 / 4 are unpacked MSB first, grey scaled by 0xff / 0x55 / 0x11, palette
 * indices not scaled; depth 16 keeps the first (high) byte of each sample; grey is replicated, alpha dropped, a palette index becomes
 * its entry of `palette` (R, G, B per entry) and an index at or above pal_len gives (0, 0, 0).
 *
 * The contract of the frame calls: table_host mirrors table_dev and is validated before anything is launched (null pointers, bpp outside
 * {1, 2, 3, 4, 6, 8}, a zero size, sizes above 32768 pixels, row_bytes no multiple of bpp, pitch < 3 * w, an unknown depth / colour
 * pair, a palette image without palette): MI355_EINVAL with a message that starts "png_unfilter:" / "png_to_rgb:", nothing is written.
 * New structs and new calls: MI355_ABI_VERSION is unchanged. */
typedef struct mi355_png_segment {    /* 32 bytes */
    const uint8_t *filtered;          /* DEVICE: rows * (1 + row_bytes) bytes */
    uint8_t *out;                     /* DEVICE: rows * row_bytes bytes */
    int row_bytes, rows;
    int bpp;                          /* 1, 2, 3, 4, 6 or 8 */
    int reserved;                     /* zero */
} mi355_png_segment;
typedef struct mi355_png_image {      /* 104 bytes */
    uint8_t *rgb;                     /* DEVICE: h rows of w interleaved RGB pixels */
    const uint8_t *palette;           /* DEVICE: [256][3], colour type 3 only */
    const uint8_t *pass[7];           /* DEVICE: the reconstructed passes (mi355_png_segment.out) */
    int w, h, pitch;
    int depth;                        /* 1, 2, 4, 8, 16 */
    int color;                        /* 0 grey, 2 RGB, 3 palette, 4 grey + alpha, 6 RGBA */
    int interlace;                    /* 0, or 1: Adam7 */
    int pal_len;
    int reserved;                     /* zero */
} mi355_png_image;
int mi355_png_unfilter(const mi355_png_segment *table_dev, const mi355_png_segment *table_host, int nsegments, void *stream);
int mi355_png_to_rgb(const mi355_png_image *table_dev, const mi355_png_image *table_host, int B, void *stream);
/* Inflate of the IDAT streams on the device: the step in front of mi355_png_unfilter.  The host walks the chunks and gathers the
 * IDAT payloads behind the two-byte zlib header into one buffer (yolo_quantization_amd/host/png_scan.h); a STREAM is that raw deflate
 * data (RFC 1951) of one image.  mi355_png_inflate is one launch for every stream of a batch, one wave per stream: deflate has no
 * block index, so a stream decodes front to back.  Lane 0 follows the symbols and fills a list of up to 64 tokens a round; all lanes
 * build the blocks' Huffman tables, place the literals, copy the matches and the stored blocks inside a 64 KiB ring of the output in
 * LDS and flush it to `out` in coalesced dword stores; see DESIGN.md.  The bytes are the host decoder's (png_decode_host's
 * `filtered`), and the decode stops at `cap`, whatever the bits say: what a stream holds beyond the bytes the image needs is not read.
 *
 * `z`: nbytes bytes, 4-byte aligned, followed by zero bytes up to at least ((nbytes + 3) & ~3) + 8; nothing beyond them is read.
 * `out`: cap bytes, 4-byte aligned; nothing outside out[0, cap) is written.  rows[k], row_bytes[k], k < npasses: the passes of the
 * image in the order of their bytes, rows[k] rows of 1 + row_bytes[k] bytes; they add up to cap.  Behind the last byte the first byte
 * of every row is checked against 4.  status_dev[s]: 0, or the first reason in the host decoder's order: what the stream raises
 * (MI355_PNG_EBLOCK .. MI355_PNG_EPAST), then MI355_PNG_EPIXELS (the final block ended short of cap), then MI355_PNG_EFILTER.  These are
 * defined returns of a bounded kernel: at most 8 * nbytes + 64 symbol steps and cap output bytes per stream, no wave waits for another.
 *
 * table_host mirrors table_dev and is validated before anything is launched (null or misaligned pointers, nbytes above 2^28, cap of 0
 * or at least 2^31, npasses outside 1..7, passes that do not add up to cap, nstreams outside 1..65535): MI355_EINVAL with a message
 * that starts "png_inflate:".  New struct and a new call: MI355_ABI_VERSION is unchanged. */
#define MI355_PNG_EBLOCK     1        /* bad block type */
#define MI355_PNG_ECORRUPT   2        /* zlib corrupt: a stored block's LEN / NLEN */
#define MI355_PNG_ELENGTHS   3        /* bad codelengths */
#define MI355_PNG_EHUFF      4        /* bad huffman code */
#define MI355_PNG_EDIST      5        /* bad dist */
#define MI355_PNG_EPREMATURE 6        /* premature end of the zlib data */
#define MI355_PNG_EPAST      7        /* read past buffer: a stored block longer than the stream */
#define MI355_PNG_EPIXELS    8        /* not enough pixels */
#define MI355_PNG_EFILTER    9        /* invalid filter */
typedef struct mi355_png_stream {     /* 88 bytes */
    const uint32_t *z;                /* DEVICE: raw deflate data */
    uint8_t *out;                     /* DEVICE: cap bytes */
    uint32_t nbytes;
    uint32_t cap;                     /* the image's filtered bytes: the stop mark */
    int npasses;
    int rows[7], row_bytes[7];
    int reserved;                     /* zero */
} mi355_png_stream;
int mi355_png_inflate(const mi355_png_stream *table_dev, const mi355_png_stream *table_host, int nstreams, int *status_dev, void *stream);
/* *sum_dev += an order-independent 64-bit checksum of `dwords` 32-bit words at buf (device pointers; zero *sum_dev first).  The
 * host's determinism self-check compares it between passes over the same input (network_selfcheck, darknet_q.h). */
int mi355_checksum_u32(const void *buf, long dwords, uint64_t *sum_dev, void *stream);
/* yolo head activations (ref: src/yolo_layer.c:132-146) on the float head tensor [B][n*(classes+5)][H*W]: entries 2 and 3 of every
 * anchor (w, h) are copied bit for bit, every other entry v becomes (float)(1 / (1 + exp(-(double)v))).  Refused with MI355_EINVAL
 * before anything is launched, mi355_last_error() "invalid argument: " and "yolo: null" (in or out is NULL) or
 * "yolo: need B, n, H, W >= 1 and classes >= 0". */
int mi355_yolo_forward(const float *in, float *out, int B, int n, int classes, int H, int W, void *stream);

/* get_yolo_detections + correct_yolo_boxes (ref: src/yolo_layer.c:246-277, 316-345) for a batch, on the device: only
 * detections cross PCIe.  yolo_out: the yolo layer's output [B][n*(classes+5)][H*W]; anchors [2*num] and mask [n] on the
 * device.  Every (cell, anchor) whose objectness exceeds thresh yields a record of 6 + classes floats
 *   {rank = cell * n + anchor, x, y, w, h, objectness, prob[classes] (objectness * class score if > thresh, else 0)}
 * in recs[b][slot] (slot order is arbitrary: sort by rank for the reference's order); counts[b] = number of detections of
 * image b (may exceed max_recs, the surplus is dropped).  Box centre, objectness and scores equal the reference's bits;
 * width / height agree to a few ulp (the reference is built with -Ofast, its exp() is not reproducible). */
int mi355_yolo_detections(const float *yolo_out, int B, int n, int classes, int H, int W, const float *anchors,
                          const int *mask, int netw, int neth, int imw, int imh, float thresh, int relative, float *recs,
                          int max_recs, int *counts, void *stream);

/* mi355_yolo_detections with one letterbox source size per image: imw_dev[b], imh_dev[b] (int, device memory). */
int mi355_yolo_detections_sizes(const float *yolo_out, int B, int n, int classes, int H, int W, const float *anchors,
                                const int *mask, int netw, int neth, const int *imw_dev, const int *imh_dev, float thresh,
                                int relative, float *recs, int max_recs, int *counts, void *stream);

/* The same decode for EVERY yolo layer ("head") of a network and every image of the batch in one call, records in the reference's order
 * straight from the device: no atomic counter decides a slot, no host sort is needed.
 *   heads[nheads]   HOST array, 1 <= nheads <= MI355_YOLO_MAX_HEADS, in network order (it travels to the kernels by value, like every
 *                   argument struct of this library); the pointers in it are device pointers as in mi355_yolo_detections
 *   imw_dev, imh_dev  [B] letterbox source sizes, device memory
 *   recs            device, records of 6 + classes floats in the format above; rank = cell * n + anchor within the record's OWN head
 *   counts          device [B][nheads]: detections FOUND per image and head (may exceed what is kept)
 *   offsets         device [B + 1]: image b's kept records are recs[offsets[b] .. offsets[b + 1]), packed back to back over the batch
 *   work            device scratch of at least mi355_yolo_detections_batch_work_ints(heads, nheads, B) ints (work_ints: what is there)
 * Order inside an image: heads as given, rank ascending inside a head -- the order of the reference's loops (ref: src/network.c:615-638).
 * An image keeps the FIRST max_per_image records of that order (deterministic); nothing is written at or beyond recs[offsets[B]], and
 * offsets[B] <= B * min(max_per_image, sum over heads of n * H * W), which is the capacity recs must have.  Every field of a record
 * carries the bits mi355_yolo_detections_sizes writes for it.  Three launches, whatever B and nheads: count per block of 256 cells,
 * one scan over (image, head, block), one write pass that places every record.
 * MI355_EINVAL before any launch: nheads outside 1..MI355_YOLO_MAX_HEADS, a head with n * H * W >= 2^24 (rank is a float) or n, H,
 * W < 1, classes < 1, max_per_image < 1, B outside 1..65535, B * candidates per image >= 2^31, a null pointer, work_ints too small.
 * A new struct and new calls: MI355_ABI_VERSION is unchanged. */
#define MI355_YOLO_MAX_HEADS 8
typedef struct mi355_yolo_head {
    const float *yolo_out;  /* DEVICE: the yolo layer's output [B][n * (classes + 5)][H * W] */
    const float *anchors;   /* DEVICE: [2 * num] */
    const int *mask;        /* DEVICE: [n] */
    int n, H, W;
    int reserved;           /* zero */
} mi355_yolo_head;
long mi355_yolo_detections_batch_work_ints(const mi355_yolo_head *heads, int nheads, int B); /* 0 on bad arguments */
int mi355_yolo_detections_batch(const mi355_yolo_head *heads, int nheads, int B, int classes, int netw, int neth, const int *imw_dev,
                                const int *imh_dev, float thresh, int relative, int max_per_image, float *recs, int *counts,
                                int *offsets, int *work, long work_ints, void *stream);

#ifdef __cplusplus
}
#endif
#endif
