/*
 * network.c -- host prep, device buffer management and the layer-loop executor.
 *
 *   quantization_weights_and_activations   ref: src/blas.c:259-346
 *   quant_multi_smaller_than_one_...       ref: src/blas.c:387-418
 *   quant_image_with_min_max               ref: src/blas.c:108-168 (quant_weights_with_min_max_channel, 1 channel)
 *   forward_network_gpu                    ref: src/network.c:835-861 with the uint8 hand-off of :248-250
 *   network_predict                        ref: src/network.c:570-581
 *   set_batch_network                      ref: src/network.c:383-397
 */
#include <assert.h>
#include <math.h>
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/time.h>
#include "host_internal.h"

/* ------------------------------------------------------------------------------------------------------ utils */
void error(const char *s) /* ref: src/utils.c:232-237 */
{
    fprintf(stderr, "darknet_q: %s\n", s);
    fflush(stderr);
    exit(-1);
}
void file_error(const char *s)
{
    fprintf(stderr, "Couldn't open file: %s\n", s);
    exit(0);
}
void check_mi355(int rc, const char *what) /* ref: check_error, src/cuda.c:27-49 */
{
    if (rc != MI355_OK) {
        fprintf(stderr, "MI355 error %d in %s: %s\n", rc, what, mi355_last_error());
        error(what);
    }
}
double what_time_is_it_now(void)
{
    struct timeval time;
    if (gettimeofday(&time, NULL)) return 0;
    return (double)time.tv_sec + (double)time.tv_usec * .000001;
}
const char *get_layer_string(LAYER_TYPE t)
{
    switch (t) {
    case CONVOLUTIONAL: return "CONV";
    case MAXPOOL: return "MAX";
    case ROUTE: return "ROUTE";
    case UPSAMPLE: return "UPSAMPLE";
    case SHORTCUT: return "SHORTCUT";
    case YOLO: return "YOLO";
    }
    return "?";
}

static void plan_fusion(network *net);
static void pi_free(network *net);
static void od_free(network *net);

/* Every wait of this file for the device goes through here and is counted (network_host_waits): a blocking copy back is always
 * followed by one. */
void net_wait(network *net)
{
    net->host_waits++;
    check_mi355(mi355_stream_sync(net->stream), "sync");
}
long network_host_waits(network *net) { return net->host_waits; }

/* ------------------------------------------------------------------------------------------------- host prep */
void quant_multi_smaller_than_one_to_scale_and_shift(float real_multiplier, int32_t *quantized_multiplier,
                                                     int *right_shift)
{
    if (!(real_multiplier > 0.f) || !(real_multiplier < 1.f)) { /* ref :391-392 asserts */
        fprintf(stderr, "requantisation multiplier %g is outside (0,1)\n", real_multiplier);
        error("quant_multi_smaller_than_one_to_scale_and_shift");
    }
    int s = 0;
    while (real_multiplier < 0.5f) {
        real_multiplier *= 2.0f;
        s++;
    }
    int64_t q = (int64_t)round((double)(real_multiplier * (float)(1ll << 31)));
    if (q == (1ll << 31)) {
        q /= 2;
        s--;
    }
    if (s < 0) error("quant_multi: negative shift");
    *quantized_multiplier = (int32_t)q;
    *right_shift = s;
}

/* scale / zero point of the layer-0 quantiser from the image's min / max (both seeded with 0.0f), ref: src/blas.c:125-150 */
void image_scale_zero_point(float min_value, float max_value, float *scale, uint8_t *zero_point)
{
    if (min_value == 0 && max_value == 0) error("input image is all zero (ref: src/blas.c:125-128 assert)");
    /* the reference binary (gcc -Ofast) multiplies by the reciprocal constant here; see oracle/oracle.c */
    float nudged_scale = (max_value - min_value) * (1.0f / 255.0f);
    if (nudged_scale == 0) error("zero input scale");
    const double initial_zero_point = (double)(0.0f - min_value / nudged_scale);
    uint8_t zp;
    if (initial_zero_point < QUANT_NEGATIVE_LIMIT) zp = QUANT_NEGATIVE_LIMIT;
    else if (initial_zero_point > QUANT_POSITIVE_LIMIT) zp = QUANT_POSITIVE_LIMIT;
    else zp = (uint8_t)round(initial_zero_point);
    *scale = nudged_scale;
    *zero_point = zp;
}

void quant_image_with_min_max(int count, const float *input, uint8_t *out, float *scale, uint8_t *zero_point)
{
    float min_value = 0.0f, max_value = 0.0f;
    for (int j = 0; j < count; ++j) {
        max_value = input[j] > max_value ? input[j] : max_value;
        min_value = input[j] < min_value ? input[j] : min_value;
    }
    image_scale_zero_point(min_value, max_value, scale, zero_point);
    const float nudged_scale = *scale;
    const uint8_t zp = *zero_point;
    for (int k = 0; k < count; ++k) {
        float t = (float)(round((double)(input[k] / nudged_scale)) + (double)zp);
        int v = (int)t;
        out[k] = (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
    }
}

/* the float bias of filter ii with batch norm folded in (ref :286 -> :594-600, evaluated in double as the C expression promotes) */
static float folded_bias(const layer *l, int ii)
{
    float b = l->biases[ii];
    if (l->batch_normalize)
        b = (float)((double)b - (double)(l->scales[ii] * l->rolling_mean[ii]) /
                                    (sqrt((double)l->rolling_variance[ii]) + (double).000001f));
    return b;
}

static void prep_conv_layer(network *net, int i)
{
    layer *l = &net->layers[i];
    if (i > 0) { /* ref :301-305: input scale / zero point are the previous layer's activation record */
        l->input_data_uint8_scales[0] = net->layers[i - 1].activ_data_uint8_scales[0];
        l->input_data_uint8_zero_point[0] = net->layers[i - 1].activ_data_uint8_zero_point[0];
    }
    const int K = l->c * l->size * l->size; /* ref :306 */
    const float s_in = l->input_data_uint8_scales[0];
    const int zp_in = l->input_data_uint8_zero_point[0];
    if (s_in == 0 || l->activ_data_uint8_scales[0] == 0) error("zero quantisation scale (ref: src/blas.c:312,332 asserts)");
    for (int ii = 0; ii < l->n; ++ii) {
        const float b = folded_bias(l, ii);
        if (l->weight_data_uint8_scales[ii] == 0) error("zero weight scale (ref: src/blas.c:293 assert)");
        l->mult_zero_point[ii] = (uint32_t)(K * zp_in * (int)l->weight_data_uint8_zero_point[ii]);
        int32_t wsum = 0;
        for (int jj = 0; jj < K; ++jj) wsum += l->weights_uint8[(size_t)ii * K + jj];
        l->weights_sum_int[ii] = (int32_t)(l->mult_zero_point[ii] - (uint32_t)(wsum * zp_in));
        l->M[ii] = s_in * l->weight_data_uint8_scales[ii] / l->activ_data_uint8_scales[0];
        quant_multi_smaller_than_one_to_scale_and_shift(l->M[ii], &l->M0[ii], &l->M0_right_shift[ii]);
        l->M0_right_shift_value[ii] = pow(2, -l->M0_right_shift[ii]);
        l->M_value[ii] = pow(2, -31) * l->M0[ii];
        float t = b / (s_in * l->weight_data_uint8_scales[ii]) + (float)l->weights_sum_int[ii]; /* ref :333 */
        l->biases_int32[ii] = (int32_t)t;
    }
}

static void alloc_layer_device(network *net, int i)
{
    layer *l = &net->layers[i];
    void *shared_blob = l->blob_shared ? l->blob_gpu : NULL; /* a replica's weights are its parent's: survive the re-allocation */
    free_layer_device(l);
    l->blob_gpu = shared_blob;
    const int B = net->batch;
    l->batch = B;
    if (l->type != YOLO) {
        size_t bytes = mi355_tensor_describe(&l->out_t, B, l->out_h, l->out_w, l->out_c);
        if (!bytes) error("bad tensor dims");
        check_mi355(mi355_alloc(&l->out_t.data, bytes), "alloc activations");
        check_mi355(mi355_tensor_fill(&l->out_t, l->activ_data_uint8_zero_point[0], net->stream), "fill activations");
        check_mi355(mi355_alloc((void **)&l->output_uint8_nchw_gpu, (size_t)B * l->outputs), "alloc nchw scratch");
    }
    if (l->type == YOLO || l->quant_stop_flag)
        check_mi355(mi355_alloc((void **)&l->output_gpu, (size_t)B * l->outputs * sizeof(float)), "alloc float out");
    if (l->type == CONVOLUTIONAL && net->dump_int32)
        check_mi355(mi355_alloc((void **)&l->output_int32_gpu, (size_t)B * l->outputs * sizeof(int32_t)), "alloc int32 out");
    free(l->output); free(l->output_int32); free(l->output_uint8_final);
    l->output = calloc((size_t)B * l->outputs, sizeof(float));
    l->output_int32 = l->type == CONVOLUTIONAL ? calloc((size_t)B * l->outputs, sizeof(int32_t)) : NULL;
    l->output_uint8_final = calloc((size_t)B * l->outputs, sizeof(uint8_t));
}

static void upload_conv(network *net, int i, int with_raw)
{
    layer *l = &net->layers[i];
    if (l->blob_shared) error("upload_conv on a replica (its packed weights belong to the parent network)");
    if (l->blob_gpu) { mi355_free(l->blob_gpu); l->blob_gpu = NULL; }
    check_mi355(mi355_alloc(&l->blob_gpu, l->blob_bytes), "alloc blob");
    check_mi355(mi355_h2d(l->blob_gpu, l->blob_host, l->blob_bytes, net->stream), "upload blob");
    if (with_raw) {
        check_mi355(mi355_alloc((void **)&l->weights_uint8_gpu, (size_t)l->nweights), "alloc raw weights");
        check_mi355(mi355_h2d(l->weights_uint8_gpu, l->weights_uint8, (size_t)l->nweights, net->stream), "upload raw weights");
        check_mi355(mi355_alloc((void **)&l->weight_zero_point_gpu, (size_t)l->n), "alloc zp_w");
        check_mi355(mi355_h2d(l->weight_zero_point_gpu, l->weight_data_uint8_zero_point, (size_t)l->n, net->stream), "upload zp_w");
    }
    l->prepared = 1;
}

/* Concat elimination.  forward_route_layer_quant (ref: src/route_layer.c:107-130) copies its inputs' bytes side by side,
 * unscaled.  When every input of a route can write its channels straight into the route's buffer -- its out_t becomes a
 * window (data + channel offset, the route's cell stride) of that buffer -- the copy disappears; a one-input route
 * simply shares its input's tensor.  A producer qualifies when nothing reads ITS pad cells with a different zero point
 * (the window's pads are the route's: a 3x3 conv consuming the producer directly needs them to be its own input zero
 * point), its channel count is a multiple of 16, and it stores its tensor at all (no conv+pool fusion). */
static int view_producer_ok(network *net, int j, int r)
{
    layer *p = &net->layers[j];
    if (j >= r || p->out_view || p->out_c % 16) return 0;
    if (p->type != CONVOLUTIONAL && p->type != UPSAMPLE && p->type != MAXPOOL) return 0;
    if (p->type == CONVOLUTIONAL && p->fuse_next == FUSE_POOL && !p->fuse_pool_keep && net->fuse_maxpool) return 0;
    if (j > 0 && net->layers[j - 1].fuse_next == FUSE_POOL && net->fuse_maxpool && p->type == MAXPOOL) return 0; /* written by the fused conv */
    const int zp_differs = p->activ_data_uint8_zero_point[0] != net->layers[r].activ_data_uint8_zero_point[0];
    if (j + 1 < net->n) {
        layer *c = &net->layers[j + 1];
        if (c->type == CONVOLUTIONAL && c->size != 1 && zp_differs) return 0;
    }
    /* a one-input route that plan_views elides shares the producer's tensor: the layer after THAT route reads the same
     * pad cells */
    for (int r2 = 0; r2 + 1 < net->n; ++r2) {
        layer *q = &net->layers[r2];
        if (q->type != ROUTE || q->n != 1 || q->input_layers[0] != j) continue;
        layer *c = &net->layers[r2 + 1];
        if (c->type == CONVOLUTIONAL && c->size != 1 && zp_differs) return 0;
    }
    return 1;
}

static void plan_views(network *net)
{
    if (net->dump_int32) return; /* parity dumps keep every tensor in its own buffer */
    for (int r = 0; r < net->n; ++r) { /* concatenating routes first: their inputs must not be shared tensors yet */
        layer *l = &net->layers[r];
        if (l->type != ROUTE || l->n < 2) continue;
        int ok = 1;
        for (int k = 0; k < l->n; ++k) {
            ok &= view_producer_ok(net, l->input_layers[k], r);
            for (int k2 = 0; k2 < k; ++k2) ok &= l->input_layers[k2] != l->input_layers[k];
        }
        if (!ok) continue;
        int off = 0;
        for (int k = 0; k < l->n; ++k) {
            layer *p = &net->layers[l->input_layers[k]];
            mi355_free(p->out_t.data);
            p->out_t = l->out_t;
            p->out_t.data = (char *)l->out_t.data + off;
            p->out_t.C = p->out_c;
            p->out_view = 1;
            off += p->out_c;
        }
        l->route_elided = 1;
    }
    for (int r = 0; r < net->n; ++r) {
        layer *l = &net->layers[r];
        if (l->type != ROUTE || l->n != 1) continue;
        layer *p = &net->layers[l->input_layers[0]];
        if (l->input_layers[0] >= r || p->type == YOLO || !p->out_t.data) continue;
        if (p->type == CONVOLUTIONAL && p->fuse_next == FUSE_POOL && !p->fuse_pool_keep && net->fuse_maxpool) continue;
        mi355_free(l->out_t.data);
        l->out_t = p->out_t;
        l->out_view = 1;
        l->route_elided = 1;
    }
}

static void alloc_network_device(network *net)
{
    if (mi355_abi_version() != MI355_ABI_VERSION) {
        fprintf(stderr, "libmi355yolo.so speaks ABI %d, this host was built against %d\n", mi355_abi_version(), MI355_ABI_VERSION);
        error("mi355 ABI mismatch");
    }
    check_mi355(mi355_init(net->gpu_index), "mi355_init");
    if (!net->stream && !net->on_default_stream) check_mi355(mi355_stream_acquire(&net->stream), "stream");
    if (net->input_uint8_gpu) mi355_free(net->input_uint8_gpu);
    if (net->input_t.data) mi355_free(net->input_t.data);
    check_mi355(mi355_alloc((void **)&net->input_uint8_gpu, (size_t)net->batch * net->inputs), "alloc input");
    size_t bytes = mi355_tensor_describe(&net->input_t, net->batch, net->h, net->w, net->c);
    check_mi355(mi355_alloc(&net->input_t.data, bytes), "alloc input tensor");
    check_mi355(mi355_tensor_fill(&net->input_t, net->layers[0].input_data_uint8_zero_point[0], net->stream), "fill input");
    mi355_tensor_describe_nchw(&net->input_nchw_t, net->batch, net->h, net->w, net->c);
    net->input_nchw_t.data = net->input_uint8_gpu;
    net->layers[0].input_direct = net->c == 3 && !net->dump_int32 && !net->input_direct_off;
    for (int i = 0; i < net->n; ++i) alloc_layer_device(net, i);
    plan_views(net);
    if (net->graph) { mi355_graph_destroy(net->graph); net->graph = NULL; }
}

/* 16.16 multipliers of the two addends of every quantized [shortcut] (mi355_shortcut_multiplier) */
static void prep_shortcut_layers(network *net)
{
    for (int i = 1; i < net->n; ++i) {
        layer *l = &net->layers[i];
        if (l->type != SHORTCUT) continue;
        const layer *a = &net->layers[i - 1], *b = &net->layers[l->index];
        if (a->type == YOLO || b->type == YOLO) error("shortcut: inputs must be quantized layers");
        check_mi355(mi355_shortcut_multiplier(a->activ_data_uint8_scales[0], l->activ_data_uint8_scales[0], &l->shortcut_Ka),
                    "mi355_shortcut_multiplier (previous layer)");
        check_mi355(mi355_shortcut_multiplier(b->activ_data_uint8_scales[0], l->activ_data_uint8_scales[0], &l->shortcut_Kb),
                    "mi355_shortcut_multiplier (`from` layer)");
    }
}

/* does any layer other than i + 1 read layer i's own tensor? (a route input, the `from` of a shortcut) */
static int output_read_elsewhere(const network *net, int i)
{
    for (int j = 0; j < net->n; ++j) {
        const layer *q = &net->layers[j];
        if (q->type == ROUTE)
            for (int k = 0; k < q->n; ++k)
                if (q->input_layers[k] == i) return 1;
        if (q->type == SHORTCUT && q->index == i) return 1;
    }
    return 0;
}

void quantization_prep_host(network *net, float in_scale, uint8_t in_zp)
{
    layer *l0 = &net->layers[0];
    if (l0->type != CONVOLUTIONAL) error("first layer must be convolutional");
    prep_shortcut_layers(net);
    l0->input_data_uint8_scales[0] = in_scale;
    l0->input_data_uint8_zero_point[0] = in_zp;
    for (int i = 0; i < net->n; ++i) {
        layer *l = &net->layers[i];
        if (l->type != CONVOLUTIONAL) continue;
        prep_conv_layer(net, i);
        /* a 3-filter conv stores 4-byte cells of plain bytes (the image's layout); only a convolution reads those */
        if (l->n == 3 && ((i + 1 < net->n && net->layers[i + 1].type != CONVOLUTIONAL && net->layers[i + 1].type != ROUTE) ||
                          output_read_elsewhere(net, i))) {
            fprintf(stderr, "layer %d: a 3-filter convolution can only feed another convolution\n", i);
            error("unsupported layer after a 3-filter convolution");
        }
        size_t sz = mi355_conv_pack_size(l->n, l->c, l->size);
        if (!sz) {
            fprintf(stderr, "layer %d: conv %dx%d, %d->%d channels is not supported by the gfx950 kernels "
                            "(sizes above 11 are refused)\n", i, l->size, l->size, l->c, l->n);
            error("unsupported convolution shape");
        }
        free(l->blob_host);
        l->blob_host = malloc(sz);
        l->blob_bytes = sz;
        check_mi355(mi355_conv_pack(l->n, l->c, l->size, l->weights_uint8, l->weight_data_uint8_zero_point,
                                    l->biases_int32, l->M_value, l->M0_right_shift_value, l->blob_host),
                    "mi355_conv_pack");
        /* the fused conv + maxpool kernels' per-channel epilogue constants for this layer's activation and zero point */
        check_mi355(mi355_conv_pack_epilogue(l->n, l->c, l->size, l->activation, l->activ_data_uint8_zero_point[0], l->blob_host),
                    "mi355_conv_pack_epilogue");
    }
    plan_fusion(net); /* pure host logic: the candidates are readable (dnq_layer_plan) without a device */
}

/* The fusion candidates: conv i can run the layer after it in its own kernel, in the one way that layer's type allows
 * (layer.fuse_next).  The planner judges by shape; the launchers have the last word at run time (layers.c).
 *   maxpool:  the reference's size-2 window, stride 2 on an even map (or stride 1 behind a 128 / 256-channel conv), behind a 3x3
 *             stride-1 conv; the conv's own tensor has no other reader, or (128 / 256 channels) is stored as well (fuse_pool_keep)
 *   upsample: the conv stores every pixel stride x stride times; its own tensor has no other reader
 *   shortcut: the conv's epilogue does the quantized residual add; its own tensor has no other reader and is not the `from`
 *   yolo:     a quant_stop head conv whose kernel writes both float tensors */
static void plan_fusion(network *net)
{
    for (int i = 0; i < net->n; ++i) net->layers[i].fuse_next = net->layers[i].fuse_pool_keep = 0;
    for (int i = 0; i + 1 < net->n; ++i) {
        layer *c = &net->layers[i], *p = &net->layers[i + 1];
        if (c->type != CONVOLUTIONAL) continue;
        switch (p->type) {
        case SHORTCUT:
            if (c->stride == 1 && !c->quant_stop_flag && !p->quant_stop_flag && c->c % 16 == 0 && p->index != i && !output_read_elsewhere(net, i))
                c->fuse_next = FUSE_SHORTCUT;
            break;
        case UPSAMPLE:
            /* (an upsample with a quant_stop float tail runs on its own: the fused store skips the layer, and with it the tail) */
            if (!c->quant_stop_flag && !p->quant_stop_flag && c->c % 64 == 0 && p->stride <= 4 && c->stride == 1 && !output_read_elsewhere(net, i))
                c->fuse_next = FUSE_UPSAMPLE;
            break;
        case YOLO:
            if (c->quant_stop_flag && c->c % 16 == 0 && c->stride == 1 && c->n == p->n * (p->classes + 5)) c->fuse_next = FUSE_YOLO;
            break;
        case MAXPOOL:
            if (c->size != 3 || c->stride != 1 || c->quant_stop_flag || p->quant_stop_flag || p->size != 2 || p->pad / 2 != 0) break;
            if (c->c == 128 || c->c == 256) {
                /* the weights-stationary kernel of the middle layers (conv_ws3.hip) pools the bytes of its tile in LDS: the stride-2
                 * window on even maps, and the reference's stride-1 window (pad = 1: same size as the conv's map; yolov3-tiny's
                 * layer 11); it stores the conv's own tensor as well when a route reads it (layer 8) */
                const int s2 = p->stride == 2 && !(c->out_h & 1) && !(c->out_w & 1);
                const int s1 = p->stride == 1 && p->pad == 1 && p->out_h == c->out_h && p->out_w == c->out_w && c->out_h > 1;
                if (!s2 && !s1) break;
                c->fuse_next = FUSE_POOL;
                c->fuse_pool_keep = output_read_elsewhere(net, i);
                break;
            }
            if (p->stride != 2 || (c->out_h & 1) || (c->out_w & 1) || (c->c != 3 && c->c % 16)) break;
            /* 64-byte-chunk layers use the row-image kernel, which has no fused form; 64 -> 64..128 has its own fused kernel */
            if (c->c % 64 == 0 && !(c->c == 64 && c->n % 32 == 0 && c->n >= 64 && c->n <= 128)) break;
            if (!output_read_elsewhere(net, i)) c->fuse_next = FUSE_POOL;
            break;
        default:
            break;
        }
    }
}

void quantization_weights_and_activations_fixed_input(network *net, float in_scale, uint8_t in_zp)
{
    if (net->n_replicas > 0 || net->replica_of) error("quantization_weights_and_activations: not while replicas share this network's packed weights");
    quantization_prep_host(net, in_scale, in_zp);
    alloc_network_device(net);
    for (int i = 0; i < net->n; ++i)
        if (net->layers[i].type == CONVOLUTIONAL) upload_conv(net, i, net->has_host_weights);
    net_wait(net);
    net->prepared = 1;
}

static void pi_bank_update(network *net, const float *scale, const uint8_t *zp);
static void od_pairs_from_host(network *net, const float *scale, const uint8_t *zp);
static void quantize_on_device(network *net, const float *input_gpu);

void quantization_weights_and_activations(network *net)
{
    if (net->per_image) { /* every image with its own min / max (the reference's batch-1 quantiser, ref :279, per image) */
        float *s = malloc(sizeof(float) * (size_t)net->batch);
        uint8_t *zp = malloc((size_t)net->batch);
        for (int b = 0; b < net->batch; ++b)
            quant_image_with_min_max(net->inputs, net->input + (size_t)b * net->inputs, net->input_uint8 + (size_t)b * net->inputs, &s[b], &zp[b]);
        if (!net->prepared) quantization_weights_and_activations_fixed_input(net, s[0], zp[0]);
        if (net->input_on_device) od_pairs_from_host(net, s, zp);
        else pi_bank_update(net, s, zp);
        free(s); free(zp);
        push_network_input_uint8(net, net->input_uint8);
        return;
    }
    /* ref :279: dynamic layer-0 quantiser on the float image in net->input (image 0 defines scale / zero point) */
    float s; uint8_t zp;
    quant_image_with_min_max(net->inputs, net->input, net->input_uint8, &s, &zp);
    quantization_weights_and_activations_fixed_input(net, s, zp);
    if (net->input_on_device) od_pairs_from_host(net, &s, &zp); /* layer 0 runs on the bank in this mode */
    for (int b = 1; b < net->batch; ++b) { /* further images: same scale (batch > 1 is our extension) */
        float *x = net->input + (size_t)b * net->inputs;
        uint8_t *o = net->input_uint8 + (size_t)b * net->inputs;
        for (int k = 0; k < net->inputs; ++k) {
            int v = (int)(float)(round((double)(x[k] / s)) + (double)zp);
            o[k] = (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
        }
    }
    push_network_input_uint8(net, net->input_uint8);
}

/* One (scale, zero point) for the whole batch, as image 0 defines it: the first call prepares the network with it; a later call
 * with another pair re-derives and re-uploads layer 0's multipliers and blob in place (no other layer depends on the input scale).
 * Shared by the device input paths (float images, 8-bit frames). */
void input_pair_shared(network *net, float s, uint8_t zp)
{
    layer *l0 = &net->layers[0];
    if (!net->prepared) {
        quantization_weights_and_activations_fixed_input(net, s, zp);
    } else if (l0->input_data_uint8_scales[0] != s || l0->input_data_uint8_zero_point[0] != zp) {
        if (net->replica_of) error("the input scale changed: a replica shares its parent's layer-0 blob and cannot re-derive it");
        if (net->n_replicas > 0) error("the input scale changed: layer 0's blob is shared with replicas that may be running; free them first");
        if (!net->has_host_weights && !net->has_l0_weights)
            error("the input scale changed but this network holds no raw layer-0 weights to re-derive layer 0 from");
        const int zp_changed = l0->input_data_uint8_zero_point[0] != zp;
        l0->input_data_uint8_scales[0] = s;
        l0->input_data_uint8_zero_point[0] = zp;
        prep_conv_layer(net, 0);
        check_mi355(mi355_conv_pack(l0->n, l0->c, l0->size, l0->weights_uint8, l0->weight_data_uint8_zero_point,
                                    l0->biases_int32, l0->M_value, l0->M0_right_shift_value, l0->blob_host), "mi355_conv_pack");
        check_mi355(mi355_conv_pack_epilogue(l0->n, l0->c, l0->size, l0->activation, l0->activ_data_uint8_zero_point[0], l0->blob_host),
                    "mi355_conv_pack_epilogue");
        check_mi355(mi355_h2d(l0->blob_gpu, l0->blob_host, l0->blob_bytes, net->stream), "upload blob 0");
        if (zp_changed) check_mi355(mi355_tensor_fill(&net->input_t, zp, net->stream), "fill input");  /* pad cells = zero point */
        net_wait(net);  /* blob_host may be repacked by the next call */
        /* a captured graph holds layer 0's kernel arguments by value: the planar first-layer kernels take the pad value
         * (the input zero point) from there, not from pad cells in memory -> re-capture on the next forward */
        if (net->graph) { mi355_graph_destroy(net->graph); net->graph = NULL; }
    }
}

/* The same on the device (quantiser half): `input_gpu` holds batch x inputs floats in HBM.  Image 0
 * defines scale / zero point as in the reference (src/blas.c:279); min / max are reduced on the device, the two floats
 * come back to the host, which evaluates the reference's scale / zero-point expressions and -- only when they differ
 * from the ones layer 0 was prepared with -- re-derives and re-uploads layer 0's multipliers and blob in place (no other
 * layer depends on the input scale); the per-element quantiser then runs on the device straight into the network's uint8
 * input.  Byte-identical to quantization_weights_and_activations() on the same floats. */
static void quantize_per_image_gpu(network *net, const float *input_gpu);

void quantization_weights_and_activations_gpu(network *net, const float *input_gpu)
{
    if (!input_gpu) error("quantization_weights_and_activations_gpu: null input");
    check_mi355(mi355_init(net->gpu_index), "mi355_init");
    if (!net->stream && !net->on_default_stream) check_mi355(mi355_stream_acquire(&net->stream), "stream");
    if (net->input_on_device) { quantize_on_device(net, input_gpu); return; }
    if (net->per_image) { quantize_per_image_gpu(net, input_gpu); return; }
    if (!net->quant_mm_gpu) check_mi355(mi355_alloc((void **)&net->quant_mm_gpu, 2 * sizeof(float)), "alloc minmax");
    float mm[2];
    check_mi355(mi355_image_minmax(input_gpu, net->inputs, net->quant_mm_gpu, net->stream), "mi355_image_minmax");
    check_mi355(mi355_d2h(mm, net->quant_mm_gpu, sizeof(mm), net->stream), "minmax d2h");
    net_wait(net);
    float s; uint8_t zp;
    image_scale_zero_point(mm[1] + 0.0f, mm[0], &s, &zp);
    input_pair_shared(net, s, zp);
    check_mi355(mi355_image_quantize(input_gpu, (long)net->batch * net->inputs, s, zp, net->input_uint8_gpu, net->stream),
                "mi355_image_quantize");
}

/* ---------------------------------------------------------------------------------- per-image input quantisation
 * Only layer 0 depends on the input scale (ref: src/blas.c:300-333).  The bank holds layer-0 blobs packed by the same code as
 * the shared-scale path (prep_conv_layer + mi355_conv_pack + mi355_conv_pack_epilogue), so every entry is bit-identical to the
 * blob a batch-1 run of its image would use.  Its slots double as a cache keyed by (scale bits, zero point): a slot is only
 * repacked and re-uploaded when a batch brings a key the bank does not hold.  Uploads are asynchronous on the network's stream;
 * the host staging of a slot is only rewritten after the next batch's min / max sync, when the previous upload is done. */
static int l0_per_image_shape_ok(const layer *l)
{
    return l->type == CONVOLUTIONAL && l->c == 3 && l->size == 3 && l->stride == 1 && l->pad == 1;
}

static network *l0_source(network *net) { return net->replica_of ? net->replica_of : net; } /* who holds layer 0's raw weights */

/* 0, or MI355_EINVAL with a message: can layer 0 run on a bank of blobs derived per input pair? */
static int l0_bank_refusal(const network *net, const char *who)
{
    const layer *l0 = &net->layers[0];
    if (!l0_per_image_shape_ok(l0)) {
        fprintf(stderr, "%s: layer 0 (%s %dx%d stride %d, %d -> %d) is not served per image: only a "
                        "3 -> n 3x3 stride-1 convolution with pad 1 runs on the first-layer kernels\n",
                who, get_layer_string(l0->type), l0->size, l0->size, l0->stride, l0->c, l0->n);
        return MI355_EINVAL;
    }
    const network *src = net->replica_of ? net->replica_of : net;
    if (src->prepared && !src->has_host_weights && !src->has_l0_weights) {
        fprintf(stderr, "%s: this network holds no raw layer-0 weights to derive per-image constants from\n", who);
        return MI355_EINVAL;
    }
    return 0;
}

int set_input_quantization_per_image(network *net, int on)
{
    if (!on) {
        if (net->per_image && net->graph) { mi355_graph_destroy(net->graph); net->graph = NULL; } /* captured with the per-image launches */
        net->per_image = 0;
        return 0;
    }
    if (l0_bank_refusal(net, "set_input_quantization_per_image")) return MI355_EINVAL;
    if (!net->per_image && net->graph) { mi355_graph_destroy(net->graph); net->graph = NULL; }
    net->per_image = 1;
    return 0;
}

void network_input_quantization(network *net, float *scale, uint8_t *zp)
{
    const int B = net->batch;
    if (net->input_on_device && net->od_idx_gpu) { /* the pairs never left the device: wait for them */
        char *pairs = malloc(5 * (size_t)B);
        check_mi355(mi355_d2h(pairs, od_scale_dev(net), 5 * (size_t)B, net->stream), "pull input pairs");
        net_wait(net);
        memcpy(scale, pairs, sizeof(float) * (size_t)B);
        memcpy(zp, pairs + 4 * (size_t)B, (size_t)B);
        free(pairs);
        return;
    }
    if (!net->per_image || !net->pi_idx_host) {
        for (int b = 0; b < B; ++b) { scale[b] = net->layers[0].input_data_uint8_scales[0]; zp[b] = net->layers[0].input_data_uint8_zero_point[0]; }
        return;
    }
    memcpy(scale, (char *)net->pi_idx_host + 4 * (size_t)B, sizeof(float) * (size_t)B);
    memcpy(zp, (char *)net->pi_idx_host + 8 * (size_t)B, (size_t)B);
}

static void pi_free(network *net)
{
    if (net->pi_bank_gpu) mi355_free(net->pi_bank_gpu);
    if (net->pi_idx_gpu) mi355_free(net->pi_idx_gpu);
    if (net->pi_mm_gpu) mi355_free(net->pi_mm_gpu);
    free(net->pi_bank_host); free(net->pi_idx_host); free(net->pi_mm_host);
    free(net->pi_key_scale); free(net->pi_key_zp); free(net->pi_stamp);
    net->pi_bank_gpu = net->pi_bank_host = net->pi_idx_gpu = net->pi_idx_host = NULL;
    net->pi_mm_gpu = net->pi_mm_host = NULL;
    net->pi_key_scale = NULL; net->pi_key_zp = NULL; net->pi_stamp = NULL;
    net->pi_cap = 0;
}

static void pi_alloc(network *net)
{
    const int B = net->batch;
    const layer *l0 = &l0_source(net)->layers[0];
    const size_t eb = (mi355_conv_pack_size(l0->n, l0->c, l0->size) + 255) & ~(size_t)255;
    if (net->pi_bank_gpu && net->pi_cap >= B && net->pi_entry_bytes == eb) return;
    pi_free(net);
    net->pi_cap = 2 * B < 8 ? 8 : 2 * B; /* a batch needs B slots at most; the rest keeps recent keys cached */
    net->pi_entry_bytes = eb;
    check_mi355(mi355_alloc(&net->pi_bank_gpu, eb * (size_t)net->pi_cap), "alloc layer-0 bank");
    net->pi_bank_host = calloc((size_t)net->pi_cap, eb);
    net->pi_key_scale = calloc((size_t)net->pi_cap, sizeof(uint32_t));
    net->pi_key_zp = malloc(sizeof(int) * (size_t)net->pi_cap);
    net->pi_stamp = calloc((size_t)net->pi_cap, sizeof(long));
    for (int k = 0; k < net->pi_cap; ++k) net->pi_key_zp[k] = -1;
    check_mi355(mi355_alloc(&net->pi_idx_gpu, 9 * (size_t)B), "alloc layer-0 index");
    net->pi_idx_host = calloc(9, (size_t)B);
    check_mi355(mi355_alloc((void **)&net->pi_mm_gpu, 2 * sizeof(float) * (size_t)B), "alloc minmax");
    net->pi_mm_host = calloc(2 * (size_t)B, sizeof(float));
}

/* layer 0's blob for input scale s / zero point zp into dst: the shared-scale path's own code (prep_conv_layer, mi355_conv_pack,
 * mi355_conv_pack_epilogue) on the network that holds the raw weights -- a replica's parent.  prep_conv_layer derives into the
 * layer's record; every field it writes is saved before and restored after, under one process-wide lock (replicas of one parent may
 * be quantised from several host threads), so the record reads as it did before the call. */
static pthread_mutex_t pi_pack_mu = PTHREAD_MUTEX_INITIALIZER;

static void pi_pack(network *net, float s, uint8_t zp, void *dst)
{
    network *src = l0_source(net);
    layer *l0 = &src->layers[0];
    if (!src->has_host_weights && !src->has_l0_weights) error("per-image input: no raw layer-0 weights to derive the constants from");
    const size_t n = (size_t)l0->n;
    pthread_mutex_lock(&pi_pack_mu);
    /* the record prep_conv_layer rewrites, saved in one scratch block */
    struct { void *p; size_t bytes; } f[] = {
        {l0->mult_zero_point, n * sizeof(*l0->mult_zero_point)}, {l0->weights_sum_int, n * sizeof(*l0->weights_sum_int)},
        {l0->M, n * sizeof(*l0->M)}, {l0->M0, n * sizeof(*l0->M0)}, {l0->M0_right_shift, n * sizeof(*l0->M0_right_shift)},
        {l0->M0_right_shift_value, n * sizeof(*l0->M0_right_shift_value)}, {l0->M_value, n * sizeof(*l0->M_value)},
        {l0->biases_int32, n * sizeof(*l0->biases_int32)}, {l0->input_data_uint8_scales, sizeof(float)},
        {l0->input_data_uint8_zero_point, sizeof(uint8_t)}};
    const int nf = (int)(sizeof(f) / sizeof(f[0]));
    size_t total = 0;
    for (int k = 0; k < nf; ++k) total += f[k].bytes;
    char *save = malloc(total), *q = save;
    for (int k = 0; k < nf; ++k) { memcpy(q, f[k].p, f[k].bytes); q += f[k].bytes; }
    l0->input_data_uint8_scales[0] = s;
    l0->input_data_uint8_zero_point[0] = zp;
    prep_conv_layer(src, 0);
    const int rc = mi355_conv_pack(l0->n, l0->c, l0->size, l0->weights_uint8, l0->weight_data_uint8_zero_point, l0->biases_int32,
                                   l0->M_value, l0->M0_right_shift_value, dst);
    const int rc2 = rc ? rc : mi355_conv_pack_epilogue(l0->n, l0->c, l0->size, l0->activation, l0->activ_data_uint8_zero_point[0], dst);
    q = save;
    for (int k = 0; k < nf; ++k) { memcpy(f[k].p, q, f[k].bytes); q += f[k].bytes; }
    free(save);
    pthread_mutex_unlock(&pi_pack_mu);
    check_mi355(rc, "mi355_conv_pack");
    check_mi355(rc2, "mi355_conv_pack_epilogue");
}

/* the same, exported for host-only checks: layer 0's bank entry for (s, zp) into dst (mi355_conv_pack_size bytes) */
void network_layer0_entry(network *net, float s, uint8_t zp, void *dst) { pi_pack(net, s, zp, dst); }

/* bank entries for this batch's (scale, zero point) pairs, the index arrays, all uploaded on the network's stream */
static void pi_bank_update(network *net, const float *scale, const uint8_t *zp)
{
    const int B = net->batch;
    pi_alloc(net);
    const long tick = ++net->pi_tick;
    int32_t *entry = (int32_t *)net->pi_idx_host;
    float *sc = (float *)((char *)net->pi_idx_host + 4 * (size_t)B);
    uint8_t *zq = (uint8_t *)net->pi_idx_host + 8 * (size_t)B;
    net->pi_packed = 0;
    for (int b = 0; b < B; ++b) {
        uint32_t bits;
        memcpy(&bits, &scale[b], 4);
        int k = -1;
        for (int j = 0; j < net->pi_cap && k < 0; ++j)
            if (net->pi_key_zp[j] == zp[b] && net->pi_key_scale[j] == bits) k = j;
        if (k < 0) { /* the least recently used slot this batch does not use */
            for (int j = 0; j < net->pi_cap; ++j)
                if (net->pi_stamp[j] != tick && (k < 0 || net->pi_stamp[j] < net->pi_stamp[k])) k = j;
            char *h = (char *)net->pi_bank_host + (size_t)k * net->pi_entry_bytes;
            pi_pack(net, scale[b], zp[b], h);
            check_mi355(mi355_h2d((char *)net->pi_bank_gpu + (size_t)k * net->pi_entry_bytes, h, net->pi_entry_bytes, net->stream),
                        "upload bank entry");
            net->pi_key_scale[k] = bits;
            net->pi_key_zp[k] = zp[b];
            net->pi_packed++;
        }
        net->pi_stamp[k] = tick;
        entry[b] = k;
        sc[b] = scale[b];
        zq[b] = zp[b];
    }
    check_mi355(mi355_h2d(net->pi_idx_gpu, net->pi_idx_host, 9 * (size_t)B, net->stream), "upload bank index");
}

/* One (scale, zero point) per image from the batch's [B][2] max / min: the first call prepares the network with image 0's pair, then
 * the bank and the index arrays (entry, scale, zero point per image) go up on the network's stream.  Shared by the device input
 * paths (float images, 8-bit frames). */
void input_pairs_per_image(network *net, const float *mm)
{
    const int B = net->batch;
    float *s = malloc(sizeof(float) * (size_t)B);
    uint8_t *zp = malloc((size_t)B);
    for (int b = 0; b < B; ++b) image_scale_zero_point(mm[2 * b + 1] + 0.0f, mm[2 * b], &s[b], &zp[b]);
    if (!net->prepared) quantization_weights_and_activations_fixed_input(net, s[0], zp[0]);
    pi_bank_update(net, s, zp);
    free(s); free(zp);
}

static void quantize_per_image_gpu(network *net, const float *input_gpu)
{
    const int B = net->batch;
    if (!net->pi_mm_gpu || net->pi_cap < B) pi_alloc(net);
    check_mi355(mi355_image_minmax_batched(input_gpu, B, net->inputs, net->pi_mm_gpu, net->stream), "mi355_image_minmax_batched");
    check_mi355(mi355_d2h(net->pi_mm_host, net->pi_mm_gpu, 2 * sizeof(float) * (size_t)B, net->stream), "minmax d2h");
    net_wait(net); /* the batch's one host sync: every earlier upload of the bank is done too */
    input_pairs_per_image(net, net->pi_mm_host);
    const char *idx = (const char *)net->pi_idx_gpu;
    check_mi355(mi355_image_quantize_per_image(input_gpu, B, net->inputs, (const float *)(idx + 4 * (size_t)B),
                                               (const uint8_t *)(idx + 8 * (size_t)B), net->input_uint8_gpu, net->stream),
                "mi355_image_quantize_per_image");
}

/* ---------------------------------------------------------------------------- input quantisation on the device
 * The same chain without the host in it: the min / max stay in HBM, mi355_input_pairs turns them into pairs there, mi355_l0_derive
 * rewrites what depends on the pair in the slots of a bank of the network's own -- one slot per image, each initialised with the
 * prepared layer-0 blob, so the weights and everything else are in place -- and the quantisers and layer 0 read pairs, entries and
 * zero points from device memory as they do per image.  Nothing here waits once the buffers exist. */
int set_input_quantization_on_device(network *net, int on)
{
    if (!on) {
        if (net->input_on_device && net->graph) { mi355_graph_destroy(net->graph); net->graph = NULL; } /* captured with the bank launches */
        net->input_on_device = 0;
        return 0;
    }
    if (l0_bank_refusal(net, "set_input_quantization_on_device")) return MI355_EINVAL;
    if (!net->input_on_device && net->graph) { mi355_graph_destroy(net->graph); net->graph = NULL; }
    net->input_on_device = 1;
    return 0;
}

/* mi355_l0_derive's constant table of this network's layer 0 (mi355_l0_consts + n mi355_l0_channel) into dst; returns its size in
 * bytes (dst == NULL: the size alone).  Host only. */
size_t network_layer0_consts(network *net, void *dst)
{
    const layer *l0 = &l0_source(net)->layers[0];
    const size_t n = (size_t)l0->n, cbytes = sizeof(mi355_l0_consts) + n * sizeof(mi355_l0_channel);
    if (!dst) return cbytes;
    memset(dst, 0, cbytes);
    mi355_l0_consts *c = dst;
    mi355_l0_channel *ch = (mi355_l0_channel *)(c + 1);
    const int K = l0->c * l0->size * l0->size;
    c->n = l0->n; c->K = K;
    c->zp_act = l0->activ_data_uint8_zero_point[0]; c->activation = l0->activation; c->s_act = l0->activ_data_uint8_scales[0];
    for (size_t ii = 0; ii < n; ++ii) {
        int32_t wsum = 0;
        for (int jj = 0; jj < K; ++jj) wsum += l0->weights_uint8[ii * K + jj];
        ch[ii].bias = folded_bias(l0, (int)ii);
        ch[ii].w_scale = l0->weight_data_uint8_scales[ii];
        ch[ii].w_zp = l0->weight_data_uint8_zero_point[ii];
        ch[ii].wsum = wsum;
    }
    return cbytes;
}

static void od_free(network *net)
{
    if (net->od_bank_gpu) mi355_free(net->od_bank_gpu);
    if (net->od_idx_gpu) mi355_free(net->od_idx_gpu);
    if (net->od_kept_gpu) mi355_free(net->od_kept_gpu);
    if (net->od_status_gpu) mi355_free(net->od_status_gpu);
    if (net->od_mm_gpu) mi355_free(net->od_mm_gpu);
    if (net->od_const_gpu) mi355_free(net->od_const_gpu);
    free(net->od_const_host);
    net->od_bank_gpu = net->od_idx_gpu = net->od_kept_gpu = net->od_const_gpu = net->od_const_host = NULL;
    net->od_status_gpu = NULL; net->od_mm_gpu = NULL;
    net->od_cap = 0;
}

/* The buffers of the mode, once per batch size (this may wait; no later call does): the network prepared, the constant table, the bank
 * with the prepared blob in every slot, and in every image's slot of the pair arrays the pair that blob was derived for. */
void od_alloc(network *net)
{
    const int B = net->batch;
    if (!net->prepared) quantization_weights_and_activations_fixed_input(net, 1.0f / 255.0f, 0);
    network *src = l0_source(net);
    const layer *l0 = &src->layers[0];
    const size_t eb = (mi355_conv_pack_size(l0->n, l0->c, l0->size) + 255) & ~(size_t)255;
    if (net->od_bank_gpu && net->od_cap == B && net->pi_entry_bytes == eb) return;
    if (!src->has_host_weights && !src->has_l0_weights) error("input quantisation on the device: no raw layer-0 weights to derive the constants from");
    od_free(net);
    net->pi_entry_bytes = eb;
    net->od_cap = B;
    const size_t cbytes = network_layer0_consts(net, NULL);
    mi355_l0_consts *c = calloc(1, cbytes);
    network_layer0_consts(net, c);
    net->od_const_host = c;
    check_mi355(mi355_alloc(&net->od_const_gpu, cbytes), "alloc layer-0 constants");
    check_mi355(mi355_h2d(net->od_const_gpu, c, cbytes, net->stream), "upload layer-0 constants");
    check_mi355(mi355_alloc(&net->od_bank_gpu, eb * (size_t)B), "alloc layer-0 bank");
    check_mi355(mi355_memset(net->od_bank_gpu, 0, eb * (size_t)B, net->stream), "clear layer-0 bank");
    const layer *mine = &net->layers[0]; /* a replica's blob_gpu is its parent's */
    for (int b = 0; b < B; ++b)
        check_mi355(mi355_d2d((char *)net->od_bank_gpu + (size_t)b * eb, mine->blob_gpu, mine->blob_bytes, net->stream), "fill layer-0 bank");
    check_mi355(mi355_alloc(&net->od_idx_gpu, 9 * (size_t)B), "alloc layer-0 index");
    check_mi355(mi355_alloc(&net->od_kept_gpu, 5 * (size_t)B), "alloc kept pairs");
    check_mi355(mi355_alloc((void **)&net->od_status_gpu, sizeof(uint32_t) * (size_t)B), "alloc input status");
    check_mi355(mi355_alloc((void **)&net->od_mm_gpu, 2 * sizeof(float) * (size_t)B), "alloc minmax");
    char *pairs = calloc(5, (size_t)B);
    for (int b = 0; b < B; ++b) {
        ((float *)pairs)[b] = mine->input_data_uint8_scales[0];
        ((uint8_t *)pairs)[4 * (size_t)B + b] = mine->input_data_uint8_zero_point[0];
    }
    check_mi355(mi355_memset(net->od_idx_gpu, 0, 4 * (size_t)B, net->stream), "clear layer-0 index");
    check_mi355(mi355_h2d((char *)net->od_idx_gpu + 4 * (size_t)B, pairs, 5 * (size_t)B, net->stream), "upload prepared pairs");
    check_mi355(mi355_h2d(net->od_kept_gpu, pairs, 5 * (size_t)B, net->stream), "upload prepared pairs");
    check_mi355(mi355_memset(net->od_status_gpu, 0, sizeof(uint32_t) * (size_t)B, net->stream), "clear input status");
    net_wait(net);
    free(pairs);
}

float *od_scale_dev(const network *net) { return (float *)((char *)net->od_idx_gpu + 4 * (size_t)net->batch); }
uint8_t *od_zp_dev(const network *net) { return (uint8_t *)net->od_idx_gpu + 8 * (size_t)net->batch; }

/* bank entries for the pairs in the pair arrays: image b's, or image 0's for everybody */
static void od_derive(network *net)
{
    const int B = net->batch;
    check_mi355(mi355_l0_derive(net->od_const_gpu, net->od_const_host, net->od_bank_gpu, net->pi_entry_bytes, B, !net->per_image, od_scale_dev(net),
                                od_zp_dev(net), (float *)net->od_kept_gpu, (uint8_t *)net->od_kept_gpu + 4 * (size_t)B, net->od_status_gpu, net->stream),
                "mi355_l0_derive");
}

/* pairs from the batch's [B][2] max / min in HBM (shared-scale mode reads image 0's), then their entries */
void od_pairs_and_entries(network *net, const float *mm_gpu)
{
    check_mi355(mi355_input_pairs(mm_gpu, net->batch, !net->per_image, (int32_t *)net->od_idx_gpu, od_scale_dev(net), od_zp_dev(net),
                                  net->od_status_gpu, net->stream), "mi355_input_pairs");
    od_derive(net);
}

/* the host quantiser's pairs (quantization_weights_and_activations: the floats are on the host) go up instead, layer 0 is derived
 * from them on the device all the same */
static void od_pairs_from_host(network *net, const float *scale, const uint8_t *zp)
{
    const int B = net->batch;
    od_alloc(net);
    char *idx = calloc(9, (size_t)B);
    for (int b = 0; b < B; ++b) {
        ((int32_t *)idx)[b] = net->per_image ? b : 0;
        ((float *)(idx + 4 * (size_t)B))[b] = scale[net->per_image ? b : 0];
        ((uint8_t *)idx)[8 * (size_t)B + b] = zp[net->per_image ? b : 0];
    }
    check_mi355(mi355_h2d(net->od_idx_gpu, idx, 9 * (size_t)B, net->stream), "upload input pairs");
    check_mi355(mi355_memset(net->od_status_gpu, 0, sizeof(uint32_t) * (size_t)B, net->stream), "clear input status");
    od_derive(net);
    net_wait(net); /* idx is freed */
    free(idx);
}

/* float images in HBM: min / max of every image (or of image 0), pairs, entries, quantiser */
static void quantize_on_device(network *net, const float *input_gpu)
{
    const int B = net->batch;
    od_alloc(net);
    check_mi355(mi355_image_minmax_batched(input_gpu, net->per_image ? B : 1, net->inputs, net->od_mm_gpu, net->stream), "mi355_image_minmax_batched");
    od_pairs_and_entries(net, net->od_mm_gpu);
    check_mi355(mi355_image_quantize_per_image(input_gpu, B, net->inputs, od_scale_dev(net), od_zp_dev(net), net->input_uint8_gpu, net->stream),
                "mi355_image_quantize_per_image");
}

int network_input_status(network *net, uint32_t *status)
{
    const int B = net->batch;
    memset(status, 0, sizeof(uint32_t) * (size_t)B);
    if (!net->input_on_device || !net->od_status_gpu) return 0;
    check_mi355(mi355_d2h(status, net->od_status_gpu, sizeof(uint32_t) * (size_t)B, net->stream), "pull input status");
    net_wait(net);
    int bad = 0;
    for (int b = 0; b < B; ++b) bad += status[b] != 0;
    return bad;
}

void network_input_bank_entry(network *net, int b, void *dst)
{
    if (b < 0 || b >= net->batch) error("network_input_bank_entry: image index");
    const char *bank = net->input_on_device ? net->od_bank_gpu : net->pi_bank_gpu;
    if (!bank || (!net->input_on_device && !net->pi_idx_host)) error("network_input_bank_entry: no batch has been quantised through a bank yet");
    int32_t e = net->input_on_device ? (net->per_image ? b : 0) : ((const int32_t *)net->pi_idx_host)[b];
    check_mi355(mi355_d2h(dst, bank + (size_t)e * net->pi_entry_bytes, net->pi_entry_bytes, net->stream), "pull bank entry");
    net_wait(net);
}

void network_letterbox_input_gpu(network *net, int slot, const float *im_gpu, int imw, int imh)
{
    if (slot < 0 || slot >= net->batch || !im_gpu) error("network_letterbox_input_gpu: bad slot / null image");
    check_mi355(mi355_init(net->gpu_index), "mi355_init");
    if (!net->stream && !net->on_default_stream) check_mi355(mi355_stream_acquire(&net->stream), "stream");
    if (!net->input_gpu)
        check_mi355(mi355_alloc((void **)&net->input_gpu, (size_t)net->batch * net->inputs * sizeof(float)), "alloc float input");
    check_mi355(mi355_letterbox_forward(im_gpu, imw, imh, net->c, net->input_gpu + (size_t)slot * net->inputs, net->w, net->h,
                                        net->stream), "mi355_letterbox_forward");
}

void network_quantize_input_gpu(network *net)
{
    if (!net->input_gpu) error("network_quantize_input_gpu before network_letterbox_input_gpu");
    quantization_weights_and_activations_gpu(net, net->input_gpu);
}

static void detb_free(network *net)
{
    if (net->detb_ints_gpu) mi355_free(net->detb_ints_gpu);
    if (net->detb_work_gpu) mi355_free(net->detb_work_gpu);
    if (net->detb_recs_gpu) mi355_free(net->detb_recs_gpu);
    free(net->detb_ints_host);
    net->detb_ints_gpu = net->detb_ints_host = net->detb_work_gpu = NULL;
    net->detb_recs_gpu = NULL;
    net->detb_batch = net->detb_nheads = 0;
    net->detb_work_ints = 0;
    net->detb_recs_cap = 0;
}

void set_batch_network(network *net, int b)
{
    if (b < 1) error("set_batch_network: batch < 1");
    if (b == net->batch && net->prepared) return;
    if (net->replica_of) error("set_batch_network on a replica: re-batch the parent and make new replicas");
    if (net->n_replicas > 0) error("set_batch_network: free this network's replicas first (they borrow its packed weights on the device)");
    net->batch = b;
    pi_free(net); /* the per-image bank and index arrays are sized by the batch */
    od_free(net); /* and the device-derived bank, its pair, status and min / max arrays */
    fr_free(net); /* so are the frame table, its min / max and the staging arena */
    network_set_frame_views(net, NULL); /* views are per slot: a new batch has none */
    detb_free(net); /* and the batched box decode's buffers */
    free(net->input); free(net->input_uint8);
    net->input = calloc((size_t)net->inputs * b, sizeof(float));
    net->input_uint8 = calloc((size_t)net->inputs * b, sizeof(uint8_t));
    for (int i = 0; i < net->n; ++i) net->layers[i].batch = b;
    if (net->input_gpu) { /* batch x inputs floats of the device input path: re-allocated lazily at the new size */
        mi355_free(net->input_gpu);
        net->input_gpu = NULL;
    }
    if (net->prepared) { /* re-size the device buffers, keep the packed weights */
        plan_fusion(net); /* launcher acceptance depends on the batch: flags an earlier EINVAL fallback cleared are re-derived */
        alloc_network_device(net);
        for (int i = 0; i < net->n; ++i)
            if (net->layers[i].type == CONVOLUTIONAL) upload_conv(net, i, net->has_host_weights);
        net_wait(net);
    }
}

/* -------------------------------------------------------------------------------------------------- execution */
void push_network_input_uint8(network *net, const uint8_t *host_nchw)
{
    if (!net->prepared) error("push_network_input_uint8 before quantization_weights_and_activations");
    check_mi355(mi355_h2d(net->input_uint8_gpu, host_nchw, (size_t)net->batch * net->inputs, net->stream), "push input");
}

void network_profile_begin(network *net, int max_steps)
{
    if (net->prof_ev) {
        for (int i = 0; i < net->prof_cap * (net->n + 2); ++i) mi355_event_destroy(net->prof_ev[i]);
        free(net->prof_ev);
        net->prof_ev = NULL;
    }
    net->prof_cap = max_steps;
    net->prof_used = 0;
    net->prof_calls = 0;
    if (net->prof_stride < 1) net->prof_stride = 1;
    if (max_steps <= 0) return;
    net->prof_ev = calloc((size_t)max_steps * (net->n + 2), sizeof(void *));
    for (int i = 0; i < max_steps * (net->n + 2); ++i) check_mi355(mi355_event_create(&net->prof_ev[i]), "event create");
}

void network_profile_set_stride(network *net, int stride) { net->prof_stride = stride < 1 ? 1 : stride; }
void network_profile_set_phase(network *net, int phase) { net->prof_phase = phase < 0 ? 0 : phase; }

int network_profile_read(network *net, float *ms_sum)
{
    for (int i = 0; i < net->n + 1; ++i) ms_sum[i] = 0;
    for (int s = 0; s < net->prof_used; ++s) {
        void **e = net->prof_ev + (size_t)s * (net->n + 2);
        for (int i = 0; i < net->n + 1; ++i) {
            float ms = 0;
            check_mi355(mi355_event_elapsed_ms(e[i], e[i + 1], &ms), "event elapsed");
            ms_sum[i] += ms;
        }
    }
    return net->prof_used;
}

static void run_layers(network *netp)
{
    network net = *netp;
    void **ev = NULL;
    const int ranged = netp->range_hi > netp->range_lo;
    if (ranged) { /* diagnostic knob: validate it instead of reading tensors nobody wrote */
        if (netp->use_graph) error("forward_network_gpu: a layer range cannot be combined with use_graph (the captured graph is the whole net)");
        if (netp->prof_ev && netp->prof_used < netp->prof_cap) error("forward_network_gpu: a layer range cannot be combined with armed per-layer events");
        if (netp->range_lo > 0) {
            const layer *pl = &netp->layers[netp->range_lo - 1];
            /* (a head conv fused with its yolo layer counts as not stored here, unlike in dnq_layer_is_fused) */
            const int stored = !(fusion_on(netp) && pl->fuse_next != FUSE_NONE && !(pl->fuse_next == FUSE_POOL && pl->fuse_pool_keep));
            if (!stored) error("forward_network_gpu: layer range starts behind a conv whose own tensor is not stored (fused with the layer after it)");
        }
    }
    if (netp->prof_ev && netp->prof_used < netp->prof_cap && !netp->use_graph && netp->prof_calls++ % netp->prof_stride == netp->prof_phase % netp->prof_stride)
        ev = netp->prof_ev + (size_t)(netp->prof_used++) * (net.n + 2);
    if (ev) check_mi355(mi355_event_record(ev[0], net.stream), "event");
    /* The first layer reads the reference's [B][3][H][W] planes in place where its kernel can (no conversion pass); else the
     * input goes through the 4-byte-cell tensor.  The conv's forward_gpu falls back itself on MI355_EINVAL and clears the flag. */
    const int direct = netp->layers[0].input_direct && net.accum_mode == MI355_ACC_EXACT && !net.dump_int32;
    const int lo = (netp->range_hi > netp->range_lo) ? netp->range_lo : 0, hi = (netp->range_hi > netp->range_lo) ? netp->range_hi : net.n;
    if (lo < 0 || hi > net.n) error("forward_network_gpu: bad layer range");
    if (!direct && lo == 0) check_mi355(mi355_nchw_to_tensor(netp->input_uint8_gpu, &netp->input_t, net.stream), "input layout");
    if (ev) check_mi355(mi355_event_record(ev[1], net.stream), "event");
    net.cur_t = direct ? &netp->input_nchw_t : &netp->input_t;
    net.cur_f32_gpu = NULL;
    if (lo > 0) net.cur_t = &netp->layers[lo - 1].out_t;
    for (int i = lo; i < hi; ++i) {
        net.index = i;
        layer l = net.layers[i];
        const int asked = fusion_on(&net) ? l.fuse_next : FUSE_NONE;
        l.forward_gpu(l, net);
        if (l.type == CONVOLUTIONAL) netp->layers[i].conv_kernel = mi355_last_conv_kernel();
        if (ev) check_mi355(mi355_event_record(ev[i + 2], net.stream), "event");
        /* plan_fusion marks candidates by shape; the launchers have the last word.  A fused call they refuse
         * (MI355_EINVAL) was re-run unfused by the conv's forward_gpu, which also cleared fuse_next for good: the layer
         * after it then runs on its own like any other.  Taken: that layer's tensor was written by the conv kernel, it is
         * handed on and the layer skipped.  A yolo layer hands on the head conv's uint8 tensor and its own activations. */
        if (asked != FUSE_NONE && netp->layers[i].fuse_next == asked) {
            ++i;
            net.cur_t = &netp->layers[asked == FUSE_YOLO ? i - 1 : i].out_t;
            net.cur_f32_gpu = asked == FUSE_YOLO ? netp->layers[i].output_gpu : NULL;
            if (ev) check_mi355(mi355_event_record(ev[i + 2], net.stream), "event");
            continue;
        }
        if (l.layer_quant_flag && !net.train) { /* ref src/network.c:248-250 */
            net.cur_t = &netp->layers[i].out_t;
            net.cur_f32_gpu = l.output_gpu;
        } else {
            net.cur_f32_gpu = l.output_gpu;
        }
        if (net.verbose) fprintf(stderr, "layer %2d %-8s done\n", i, get_layer_string(l.type));
    }
}

void forward_network_gpu(network *netp)
{
    if (!netp->prepared) error("forward_network_gpu before quantization_weights_and_activations");
    if (netp->accum_mode == MI355_ACC_REF_F32 && !netp->has_host_weights)
        error("-accum ref-f32 reads the raw weights_uint8 of every layer; a network imported from packed blobs does not hold them");
    if (netp->use_graph && netp->on_default_stream) error("use_graph: the default stream cannot be captured; run this executor eagerly");
    if (netp->use_graph) {
        if (!netp->graph) {
            run_layers(netp); /* warm-up outside capture (module load, attribute calls) */
            net_wait(netp);
            check_mi355(mi355_graph_begin(netp->stream), "graph begin");
            run_layers(netp);
            check_mi355(mi355_graph_end(netp->stream, &netp->graph), "graph end");
        }
        check_mi355(mi355_graph_launch(netp->graph, netp->stream), "graph launch");
    } else {
        run_layers(netp);
    }
}

void forward_network(network *net) { forward_network_gpu(net); }

void network_selfcheck(network *net, int passes)
{
    if (passes < 2) passes = 2;
    if (net->selfcheck_gpu) mi355_free(net->selfcheck_gpu);
    check_mi355(mi355_alloc((void **)&net->selfcheck_gpu, (size_t)passes * sizeof(uint64_t)), "alloc selfcheck");
    uint64_t *zeros = calloc((size_t)passes, sizeof(uint64_t));
    check_mi355(mi355_h2d(net->selfcheck_gpu, zeros, (size_t)passes * sizeof(uint64_t), net->stream), "zero selfcheck");
    net_wait(net);
    free(zeros);
    net->selfcheck_passes = passes;
    for (int p = 0; p < passes; ++p) {
        forward_network_gpu(net);
        for (int i = 0; i < net->n; ++i) {
            const layer *l = &net->layers[i];
            if (l->type != YOLO || !l->output_gpu) continue;
            check_mi355(mi355_checksum_u32(l->output_gpu, (long)net->batch * l->outputs, net->selfcheck_gpu + p, net->stream), "checksum");
        }
    }
}

int network_selfcheck_result(network *net)
{
    if (!net->selfcheck_gpu || net->selfcheck_passes < 1) return -1;
    const int passes = net->selfcheck_passes;
    uint64_t *sums = calloc((size_t)passes, sizeof(uint64_t));
    check_mi355(mi355_d2h(sums, net->selfcheck_gpu, (size_t)passes * sizeof(uint64_t), net->stream), "pull selfcheck");
    net_wait(net);
    int bad = 0;
    for (int p = 1; p < passes; ++p) bad += sums[p] != sums[0];
    free(sums);
    mi355_free(net->selfcheck_gpu);
    net->selfcheck_gpu = NULL;
    net->selfcheck_passes = 0;
    return bad;
}

float *network_predict(network *net, float *input)
{
    /* ref src/network.c:570-581; the integer path ignores `input` after the prep quantised it (examples/detector.c
     * :914-921), so does this one: the uint8 image must already be on the device. */
    (void)input;
    net->train = 0;
    forward_network_gpu(net);
    net_wait(net);
    layer *last = &net->layers[net->n - 1];
    if (last->output_gpu) {
        check_mi355(mi355_d2h(last->output, last->output_gpu, (size_t)net->batch * last->outputs * sizeof(float), net->stream), "pull output");
        net_wait(net);
    }
    net->output = last->output;
    return net->output;
}

void pull_layer_output(network *net, int i)
{
    if (i < 0 || i >= net->n) error("pull_layer_output: index");
    layer *l = &net->layers[i];
    const size_t cnt = (size_t)net->batch * l->outputs;
    if (l->type != YOLO) {
        check_mi355(mi355_tensor_to_nchw(&l->out_t, l->output_uint8_nchw_gpu, net->stream), "layout");
        check_mi355(mi355_d2h(l->output_uint8_final, l->output_uint8_nchw_gpu, cnt, net->stream), "pull u8");
    }
    if (l->output_gpu) check_mi355(mi355_d2h(l->output, l->output_gpu, cnt * sizeof(float), net->stream), "pull f32");
    if (l->output_int32_gpu) check_mi355(mi355_d2h(l->output_int32, l->output_int32_gpu, cnt * sizeof(int32_t), net->stream), "pull i32");
    net_wait(net);
}

static int cmp_rec_rank(const void *a, const void *b)
{
    const float x = *(const float *)a, y = *(const float *)b;
    return (x > y) - (x < y);
}

/* anchors, masks and room for max_recs records per image of yolo layer l on the device (kept on the layer) */
static void det_anchors(network *net, layer *l)
{
    if (!l->anchors_gpu) {
        check_mi355(mi355_alloc((void **)&l->anchors_gpu, sizeof(float) * 2 * (size_t)l->total), "alloc anchors");
        check_mi355(mi355_h2d(l->anchors_gpu, l->anchors, sizeof(float) * 2 * (size_t)l->total, net->stream), "anchors");
        check_mi355(mi355_alloc((void **)&l->mask_gpu, sizeof(int) * (size_t)l->n), "alloc mask");
        check_mi355(mi355_h2d(l->mask_gpu, l->mask, sizeof(int) * (size_t)l->n, net->stream), "mask");
    }
}

static void det_buffers(network *net, layer *l, int max_recs)
{
    const int B = net->batch, rl = 6 + l->classes;
    det_anchors(net, l);
    if (l->det_cap < max_recs) {
        if (l->det_recs_gpu) { mi355_free(l->det_recs_gpu); mi355_free(l->det_counts_gpu); }
        check_mi355(mi355_alloc((void **)&l->det_recs_gpu, sizeof(float) * (size_t)B * max_recs * rl), "alloc records");
        check_mi355(mi355_alloc((void **)&l->det_counts_gpu, sizeof(int) * (size_t)B), "alloc counts");
        l->det_cap = max_recs;
    }
}

/* records of every image back to the host, each image's in reference order (ascending rank) */
static void det_pull(network *net, layer *l, float *recs, int max_recs, int *counts)
{
    const int B = net->batch, rl = 6 + l->classes;
    check_mi355(mi355_d2h(counts, l->det_counts_gpu, sizeof(int) * (size_t)B, net->stream), "pull counts");
    net_wait(net);
    for (int b = 0; b < B; ++b) { /* only the records that exist cross PCIe; reference order = ascending rank */
        const int k = counts[b] < max_recs ? counts[b] : max_recs;
        if (!k) continue;
        float *dst = recs + (size_t)b * max_recs * rl;
        check_mi355(mi355_d2h(dst, l->det_recs_gpu + (size_t)b * max_recs * rl, sizeof(float) * (size_t)k * rl, net->stream), "pull records");
        net_wait(net);
        qsort(dst, (size_t)k, sizeof(float) * rl, cmp_rec_rank);
    }
}

void network_yolo_detections_gpu(network *net, int i, int imw, int imh, float thresh, int relative, float *recs,
                                 int max_recs, int *counts)
{
    if (i < 0 || i >= net->n || net->layers[i].type != YOLO) error("network_yolo_detections_gpu: not a yolo layer");
    layer *l = &net->layers[i];
    const int B = net->batch;
    det_buffers(net, l, max_recs);
    check_mi355(mi355_yolo_detections(l->output_gpu, B, l->n, l->classes, l->h, l->w, l->anchors_gpu, l->mask_gpu, net->w,
                                      net->h, imw, imh, thresh, relative, l->det_recs_gpu, max_recs, l->det_counts_gpu,
                                      net->stream), "mi355_yolo_detections");
    det_pull(net, l, recs, max_recs, counts);
}

void network_yolo_detections_gpu_sizes(network *net, int i, const int *imw, const int *imh, float thresh, int relative, float *recs,
                                       int max_recs, int *counts)
{
    if (i < 0 || i >= net->n || net->layers[i].type != YOLO) error("network_yolo_detections_gpu_sizes: not a yolo layer");
    const int B = net->batch;
    for (int b = 0; b < B; ++b)
        if (imw[b] < 1 || imh[b] < 1) error("network_yolo_detections_gpu_sizes: image sizes must be positive");
    layer *l = &net->layers[i];
    det_buffers(net, l, max_recs);
    if (!l->det_sizes_gpu) check_mi355(mi355_alloc((void **)&l->det_sizes_gpu, 2 * sizeof(int) * (size_t)B), "alloc sizes");
    check_mi355(mi355_h2d(l->det_sizes_gpu, imw, sizeof(int) * (size_t)B, net->stream), "sizes");
    check_mi355(mi355_h2d(l->det_sizes_gpu + B, imh, sizeof(int) * (size_t)B, net->stream), "sizes");
    check_mi355(mi355_yolo_detections_sizes(l->output_gpu, B, l->n, l->classes, l->h, l->w, l->anchors_gpu, l->mask_gpu, net->w, net->h,
                                            l->det_sizes_gpu, l->det_sizes_gpu + B, thresh, relative, l->det_recs_gpu, max_recs,
                                            l->det_counts_gpu, net->stream),
                "mi355_yolo_detections_sizes");
    det_pull(net, l, recs, max_recs, counts); /* (its first sync also retires the size uploads from the caller's arrays) */
}

/* ------------------------------------------------------------------------------------ batched box decode
 * Every yolo layer, every image, one call (detect.hip).  The records leave the device in the reference's order, so nothing is sorted
 * here and the number of copies and synchronisations does not depend on the batch. */
static int detb_refuse(const char *why)
{
    fprintf(stderr, "darknet_q: batched detections: %s\n", why);
    return MI355_EINVAL;
}

/* the yolo layers in network order -> idx[], or MI355_EINVAL */
static int detb_heads(network *net, int *idx, int *nheads, int *classes, int *candidates)
{
    int nh = 0, cls = 0;
    long cand = 0;
    for (int i = 0; i < net->n; ++i) {
        const layer *l = &net->layers[i];
        if (l->type != YOLO) continue;
        if (nh == MI355_YOLO_MAX_HEADS) return detb_refuse("more yolo layers than MI355_YOLO_MAX_HEADS");
        if (nh && l->classes != cls) return detb_refuse("the yolo layers differ in `classes`: decode them one by one (network_yolo_detections_gpu)");
        cls = l->classes;
        cand += (long)l->n * l->h * l->w;
        idx[nh++] = i;
    }
    if (!nh) return detb_refuse("the network has no yolo layer");
    if (cand * net->batch >= (1L << 31)) return detb_refuse("batch * candidates per image >= 2^31");
    *nheads = nh; *classes = cls; *candidates = (int)cand;
    return 0;
}

int network_detections_batch_shape(network *net, int *nheads, int *classes, int *candidates)
{
    int idx[MI355_YOLO_MAX_HEADS], nh, cls, cand;
    const int rc = detb_heads(net, idx, &nh, &cls, &cand);
    if (rc) return rc;
    if (nheads) *nheads = nh;
    if (classes) *classes = cls;
    if (candidates) *candidates = cand;
    return 0;
}

int network_detb_run(network *net, const int *imw, const int *imh, float thresh, int relative, int max_per_image, int *counts, int *offsets)
{
    int idx[MI355_YOLO_MAX_HEADS], nh, classes, cand;
    const int rc = detb_heads(net, idx, &nh, &classes, &cand);
    if (rc) return rc;
    const int B = net->batch;
    for (int b = 0; b < B; ++b)
        if (imw[b] < 1 || imh[b] < 1) return detb_refuse("image sizes must be positive");
    if (!net->prepared) error("network_yolo_detections_batch_gpu before quantization_weights_and_activations");
    const int cap = max_per_image <= 0 || max_per_image > cand ? cand : max_per_image; /* records an image can keep */
    mi355_yolo_head heads[MI355_YOLO_MAX_HEADS];
    memset(heads, 0, sizeof(heads));
    for (int k = 0; k < nh; ++k) {
        layer *l = &net->layers[idx[k]];
        det_anchors(net, l);
        heads[k].yolo_out = l->output_gpu; heads[k].anchors = l->anchors_gpu; heads[k].mask = l->mask_gpu;
        heads[k].n = l->n; heads[k].H = l->h; heads[k].W = l->w;
    }
    const size_t nints = 2 * (size_t)B + (size_t)B * nh + B + 1;
    if (net->detb_batch != B || net->detb_nheads != nh) {
        if (net->detb_ints_gpu) mi355_free(net->detb_ints_gpu);
        free(net->detb_ints_host);
        check_mi355(mi355_alloc((void **)&net->detb_ints_gpu, sizeof(int) * nints), "alloc detection counts");
        net->detb_ints_host = calloc(nints, sizeof(int));
        net->detb_batch = B; net->detb_nheads = nh;
    }
    const long work = mi355_yolo_detections_batch_work_ints(heads, nh, B);
    if (!work) { fprintf(stderr, "MI355: %s\n", mi355_last_error()); return detb_refuse("a yolo layer the device decode does not serve"); }
    if (net->detb_work_ints < work) {
        if (net->detb_work_gpu) mi355_free(net->detb_work_gpu);
        check_mi355(mi355_alloc((void **)&net->detb_work_gpu, sizeof(int) * (size_t)work), "alloc detection scratch");
        net->detb_work_ints = work;
    }
    if (net->detb_recs_cap < (size_t)B * cap) {
        if (net->detb_recs_gpu) mi355_free(net->detb_recs_gpu);
        check_mi355(mi355_alloc((void **)&net->detb_recs_gpu, sizeof(float) * (size_t)B * cap * (6 + classes)), "alloc records");
        net->detb_recs_cap = (size_t)B * cap;
    }
    int *hs = net->detb_ints_host, *ds = net->detb_ints_gpu;
    memcpy(hs, imw, sizeof(int) * (size_t)B);
    memcpy(hs + B, imh, sizeof(int) * (size_t)B);
    check_mi355(mi355_h2d(ds, hs, 2 * sizeof(int) * (size_t)B, net->stream), "sizes");
    int *counts_gpu = ds + 2 * B, *offsets_gpu = counts_gpu + (size_t)B * nh;
    check_mi355(mi355_yolo_detections_batch(heads, nh, B, classes, net->w, net->h, ds, ds + B, thresh, relative, cap, net->detb_recs_gpu,
                                            counts_gpu, offsets_gpu, net->detb_work_gpu, net->detb_work_ints, net->stream),
                "mi355_yolo_detections_batch");
    check_mi355(mi355_d2h(hs + 2 * B, counts_gpu, sizeof(int) * ((size_t)B * nh + B + 1), net->stream), "pull counts + offsets");
    net_wait(net);
    memcpy(counts, hs + 2 * B, sizeof(int) * (size_t)B * nh);
    memcpy(offsets, hs + 2 * B + (size_t)B * nh, sizeof(int) * ((size_t)B + 1));
    return offsets[B];
}

void network_detb_pull(network *net, float *recs, int total)
{
    if (total <= 0) return;
    int classes = 0;
    network_detections_batch_shape(net, NULL, &classes, NULL);
    check_mi355(mi355_d2h(recs, net->detb_recs_gpu, sizeof(float) * (size_t)total * (6 + classes), net->stream), "pull records");
    net_wait(net);
}

int network_yolo_detections_batch_gpu(network *net, const int *imw, const int *imh, float thresh, int relative, int max_per_image,
                                      float *recs, int *counts, int *offsets)
{
    const int total = network_detb_run(net, imw, imh, thresh, relative, max_per_image, counts, offsets);
    if (total < 0) return total;
    network_detb_pull(net, recs, total);
    return 0;
}

/* ------------------------------------------------------------------------------------ packed-weight exchange */
/* Layout (little endian, position independent): pack_head | pack_rec[nlayers] | blobs (16-byte aligned, conv layers in
 * order) | layer-0 raw record.  The last part carries what prep_conv_layer needs to RE-DERIVE layer 0 when an image's
 * dynamic input scale / zero point differs from the exporter's (ref: src/blas.c:279 recomputes them per image): biases,
 * batch-norm statistics, weight scales / zero points and the 3-channel layer's few raw weights.  No other layer depends on
 * the input scale, so the other layers travel as packed blobs only (an imported network therefore cannot serve the
 * MI355_ACC_REF_F32 verification mode, which reads raw weights: has_host_weights == 0 refuses it). */
typedef struct { uint32_t magic; int32_t nlayers; float in_scale; int32_t in_zp; uint64_t total; uint64_t l0_bytes; } pack_head;
typedef struct { float s_act, s_in; int32_t zp_act, zp_in; uint64_t blob_bytes; } pack_rec;
typedef struct { int32_t n, c, size, batch_normalize; } pack_l0;
#define PACK_MAGIC 0x35444B4Eu /* "NKD5": the LEAKY byte table in every epilogue table (conv_pool16.hip); NKD4: round 5 added the epilogue table to the blobs of the conv + maxpool shapes (common.h EptHeader); NKD3: permuted A rows (kargs.h ws_row_filter) */

static size_t l0_record_bytes(const layer *l)
{
    size_t sz = sizeof(pack_l0) + (size_t)l->n * sizeof(float) * (l->batch_normalize ? 4 : 1) /* biases (+ scales, mean, var) */
                + (size_t)l->n * sizeof(float) + (size_t)l->n + (size_t)l->nweights;            /* w scales, w zp, weights */
    return (sz + 15) & ~(size_t)15;
}

size_t network_packed_size(network *net) /* a function of the cfg alone: every rank knows it without communication */
{
    size_t sz = sizeof(pack_head) + (size_t)net->n * sizeof(pack_rec);
    sz = (sz + 15) & ~(size_t)15;
    for (int i = 0; i < net->n; ++i) {
        layer *l = &net->layers[i];
        if (l->type != CONVOLUTIONAL) continue;
        const size_t b = mi355_conv_pack_size(l->n, l->c, l->size);
        if (!b) error("network_packed_size: unsupported convolution shape");
        sz += (b + 15) & ~(size_t)15;
    }
    return sz + l0_record_bytes(&net->layers[0]);
}

void network_export_packed(network *net, void *buf)
{
    if (!net->layers[0].blob_host) error("network_export_packed before the host prep");
    char *p = buf;
    const size_t total = network_packed_size(net);
    memset(buf, 0, total);
    layer *l0 = &net->layers[0];
    pack_head h = {PACK_MAGIC, net->n, l0->input_data_uint8_scales[0], l0->input_data_uint8_zero_point[0], total,
                   l0_record_bytes(l0)};
    memcpy(p, &h, sizeof(h)); p += sizeof(h);
    for (int i = 0; i < net->n; ++i) {
        layer *l = &net->layers[i];
        pack_rec r;
        memset(&r, 0, sizeof(r));
        if (l->activ_data_uint8_scales) { r.s_act = l->activ_data_uint8_scales[0]; r.zp_act = l->activ_data_uint8_zero_point[0]; }
        if (l->type == CONVOLUTIONAL) { r.s_in = l->input_data_uint8_scales[0]; r.zp_in = l->input_data_uint8_zero_point[0]; }
        r.blob_bytes = l->blob_bytes;
        memcpy(p, &r, sizeof(r)); p += sizeof(r);
    }
    p = (char *)buf + ((sizeof(pack_head) + (size_t)net->n * sizeof(pack_rec) + 15) & ~(size_t)15);
    for (int i = 0; i < net->n; ++i) {
        layer *l = &net->layers[i];
        if (!l->blob_bytes) continue;
        memcpy(p, l->blob_host, l->blob_bytes);
        p += (l->blob_bytes + 15) & ~(size_t)15;
    }
    pack_l0 r0 = {l0->n, l0->c, l0->size, l0->batch_normalize};
    memcpy(p, &r0, sizeof(r0)); p += sizeof(r0);
    memcpy(p, l0->biases, (size_t)l0->n * sizeof(float)); p += (size_t)l0->n * sizeof(float);
    if (l0->batch_normalize) {
        memcpy(p, l0->scales, (size_t)l0->n * sizeof(float)); p += (size_t)l0->n * sizeof(float);
        memcpy(p, l0->rolling_mean, (size_t)l0->n * sizeof(float)); p += (size_t)l0->n * sizeof(float);
        memcpy(p, l0->rolling_variance, (size_t)l0->n * sizeof(float)); p += (size_t)l0->n * sizeof(float);
    }
    memcpy(p, l0->weight_data_uint8_scales, (size_t)l0->n * sizeof(float)); p += (size_t)l0->n * sizeof(float);
    memcpy(p, l0->weight_data_uint8_zero_point, (size_t)l0->n); p += l0->n;
    memcpy(p, l0->weights_uint8, (size_t)l0->nweights);
}

void network_import_packed_host(network *net, const void *buf, size_t bytes)
{
    const char *p = buf;
    pack_head h;
    if (bytes < sizeof(h)) error("network_import_packed: truncated");
    memcpy(&h, p, sizeof(h)); p += sizeof(h);
    if (h.magic != PACK_MAGIC || h.nlayers != net->n || h.total != bytes) error("network_import_packed: header mismatch (different cfg or format version?)");
    /* the size is a pure function of the cfg: a buffer of any other length (truncated / corrupt file) is refused before
     * anything is read through the offsets below */
    if (bytes != network_packed_size(net)) error("network_import_packed: size does not match this cfg (truncated or corrupt packed data)");
    const pack_rec *recs = (const pack_rec *)p;
    p = (const char *)buf + ((sizeof(pack_head) + (size_t)net->n * sizeof(pack_rec) + 15) & ~(size_t)15);
    for (int i = 0; i < net->n; ++i) {
        layer *l = &net->layers[i];
        pack_rec r;
        memcpy(&r, &recs[i], sizeof(r));
        if (l->activ_data_uint8_scales) { l->activ_data_uint8_scales[0] = r.s_act; l->activ_data_uint8_zero_point[0] = (uint8_t)r.zp_act; }
        if (l->type == CONVOLUTIONAL) {
            l->input_data_uint8_scales[0] = r.s_in; l->input_data_uint8_zero_point[0] = (uint8_t)r.zp_in;
            if (r.blob_bytes != mi355_conv_pack_size(l->n, l->c, l->size)) error("network_import_packed: blob size mismatch");
            free(l->blob_host);
            l->blob_host = malloc(r.blob_bytes);
            l->blob_bytes = r.blob_bytes;
            memcpy(l->blob_host, p, r.blob_bytes);
            p += (r.blob_bytes + 15) & ~(size_t)15;
        }
    }
    layer *l0 = &net->layers[0];
    pack_l0 r0;
    memcpy(&r0, p, sizeof(r0)); p += sizeof(r0);
    if (r0.n != l0->n || r0.c != l0->c || r0.size != l0->size || r0.batch_normalize != l0->batch_normalize ||
        h.l0_bytes != l0_record_bytes(l0)) error("network_import_packed: layer-0 record mismatch");
    memcpy(l0->biases, p, (size_t)l0->n * sizeof(float)); p += (size_t)l0->n * sizeof(float);
    if (l0->batch_normalize) {
        memcpy(l0->scales, p, (size_t)l0->n * sizeof(float)); p += (size_t)l0->n * sizeof(float);
        memcpy(l0->rolling_mean, p, (size_t)l0->n * sizeof(float)); p += (size_t)l0->n * sizeof(float);
        memcpy(l0->rolling_variance, p, (size_t)l0->n * sizeof(float)); p += (size_t)l0->n * sizeof(float);
    }
    memcpy(l0->weight_data_uint8_scales, p, (size_t)l0->n * sizeof(float)); p += (size_t)l0->n * sizeof(float);
    memcpy(l0->weight_data_uint8_zero_point, p, (size_t)l0->n); p += l0->n;
    memcpy(l0->weights_uint8, p, (size_t)l0->nweights);
    prep_shortcut_layers(net);
    net->has_host_weights = 0; /* blobs only (plus layer 0's raw record) */
    net->has_l0_weights = 1;
}

/* On-disk form of the same bytes: what `load_weights` + the host prep + packing produce, written once
 * and read back with one fread -- replaces, for a deployed model, the per-layer reader ref: src/parser.c:1124-1159, the
 * per-channel prep ref: src/blas.c:285-334 and the MFMA-order packing at every start-up. */
void network_save_packed(network *net, char *filename)
{
    const size_t sz = network_packed_size(net);
    void *buf = malloc(sz);
    network_export_packed(net, buf);
    FILE *fp = fopen(filename, "wb");
    if (!fp) file_error(filename);
    if (fwrite(buf, 1, sz, fp) != sz) error("network_save_packed: short write");
    fclose(fp);
    free(buf);
}

static void *read_packed_file(const char *filename, size_t *bytes)
{
    FILE *fp = fopen(filename, "rb");
    if (!fp) file_error(filename);
    fseek(fp, 0, SEEK_END);
    const long sz = ftell(fp);
    fseek(fp, 0, SEEK_SET);
    if (sz < (long)sizeof(pack_head)) error("network_load_packed: file too small");
    void *buf = malloc((size_t)sz);
    if (fread(buf, 1, (size_t)sz, fp) != (size_t)sz) error("network_load_packed: short read");
    fclose(fp);
    *bytes = (size_t)sz;
    return buf;
}

void network_load_packed(network *net, char *filename)
{
    size_t sz = 0;
    void *buf = read_packed_file(filename, &sz);
    network_import_packed(net, buf, sz);
    free(buf);
}

void network_import_packed(network *net, const void *buf, size_t bytes)
{
    if (net->n_replicas > 0 || net->replica_of) error("network_import_packed: not while replicas share this network's packed weights");
    network_import_packed_host(net, buf, bytes);
    plan_fusion(net);
    alloc_network_device(net);
    for (int i = 0; i < net->n; ++i)
        if (net->layers[i].type == CONVOLUTIONAL) upload_conv(net, i, 0);
    net_wait(net);
    net->prepared = 1;
}

void network_import_packed_gpu(network *net, const void *dev_buf, size_t bytes)
{
    check_mi355(mi355_init(net->gpu_index), "mi355_init");
    void *host = malloc(bytes);
    check_mi355(mi355_d2h(host, dev_buf, bytes, NULL), "d2h packed");
    check_mi355(mi355_stream_sync(NULL), "sync");
    network_import_packed(net, host, bytes);
    free(host);
}

/* Multi-GPU start-up behind the C ABI (SURVEY 8(b) `mi355_bcast_weights`, 8(e)): the root rank holds a prepared network
 * (weights file read, per-channel integers derived, blobs packed); every rank calls this with its communicator rank and
 * ends up with the packed state on its device.  One RCCL broadcast of network_packed_size() bytes, in place in HBM. */
void network_bcast_packed(network *net, void *comm, int rank, int root)
{
    check_mi355(mi355_init(net->gpu_index), "mi355_init");
    if (!net->stream && !net->on_default_stream) check_mi355(mi355_stream_acquire(&net->stream), "stream");
    const size_t sz = network_packed_size(net);
    void *dev = NULL;
    check_mi355(mi355_alloc(&dev, sz), "alloc packed");
    void *host = NULL;
    if (rank == root) {
        host = malloc(sz);
        network_export_packed(net, host);
        check_mi355(mi355_h2d(dev, host, sz, net->stream), "upload packed");
    }
    int rc = mi355_bcast_blob(comm, dev, sz, root, net->stream);
    if (rc) { fprintf(stderr, "%s\n", mi355_comm_last_error()); error("mi355_bcast_blob"); }
    net_wait(net);
    free(host);
    if (rank != root) network_import_packed_gpu(net, dev, sz);
    mi355_free(dev);
}

/* A second executor of the same prepared model (darknet_q.h).  The cfg is parsed again (layer geometry, host-side arrays),
 * the per-layer quantisation records and the fusion plan's inputs are copied from the parent, every conv layer borrows the
 * parent's packed blob on the device; activations, input buffers and the stream are the replica's own. */
static void set_plan_internal(network *net, int plan)
{
    /* the executor may still have a pass (or its captured graph) in flight on its stream */
    if (net->prepared && (net->stream || net->on_default_stream)) net_wait(net);
    if (net->graph) { mi355_graph_destroy(net->graph); net->graph = NULL; } /* captured with the other plan's kernels */
    net->plan = plan;
    /* fused calls a launcher refused under the old plan (conv_ws3's fused pools under the throughput plan: flags cleared at run
     * time, layers.c) are candidates again; the tensor views were planned with the flags set, so both forms stay valid */
    if (net->prepared) plan_fusion(net);
}

void network_set_plan(network *net, int plan)
{
    net->plan_user = plan;
    set_plan_internal(net, plan);
}

network *network_replica(network *parent)
{
    if (!parent) error("network_replica: no parent");
    const int ds = parent->replica_default_stream; /* one-shot request of the parent (darknet_q.h) */
    parent->replica_default_stream = 0;
    return network_replica_ex(parent, ds);
}

network *network_replica_ex(network *parent, int default_stream)
{
    if (!parent || !parent->prepared) error("network_replica: the parent network is not prepared");
    if (!parent->cfg_path) error("network_replica: the parent network was not parsed from a cfg file");
    network *net = parse_network_cfg(parent->cfg_path, 0);
    if (net->n != parent->n) error("network_replica: the cfg changed on disk");
    net->gpu_index = parent->gpu_index;
    net->accum_mode = parent->accum_mode; net->store_mode = parent->store_mode;
    net->fuse_maxpool = parent->fuse_maxpool; net->keep_head_float = parent->keep_head_float;
    net->use_graph = parent->use_graph; net->input_direct_off = parent->input_direct_off;
    net->per_image = parent->per_image; /* its own bank (allocated by its first per-image batch); layer 0's raw weights are the parent's */
    net->input_on_device = parent->input_on_device; /* its own bank, pair and status arrays and copy of the constant table */
    net->jpg_entropy_on_device = parent->jpg_entropy_on_device; net->jpg_subseq_bits = parent->jpg_subseq_bits;
    net->png_inflate_on_device = parent->png_inflate_on_device;
    net->dump_int32 = 0;
    if (parent->accum_mode == MI355_ACC_REF_F32) error("network_replica: MI355_ACC_REF_F32 reads raw weights, which a replica does not hold");
    net->replica_of = parent;
    parent->n_replicas++;
    net->on_default_stream = default_stream != 0;
    /* more than one batch in flight from here on: both executors ask the launchers for kernels that share a CU (the parent keeps
     * a plan its caller set explicitly after the first replica: only the first replica switches it) */
    if (parent->n_replicas == 1 && parent->plan != MI355_PLAN_THROUGHPUT) set_plan_internal(parent, MI355_PLAN_THROUGHPUT);
    net->plan = net->plan_user = parent->plan;
    net->batch = parent->batch;
    free(net->input); free(net->input_uint8);
    net->input = calloc((size_t)net->inputs * net->batch, sizeof(float));
    net->input_uint8 = calloc((size_t)net->inputs * net->batch, sizeof(uint8_t));
    for (int i = 0; i < net->n; ++i) {
        layer *l = &net->layers[i];
        const layer *p = &parent->layers[i];
        if (l->type != p->type || l->outputs != p->outputs) error("network_replica: the cfg changed on disk");
        l->batch = net->batch;
        if (l->activ_data_uint8_scales && p->activ_data_uint8_scales) {
            l->activ_data_uint8_scales[0] = p->activ_data_uint8_scales[0];
            l->activ_data_uint8_zero_point[0] = p->activ_data_uint8_zero_point[0];
        }
        if (l->type == CONVOLUTIONAL) {
            l->input_data_uint8_scales[0] = p->input_data_uint8_scales[0];
            l->input_data_uint8_zero_point[0] = p->input_data_uint8_zero_point[0];
            l->blob_gpu = p->blob_gpu;
            l->blob_bytes = p->blob_bytes;
            l->blob_shared = 1;
            l->prepared = 1;
        }
    }
    prep_shortcut_layers(net);
    net->has_host_weights = 0;
    net->has_l0_weights = 0;
    plan_fusion(net);
    alloc_network_device(net);
    net_wait(net);
    net->prepared = 1;
    return net;
}

void free_network(network *net)
{
    if (!net) return;
    if (net->n_replicas > 0) error("free_network: free this network's replicas first (they borrow its packed weights on the device)");
    if (net->replica_of && --net->replica_of->n_replicas == 0) /* the parent is alone on the device again: back to the plan its caller chose
                                                                  (whole-chip kernels by default), fused launches re-planned */
        set_plan_internal(net->replica_of, net->replica_of->plan_user);
    for (int i = 0; i < net->n; ++i) {
        layer *l = &net->layers[i];
        free_layer_device(l);
        free(l->input_data_uint8_scales); free(l->activ_data_uint8_scales); free(l->weight_data_uint8_scales);
        free(l->input_data_uint8_zero_point); free(l->activ_data_uint8_zero_point); free(l->weight_data_uint8_zero_point);
        free(l->weights_sum_int); free(l->mult_zero_point); free(l->M); free(l->M0); free(l->M0_right_shift);
        free(l->M_value); free(l->M0_right_shift_value); free(l->weights_uint8); free(l->biases_int32);
        free(l->biases); free(l->scales); free(l->rolling_mean); free(l->rolling_variance);
        free(l->input_layers); free(l->input_sizes); free(l->mask); free(l->anchors);
        free(l->output); free(l->output_int32); free(l->output_uint8_final); free(l->blob_host);
    }
    network_profile_begin(net, 0);
    if (net->graph) mi355_graph_destroy(net->graph);
    if (net->input_uint8_gpu) mi355_free(net->input_uint8_gpu);
    if (net->input_t.data) mi355_free(net->input_t.data);
    if (net->input_gpu) mi355_free(net->input_gpu);
    if (net->quant_mm_gpu) mi355_free(net->quant_mm_gpu);
    pi_free(net);
    od_free(net);
    fr_free(net);
    network_set_frame_views(net, NULL);
    coded_free(net);
    detb_free(net);
    if (net->selfcheck_gpu) mi355_free(net->selfcheck_gpu);
    if (net->stream) mi355_stream_release(net->stream);
    free(net->layers); free(net->input); free(net->input_uint8); free(net->seen); free(net->cfg_path);
    free(net);
}
