/* host_internal.h -- internal declarations of libdarknet_q */
#ifndef HOST_INTERNAL_H
#define HOST_INTERNAL_H
#include "darknet_q.h"

void check_mi355(int rc, const char *what); /* maps shim error codes to error(), like the reference's check_error */

/* network.c, for the input paths (input_frames.c, input_coded.c) */
void net_wait(network *net); /* every wait for the network's stream: counted (network_host_waits) */
void image_scale_zero_point(float min_value, float max_value, float *scale, uint8_t *zero_point); /* the layer-0 quantiser's pair from an image's min / max */
void input_pair_shared(network *net, float s, uint8_t zp); /* the whole batch is quantised with this pair: layer 0 follows */
void input_pairs_per_image(network *net, const float *mm); /* [B][2] max, min on the host -> every image's pair and layer-0 bank entry */
void od_alloc(network *net); /* the arrays of the on-device input quantisation, sized by the batch */
void od_pairs_and_entries(network *net, const float *mm_gpu); /* [B][2] max, min on the device -> pairs and bank entries, no wait */
float *od_scale_dev(const network *net); /* where od_pairs_and_entries leaves the [B] scales on the device */
uint8_t *od_zp_dev(const network *net);  /* and the [B] zero points */
/* input_frames.c */
void fr_free(network *net); /* the frame table, its min / max and pair arrays and the staging arena */
size_t fr_round(size_t bytes); /* up to the next multiple of 256 */
/* input_coded.c */
void coded_free(network *net); /* the buffers of the JPEG and PNG input paths */

/* Does this run mode honour the planner's fused forms (layer.fuse_next)?  Parity dumps (fuse_maxpool = 0, dump_int32) and the ref-f32
 * twin run every layer on its own. */
static inline int fusion_on(const network *net) { return net->fuse_maxpool && !net->dump_int32 && net->accum_mode == MI355_ACC_EXACT; }

layer make_convolutional_layer(int batch, int h, int w, int c, int n, int groups, int size, int stride, int padding,
                               ACTIVATION activation, int batch_normalize, int quant_stop_flag,
                               int close_quantization, int layer_quantization, int count);
layer make_maxpool_layer(int batch, int h, int w, int c, int size, int stride, int padding, int layer_quant_flag,
                         int quant_stop_flag, int close_quantization, int count);
layer make_upsample_layer(int batch, int w, int h, int c, int stride, int layer_quant_flag, int quant_stop_flag,
                          int close_quantization, int count);
layer make_route_layer(int batch, int n, int *input_layers, int *input_sizes, int layer_quant_flag,
                       int quant_stop_flag, int close_quantization, int count);
layer make_shortcut_layer(int batch, int index, int w, int h, int c, int w2, int h2, int c2, int layer_quant_flag,
                          int quant_stop_flag, int close_quantization, int count);
layer make_yolo_layer(int batch, int w, int h, int n, int total, int *mask, int classes, int count);

void free_layer_device(layer *l);
/* network_yolo_detections_batch_gpu in its two halves (detect.c sizes its host copy by what was found): launch + counts / offsets back,
 * first sync -> records kept in the batch (or MI355_EINVAL); then the records, second sync */
int network_detb_run(network *net, const int *imw, const int *imh, float thresh, int relative, int max_per_image, int *counts, int *offsets);
void network_detb_pull(network *net, float *recs, int total);
#endif
