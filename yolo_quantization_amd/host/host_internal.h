/* host_internal.h -- internal declarations of libdarknet_q */
#ifndef HOST_INTERNAL_H
#define HOST_INTERNAL_H
#include "darknet_q.h"

void check_mi355(int rc, const char *what); /* maps shim error codes to error(), like the reference's check_error */

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
