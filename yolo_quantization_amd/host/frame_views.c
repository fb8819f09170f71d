/*
 * frame_views.c -- the host side of frame views (mi355_frame_view): the network's view table, tiles of a frame, boxes of a view back
 * into its frame, and the detections of a batch of views per frame.  The device side is the view pair of every kind's C-ABI calls,
 * which input_frames.c makes in its common tail while views are set.
 */
#include <stdlib.h>
#include <string.h>
#include "host_internal.h"

void network_set_frame_views(network *net, const mi355_frame_view *views)
{
    free(net->fr_views);
    net->fr_views = NULL;
    if (!views) return;
    net->fr_views = malloc(sizeof(mi355_frame_view) * (size_t)net->batch);
    memcpy(net->fr_views, views, sizeof(mi355_frame_view) * (size_t)net->batch);
}

/* one axis of network_tile_views: the tile's size, or -1 */
static int tile_size(int frame, int count, int overlap)
{
    if (frame < 1 || count < 1 || overlap < 0 || frame > 32768 || count > 32768 || overlap > 32768) return -1;
    const int size = (frame + (count - 1) * overlap + count - 1) / count;
    if (size > frame || overlap >= size) return -1;
    return size;
}

/* where tile i of `size` starts: at i strides, the last one (and any that would pass the edge) on the frame's edge */
static int tile_start(int frame, int size, int overlap, int i)
{
    const int at = i * (size - overlap);
    return at < frame - size ? at : frame - size;
}

int network_tile_views(int frame_w, int frame_h, int cols, int rows, int overlap, int orient, mi355_frame_view *out)
{
    const int tw = tile_size(frame_w, cols, overlap), th = tile_size(frame_h, rows, overlap);
    if (tw < 0 || th < 0 || orient < 1 || orient > 8 || !out) return MI355_EINVAL;
    for (int r = 0; r < rows; ++r)
        for (int c = 0; c < cols; ++c) {
            mi355_frame_view *v = out + (size_t)r * cols + c;
            memset(v, 0, sizeof(*v));
            v->x0 = c == cols - 1 ? frame_w - tw : tile_start(frame_w, tw, overlap, c);
            v->y0 = r == rows - 1 ? frame_h - th : tile_start(frame_h, th, overlap, r);
            v->w = tw; v->h = th; v->orient = orient;
        }
    return cols * rows;
}

void network_view_box_to_frame(const mi355_frame_view *v, int frame_w, int frame_h, box *b)
{
    const int turned = v->orient >= 5;
    const double cw = v->w, ch = v->h, vw = turned ? ch : cw, vh = turned ? cw : ch;
    const double u = (double)b->x * vw, t = (double)b->y * vh, bw = (double)b->w * vw, bh = (double)b->h * vh;
    double cx, cy; /* the centre in the crop */
    switch (v->orient) {
    case 2: cx = cw - u; cy = t; break;
    case 3: cx = cw - u; cy = ch - t; break;
    case 4: cx = u; cy = ch - t; break;
    case 5: cx = t; cy = u; break;
    case 6: cx = t; cy = ch - u; break;
    case 7: cx = cw - t; cy = ch - u; break;
    case 8: cx = cw - t; cy = u; break;
    default: cx = u; cy = t; break;
    }
    b->x = (float)(((double)v->x0 + cx) / (double)frame_w);
    b->y = (float)(((double)v->y0 + cy) / (double)frame_h);
    b->w = (float)((turned ? bh : bw) / (double)frame_w);
    b->h = (float)((turned ? bw : bh) / (double)frame_h);
}

int detections_views_merge(detection **slot_dets, int *slot_num, int B, const mi355_frame_view *views, const int *frame_w,
                           const int *frame_h, const int *frame_of_slot, int classes, float nms, detection **dets, int *num)
{
    if (B < 1) return MI355_EINVAL;
    for (int f = 0; f < B; ++f) { dets[f] = NULL; num[f] = 0; }
    int bad = 0;
    for (int b = 0; b < B; ++b) bad |= frame_of_slot[b] < 0 || frame_of_slot[b] >= B;
    if (bad) {
        free_detections_batch(slot_dets, slot_num, B);
        return MI355_EINVAL;
    }
    for (int b = 0; b < B; ++b) num[frame_of_slot[b]] += slot_num[b];
    for (int f = 0; f < B; ++f) {
        int named = 0;
        for (int b = 0; b < B; ++b) named |= frame_of_slot[b] == f;
        if (!named) continue;
        detection *d = calloc((size_t)num[f] + 1, sizeof(detection));
        int n = 0;
        for (int b = 0; b < B; ++b) {
            if (frame_of_slot[b] != f) continue;
            const mi355_frame_view whole = {0, 0, frame_w[b], frame_h[b], 1, {0, 0, 0}};
            const mi355_frame_view *v = views ? &views[b] : &whole;
            for (int k = 0; k < slot_num[b]; ++k) {
                d[n] = slot_dets[b][k]; /* the entry moves, its prob array with it */
                network_view_box_to_frame(v, frame_w[b], frame_h[b], &d[n].bbox);
                ++n;
            }
            free(slot_dets[b]);
            slot_dets[b] = NULL; slot_num[b] = 0;
        }
        if (nms > 0) do_nms_sort(d, n, classes, nms);
        dets[f] = d;
    }
    return 0;
}

int network_detections_views(network *net, const int *frame_w, const int *frame_h, const int *frame_of_slot, float thresh, float nms,
                             int max_per_image, detection **dets, int *num)
{
    const int B = net->batch;
    int classes = 0;
    if (B < 1) return MI355_EINVAL;
    for (int f = 0; f < B; ++f) { dets[f] = NULL; num[f] = 0; }
    int rc = network_detections_batch_shape(net, NULL, &classes, NULL);
    if (rc) return rc;
    int *vw = calloc((size_t)B, sizeof(int)), *vh = calloc((size_t)B, sizeof(int)), *slot_num = calloc((size_t)B, sizeof(int));
    detection **slot_dets = calloc((size_t)B, sizeof(detection *));
    for (int b = 0; b < B; ++b) { /* the views' oriented sizes */
        const mi355_frame_view *v = net->fr_views ? &net->fr_views[b] : NULL;
        vw[b] = !v ? frame_w[b] : v->orient >= 5 ? v->h : v->w;
        vh[b] = !v ? frame_h[b] : v->orient >= 5 ? v->w : v->h;
    }
    rc = network_detections_batch(net, vw, vh, thresh, 1, 0.f, max_per_image, slot_dets, slot_num);
    if (!rc) rc = detections_views_merge(slot_dets, slot_num, B, net->fr_views, frame_w, frame_h, frame_of_slot, classes, nms, dets, num);
    free(vw); free(vh); free(slot_num); free(slot_dets);
    return rc;
}
