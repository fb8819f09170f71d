// detect.hip -- get_yolo_detections + correct_yolo_boxes (ref: src/yolo_layer.c:83-91, 246-277, 316-345) for every yolo layer ("head") of a
// network and every image of the batch in one call, records packed per image in the order of the reference's loops (ref:
// src/network.c:615-638: heads in network order, cells row-major, anchors innermost).
//
// No atomic decides a slot.  A block owns 256 consecutive cells of one head of one image (grid: x = block of cells over all heads,
// y = image); a thread owns one cell, i.e. the n consecutive ranks cell * n .. cell * n + n - 1, and reads the n objectness values of the
// [b][anchor][entry][cell] layout coalesced.  Three launches, whatever the batch and the number of heads:
//   1. det_count_kernel   work[b][blk] = candidates above thresh in the block
//   2. det_scan_kernel    counts[b][head], work[b][blk] -> exclusive offset of the block inside its image, offsets[b] = prefix sum of
//                         min(found, max_per_image) over the images (one workgroup; the table has B * (blocks per image) entries)
//   3. det_write_kernel   recomputes the block's flags; record position = offsets[b] + work[b][blk] + (prefix of the flags in front of
//                         it inside the block: 64-bit ballots + popcount inside a wave, the waves' totals through LDS); records whose
//                         position inside the image is >= max_per_image are dropped, so an image keeps the FIRST max_per_image.
// The decode arithmetic is yolo_detections_sizes_kernel's (glue.hip), expression by expression: float / double promotion follows the
// reference's C, and this file is built with the same -ffp-contract=off.
#include "kargs.h"

// where the block blockIdx.x works: which head, which cells
struct DetWhere { int hd, cell0; };
__device__ __forceinline__ DetWhere det_where(const DetBatchArgs &a, int blk)
{
    int hd = 0;
#pragma unroll
    for (int k = 1; k < MI355_YOLO_MAX_HEADS; ++k)
        if (k < a.nheads && blk >= a.head[k].blk0) hd = k;
    DetWhere wh;
    wh.hd = hd;
    wh.cell0 = (blk - a.head[hd].blk0) * 256;
    return wh;
}

// Flags of this thread's n candidates, folded as they come: `before` = flagged candidates of the wave's lower lanes (their ranks are all
// smaller), `wave_total` = flagged candidates of the whole wave.  Every lane of the wave calls it (lanes past the map pass valid == false).
__device__ __forceinline__ void det_wave_prefix(const float *obj0, size_t anchor_stride, int n, bool valid, float thresh, int &before,
                                                int &wave_total)
{
    const unsigned long long lower = (1ull << (threadIdx.x & 63)) - 1ull;
    before = 0;
    wave_total = 0;
    for (int an = 0; an < n; ++an) {
        const bool f = valid && obj0[an * anchor_stride] > thresh;
        const unsigned long long m = __ballot(f);
        before += __popcll(m & lower);
        wave_total += __popcll(m);
    }
}

__global__ __launch_bounds__(256) void det_count_kernel(const DetBatchArgs a)
{
    __shared__ int wsum[4];
    const int blk = blockIdx.x, b = blockIdx.y;
    const DetWhere wh = det_where(a, blk);
    const DetHead &hd = a.head[wh.hd];
    const int hw = hd.h * hd.w, per = a.classes + 5;
    const int i = wh.cell0 + (int)threadIdx.x;
    const bool valid = i < hw;
    const float *obj0 = hd.out + (size_t)b * hd.n * per * hw + (size_t)4 * hw + (valid ? i : 0);
    int before, wave_total;
    det_wave_prefix(obj0, (size_t)per * hw, hd.n, valid, a.thresh, before, wave_total);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = wave_total;
    __syncthreads();
    if (threadIdx.x == 0) a.work[(size_t)b * a.nblk + blk] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// One workgroup.  Thread t serves the images t, t + 256, ...: a serial walk over the image's blocks (a handful: 4 for yolov3-tiny at 416,
// 31 for YOLOv3 at 608), then a block-wide inclusive scan of the kept counts, 256 images at a time with the running sum carried on.
__global__ __launch_bounds__(256) void det_scan_kernel(const DetBatchArgs a)
{
    __shared__ int sc[256];
    __shared__ int carry;
    if (threadIdx.x == 0) { carry = 0; a.offsets[0] = 0; }
    __syncthreads();
    for (int b0 = 0; b0 < a.B; b0 += 256) {
        const int b = b0 + (int)threadIdx.x;
        int kept = 0;
        if (b < a.B) {
            int *wk = a.work + (size_t)b * a.nblk;
            int run = 0;
            for (int k = 0; k < a.nheads; ++k) {
                const int end = k + 1 < a.nheads ? a.head[k + 1].blk0 : a.nblk;
                int found = 0;
                for (int blk = a.head[k].blk0; blk < end; ++blk) {
                    const int c = wk[blk];
                    wk[blk] = run + found;
                    found += c;
                }
                a.counts[(size_t)b * a.nheads + k] = found;
                run += found;
            }
            kept = run < a.max_per_image ? run : a.max_per_image;
        }
        sc[threadIdx.x] = kept;
        __syncthreads();
        for (int d = 1; d < 256; d <<= 1) {  // Hillis-Steele inclusive scan
            const int v = threadIdx.x >= (unsigned)d ? sc[threadIdx.x - d] : 0;
            __syncthreads();
            sc[threadIdx.x] += v;
            __syncthreads();
        }
        const int base = carry;
        if (b < a.B) a.offsets[b + 1] = base + sc[threadIdx.x];
        __syncthreads();
        if (threadIdx.x == 255) carry = base + sc[255];
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void det_write_kernel(const DetBatchArgs a)
{
    __shared__ int wsum[4];
    const int blk = blockIdx.x, b = blockIdx.y;
    const DetWhere wh = det_where(a, blk);
    const DetHead &hd = a.head[wh.hd];
    const int n = hd.n, h = hd.h, w = hd.w;
    const int hw = h * w, per = a.classes + 5, rl = 6 + a.classes, classes = a.classes;
    const int i = wh.cell0 + (int)threadIdx.x;
    const bool valid = i < hw;
    const float *cell = hd.out + (size_t)b * n * per * hw + (valid ? i : 0);  // entry e of anchor an: cell[(an * per + e) * hw]
    int before, wave_total;
    det_wave_prefix(cell + (size_t)4 * hw, (size_t)per * hw, n, valid, a.thresh, before, wave_total);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = wave_total;
    __syncthreads();
    const int wave = threadIdx.x >> 6;
    int pos = a.work[(size_t)b * a.nblk + blk] + before;  // position inside the image
#pragma unroll
    for (int k = 0; k < 3; ++k)
        if (k < wave) pos += wsum[k];
    if (!valid || pos >= a.max_per_image) return;
    const float thresh = a.thresh;
    const int netw = a.netw, neth = a.neth, relative = a.relative;
    const int imw = a.imw[b], imh = a.imh[b];
    const float *biases = hd.biases;
    const int *mask = hd.mask;
    float *rbase = a.recs + (size_t)a.offsets[b] * rl;
    for (int an = 0; an < n; ++an) {
        const float *p = cell + (size_t)an * per * hw;
        const float objectness = p[4 * hw];
        if (objectness <= thresh) continue;
        if (pos >= a.max_per_image) return;
        int new_w, new_h;
        if (((float)netw / imw) < ((float)neth / imh)) { new_w = netw; new_h = (imh * netw) / imw; }
        else { new_h = neth; new_w = (imw * neth) / imh; }
        const int row = i / w, col = i % w;
        float bx = (col + p[0 * hw]) / w;
        float by = (row + p[1 * hw]) / h;
        float bw = (float)(exp((double)p[2 * hw]) * biases[2 * mask[an]] / netw);
        float bh = (float)(exp((double)p[3 * hw]) * biases[2 * mask[an] + 1] / neth);
        bx = (float)((bx - (netw - new_w) / 2. / netw) / ((float)new_w / netw));
        by = (float)((by - (neth - new_h) / 2. / neth) / ((float)new_h / neth));
        bw *= (float)netw / new_w;
        bh *= (float)neth / new_h;
        if (!relative) { bx *= imw; bw *= imw; by *= imh; bh *= imh; }
        float *r = rbase + (size_t)pos * rl;
        r[0] = (float)(i * n + an);
        r[1] = bx; r[2] = by; r[3] = bw; r[4] = bh;
        r[5] = objectness;
        for (int j = 0; j < classes; ++j) {
            const float prob = objectness * p[(5 + j) * hw];
            r[6 + j] = (prob > thresh) ? prob : 0.f;
        }
        ++pos;
    }
}

int yolo_detections_batch_launch(const DetBatchArgs &a, hipStream_t st)
{
    hipLaunchKernelGGL(det_count_kernel, dim3(a.nblk, a.B), dim3(256), 0, st, a);
    hipLaunchKernelGGL(det_scan_kernel, dim3(1), dim3(256), 0, st, a);
    hipLaunchKernelGGL(det_write_kernel, dim3(a.nblk, a.B), dim3(256), 0, st, a);
    return hipGetLastError() == hipSuccess ? MI355_OK : MI355_EHIP;
}
