"""Times the output step alone: from yolo tensors that are ready on the device to every image's detection records on the host.

yolov3-tiny @416, batch 64, seeded synthetic weights and images; one forward pass, then the output step over and over on its result:
  per_head    the cheapest use of the per-layer entry point: one network_yolo_detections_gpu_sizes call per yolo layer with room for
              every candidate (atomic slots on the device; per image one copy, one synchronise and one host sort by rank)
  per_slot    what `detector test -list ... -batch B` did: get_network_boxes_batch once per batch slot, each of which decodes the whole
              batch for every yolo layer (+ free_detections)
  batch       network_yolo_detections_batch_gpu: all yolo layers and all images in one call, records in reference order from the device
at thresh 0.5 and 0.25.  The three alternate within a repeat, after a warm-up; a step is timed with the host clock (every path ends
synchronised and hands the records to the host).  Before timing, `batch`'s records are compared with `per_head`'s, bit for bit.
Reported per path: median, min, max, 10th / 90th percentile over the repeats, and the detections per image (they drive the cost).
Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from yolo_quantization_amd import binding, synth  # noqa: E402

CFG = os.path.join(ROOT, "cfg", "yolov3-tiny_quant.cfg")


def stats(ms):
    a = np.asarray(ms)
    return {"median_ms": round(float(np.median(a)), 4), "min_ms": round(float(a.min()), 4), "max_ms": round(float(a.max()), 4),
            "p10_ms": round(float(np.percentile(a, 10)), 4), "p90_ms": round(float(np.percentile(a, 90)), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    a = ap.parse_args()
    binding.init(0)  # raises without a gfx950: nothing is timed on a CPU
    wts = "/tmp/output_path_bench.weights"
    synth.synth_weights(CFG, wts, seed=1234)
    B = a.batch
    x = np.stack([synth.synth_image_u8(3, 416, 416, seed=7 + b) for b in range(B)])
    net = binding.Net(CFG, wts, batch=B)
    net.prepare_fixed(1.0 / 255.0, 0)
    net.push_input(x)
    net.forward()
    net.sync()
    H = net.H
    H.get_network_boxes_batch.restype = C.c_void_p
    H.get_network_boxes_batch.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    H.free_detections.argtypes = [C.c_void_p, C.c_int]
    nh, classes, cand = net.detections_shape()
    heads = [i for i, inf in enumerate(net.info) if inf["type"] == binding.T_YOLO]
    cands = [net.info[i]["outputs"] // (classes + 5) for i in heads]
    imw = np.asarray([640 + 8 * (b % 7) for b in range(B)], np.int32)
    imh = np.asarray([480 - 8 * (b % 5) for b in range(B)], np.int32)
    old_recs = [np.zeros((B, c, 6 + classes), np.float32) for c in cands]
    old_counts = [np.zeros(B, np.int32) for _ in heads]
    recs = np.zeros((B * cand, 6 + classes), np.float32)
    counts, offsets = np.zeros((B, nh), np.int32), np.zeros(B + 1, np.int32)

    def per_head(th):
        for k, i in enumerate(heads):
            H.network_yolo_detections_gpu_sizes(net.h, i, imw.ctypes.data, imh.ctypes.data, C.c_float(th), 1, old_recs[k].ctypes.data,
                                                cands[k], old_counts[k].ctypes.data)

    def per_slot(th):
        n = C.c_int()
        for b in range(B):
            d = H.get_network_boxes_batch(net.h, b, int(imw[b]), int(imh[b]), C.c_float(th), C.c_float(0.5), None, 1, C.byref(n))
            H.free_detections(d, n.value)

    def batch(th):
        rc = H.network_yolo_detections_batch_gpu(net.h, imw.ctypes.data, imh.ctypes.data, C.c_float(th), 1, 0, recs.ctypes.data,
                                                 counts.ctypes.data, offsets.ctypes.data)
        assert rc == 0

    paths = {"per_head": per_head, "per_slot": per_slot, "batch": batch}
    res = {}
    for th in (0.5, 0.25):
        for _ in range(a.warmup):
            for f in paths.values():
                f(th)
        same = all(np.array_equal(np.concatenate([old_recs[k][b, :old_counts[k][b]] for k in range(nh)]).view(np.uint32),
                                  recs[offsets[b]:offsets[b + 1]].view(np.uint32)) for b in range(B))
        same = bool(same and np.array_equal(np.stack(old_counts, axis=1), counts))
        ms = {k: [] for k in paths}
        for _ in range(a.repeats):
            for k, f in paths.items():  # alternating
                net.sync()
                t0 = time.perf_counter()
                f(th)
                ms[k].append((time.perf_counter() - t0) * 1e3)
        per_image = counts.sum(axis=1)
        r = {k: stats(v) for k, v in ms.items()}
        r["batch_identical_to_per_head"] = same
        r["detections_per_image"] = {"min": int(per_image.min()), "median": float(np.median(per_image)), "max": int(per_image.max()),
                                     "total": int(per_image.sum())}
        r["batch_outside_per_head_spread"] = bool(r["batch"]["max_ms"] < r["per_head"]["min_ms"] or r["batch"]["min_ms"] > r["per_head"]["max_ms"])
        r["per_head_over_batch"] = round(r["per_head"]["median_ms"] / r["batch"]["median_ms"], 3)
        r["per_slot_over_batch"] = round(r["per_slot"]["median_ms"] / r["batch"]["median_ms"], 3)
        res[f"thresh_{th}"] = r
    net.close()
    res["config"] = {"cfg": "yolov3-tiny_quant.cfg", "batch": B, "classes": classes, "yolo_layers": nh, "candidates_per_image": cand,
                     "repeats": a.repeats, "warmup": a.warmup,
                     "values": "host clock around one output step, one step per path per repeat, paths alternating; *_over_batch = ratio of medians"}
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
