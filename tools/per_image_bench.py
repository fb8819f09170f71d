"""A/B of per-image input quantisation against the shared-scale default.

yolov3-tiny @416, batch 64 (BASELINE config[2] shapes), synthetic weights, float images whose ranges all differ.  Legs, each
alternating shared / per-image, `--repeats` times:
  step1     one batch at a time: quantiser (device min / max, host sync, bank, quantise) + forward + sync, median per step
  inflight  four executors (network_replica), each with its own batch already quantised: forwards dealt round-robin, rate per step
  bank      host time of one per-image quantiser call whose 64 keys are all new (64 entries packed and uploaded) vs all cached
--kernels: only run `--iters` forwards of each mode (for `rocprofv3 --kernel-trace --stats` in a run of its own: layer 0 is
conv_first_mfma_pool_kernel<..., PI=false> vs <..., PI=true>).
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from yolo_quantization_amd import binding, synth  # noqa: E402

CFG = os.path.join(ROOT, "cfg", "yolov3-tiny_quant.cfg")


def images(B, salt):
    rng = np.random.default_rng(1000 + salt)
    x = rng.random((B, 3, 416, 416), dtype=np.float32)
    scale = (np.float32(0.5) + np.float32(0.01) * np.arange(B, dtype=np.float32) + np.float32(1e-4 * salt))[:, None, None, None]
    return np.ascontiguousarray(x * scale - np.float32(0.002) * np.arange(B, dtype=np.float32)[:, None, None, None], np.float32)


def make(wts, B, per_image):
    net = binding.Net(CFG, wts, batch=B)
    if per_image:
        net.set_input_per_image(True)
    return net


def step1(wts, B, buf, per_image, iters):
    net = make(wts, B, per_image)
    q = lambda: net.H.quantization_weights_and_activations_gpu(net.h, buf.ptr)  # noqa: E731
    q(); net.forward(); net.sync()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        q(); net.forward(); net.sync()
        ts.append(time.perf_counter() - t0)
    net.close()
    return float(np.median(ts)) * 1e3


def inflight(wts, B, bufs, per_image, iters):
    parent = make(wts, B, per_image)
    parent.H.quantization_weights_and_activations_gpu(parent.h, bufs[0].ptr)
    ex = [parent] + [parent.replica(default_stream=(k == 3)) for k in range(1, 4)]
    for k, n in enumerate(ex):  # shared scale: every executor has image 0's scale, so all take batch 0; per image: own batches
        n.H.quantization_weights_and_activations_gpu(n.h, bufs[k if per_image else 0].ptr)
        n.sync()
    for n in ex:
        n.forward()
    for n in ex:
        n.sync()
    t0 = time.perf_counter()
    for it in range(iters * 4):
        ex[it % 4].forward()
    for n in ex:
        n.sync()
    dt = (time.perf_counter() - t0) / (iters * 4)
    for r in ex[1:]:
        r.close()
    parent.close()
    return dt * 1e3


def bank(wts, B, iters):
    net = make(wts, B, True)
    buf0 = binding.DevBuf.from_numpy(images(B, 0).ravel())
    net.H.quantization_weights_and_activations_gpu(net.h, buf0.ptr)
    net.sync()
    fresh, cached = [], []
    for it in range(iters):
        b = binding.DevBuf.from_numpy(images(B, 1 + it).ravel())  # 64 keys nobody has seen
        t0 = time.perf_counter()
        net.H.quantization_weights_and_activations_gpu(net.h, b.ptr)
        net.sync()
        fresh.append(time.perf_counter() - t0)
        assert net.bank_packed() == B
        t0 = time.perf_counter()
        net.H.quantization_weights_and_activations_gpu(net.h, b.ptr)  # the same keys again: all cached
        net.sync()
        cached.append(time.perf_counter() - t0)
        assert net.bank_packed() == 0
        b.free()
    buf0.free()
    net.close()
    return float(np.median(fresh)) * 1e3, float(np.median(cached)) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--kernels", action="store_true")
    a = ap.parse_args()
    binding.init(0)
    wts = "/tmp/per_image_bench.weights"
    synth.synth_weights(CFG, wts, seed=5)
    B = a.batch
    bufs = [binding.DevBuf.from_numpy(images(B, 100 + k).ravel()) for k in range(4)]
    if a.kernels:
        for per_image in (False, True):
            net = make(wts, B, per_image)
            net.H.quantization_weights_and_activations_gpu(net.h, bufs[0].ptr)
            for _ in range(a.iters):
                net.forward()
            net.sync()
            net.close()
        print(json.dumps({"kernels": "done", "iters": a.iters, "batch": B}))
        return
    res = {"step1_ms": {"shared": [], "per_image": []}, "inflight4_ms_per_step": {"shared": [], "per_image": []},
           "bank64_host_ms": {"fresh": [], "cached": []}}
    for _ in range(a.repeats):
        for mode in ("shared", "per_image"):
            res["step1_ms"][mode].append(round(step1(wts, B, bufs[0], mode == "per_image", a.iters), 4))
        for mode in ("shared", "per_image"):
            res["inflight4_ms_per_step"][mode].append(round(inflight(wts, B, bufs, mode == "per_image", a.iters), 4))
        f, c = bank(wts, B, 5)
        res["bank64_host_ms"]["fresh"].append(round(f, 4))
        res["bank64_host_ms"]["cached"].append(round(c, 4))
    res["config"] = {"cfg": "yolov3-tiny_quant.cfg", "batch": B, "iters": a.iters, "repeats": a.repeats,
                     "step1": "quantiser + forward + sync, median", "inflight4": "forwards only, four executors, mean per step",
                     "bank64": "one quantiser call + sync, median of 5 (fresh: 64 entries packed and uploaded)"}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
