"""Times the input step alone: from the batch's first upload to the network's uint8 input being ready on the device.

yolov3-tiny @416, batch 64, 640 x 480 RGB frames (synthetic bytes, every frame its own range), two variants:
  float   the float entry points: per frame one upload of the planar float image (byte / 255, converted before the clock starts)
          and one network_letterbox_input_gpu, then network_quantize_input_gpu (min / max, host sync, quantise)
  frames  network_frames_u8_input_gpu: the bytes go up as they are, two launches for the whole batch
each in shared-scale and per-image mode.  A step is timed twice: HIP events on the network's stream around it, and the host clock
from before the first upload to after a stream synchronise.  The variants alternate within a repeat; the same batch is fed every step
(steady state: layer 0 is not re-derived, the per-image bank serves every key from its cache).  Before timing, the two variants' uint8
inputs, scales and zero points are compared for equality.  `host_convert_ms` is the byte -> planar float conversion the float variant
needs before its first upload, done with numpy here: an indication only, not part of either timed step.
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


def make_frames(B, w, h):
    rng = np.random.default_rng(7)
    return [rng.integers(b % 40, 256 - (3 * b) % 90, (h, w, 3), dtype=np.uint8) for b in range(B)]


class Events:
    def __init__(self):
        self.a, self.b = C.c_void_p(), C.c_void_p()
        binding.check(binding.shim().mi355_event_create(C.byref(self.a)), "event")
        binding.check(binding.shim().mi355_event_create(C.byref(self.b)), "event")

    def ms(self):
        out = C.c_float()
        binding.check(binding.shim().mi355_event_elapsed_ms(self.a, self.b, C.byref(out)), "elapsed")
        return out.value


class FloatVariant:
    def __init__(self, net, frames):
        self.net = net
        self.planes = [np.ascontiguousarray(f.transpose(2, 0, 1)).astype(np.float32) / np.float32(255) for f in frames]
        self.bufs = [binding.DevBuf(p.nbytes) for p in self.planes]

    def step(self):
        net, S = self.net, binding.shim()
        for slot, (p, buf) in enumerate(zip(self.planes, self.bufs)):
            binding.check(S.mi355_h2d(buf.ptr, p.ctypes.data, p.nbytes, net.stream()), "h2d")
            net.H.network_letterbox_input_gpu(net.h, slot, buf.ptr, p.shape[2], p.shape[1])
        net.H.network_quantize_input_gpu(net.h)


class FramesVariant:
    def __init__(self, net, frames):
        B = len(frames)
        self.net, self.frames = net, frames
        self.ptrs, self.w, self.h = (C.c_void_p * B)(), (C.c_int * B)(), (C.c_int * B)()
        for b, f in enumerate(frames):
            self.ptrs[b], self.h[b], self.w[b] = f.ctypes.data, f.shape[0], f.shape[1]

    def step(self):
        self.net.H.network_frames_u8_input_gpu(self.net.h, self.ptrs, self.w, self.h, None, 0, 0)


def timed(variant, ev, iters):
    net, S = variant.net, binding.shim()
    dev, wall = [], []
    for _ in range(iters):
        net.sync()
        t0 = time.perf_counter()
        binding.check(S.mi355_event_record(ev.a, net.stream()), "record")
        variant.step()
        binding.check(S.mi355_event_record(ev.b, net.stream()), "record")
        net.sync()
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(ev.ms())
    return float(np.median(dev)), float(np.median(wall))


def pull_input(net):
    net.sync()
    out = np.empty(net.batch * net.inputs, np.uint8)
    binding.check(binding.shim().mi355_d2h(out.ctypes.data, net.input_gpu_ptr(), out.nbytes, None), "d2h")
    binding.check(binding.shim().mi355_stream_sync(None), "sync")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--src", default="640x480")
    a = ap.parse_args()
    binding.init(0)  # raises without a gfx950: nothing is timed on a CPU
    wts = "/tmp/input_path_bench.weights"
    synth.synth_weights(CFG, wts, seed=5)
    sw, sh = (int(v) for v in a.src.split("x"))
    frames = make_frames(a.batch, sw, sh)
    t0 = time.perf_counter()
    for f in frames:
        np.ascontiguousarray(f.transpose(2, 0, 1)).astype(np.float32) / np.float32(255)
    convert_ms = (time.perf_counter() - t0) * 1e3
    ev = Events()
    res = {}
    for mode in ("shared", "per_image"):
        nets = {k: binding.Net(CFG, wts, batch=a.batch) for k in ("float", "frames")}
        if mode == "per_image":
            for n in nets.values():
                n.set_input_per_image(True)
        var = {"float": FloatVariant(nets["float"], frames), "frames": FramesVariant(nets["frames"], frames)}
        for _ in range(a.warmup):
            for v in var.values():
                v.step()
        same = np.array_equal(pull_input(nets["float"]), pull_input(nets["frames"]))
        qa, qb = nets["float"].input_quantization(), nets["frames"].input_quantization()
        same = bool(same and np.array_equal(qa[0].view(np.uint32), qb[0].view(np.uint32)) and np.array_equal(qa[1], qb[1]))
        runs = {k: {"device_ms": [], "wall_ms": []} for k in var}
        for _ in range(a.repeats):
            for k, v in var.items():  # alternating
                d, w = timed(v, ev, a.iters)
                runs[k]["device_ms"].append(round(d, 4))
                runs[k]["wall_ms"].append(round(w, 4))
        med = {k: {m: float(np.median(r[m])) for m in r} for k, r in runs.items()}
        res[mode] = {"identical_input": same, "float": runs["float"], "frames": runs["frames"],
                     "speedup_device": round(med["float"]["device_ms"] / med["frames"]["device_ms"], 3),
                     "speedup_wall": round(med["float"]["wall_ms"] / med["frames"]["wall_ms"], 3)}
        for n in nets.values():
            n.close()
    res["host_convert_ms_numpy"] = round(convert_ms, 3)
    res["config"] = {"cfg": "yolov3-tiny_quant.cfg", "batch": a.batch, "src": a.src, "iters": a.iters, "warmup": a.warmup,
                     "repeats": a.repeats, "values": "median of `iters` steps per repeat; speedup = median over repeats, float / frames"}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
