#!/usr/bin/env python3
"""Timing of the general-shape convolution (conv_kxk.hip) on the shapes of DESIGN.md's kxk table, through the C-ABI with HIP
events on one stream: warm-up launches, then --iters launches back to back on seeded random operands.  Prints one JSON line
per shape: microseconds per launch, TOP/s (2 n c k^2 OH OW B useful operations), and the share of the larger of the two
bounds (nominal INT8 MFMA peak 5 033 TOP/s; 8 TB/s HBM for the input + output bytes).

  python tools/kxk_bench.py [--iters 200] [--warmup 20] [--only P1,P3]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
from yolo_quantization_amd import binding  # noqa: E402

PEAK_TOPS = 5033.0
HBM_TBS = 8.0
# name: (B, c, n, H, W, k, stride, pad)
SHAPES = {
    "P1": (64, 256, 256, 26, 26, 5, 1, 2),
    "P2": (64, 128, 256, 52, 52, 5, 2, 2),
    "P3": (32, 3, 64, 608, 608, 7, 2, 3),
    "P4": (64, 3, 96, 227, 227, 11, 4, 0),
}


def run(name, iters, warmup):
    B, c, n, H, W, k, s, pad = SHAPES[name]
    S = binding.shim()
    rng = np.random.default_rng(1)
    OH, OW = (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1
    wq = rng.integers(0, 256, (n, c * k * k), dtype=np.uint8)
    zp_w = rng.integers(100, 157, n, dtype=np.uint8)
    bias = np.zeros(n, np.int32)
    mv, sv = np.full(n, 0.75), np.full(n, 2.0 ** -13)
    xt = binding.DevTensor(B, H, W, c, 0)
    # random bytes over the whole buffer (pad cells included: the kernel never reads them)
    raw = rng.integers(0, 256, xt.buf.nbytes, dtype=np.uint8)
    binding.check(S.mi355_h2d(xt.buf.ptr, raw.ctypes.data, raw.nbytes, None), "h2d")
    y = binding.DevTensor(B, OH, OW, n, 23)
    blob = binding.DevBuf.from_numpy(binding.conv_pack(wq, zp_w, c, k, bias, mv, sv, binding.ACT["leaky"], 23))
    d = binding.ConvDesc(n, c, k, s, pad, binding.ACT["leaky"], binding.STORE_WRAP, binding.ACC_EXACT, 0, 23, 0.05)
    d.epilogue_packed = 1
    st = C.c_void_p()
    binding.check(S.mi355_stream_create(C.byref(st)), "stream")

    def launch():
        binding.check(S.mi355_conv_forward(C.byref(d), xt.ref(), blob.ptr, None, None, y.ref(), None, None, st), "conv_forward")

    for _ in range(warmup):
        launch()
    assert S.mi355_last_conv_kernel() == 9
    e0, e1 = C.c_void_p(), C.c_void_p()
    binding.check(S.mi355_event_create(C.byref(e0)), "event")
    binding.check(S.mi355_event_create(C.byref(e1)), "event")
    binding.check(S.mi355_event_record(e0, st), "record")
    for _ in range(iters):
        launch()
    binding.check(S.mi355_event_record(e1, st), "record")
    ms = C.c_float()
    binding.check(S.mi355_event_elapsed_ms(e0, e1, C.byref(ms)), "elapsed")
    S.mi355_event_destroy(e0); S.mi355_event_destroy(e1)
    binding.check(S.mi355_stream_sync(st), "sync")
    S.mi355_stream_destroy(st)
    us = ms.value * 1e3 / iters
    ops = 2.0 * n * c * k * k * OH * OW * B
    io_bytes = B * H * W * xt.t.cs + B * OH * OW * y.t.cs  # the tensors' cells (channel padding included)
    t_mfma, t_hbm = ops / (PEAK_TOPS * 1e12) * 1e6, io_bytes / (HBM_TBS * 1e12) * 1e6
    bound = "MFMA" if t_mfma >= t_hbm else "HBM"
    return {"shape": name, "B": B, "c": c, "n": n, "H": H, "W": W, "k": k, "stride": s, "pad": pad, "OH": OH, "OW": OW,
            "iters": iters, "us": round(us, 2), "tops": round(ops / us / 1e6, 1), "gop": round(ops / 1e9, 2),
            "io_mb": round(io_bytes / 1e6, 1), "bound": bound, "bound_us": round(max(t_mfma, t_hbm), 2),
            "share_of_bound": round(max(t_mfma, t_hbm) / us, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--only", default="")
    args = ap.parse_args()
    binding.init(0)
    names = [s for s in args.only.split(",") if s] or list(SHAPES)
    for name in names:
        print(json.dumps(run(name, args.iters, args.warmup)), flush=True)


if __name__ == "__main__":
    main()
