#!/usr/bin/env python3
"""One-kernel microbench of the MFMA implicit-GEMM conv through the C-ABI (BASELINE config[1] by default:
3x3 s1 conv 256->256, 52x52, batch 32).  Prints achieved TOP/s from HIP events on the launch stream.

  python tools/conv_microbench.py [--c 256 --n 256 --hw 52 --batch 32 --k 3] [--iters 20] [--tile BM BN] [--mode flat|patch]
  python tools/conv_microbench.py --net       # every conv shape of yolov3-tiny at batch 64
  python tools/conv_microbench.py --dw [--out FILE]   # depthwise 3x3 (conv_dw.hip) against its dense twin and the HBM floor
  python tools/conv_microbench.py --spp [--out FILE]  # the fused SPP pools (spp.hip) against the three plain pools and the HBM floor
  python tools/conv_microbench.py --tr [--out FILE]   # transposed k4 s2 / k2 s2 (conv_tr.hip) against its stuffed dense twin and the HBM floor
  python tools/conv_microbench.py --group [--out FILE]  # grouped 3x3 (conv_group.hip) against its dense twin and the HBM floor
  python tools/conv_microbench.py --dil [--out FILE]  # dilated 3x3 (conv_dil.hip) against the same layer at d = 1, its stuffed twin and the HBM floor
  python tools/conv_microbench.py --fc [--out FILE]   # connected / avgpool (classify.hip) against the layer spelled as a convolution and the HBM floor
  python tools/conv_microbench.py --sep [--out FILE]  # the fused depthwise-separable launch (conv_sep.hip) against conv_dw + the 1x1 layer and the HBM floor
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

PEAK = 256 * 4 * 2048 * 2.4e9 / 1e12
SHIFT = 13  # requantised values of random data then stay in the few-hundred range, like a real net's

NET = [(16, 32, 208, 3), (32, 64, 104, 3), (64, 128, 52, 3), (128, 256, 26, 3), (256, 512, 13, 3), (512, 1024, 13, 3),
       (1024, 256, 13, 1), (512, 30, 13, 1), (256, 128, 13, 1), (384, 256, 26, 3), (256, 30, 26, 1)]


def run(c, n, hw, k, batch, iters, tile=None, mode=None, check=False, nt=0):
    S = binding.shim()
    rng = np.random.default_rng(1)
    x = rng.integers(0, 256, (batch, c, hw, hw), dtype=np.uint8)
    wq = np.random.default_rng(2).integers(0, 256, (n, c * k * k), dtype=np.uint8)
    if os.environ.get("UBENCH_DATA") == "const":   # constant operands: the matrix pipe toggles little -> is the kernel power / clock bound?
        x[:] = 128; wq[:] = 128
    elif os.environ.get("UBENCH_DATA") == "small":  # low-entropy operands
        x = (x & 3).astype(np.uint8) + 126; wq = (wq & 3).astype(np.uint8) + 126
    zp_w = np.random.default_rng(3).integers(100, 157, n, dtype=np.uint8)
    bias = np.zeros(n, np.int32)
    mv = np.full(n, 0.75); sv = np.full(n, 2.0 ** -SHIFT)
    xt = binding.DevTensor.from_nchw(x, 0)
    y = binding.DevTensor(batch, hw, hw, n, 23)
    blob = binding.DevBuf.from_numpy(binding.conv_pack(wq, zp_w, c, k, bias, mv, sv))
    d = binding.ConvDesc(n, c, k, 1, k // 2, binding.ACT["leaky"], 0, 0, 0, 23, 1.0)
    if tile or mode:
        bm, bn = tile if tile else (0, 0)
        bm |= nt << 16
        flag = (1 << 30) if mode == "patch" else ((1 << 29) if mode == "flat" else 0)
        S.mi355_conv_set_tile(bm, bn | flag)
    st = C.c_void_p(); binding.check(S.mi355_stream_create(C.byref(st)))
    e0 = C.c_void_p(); e1 = C.c_void_p()
    S.mi355_event_create(C.byref(e0)); S.mi355_event_create(C.byref(e1))

    def launch():
        binding.check(S.mi355_conv_forward(C.byref(d), xt.ref(), blob.ptr, None, None, y.ref(), None, None, st), "conv")
    for _ in range(3):
        launch()
    S.mi355_stream_sync(st)
    S.mi355_event_record(e0, st)
    for _ in range(iters):
        launch()
    S.mi355_event_record(e1, st)
    ms = C.c_float()
    binding.check(S.mi355_event_elapsed_ms(e0, e1, C.byref(ms)), "elapsed")
    S.mi355_conv_set_tile(0, 0)
    t = ms.value / iters * 1e-3
    ops = 2.0 * n * c * k * k * hw * hw * batch
    byt = x.size + wq.size + n * hw * hw * batch
    return {"c": c, "n": n, "hw": hw, "k": k, "batch": batch, "us": round(t * 1e6, 2), "tops": round(ops / t / 1e12, 1),
            "frac_mfma_peak": round(ops / t / 1e12 / PEAK, 4), "gbs": round(byt / t / 1e9, 1), "tile": tile, "mode": mode, "nt": nt}


def _time_us(launch, st, iters):
    """device events around `iters` launches on stream st, after a warm-up"""
    S = binding.shim()
    e0 = C.c_void_p(); e1 = C.c_void_p()
    S.mi355_event_create(C.byref(e0)); S.mi355_event_create(C.byref(e1))
    for _ in range(3):
        launch()
    S.mi355_stream_sync(st)
    S.mi355_event_record(e0, st)
    for _ in range(iters):
        launch()
    S.mi355_event_record(e1, st)
    ms = C.c_float()
    binding.check(S.mi355_event_elapsed_ms(e0, e1, C.byref(ms)), "elapsed")
    S.mi355_event_destroy(e0); S.mi355_event_destroy(e1)
    return ms.value / iters * 1e3


def run_dw(iters, repeats):
    """The depthwise kernel on 3x3 stride 1 | 2, 64 x 208 x 208 and 256 x 52 x 52 at batch 32, each against two baselines: its dense
    twin (off-diagonal weights = the filter's zero point: the same bytes out) on the dense kernels, and the HBM floor, tensor bytes in
    + out over the bandwidth a device-to-device copy of 256 MiB reaches in this process.  The two kernels alternate, `repeats` rounds;
    medians and ranges in microseconds."""
    S = binding.shim()
    st = C.c_void_p(); binding.check(S.mi355_stream_create(C.byref(st)))
    nb = 256 << 20
    src, dst = binding.DevBuf(nb), binding.DevBuf(nb)
    copy_us = [_time_us(lambda: binding.check(S.mi355_d2d(dst.ptr, src.ptr, nb, st), "d2d"), st, 10) for _ in range(repeats)]
    bw = 2.0 * nb / (np.median(copy_us) * 1e-6)  # bytes read + written per second
    src.free(); dst.free()
    out = {"copy_256MiB_us": copy_us, "copy_bytes_per_s": bw, "iters": iters, "cases": []}
    for c, hw in ((64, 208), (256, 52)):
        for stride in (1, 2):
            rng = np.random.default_rng(c + stride)
            B, k = 32, 3
            x = rng.integers(0, 256, (B, c, hw, hw), dtype=np.uint8)
            wq = rng.integers(0, 256, (c, k * k), dtype=np.uint8)
            zp_w = rng.integers(100, 157, c, dtype=np.uint8)
            bias = np.zeros(c, np.int32); mv = np.full(c, 0.75); sv = np.full(c, 2.0 ** -7)
            wd = np.repeat(zp_w[:, None], c * k * k, axis=1).reshape(c, c, k * k)
            wd[np.arange(c), np.arange(c)] = wq
            ohw = (hw + 2 - k) // stride + 1
            xt = binding.DevTensor.from_nchw(x, 0)
            y, yd = binding.DevTensor(B, ohw, ohw, c, 23), binding.DevTensor(B, ohw, ohw, c, 23)
            blob = binding.DevBuf.from_numpy(binding.conv_dw_pack(wq, zp_w, k, bias, mv, sv))
            blobd = binding.DevBuf.from_numpy(binding.conv_pack(wd.reshape(c, -1), zp_w, c, k, bias, mv, sv))
            d = binding.ConvDesc(c, c, k, stride, 1, binding.ACT["leaky"], 0, 0, 0, 23, 1.0)
            dw = lambda: binding.check(S.mi355_conv_dw_forward(C.byref(d), xt.ref(), blob.ptr, y.ref(), None, None, st), "dw")
            dense = lambda: binding.check(S.mi355_conv_forward(C.byref(d), xt.ref(), blobd.ptr, None, None, yd.ref(), None, None, st), "dense")
            t_dw, t_dense = [], []
            for _ in range(repeats):
                t_dw.append(_time_us(dw, st, iters)); t_dense.append(_time_us(dense, st, iters))
            S.mi355_stream_sync(st)
            same = bool(np.array_equal(y.to_nchw(), yd.to_nchw()))
            floor_us = (B * c * (hw * hw + ohw * ohw)) / bw * 1e6
            out["cases"].append({"c": c, "hw": hw, "stride": stride, "batch": B, "dw_us": t_dw, "dense_twin_us": t_dense,
                                 "dense_kernel": binding.last_conv_kernel(), "bytes_equal": same, "hbm_floor_us": floor_us,
                                 "dw_over_dense": float(np.median(t_dw) / np.median(t_dense)),
                                 "dw_over_floor": float(np.median(t_dw) / floor_us)})
    return out


def run_sep(iters, repeats):
    """The fused depthwise-separable launch (conv_sep.hip) against the two-launch pair, conv_dw + the 1x1 layer, on the same buffers:
    five MobileNet-style shapes at batch 32, 3x3 depthwise.  The two alternate, `repeats` rounds; medians and ranges in microseconds,
    the HBM floor of input + output bytes, and equal output bytes checked in the run."""
    S = binding.shim()
    st = C.c_void_p(); binding.check(S.mi355_stream_create(C.byref(st)))
    nb = 256 << 20
    src, dst = binding.DevBuf(nb), binding.DevBuf(nb)
    copy_us = [_time_us(lambda: binding.check(S.mi355_d2d(dst.ptr, src.ptr, nb, st), "d2d"), st, 10) for _ in range(repeats)]
    bw = 2.0 * nb / (np.median(copy_us) * 1e-6)
    src.free(); dst.free()
    out = {"copy_256MiB_us": copy_us, "copy_bytes_per_s": bw, "iters": iters, "cases": []}
    for c, hw, stride, n in ((64, 208, 1, 128), (128, 104, 2, 256), (256, 52, 1, 256), (512, 26, 1, 512), (960, 13, 1, 320)):
        rng = np.random.default_rng(c + n)
        B, k = 32, 3
        x = rng.integers(0, 256, (B, c, hw, hw), dtype=np.uint8)
        wd = rng.integers(0, 256, (c, k * k), dtype=np.uint8)
        wp = rng.integers(0, 256, (n, c), dtype=np.uint8)
        zd, zp = rng.integers(100, 157, c, dtype=np.uint8), rng.integers(100, 157, n, dtype=np.uint8)
        ohw = (hw + 2 - k) // stride + 1
        xt = binding.DevTensor.from_nchw(x, 0)
        mid = binding.DevTensor(B, ohw, ohw, c, 23)
        y, yf = binding.DevTensor(B, ohw, ohw, n, 23), binding.DevTensor(B, ohw, ohw, n, 23)
        bd = binding.DevBuf.from_numpy(binding.conv_dw_pack(wd, zd, k, np.zeros(c, np.int32), np.full(c, 0.75), np.full(c, 2.0 ** -7)))
        bp = binding.DevBuf.from_numpy(binding.conv_pack(wp, zp, c, 1, np.zeros(n, np.int32), np.full(n, 0.75), np.full(n, 2.0 ** -SHIFT)))
        dd = binding.ConvDesc(c, c, k, stride, 1, binding.ACT["leaky"], 0, 0, 0, 23, 1.0)
        dp = binding.ConvDesc(n, c, 1, 1, 0, binding.ACT["leaky"], 0, 0, 23, 23, 1.0)

        def pair():
            binding.check(S.mi355_conv_dw_forward(C.byref(dd), xt.ref(), bd.ptr, mid.ref(), None, None, st), "dw")
            binding.check(S.mi355_conv_forward(C.byref(dp), mid.ref(), bp.ptr, None, None, y.ref(), None, None, st), "pw")

        def fused():
            binding.check(S.mi355_conv_sep_forward(C.byref(dd), C.byref(dp), xt.ref(), bd.ptr, bp.ptr, yf.ref(), None, None, st), "sep")
        t_f, t_p = [], []
        for _ in range(repeats):
            t_f.append(_time_us(fused, st, iters)); t_p.append(_time_us(pair, st, iters))
        pair()
        pw_kernel = binding.last_conv_kernel()
        fused()
        launch = binding.last_conv_launch()
        S.mi355_stream_sync(st)
        same = bool(np.array_equal(y.to_nchw(), yf.to_nchw()))
        floor_us = B * (c * hw * hw + n * ohw * ohw) / bw * 1e6
        out["cases"].append({"c": c, "hw": hw, "stride": stride, "n": n, "batch": B, "fused_us": t_f, "pair_us": t_p, "pw_kernel": pw_kernel,
                             "fused_launch": launch, "bytes_equal": same, "hbm_floor_us": floor_us,
                             "fused_over_pair": float(np.median(t_f) / np.median(t_p)), "fused_over_floor": float(np.median(t_f) / floor_us)})
    return out


def run_spp(iters, repeats):
    """mi355_spp_forward (5, 9, 13) on 512 x 13 x 13 and 512 x 19 x 19 at batch 32 and 64 against the three mi355_maxpool_forward launches
    it replaces, both writing into the windows of one concat buffer (p13, p9, p5, x), and against the HBM floor: x in plus three outputs
    out over the bandwidth a device-to-device copy of 256 MiB reaches in this process.  The two alternate, `repeats` rounds; medians and
    ranges in microseconds.  The bytes of the two are compared in the run."""
    S = binding.shim()
    st = C.c_void_p(); binding.check(S.mi355_stream_create(C.byref(st)))
    nb = 256 << 20
    src, dst = binding.DevBuf(nb), binding.DevBuf(nb)
    copy_us = [_time_us(lambda: binding.check(S.mi355_d2d(dst.ptr, src.ptr, nb, st), "d2d"), st, 10) for _ in range(repeats)]
    bw = 2.0 * nb / (np.median(copy_us) * 1e-6)  # bytes read + written per second
    src.free(); dst.free()
    out = {"copy_256MiB_us": copy_us, "copy_bytes_per_s": bw, "iters": iters, "sizes": [5, 9, 13], "cases": []}
    sizes, c = (5, 9, 13), 512
    for hw in (13, 19):
        for B in (32, 64):
            rng = np.random.default_rng(hw + B)
            full = np.zeros((B, 4 * c, hw, hw), np.uint8)
            full[:, 3 * c:] = rng.integers(0, 256, (B, c, hw, hw), dtype=np.uint8)
            cats = []
            for _ in range(2):  # one concat buffer for the fused launch, one for the plain ones: the same x in both
                cat = binding.DevTensor.from_nchw(full, 0)
                win = []
                for k in range(4):
                    t = binding.Tensor.from_buffer_copy(cat.t)
                    t.data, t.C = cat.buf.ptr.value + k * c, c
                    win.append(t)
                cats.append((cat, win[3], win[2::-1]))  # x is the last window, the pools in front of it, largest first
            (fcat, fx, fys), (pcat, px, pys) = cats
            fused = lambda: binding.check(binding.spp_forward(fx, sizes, fys, st), "spp")

            def plain():
                for k, y in zip(sizes, pys):
                    binding.check(S.mi355_maxpool_forward(px, y, k, 1, k - 1, st), "maxpool")
            t_f, t_p = [], []
            for _ in range(repeats):
                t_f.append(_time_us(fused, st, iters)); t_p.append(_time_us(plain, st, iters))
            S.mi355_stream_sync(st)
            same = bool(np.array_equal(fcat.to_nchw(), pcat.to_nchw()))
            floor_us = 4.0 * B * c * hw * hw / bw * 1e6
            out["cases"].append({"c": c, "hw": hw, "batch": B, "spp_us": t_f, "three_maxpools_us": t_p, "bytes_equal": same,
                                 "hbm_floor_us": floor_us, "spp_over_plain": float(np.median(t_f) / np.median(t_p)),
                                 "spp_over_floor": float(np.median(t_f) / floor_us)})
    return out


def run_tr(iters, repeats):
    """The transposed kernel (conv_tr.hip) on k4 s2 p1 and k2 s2 p0, 256 x 26 x 26 -> 128 and 128 x 52 x 52 -> 64 at batch 32, each
    against two baselines: its stuffed dense twin (the zero-point-stuffed map, built before the clock, through the dense
    kernels with the flipped weights: the same bytes out) and the HBM floor, tensor bytes in + out over the bandwidth a device-to-device
    copy of 256 MiB reaches in this process.  The two kernels alternate, `repeats` rounds; medians and ranges in microseconds."""
    S = binding.shim()
    st = C.c_void_p(); binding.check(S.mi355_stream_create(C.byref(st)))
    nb = 256 << 20
    src, dst = binding.DevBuf(nb), binding.DevBuf(nb)
    copy_us = [_time_us(lambda: binding.check(S.mi355_d2d(dst.ptr, src.ptr, nb, st), "d2d"), st, 10) for _ in range(repeats)]
    bw = 2.0 * nb / (np.median(copy_us) * 1e-6)  # bytes read + written per second
    src.free(); dst.free()
    out = {"copy_256MiB_us": copy_us, "copy_bytes_per_s": bw, "iters": iters, "cases": []}
    for c, hw, n in ((256, 26, 128), (128, 52, 64)):
        for k, s, p in ((4, 2, 1), (2, 2, 0)):
            rng = np.random.default_rng(c + k)
            B, zp_in = 32, 5
            x = rng.integers(0, 256, (B, c, hw, hw), dtype=np.uint8)
            w = rng.integers(0, 256, (c, n, k, k), dtype=np.uint8)
            zp_w = rng.integers(100, 157, n, dtype=np.uint8)
            bias = np.zeros(n, np.int32); mv = np.full(n, 0.75); sv = np.full(n, 2.0 ** -12)
            ohw, shw = (hw - 1) * s + k - 2 * p, (hw - 1) * s + 1
            xh = np.full((B, c, shw, shw), zp_in, np.uint8)
            xh[:, :, ::s, ::s] = x
            wh = np.ascontiguousarray(w.transpose(1, 0, 2, 3)[:, :, ::-1, ::-1]).reshape(n, -1)
            xt, xht = binding.DevTensor.from_nchw(x, zp_in), binding.DevTensor.from_nchw(xh, zp_in)
            y, yd = binding.DevTensor(B, ohw, ohw, n, 23), binding.DevTensor(B, ohw, ohw, n, 23)
            blob = binding.DevBuf.from_numpy(binding.conv_tr_pack(w, zp_w, k, s, bias, mv, sv))
            blobd = binding.DevBuf.from_numpy(binding.conv_pack(wh, zp_w, c, k, bias, mv, sv))
            d = binding.ConvDesc(n, c, k, s, p, binding.ACT["leaky"], 0, 0, zp_in, 23, 1.0)
            dd = binding.ConvDesc(n, c, k, 1, k - 1 - p, binding.ACT["leaky"], 0, 0, zp_in, 23, 1.0)
            tr = lambda: binding.check(S.mi355_conv_tr_forward(C.byref(d), xt.ref(), blob.ptr, y.ref(), None, None, st), "tr")
            dense = lambda: binding.check(S.mi355_conv_forward(C.byref(dd), xht.ref(), blobd.ptr, None, None, yd.ref(), None, None, st), "dense")
            t_tr, t_dense = [], []
            for _ in range(repeats):
                t_tr.append(_time_us(tr, st, iters)); t_dense.append(_time_us(dense, st, iters))
            S.mi355_stream_sync(st)
            same = bool(np.array_equal(y.to_nchw(), yd.to_nchw()))
            floor_us = (B * (c * hw * hw + n * ohw * ohw)) / bw * 1e6
            out["cases"].append({"c": c, "hw": hw, "n": n, "k": k, "stride": s, "pad": p, "batch": B, "tr_us": t_tr, "dense_twin_us": t_dense,
                                 "dense_kernel": binding.last_conv_kernel(), "bytes_equal": same, "hbm_floor_us": floor_us,
                                 "tr_over_dense": float(np.median(t_tr) / np.median(t_dense)),
                                 "tr_over_floor": float(np.median(t_tr) / floor_us)})
    return out


def run_group(iters, repeats):
    """The grouped kernel (conv_group.hip) on 3x3 layers of cardinality 32 -- 128 x 52 x 52, 256 x 26 x 26 at stride 1 and 2,
    512 x 13 x 13 -- and on 256 x 26 x 26 with two groups, n = c, batch 32, each against two baselines: its dense twin (DESIGN.md 7e:
    weights outside a filter's group = the filter's zero point: the same bytes out) on the dense kernels, and the HBM floor, tensor
    bytes in + out over the bandwidth a device-to-device copy of 256 MiB reaches in this process.  The two kernels alternate,
    `repeats` rounds; medians and ranges in microseconds."""
    S = binding.shim()
    st = C.c_void_p(); binding.check(S.mi355_stream_create(C.byref(st)))
    nb = 256 << 20
    src, dst = binding.DevBuf(nb), binding.DevBuf(nb)
    copy_us = [_time_us(lambda: binding.check(S.mi355_d2d(dst.ptr, src.ptr, nb, st), "d2d"), st, 10) for _ in range(repeats)]
    bw = 2.0 * nb / (np.median(copy_us) * 1e-6)  # bytes read + written per second
    src.free(); dst.free()
    out = {"copy_256MiB_us": copy_us, "copy_bytes_per_s": bw, "iters": iters, "cases": []}
    for c, hw, g, stride in ((128, 52, 32, 1), (256, 26, 32, 1), (256, 26, 32, 2), (512, 13, 32, 1), (256, 26, 2, 1)):
        rng = np.random.default_rng(c + g + stride)
        B, k, n, cg = 32, 3, c, c // g
        x = rng.integers(0, 256, (B, c, hw, hw), dtype=np.uint8)
        wq = rng.integers(0, 256, (n, cg * k * k), dtype=np.uint8)
        zp_w = rng.integers(100, 157, n, dtype=np.uint8)
        bias = np.zeros(n, np.int32); mv = np.full(n, 0.75); sv = np.full(n, 2.0 ** -(7 + int(np.log2(cg))))
        wd = np.repeat(zp_w[:, None], c * k * k, axis=1).reshape(n, c, k * k)
        for j in range(n):
            wd[j, j // cg * cg:(j // cg + 1) * cg] = wq[j].reshape(cg, k * k)  # (n == c: ng == cg)
        ohw = (hw + 2 - k) // stride + 1
        xt = binding.DevTensor.from_nchw(x, 0)
        y, yd = binding.DevTensor(B, ohw, ohw, n, 23), binding.DevTensor(B, ohw, ohw, n, 23)
        blob = binding.DevBuf.from_numpy(binding.conv_group_pack(wq, zp_w, g, c, k, bias, mv, sv))
        blobd = binding.DevBuf.from_numpy(binding.conv_pack(wd.reshape(n, -1), zp_w, c, k, bias, mv, sv))
        d = binding.ConvDesc(n, c, k, stride, 1, binding.ACT["leaky"], 0, 0, 0, 23, 1.0)
        grp = lambda: binding.check(S.mi355_conv_group_forward(C.byref(d), xt.ref(), blob.ptr, g, y.ref(), None, None, st), "group")
        dense = lambda: binding.check(S.mi355_conv_forward(C.byref(d), xt.ref(), blobd.ptr, None, None, yd.ref(), None, None, st), "dense")
        t_grp, t_dense = [], []
        for _ in range(repeats):
            t_grp.append(_time_us(grp, st, iters)); t_dense.append(_time_us(dense, st, iters))
        S.mi355_stream_sync(st)
        same = bool(np.array_equal(y.to_nchw(), yd.to_nchw()))
        floor_us = (B * (c * hw * hw + n * ohw * ohw)) / bw * 1e6
        out["cases"].append({"c": c, "hw": hw, "n": n, "groups": g, "k": k, "stride": stride, "batch": B, "group_us": t_grp,
                             "dense_twin_us": t_dense, "dense_kernel": binding.last_conv_kernel(), "bytes_equal": same,
                             "hbm_floor_us": floor_us, "group_over_dense": float(np.median(t_grp) / np.median(t_dense)),
                             "group_over_floor": float(np.median(t_grp) / floor_us)})
    return out


def run_dil(iters, repeats):
    """The dilated kernel (conv_dil.hip) on 3x3 "same" layers, n = c, batch 32 -- 256 x 33 x 33 at d = 6, 12, 18 (ASPP) and 128 x 65 x 65
    at d = 2, 4 -- each against: the same layer at d = 1, pad 1 on whichever dense kernel serves it (equal MACs and bytes); where
    D = 2 d + 1 <= 11 its stuffed dense twin (weights off the tap lattice = the filter's zero point, the same bytes out)
    on conv_kxk.hip; and the HBM floor, tensor bytes in + out over the bandwidth a device-to-device copy of 256 MiB reaches in this
    process.  The kernels of a case alternate, `repeats` rounds; medians and ranges in microseconds."""
    S = binding.shim()
    st = C.c_void_p(); binding.check(S.mi355_stream_create(C.byref(st)))
    nb = 256 << 20
    src, dst = binding.DevBuf(nb), binding.DevBuf(nb)
    copy_us = [_time_us(lambda: binding.check(S.mi355_d2d(dst.ptr, src.ptr, nb, st), "d2d"), st, 10) for _ in range(repeats)]
    bw = 2.0 * nb / (np.median(copy_us) * 1e-6)  # bytes read + written per second
    src.free(); dst.free()
    out = {"copy_256MiB_us": copy_us, "copy_bytes_per_s": bw, "iters": iters, "cases": []}
    for c, hw, dil in ((256, 33, 6), (256, 33, 12), (256, 33, 18), (128, 65, 2), (128, 65, 4)):
        rng = np.random.default_rng(c + dil)
        B, k, n, D = 32, 3, c, 2 * dil + 1
        x = rng.integers(0, 256, (B, c, hw, hw), dtype=np.uint8)
        wq = rng.integers(0, 256, (n, c * k * k), dtype=np.uint8)
        zp_w = rng.integers(100, 157, n, dtype=np.uint8)
        bias = np.zeros(n, np.int32); mv = np.full(n, 0.75); sv = np.full(n, 2.0 ** -(7 + int(np.log2(c))))
        xt = binding.DevTensor.from_nchw(x, 0)
        y, y1, yt = (binding.DevTensor(B, hw, hw, n, 23) for _ in range(3))
        blob = binding.DevBuf.from_numpy(binding.conv_pack(wq, zp_w, c, k, bias, mv, sv))
        desc = lambda kk, pad: binding.ConvDesc(n, c, kk, 1, pad, binding.ACT["leaky"], 0, 0, 0, 23, 1.0)
        dd, d1, dt = desc(k, dil), desc(k, 1), desc(D, dil)
        runs = {"dil": lambda: binding.check(S.mi355_conv_dil_forward(C.byref(dd), xt.ref(), blob.ptr, dil, y.ref(), None, None, st), "dil"),
                "dense_d1": lambda: binding.check(S.mi355_conv_forward(C.byref(d1), xt.ref(), blob.ptr, None, None, y1.ref(), None, None, st), "d1")}
        if D <= 11:
            wt = np.repeat(zp_w[:, None], c * D * D, axis=1).reshape(n, c, D, D)
            wt[:, :, ::dil, ::dil] = wq.reshape(n, c, k, k)
            blobt = binding.DevBuf.from_numpy(binding.conv_pack(wt.reshape(n, -1), zp_w, c, D, bias, mv, sv))
            runs["stuffed_twin"] = lambda: binding.check(S.mi355_conv_forward(C.byref(dt), xt.ref(), blobt.ptr, None, None, yt.ref(), None, None, st), "twin")
        times, kern = {key: [] for key in runs}, {}
        for _ in range(repeats):
            for key, fn in runs.items():
                times[key].append(_time_us(fn, st, iters)); kern[key] = binding.last_conv_kernel()
        S.mi355_stream_sync(st)
        floor_us = (B * (c + n) * hw * hw) / bw * 1e6
        med = {key: float(np.median(v)) for key, v in times.items()}
        case = {"c": c, "hw": hw, "n": n, "k": k, "dilation": dil, "batch": B, "us": times, "kernel": kern, "hbm_floor_us": floor_us,
                "dil_over_dense_d1": med["dil"] / med["dense_d1"], "dil_over_floor": med["dil"] / floor_us}
        if D <= 11:
            case.update(bytes_equal=bool(np.array_equal(y.to_nchw(), yt.to_nchw())), dil_over_stuffed_twin=med["dil"] / med["stuffed_twin"])
        out["cases"].append(case)
    return out


def run_fc(iters, repeats):
    """The classifier tail (classify.hip).  Connected: 1024 -> 1000, 2048 -> 1000 on a 1 x 1 map and 512 x 7 x 7 -> 4096,
    at batch 32 and 64, each against the same layer through mi355_conv_forward (a 1x1 layer on the 1 x 1 map; the 7 x 7 layer on the
    7 x 7 map, pad 0) and the HBM floor: blob + input + output bytes over the bandwidth a device-to-device copy of 256 MiB reaches in
    this process.  Average pool: 1024 x 7 x 7 and 1280 x 13 x 13 against its floor.  The kernels of a case alternate, `repeats` rounds;
    medians and ranges in microseconds."""
    S = binding.shim()
    st = C.c_void_p(); binding.check(S.mi355_stream_create(C.byref(st)))
    nb = 256 << 20
    src, dst = binding.DevBuf(nb), binding.DevBuf(nb)
    copy_us = [_time_us(lambda: binding.check(S.mi355_d2d(dst.ptr, src.ptr, nb, st), "d2d"), st, 10) for _ in range(repeats)]
    bw = 2.0 * nb / (np.median(copy_us) * 1e-6)  # bytes read + written per second
    src.free(); dst.free()
    out = {"copy_256MiB_us": copy_us, "copy_bytes_per_s": bw, "iters": iters, "connected": [], "avgpool": []}
    for c, hw, n in ((1024, 1, 1000), (2048, 1, 1000), (512, 7, 4096)):
        rng = np.random.default_rng(c + n)
        K = c * hw * hw
        wq = rng.integers(0, 256, (n, K), dtype=np.uint8)
        zp_w = rng.integers(100, 157, n, dtype=np.uint8)
        bias = np.zeros(n, np.int32); mv = np.full(n, 0.75); sv = np.full(n, 2.0 ** -(7 + int(np.log2(K))))
        pack = binding.connected_pack(wq, zp_w, c, hw, hw, c, bias, mv, sv)
        blob, blobc = binding.DevBuf.from_numpy(pack), binding.DevBuf.from_numpy(binding.conv_pack(wq, zp_w, c, hw, bias, mv, sv))
        for B in (32, 64):
            xt = binding.DevTensor.from_nchw(rng.integers(0, 256, (B, c, hw, hw), dtype=np.uint8), 0)
            y, yc = binding.DevTensor(B, 1, 1, n, 23), binding.DevTensor(B, 1, 1, n, 23)
            wsz = S.mi355_connected_workspace_size(n, K, B)
            ws = binding.DevBuf(wsz) if wsz else None
            df = binding.ConvDesc(n, K, 1, 1, 0, binding.ACT["leaky"], 0, 0, 0, 23, 1.0)
            dc = binding.ConvDesc(n, c, hw, 1, 0, binding.ACT["leaky"], 0, 0, 0, 23, 1.0)
            runs = {"connected": lambda: binding.check(S.mi355_connected_forward(C.byref(df), xt.ref(), blob.ptr, y.ref(), None, None,
                                                                                  ws.ptr if ws else None, st), "fc"),
                    "conv_forward": lambda: binding.check(S.mi355_conv_forward(C.byref(dc), xt.ref(), blobc.ptr, None, None, yc.ref(), None, None, st), "conv")}
            times, kern, grid = {key: [] for key in runs}, {}, {}
            for _ in range(repeats):
                for key, fn in runs.items():
                    times[key].append(_time_us(fn, st, iters)); kern[key] = binding.last_conv_kernel(); grid[key] = binding.last_conv_launch()
            S.mi355_stream_sync(st)
            floor_us = (pack.size + B * (K + n)) / bw * 1e6
            med = {key: float(np.median(v)) for key, v in times.items()}
            out["connected"].append({"c": c, "hw": hw, "n": n, "batch": B, "blob_bytes": int(pack.size), "us": times, "kernel": kern, "launch": grid,
                                     "hbm_floor_us": floor_us, "bytes_equal": bool(np.array_equal(y.to_nchw(), yc.to_nchw())),
                                     "connected_over_conv_forward": med["connected"] / med["conv_forward"],
                                     "connected_over_floor": med["connected"] / floor_us})
    for c, hw in ((1024, 7), (1280, 13)):
        B = 32
        xt = binding.DevTensor.from_nchw(np.random.default_rng(c).integers(0, 256, (B, c, hw, hw), dtype=np.uint8), 0)
        y = binding.DevTensor(B, 1, 1, c, 0)
        fn = lambda: binding.check(S.mi355_avgpool_forward(xt.ref(), y.ref(), st), "avgpool")
        times = [_time_us(fn, st, iters) for _ in range(repeats)]
        S.mi355_stream_sync(st)
        floor_us = B * c * (hw * hw + 1) / bw * 1e6
        out["avgpool"].append({"c": c, "hw": hw, "batch": B, "us": times, "hbm_floor_us": floor_us, "avgpool_over_floor": float(np.median(times)) / floor_us})
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--fc", action="store_true", help="connected / avgpool against the layer spelled as a convolution and the HBM floor")
    ap.add_argument("--sep", action="store_true", help="fused depthwise + 1x1 against the two-launch pair and the HBM floor")
    ap.add_argument("--dil", action="store_true", help="dilated 3x3 against the same layer at d = 1, its stuffed twin and the HBM floor")
    ap.add_argument("--group", action="store_true", help="grouped 3x3 against its dense twin and the HBM floor")
    ap.add_argument("--tr", action="store_true", help="transposed k4 s2 / k2 s2 against the stuffed dense twin and the HBM floor")
    ap.add_argument("--dw", action="store_true", help="depthwise 3x3 against its dense twin and the HBM floor")
    ap.add_argument("--spp", action="store_true", help="the fused SPP pools against the three plain pools and the HBM floor")
    ap.add_argument("--out", default="", help="--dw, --spp, --tr, --group, --dil, --fc: also write the JSON here")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--c", type=int, default=256); ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--hw", type=int, default=52); ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32); ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--tile", type=int, nargs=2); ap.add_argument("--mode", choices=["flat", "patch"])
    ap.add_argument("--net", action="store_true"); ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--shift", type=int, default=13); ap.add_argument("--plan", action="store_true")
    ap.add_argument("--nt", type=int, default=0); ap.add_argument("--dbg", type=int, default=0, help="mi355_debug_flags value (512 = no chunk rotation)"); ap.add_argument("--timeline", action="store_true"); ap.add_argument("--timeline3", action="store_true"); ap.add_argument("--waveprof", action="store_true")
    ap.add_argument("--ablate", action="store_true", help="timing ablation of the K loop (results are wrong)")
    ap.add_argument("--timeline1", action="store_true", help="conv1x1_ws: per-workgroup phase timestamps (-DMI355_ABLATE build)")
    ap.add_argument("--timeline16", action="store_true", help="conv_rows16: per-workgroup phase timestamps (-DMI355_ABLATE build)")
    ap.add_argument("--timelinem", action="store_true", help="conv_mid_pool: per-workgroup phase timestamps (-DMI355_ABLATE build)")
    a = ap.parse_args()
    SHIFT = a.shift
    binding.init(0)
    if a.dbg:
        binding.shim().mi355_debug_flags(a.dbg)
    if a.dw or a.spp or a.tr or a.group or a.dil or a.fc or a.sep:
        fn = run_sep if a.sep else run_fc if a.fc else run_dil if a.dil else (run_group if a.group else (run_tr if a.tr else (run_spp if a.spp else run_dw)))
        r = fn(a.iters, a.repeats)
        print(json.dumps(r))
        if a.out:
            with open(a.out, "w") as f:
                json.dump(r, f, indent=1)
    elif a.ablate:
        S = binding.shim()
        for flags, name in [(0, "full"), (1, "no-dma"), (2, "no-barrier"), (4, "no-mfma"), (16, "no-cellsum"), (3, "no-dma,no-barrier"), (5, "no-dma,no-mfma"), (7, "only-lds-reads"), (15, "nothing-in-loop"), (32, "no-epilogue"), (47, "empty-kernel"), (63, "empty-kernel-no-cellsum"), (11, "only-mfma"), (9, "mfma+barrier"), (3, "lds+mfma"), (15 + 64, "epi-no-requant"), (15 + 128, "epi-no-copyout"), (15 + 64 + 128, "epi-neither")]:
            S.mi355_debug_flags(flags)
            r = run(a.c, a.n, a.hw, a.k, a.batch, a.iters, tuple(a.tile) if a.tile else None, a.mode)
            print(name, r["us"], "us", r["tops"], "TOPS")
        S.mi355_debug_flags(0)
    elif a.timeline1:
        S = binding.shim()
        S.mi355_debug_flags(a.dbg)
        r = run(a.c, a.n, a.hw, a.k, a.batch, 1, None, None)
        S.mi355_stream_sync(None)
        ts = np.zeros((4, 8192), np.int64)
        S.mi355_debug_read_ts1.argtypes = [C.c_void_p]
        assert S.mi355_debug_read_ts1(ts.ctypes.data) == 0
        nb = int((ts[0] > 0).sum())
        t = ts[:, :nb].astype(np.float64) / 100.0
        t0 = t[0].min()
        st = np.sort(t[0] - t0)
        print(f"blocks {nb}; span {t[3].max() - t0:.2f} us; starts: p25 {st[nb // 4]:.2f} p50 {st[nb // 2]:.2f} p75 {st[3 * nb // 4]:.2f} max {st[-1]:.2f}")
        for i, nm in [(0, "pixel tables + image DMA issued"), (1, "parameters, A fragments, everything landed, barrier"), (2, "groups: MFMAs + requantise + stores")]:
            d = t[i + 1] - t[i]
            print(f"  {nm:52s} p50 {np.median(d):6.2f}  min {d.min():6.2f}  max {d.max():6.2f} us")
        d = t[3] - t[0]
        print(f"  {'whole workgroup':52s} p50 {np.median(d):6.2f}  min {d.min():6.2f}  max {d.max():6.2f} us")
    elif a.timelinem:  # conv_mid_pool_kernel (64 -> 128 + pool): needs --pool and the -DMI355_ABLATE build
        S = binding.shim()
        r = run(a.c, a.n, a.hw, a.k, a.batch, 1, None, a.mode)
        S.mi355_stream_sync(None)
        ts = np.zeros((6, 4096), np.int64)
        S.mi355_debug_read_tsm.argtypes = [C.c_void_p]
        assert S.mi355_debug_read_tsm(ts.ctypes.data) == 0
        nb = int((ts[0] > 0).sum())
        t = ts[:, :nb].astype(np.float64) / 100.0
        t0 = t[0].min()
        print(json.dumps(r))
        print(f"blocks {nb}; span first start .. last end {t[5].max() - t0:.2f} us; starts: p50 {np.median(t[0]) - t0:.2f}, p90 {np.percentile(t[0], 90) - t0:.2f}, max {t[0].max() - t0:.2f}")
        for i, nm in [(0, "geometry, image DMA issued"), (1, "parameters to LDS, A fragments issued, pixel tables"), (2, "image / fragments landed, barrier"),
                      (3, "cell sums, box sums (two barriers)"), (4, "groups: MFMA chains + epilogues + stores issued")]:
            d = t[i + 1] - t[i]
            print(f"  {nm:52s} p50 {np.median(d):6.2f}  min {d.min():6.2f}  max {d.max():6.2f} us")
        d = t[5] - t[0]
        print(f"  {'whole workgroup':52s} p50 {np.median(d):6.2f}  min {d.min():6.2f}  max {d.max():6.2f} us")
    elif a.timeline16:
        S = binding.shim()
        S.mi355_debug_flags(a.dbg)
        r = run(a.c, a.n, a.hw, a.k, a.batch, 1, tuple(a.tile) if a.tile else None, a.mode, nt=a.nt)
        S.mi355_stream_sync(None)
        ts = np.zeros((6, 4096), np.int64)
        S.mi355_debug_read_ts16.argtypes = [C.c_void_p]
        assert S.mi355_debug_read_ts16(ts.ctypes.data) == 0
        nb = int((ts[0] > 0).sum())
        t = ts[:, :nb].astype(np.float64) / 100.0  # us
        t0 = t[0].min()
        print(f"blocks {nb}; span first start .. last end {t[5].max() - t0:.2f} us; starts: p50 {np.median(t[0]) - t0:.2f}, p90 {np.percentile(t[0], 90) - t0:.2f}, max {t[0].max() - t0:.2f}")
        for i, nm in [(0, "index math, DMA tables, prologue loads issued"), (1, "accumulator seeds, parameters, first image landed"), (2, "K loop"), (3, "epilogue: box sums + requantise"), (4, "copy-out")]:
            d = t[i + 1] - t[i]
            print(f"  {nm:52s} p50 {np.median(d):6.2f}  min {d.min():6.2f}  max {d.max():6.2f} us")
        d = t[5] - t[0]
        print(f"  {'whole workgroup':52s} p50 {np.median(d):6.2f}  min {d.min():6.2f}  max {d.max():6.2f} us")
    elif a.timeline:  # per-workgroup phase timestamps (needs the -DMI355_ABLATE build)
        S = binding.shim()
        r = run(a.c, a.n, a.hw, a.k, a.batch, 1, tuple(a.tile) if a.tile else None, a.mode, nt=a.nt)
        S.mi355_stream_sync(None)
        ts = np.zeros((6, 4096), np.int64)
        S.mi355_debug_read_ts.argtypes = [C.c_void_p]
        assert S.mi355_debug_read_ts(ts.ctypes.data) == 0
        nb = int((ts[0] > 0).sum())
        t = ts[:, :nb].astype(np.float64) / 100.0  # us
        t0 = t[0].min()
        print(json.dumps(r))
        print(f"blocks {nb}; kernel span first-start..last-end {t[5].max() - t0:.2f} us; start skew p50 {np.median(t[0]) - t0:.2f} max {t[0].max() - t0:.2f}")
        names = ["setup(index math, acc zero, params)", "first DMA wait", "K loop", "epilogue requant", "copy-out"]
        for i, nm in enumerate(names):
            d = t[i + 1] - t[i]
            print(f"  {nm:40s} p50 {np.median(d):6.2f}  min {d.min():6.2f}  max {d.max():6.2f} us")
        d = t[5] - t[0]
        print(f"  {'whole workgroup':40s} p50 {np.median(d):6.2f}  min {d.min():6.2f}  max {d.max():6.2f} us")
        order = np.argsort(t[0])
        late = order[256:] if nb > 256 else []
        if len(late):
            print(f"  second-round blocks: {len(late)}, start p50 {np.median(t[0][late]) - t0:.2f} us")
    elif a.timeline3:  # conv_ws3.hip per-wave phase timestamps (needs the -DMI355_ABLATE build)
        S = binding.shim()
        r = run(a.c, a.n, a.hw, a.k, a.batch, 1, None, None)
        S.mi355_stream_sync(None)
        ts = np.zeros((8, 4096, 8), np.int64)
        S.mi355_debug_read_ts3.argtypes = [C.c_void_p]
        assert S.mi355_debug_read_ts3(ts.ctypes.data) == 0
        nb = int((ts[0, :, 0] > 0).sum())
        t = ts[:, :nb, :].astype(np.float64) / 100.0
        t0 = t[0].min()
        print(json.dumps(r), "last kernel", S.mi355_last_conv_kernel())
        print(f"blocks {nb}; span {t[7].max() - t0:.2f} us; start skew p50 {np.median(t[0]) - t0:.2f} max {t[0].max() - t0:.2f}")
        names = ["stage image (loads + A issue + LDS writes)", "params + tables -> barrier", "box sums -> barrier", "A fragments landed", "phase 1 (partner's groups)", "barrier", "phase 2 / all groups (+ epilogue)"]
        for i, nm in enumerate(names):
            d = t[i + 1] - t[i]
            if (t[i + 1] > 0).all() and (t[i] > 0).all():
                print(f"  {nm:46s} p50 {np.median(d):6.2f}  min {d.min():6.2f}  max {d.max():6.2f} us")
        if hasattr(S, "mi355_debug_read_acc3"):
            ac = np.zeros((8, 4096), np.int64)
            S.mi355_debug_read_acc3.argtypes = [C.c_void_p]
            if S.mi355_debug_read_acc3(ac.ctypes.data) == 0 and ac[6, :nb].max() > 0:
                av = ac[:, :nb].astype(np.float64) / 100.0
                print(f"  persistent form, sums over a workgroup's {av[6].mean() * 100:.1f} tiles (us, thread 0): top-of-tile wait + barrier / staging pass {av[0].mean():.2f} | "
                      f"next tile's DMA issue {av[1].mean():.2f} | cell sums {av[2].mean():.2f} | parameters + tables + barrier {av[3].mean():.2f} | box sums + barrier {av[4].mean():.2f} | "
                      f"group loops {av[5].mean():.2f} | before the first tile {av[7].mean():.2f}")
        print("  phase 4->7:", f"p50 {np.median(t[7] - t[4]):6.2f}  max {(t[7] - t[4]).max():6.2f}")
        d47 = (t[7] - t[4]).mean(axis=1)
        print("  4->7 mean per workgroup, by blockIdx % 8 (XCD):", [round(float(d47[k::8].mean()), 2) for k in range(8)])
        print("  4->7 of workgroups 0..31:", [round(float(v), 1) for v in d47[:32]])
        print("  4->7 per wave index (mean):", [round(float(v), 2) for v in (t[7] - t[4]).mean(axis=0)])
        wp = np.zeros((4096, 8, 4), np.int64)
        S.mi355_debug_read_wp3.argtypes = [C.c_void_p]
        assert S.mi355_debug_read_wp3(wp.ctypes.data) == 0
        w = wp[:nb].astype(np.float64)
        ng = np.full_like(w[:, :, 3], float(os.environ.get("WS3_GROUPS", "6")))
        print("  shader clock over phases 4->7 (cycle counter / wall clock), GHz, by wave:", [round(float(v), 3) for v in (w[:, :, 3] / ((t[7] - t[4]) * 1e3)).mean(axis=0)])
        for k, nm in enumerate(["tap offsets + first 4 B reads", "36-MFMA loop", "epilogue / partial store"]):
            print(f"  shader clocks per group, {nm:32s} mean {np.mean(w[:, :, k] / ng):8.0f}   by wave {[int(v) for v in (w[:, :, k] / ng).mean(axis=0)]}")
        print("  start (t4 - t0min) of workgroups 0..31:", [round(float(v), 1) for v in (t[4].mean(axis=1) - t0)[:32]])
        d = t[7] - t[0]
        print(f"  {'whole wave':46s} p50 {np.median(d):6.2f}  min {d.min():6.2f}  max {d.max():6.2f} us")
    elif a.waveprof:  # per-wave stall profile of the 3x3 K loop (needs the -DMI355_ABLATE build)
        S = binding.shim()
        S.mi355_debug_flags(256 | a.dbg)
        r = run(a.c, a.n, a.hw, a.k, a.batch, 1, tuple(a.tile) if a.tile else None, a.mode, nt=a.nt)
        S.mi355_stream_sync(None)
        S.mi355_debug_flags(0)
        wp = np.zeros((4096, 8, 5), np.int64)
        S.mi355_debug_read_wp.argtypes = [C.c_void_p]
        assert S.mi355_debug_read_wp(wp.ctypes.data) == 0
        nb = int((wp.sum(axis=(1, 2)) > 0).sum())
        w = wp[:nb].astype(np.float64)
        print(json.dumps(r))
        names = ["drain LDS reads of previous step", "s_waitcnt vmcnt (DMA landed)", "s_barrier", "k-half 0 (6 MFMA + DMA issue + 5 reads)", "k-half 1 (6 MFMA + 5 reads)"]
        tot = w.sum(axis=2)
        print(f"blocks {nb}; shader-clock ticks per wave in the K loop: p50 {np.median(tot):.0f}")
        for k, nm in enumerate(names):
            print(f"  {nm:44s} {100 * w[:, :, k].sum() / tot.sum():5.1f} %   per wave p50 {np.median(w[:, :, k]):9.0f}")
        print("  per wave index (mean ticks):", [int(v) for v in w.mean(axis=0).sum(axis=1)])
        for k in range(5):
            print(f"    phase {k} by wave:", [int(v) for v in w[:, :, k].mean(axis=0)])
    elif a.plan:  # rows-kernel tile plan sweep: capacity x tile count, per conv shape of the net
        for c, n, hw, k in NET:
            if c % 64:
                continue
            bm = 128 if n >= 128 else (64 if n > 32 else 32)
            mt = (n + bm - 1) // bm
            total = 64 * hw * hw
            print(json.dumps({"auto": run(c, n, hw, k, 64, a.iters)}))
            for bn in (384, 256, 128):
                if bn == 384 and bm != 128:
                    continue
                nt0 = -(-total // bn)
                cands = {nt0}
                for blocks in (256, 512, 768, 1024, 1536, 2048):
                    if blocks // mt >= nt0:
                        cands.add(blocks // mt)
                for nt in sorted(cands)[:4]:
                    try:
                        r = run(c, n, hw, k, 64, a.iters, (bm, bn), None, nt=nt)
                        print(json.dumps({"c": c, "n": n, "hw": hw, "bn": bn, "nt": nt, "blocks": nt * mt, "us": r["us"], "tops": r["tops"]}))
                    except Exception as e:  # noqa: BLE001
                        print(json.dumps({"c": c, "n": n, "hw": hw, "bn": bn, "nt": nt, "error": str(e)[:80]}))
    elif a.net:
        for c, n, hw, k in NET:
            print(json.dumps(run(c, n, hw, k, 64, a.iters)))
    elif a.sweep:
        for bm, bn in [(128, 256), (128, 128)]:
            for mode in ["flat", "patch"]:
                try:
                    print(json.dumps(run(a.c, a.n, a.hw, a.k, a.batch, a.iters, (bm, bn), mode)))
                except Exception as e:  # noqa: BLE001
                    print(json.dumps({"tile": [bm, bn], "mode": mode, "error": str(e)[:100]}))
    else:
        print(json.dumps(run(a.c, a.n, a.hw, a.k, a.batch, a.iters, tuple(a.tile) if a.tile else None, a.mode, nt=a.nt)))
