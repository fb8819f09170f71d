"""conv1x1.hip's head path (one filter quad with fewer than 32 filters), through mi355_conv_forward / mi355_conv_yolo_forward against the oracle.

A launch with n < 32 runs the kernel's ROW form: accumulator row 31 of the 32 x 32 tile belongs to no filter, its A row is set to ones in
registers and the MFMAs leave the pixel's sum of x' there; the epilogue takes "which filter exists" and "which yolo entry stays linear" from
two masks per wave and indexes the float tensors with 32 bits.  Under the throughput plan such a launch also gets workgroups with as many
waves as the tile has groups of 32 pixels.  n == 32 has no spare row and keeps the kernel and the geometry of before, and so does every
launch under mi355_debug_flags bit 16 -- which must give the same bytes.

Shapes: the smallest at which each path can go wrong -- 13 x 13 and 5 x 3 maps at batch 1..3 (total pixels no multiple of 32 or of the tile,
tiles that cross an image boundary, a ragged last tile, one launch with fewer than 32 pixels), 18 / 30 / 31 filters (one to fourteen pad
rows; with 31 the sum row is the only one) and 32 (the old path), every channel depth the kernel is compiled for, both plans, both stores,
the three outputs (fused yolo store, quant_stop float tail, plain LEAKY bytes).  Weight zero points 0, 128 and 255 sit in filters 0..2 of
every case (128 - zp_w = 128 and -127: the extremes of the __mul24(dz, sx) term); two cases feed bytes that are all 0 / all 255, where the
sum row reaches +-c * 128.  The 1024 -> 256 neck at 3, 4 and 2 tiles of 128 pixels (batch 2, 3, 1) is compared as well.

Uint8 and the float tail are compared exactly; the yolo logistic to 1 ulp (atol 2e-7), as everywhere in this suite."""
import numpy as np
import pytest

import oracle
from yolo_quantization_amd import binding

pytestmark = pytest.mark.gpu

OLD_PATH = 1 << 16  # mi355_debug_flags: heads on the kernel and geometry of before
ZP_IN, S_ACT = 23, np.float32(0.0625)


@pytest.fixture(scope="module", autouse=True)
def device():
    binding.init(0)


def _cdiv(a, b):
    return -(-a // b)


def head_launch(c, n, total, plan, old):
    """(grid, threads) conv1x1_ws_launch chooses for a one-round launch of a single filter quad"""
    tp = max(16, _cdiv(total, 256))
    head = n < 32 and plan == 1 and not old
    if plan == 1:
        tp = (tp + 31) & ~31
    if head:
        while tp < 128 and tp < total and (c // 64) * 2 * ((tp + 32) // 32) * 1024 <= 64 * 1024:
            tp += 32
    G = _cdiv(tp, 32)
    sets = _cdiv(G, _cdiv(G, 8)) if head else 8
    return _cdiv(total, tp), 64 * sets


def _layer(c, n, seed):
    rng = np.random.default_rng(seed)
    wq = rng.integers(0, 256, (n, c), dtype=np.uint8)
    zp_w = rng.integers(90, 166, n, dtype=np.uint8)
    zp_w[:3] = (0, 128, 255)
    bias = rng.integers(-20000, 20000, n).astype(np.int32)
    M = rng.uniform(2.0 ** -13, 2.0 ** -10, n) * (256.0 / c)
    shift = np.floor(-np.log2(M)).astype(int)
    M0 = np.round(M * 2.0 ** shift * 2 ** 31)
    return wq, zp_w, bias, M0 * 2.0 ** -31, 2.0 ** -shift.astype(np.float64)


_REF = {}


def _reference(c, n, H, W, B, out, store, fill=None):
    """operands and the oracle's outputs of one case, computed once and shared by the plans and the switch"""
    key = (c, n, H, W, B, out, store, fill)
    if key not in _REF:
        rng = np.random.default_rng(c + 31 * n + 7 * H + W + B)
        x = rng.integers(0, 256, (B, c, H, W), dtype=np.uint8) if fill is None else np.full((B, c, H, W), fill, np.uint8)
        L = _layer(c, n, c + n)
        act = "leaky" if out == "leaky" else "linear"
        zp_act = 23 if out == "leaky" else 128
        u8 = np.stack([oracle.requant(oracle.conv_acc(x[b], L[0], L[1], 1, 1, 0, ZP_IN, oracle.ACC_EXACT), L[2], L[3], L[4], zp_act,
                                      oracle.ACT[act], store) for b in range(B)])
        want = {"u8": u8}
        if out != "leaky":
            want["f32"] = oracle.dequant(u8, zp_act, S_ACT)
        if out == "yolo":
            classes = _classes(n)
            yo = np.empty_like(want["f32"])
            for b in range(B):
                fb = np.ascontiguousarray(want["f32"][b])
                ob = np.empty_like(fb)
                oracle.lib().orc_yolo_forward(fb.ctypes.data, n // (classes + 5), classes, H, W, ob.ctypes.data)
                yo[b] = ob
            want["yolo"] = yo
        for v in want.values():
            v.setflags(write=False)
        _REF[key] = (x, L, act, zp_act, want)
    return _REF[key]


def _classes(n):
    return {30: 5, 18: 1, 31: 26, 32: 11}[n]  # 3 x 10, 3 x 6, 1 x 31, 2 x 16 entries


def _run(x, L, act, zp_act, out, store, plan, flags):
    xt = binding.DevTensor.from_nchw(x, ZP_IN)
    args = (xt, L[0], L[1], 1, L[2], L[3], L[4], ZP_IN, zp_act, S_ACT, binding.ACT[act])
    binding.shim().mi355_debug_flags(flags)
    try:
        if out == "yolo":
            o = binding.conv_fused_forward(*args, "yolo", store=store, plan=plan, classes=_classes(L[0].shape[0]))
        else:
            o = binding.conv_forward(*args, store, binding.ACC_EXACT, want_acc=False, want_f32=out == "f32", plan=plan)
    finally:
        binding.shim().mi355_debug_flags(0)
    return o, binding.last_conv_kernel(), binding.last_conv_launch()


def _check(c, n, H, W, B, out, store, plan, fill=None):
    x, L, act, zp_act, want = _reference(c, n, H, W, B, out, store, fill)
    hw = H * W
    got = {}
    for old in (False, True):
        o, kern, (grid, threads, _) = _run(x, L, act, zp_act, out, store, plan, OLD_PATH if old else 0)
        what = f"{c}->{n} @{H}x{W} B{B} {out} store {store} plan {plan} {'old path' if old else 'head path'}"
        assert kern == 3, f"{what}: conv1x1.hip should serve the call, kernel {kern} did"
        assert (grid, threads) == head_launch(c, n, B * hw, plan, old), f"{what}: launch geometry"
        assert np.array_equal(o["u8"].reshape(B, n, hw), want["u8"]), f"{what}: uint8"
        if "f32" in want:
            assert np.array_equal(o["f32"], want["f32"]), f"{what}: float tail"
        if "yolo" in want:
            assert np.allclose(o["yolo"], want["yolo"], rtol=0, atol=2e-7), f"{what}: yolo activations"
            lin = [e for e in range(n) if e % (_classes(n) + 5) in (2, 3)]
            assert np.array_equal(o["yolo"][:, lin], want["f32"][:, lin]), f"{what}: the w, h entries stay linear, bit for bit"
        got[old] = o
    for k in ("u8", "f32", "yolo"):
        if k in got[False]:
            assert np.array_equal(got[False][k], got[True][k]), f"{k}: the head path and the old path store different bytes"


# (c, n, H, W, B)
SHAPES = [
    (256, 30, 13, 13, 2),   # 338 pixels: plan 1 = three tiles of 128, the last with 82 pixels; tiles cross the image boundary
    (512, 30, 13, 13, 3),   # 507 pixels: four tiles, the 512-channel head at four waves per SIMD
    (512, 18, 5, 3, 3),     # 45 pixels: one tile of two groups, the second ragged; fourteen pad rows
    (256, 31, 13, 13, 1),   # 169 pixels; row 31 is the only pad row
    (256, 31, 5, 3, 2),     # 30 pixels: fewer than one group
    (256, 30, 5, 3, 1),     # 15 pixels: fewer than the 16-pixel tile floor
    (512, 18, 13, 13, 1),
    (512, 32, 13, 13, 2),   # no spare row: the old kernel, the old geometry
    (256, 32, 5, 3, 3),
    (1024, 30, 5, 3, 3),    # the other depths the ROW form is compiled for
    (128, 30, 13, 13, 1),
    (64, 18, 5, 3, 2),
]


@pytest.mark.parametrize("store", [binding.STORE_WRAP, binding.STORE_SATURATE], ids=["wrap", "saturate"])
@pytest.mark.parametrize("plan", [0, 1], ids=["latency", "throughput"])
@pytest.mark.parametrize("out", ["yolo", "f32", "leaky"])
@pytest.mark.parametrize("c,n,H,W,B", SHAPES, ids=lambda v: str(v))
def test_head_against_oracle(c, n, H, W, B, out, plan, store):
    _check(c, n, H, W, B, out, store, plan)


@pytest.mark.parametrize("plan", [0, 1], ids=["latency", "throughput"])
@pytest.mark.parametrize("fill", [0, 255])
@pytest.mark.parametrize("c,n", [(512, 30), (1024, 18), (256, 31)])
def test_head_sum_row_at_its_extremes(c, n, fill, plan):
    """every input byte 0 / 255: x' = -128 / 127 in every channel, the sum row holds -c * 128 / c * 127"""
    _check(c, n, 5, 3, 3, "yolo", binding.STORE_WRAP, plan, fill=fill)
    _check(c, n, 5, 3, 3, "leaky", binding.STORE_SATURATE, plan, fill=fill)


def test_throughput_plan_sizes_head_workgroups_to_their_groups():
    """the two heads of yolov3-tiny at batch 64, launcher arithmetic only: 512 -> 30 @13 runs four-wave workgroups of 128 pixels,
    256 -> 30 @26 six-wave workgroups of 192; before, both ran eight waves (169 x 512 and 226 x 512 threads)"""
    assert head_launch(512, 30, 64 * 169, 1, False) == (85, 256) and head_launch(512, 30, 64 * 169, 1, True) == (169, 512)
    assert head_launch(256, 30, 64 * 676, 1, False) == (226, 384) and head_launch(256, 30, 64 * 676, 1, True) == (226, 512)


@pytest.mark.parametrize("plan", [0, 1], ids=["latency", "throughput"])
@pytest.mark.parametrize("B", [1, 2, 3])
def test_neck_1024_to_256_tiles(B, plan):
    """the 1024 -> 256 neck at 13 x 13: 169 / 338 / 507 pixels = 2 / 3 / 4 tiles of 128 under the throughput plan (a ragged last tile)"""
    rng = np.random.default_rng(B)
    x = rng.integers(0, 256, (B, 1024, 13, 13), dtype=np.uint8)
    L = _layer(1024, 256, 5)
    want = np.stack([oracle.requant(oracle.conv_acc(x[b], L[0], L[1], 1, 1, 0, ZP_IN, oracle.ACC_EXACT), L[2], L[3], L[4], 23, oracle.LEAKY,
                                    binding.STORE_WRAP) for b in range(B)])
    o, kern, _ = _run(x, L, "leaky", 23, "leaky", binding.STORE_WRAP, plan, 0)
    assert kern == 3
    assert np.array_equal(o["u8"].reshape(B, 256, 169), want)
