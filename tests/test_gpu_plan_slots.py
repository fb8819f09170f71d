"""Every batch slot under both kernel plans, against the oracle.

The benchmark times large batches of DIFFERENT images under the throughput plan (mi355_conv_desc.plan = 1, set by network_replica),
which picks other tile sizes, workgroup shapes and even kernel families than the latency plan.  A kernel that reads the wrong image
-- a halo or a whole tile taken from image b +- 1 where a tile straddles two images, a wrong image stride in a persistent workgroup's
second tile -- cannot be seen with the same image in every slot.  So every case here runs distinct images in every slot and checks:

  * chosen slots (0, 1, the two around B/2, the last two, two seeded random ones) against the oracle, byte for byte;
  * every slot: plan 0 == plan 1 == the generic route (debug flags 1024 | 8192 | 16384), with and without the epilogue table;
  * every slot: the batch rolled by r in {1, 5} gives the rolled outputs, Y_r[b] == Y[(b - r) mod B];
  * that the checks can fail: the chosen slots' inputs are pairwise distinct, neighbouring slots' outputs differ;
  * the kernel family and launch geometry each case is meant to reach (mi355_last_conv_kernel / mi355_last_conv_launch).

Tensors are compared through per-slot SHA-256 digests, so that batch-64 / batch-32 tensors do not have to be kept in host memory.
The yolo logistic is compared with the oracle to 1 ulp (atol 2e-7, as everywhere in this suite); everything else exactly."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

import oracle
from launch_geometry import geom_conv1x1, geom_small64
from yolo_quantization_amd import binding, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GENERIC = 1024 | 8192 | 16384  # mi355_debug_flags: no conv_small / first-layer MFMA / conv_pool16, no conv1x1.hip, no conv_ws3.hip


@pytest.fixture(scope="module", autouse=True)
def device():
    binding.init(0)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def slot_digests(t):
    """t: [B, ...] -> one digest per slot"""
    return [sha(t[b]) for b in range(t.shape[0])]


def chosen_slots(B, seed):
    rng = np.random.default_rng(seed)
    s = {0, 1, B // 2 - 1, B // 2, B - 2, B - 1}
    while len(s) < min(8, B):
        s.add(int(rng.integers(0, B)))
    return sorted(s)


def check_roll(d, d_r, r, what):
    """d, d_r: per-slot digests of the batch and of the batch rolled by r"""
    B = len(d)
    bad = [b for b in range(B) if d_r[b] != d[(b - r) % B]]
    assert not bad, f"{what}: rolled by {r}, slots {bad[:8]} do not hold their image's outputs (cross-image read)"


def check_can_fail(x, slots, d, what):
    """the roll and slot checks prove something only when the images -- and so the outputs -- differ"""
    hs = [sha(x[b]) for b in slots]
    assert len(set(hs)) == len(hs), f"{what}: chosen slots' inputs are not pairwise distinct"
    same = [b for b in range(len(d) - 1) if d[b] == d[b + 1]]
    assert not same, f"{what}: neighbouring slots {same[:8]} have equal outputs"


def ceil_div(a, b):
    return -(-a // b)


# --------------------------------------------------------------------------------------------------- layer-level matrix
def rand_layer(rng, n, c, k, gain):
    """weights in the suite's wrap regimes (test_gpu_parity.py), the multiplier range scaled with K from the 144 of a 16-channel 3x3"""
    K = c * k * k
    wq = rng.integers(0, 256, (n, K), dtype=np.uint8)
    zp_w = rng.integers(90, 166, n, dtype=np.uint8)
    zp_w[0], zp_w[1] = 0, 255  # zero points whose 128 - zp_w leaves the int8 range (the correction MFMA of the 16-channel kernels)
    bias = rng.integers(-20000, 20000, n).astype(np.int32)
    lo, hi = {"some-wrap": (2.0 ** -14, 2.0 ** -12), "much-wrap": (2.0 ** -11, 2.0 ** -7)}[gain]
    f = 144.0 / K
    M = rng.uniform(lo * f, hi * f, n)
    shift = np.floor(-np.log2(M)).astype(int)
    M0 = np.round(M * 2.0 ** shift * 2 ** 31)
    if gain == "some-wrap":
        bias = (bias // 16).astype(np.int32)
    return wq, zp_w, bias, M0 * 2.0 ** -31, 2.0 ** -shift.astype(np.float64)


class Case:
    def __init__(self, name, c, n, H, W, B, k=3, stride=1, fuse=None, act="leaky", gain="much-wrap", kern=(None, None),
                 geom=None, planar=False, refused_plan1=False):
        self.name, self.c, self.n, self.H, self.W, self.B, self.k, self.stride = name, c, n, H, W, B, k, stride
        self.fuse, self.act, self.gain, self.kern, self.geom, self.planar = fuse, act, gain, kern, geom, planar
        self.refused_plan1 = refused_plan1  # the fused call is refused under plan 1 (the host then runs the conv and the glue apart)

    def __repr__(self):
        return self.name


# ---- launch geometry the launchers must choose: restated in tests/launch_geometry.py (a changed threshold shows up here)


def expect_geom(case, plan, got):
    """assert that the launch reached the regime the case names"""
    kern, (grid, threads, lds) = got
    B, H, W = case.B, case.H, case.W
    OH, OW = (H + 2 * (case.k // 2) - case.k) // case.stride + 1, (W + 2 * (case.k // 2) - case.k) // case.stride + 1
    g = case.geom
    if g == "conv1x1":
        e = geom_conv1x1(case.c, case.n, B, H, W, plan)
        assert (grid, threads, lds) == (e["grid"], e["threads"], e["lds"]), (plan, e)
        if plan == 1:
            assert e["tp"] % 32 == 0
    elif g == "small64":
        e = geom_small64(case.n, B, H, W, plan)
        assert (grid, threads) == (e["grid"], e["threads"]), (plan, e)
        assert e["half"] and threads == case.n // 32 * 64, "half workgroups"
        if plan == 0:
            assert e["ntiles"] > 256 and e["tp"] % 32 != 0, "latency plan: several rounds with a ragged tile (ADVICE r06)"
    elif g == "small64_1r":  # one round of the chip: whole workgroups under plan 0, half workgroups under plan 1
        e = geom_small64(case.n, B, H, W, plan)
        assert (grid, threads) == (e["grid"], e["threads"]) and e["half"] == (plan == 1), (plan, e)
    elif g == "small64w":  # wide maps: 8 x 16 patches of one image each, half workgroups under both plans
        assert grid == B * ceil_div(W // 2, 16) * ceil_div(H // 2, 8) and threads == case.n // 32 * 64, "half workgroups"
        assert plan == 1 or grid > 256, "latency plan: half workgroups only where the launch needs several rounds"
    elif g == "small16":  # persistent 4-wave workgroups over flat 128-pixel tiles that cross rows and images
        ntiles = ceil_div(B * (H // 2) * (W // 2), 128)
        if kern == 2:
            assert threads == 256 and grid in (256, 512, 768) and grid < ntiles, "persistent workgroups with several tiles"
    if kern == 7:  # conv_pool16: three persistent workgroups per CU, several tiles each
        tiles = B * ceil_div(W // 2, 16) * ceil_div(H // 2, 8)
        assert threads == 256 and grid == 768 and tiles > grid
    if g == "ws3_persistent" and kern == 4:
        assert threads == 512 and grid == 256 and B * OH * OW > 256 * grid, "several tiles per persistent workgroup"
    if kern == 5 and plan == 1 and g == "replanned":  # row-image kernel: workgroups of which two share a CU
        assert threads <= 256 and lds <= 80 * 1024, (threads, lds)
    if kern == 1:  # first layer: the MFMA kernels (no dynamic LDS), 256 threads
        assert threads == 256 and lds == 0 and grid > 0


CASES = [
    # conv1x1.hip (3): plan-1 tiles rounded to whole groups of 32; the one-round growth loop; two / four filter tiles; heads
    Case("c1x1_256_128_13_B64", 256, 128, 13, 13, 64, k=1, kern=(3, 3), geom="conv1x1", gain="some-wrap"),
    Case("c1x1_1024_256_13_B64_grow", 1024, 256, 13, 13, 64, k=1, kern=(3, 3), geom="conv1x1"),
    Case("c1x1_256_512_13_B64_mtiles2", 256, 512, 13, 13, 64, k=1, kern=(3, 3), geom="conv1x1", act="relu6"),
    Case("c1x1_512_1024_13_B16_mtiles4", 512, 1024, 13, 13, 16, k=1, kern=(3, 3), geom="conv1x1", gain="some-wrap"),
    Case("c1x1_512_255_13_B64_f32", 512, 255, 13, 13, 64, k=1, fuse="f32", act="linear", kern=(3, 3), geom="conv1x1"),
    Case("c1x1_512_255_13_B64_yolo", 512, 255, 13, 13, 64, k=1, fuse="yolo", act="linear", kern=(3, 3), geom="conv1x1"),
    Case("c1x1_256_128_13_B64_up", 256, 128, 13, 13, 64, k=1, fuse="upsample", kern=(3, 3), geom="conv1x1"),
    # conv_small.hip (2), 16 / 32 channels, pooled: persistent workgroups, 128-pixel tiles crossing images (2500 pooled pixels an image);
    # plan 1 + wrap store: the zero-point-correction instantiation (n 32 without the epilogue hint, n 64); with the hint the 16 -> 32 layer
    # goes to conv_pool16.hip (7)
    Case("small_16_32_100_B60_pool", 16, 32, 100, 100, 60, fuse="pool2", kern=(2, 2), geom="small16"),
    Case("small_16_64_100_B60_pool", 16, 64, 100, 100, 60, fuse="pool2", kern=(2, 2), geom="small16", act="relu6", gain="some-wrap"),
    Case("small_32_64_104_B64_pool", 32, 64, 104, 104, 64, fuse="pool2", kern=(2, 2), geom="small16"),
    # conv_small.hip (2), 64 channels: half workgroups under plan 1, and under plan 0 where a launch needs several rounds (ntiles > 256)
    # with a ragged tile (133 pooled pixels): pooled, stride 1, stride 2
    Case("small_64_128_52_B100_pool", 64, 128, 52, 52, 100, fuse="pool2", kern=(2, 2), geom="small64"),
    Case("small_64_64_52_B100_s1", 64, 64, 52, 52, 100, kern=(2, 2), geom="small64", gain="some-wrap"),
    Case("small_64_128_52_B100_s2", 64, 128, 52, 52, 100, stride=2, kern=(2, 2), geom="small64", act="relu6"),
    Case("small_64_128_52_B64_pool_tiny6", 64, 128, 52, 52, 64, fuse="pool2", kern=(2, 2), geom="small64_1r"),
    # ... and on wide maps (YOLOv3-608's 64 -> 128 layers at batch 32 take this form): stride 1 at 152, stride 2 at 304
    Case("small_64_128_152_B6_wide", 64, 128, 152, 152, 6, kern=(2, 2), geom="small64w"),
    Case("small_64_128_304_B2_wide_s2", 64, 128, 304, 304, 2, stride=2, kern=(2, 2), geom="small64w", gain="some-wrap"),
    # conv_ws3.hip (4) / row image (5): one-round launches re-planned under plan 1; several rounds (persistent workgroups) and 19-wide
    # maps keep conv_ws3; the fused 2x2/2 and 2x2/1 pools (refused under plan 1 where the launch would be re-planned); the residual add
    Case("ws3_256_512_13_B64_replanned", 256, 512, 13, 13, 64, kern=(4, 5), geom="replanned"),
    Case("ws3_128_256_76_B16_persistent", 128, 256, 76, 76, 16, kern=(4, 4), geom="ws3_persistent", gain="some-wrap"),
    Case("ws3_256_512_19_B16_w19", 256, 512, 19, 19, 16, kern=(4, 4)),
    Case("ws3_128_256_26_B64_pool2", 128, 256, 26, 26, 64, fuse="pool2", kern=(4, 5), geom="replanned", refused_plan1=True),
    Case("ws3_256_512_13_B64_pool1", 256, 512, 13, 13, 64, fuse="pool1", kern=(4, 5), geom="replanned", refused_plan1=True),
    Case("ws3_128_256_38_B12_shortcut", 128, 256, 38, 38, 12, fuse="shortcut", act="linear", kern=(4, 4)),
    # first layer (1): batch 64 @416 fused with its pool (yolov3-tiny), batch 32 @608 (YOLOv3), planar and cs = 4 input
    Case("first_3_16_416_B64_pool_planar", 3, 16, 416, 416, 64, fuse="pool2", kern=(1, 1), planar=True),
    Case("first_3_16_416_B64_pool_cs4", 3, 16, 416, 416, 64, fuse="pool2", kern=(1, 1), gain="some-wrap"),
    Case("first_3_32_608_B32_planar", 3, 32, 608, 608, 32, kern=(1, 1), planar=True),
    Case("first_3_32_608_B32_cs4", 3, 32, 608, 608, 32, kern=(1, 1), act="relu6"),
]


def _input_tensor(case, x, zp_in):
    if not case.planar:
        return binding.DevTensor.from_nchw(x, zp_in), None
    buf = binding.DevBuf.from_numpy(x)  # the reference's [B][3][H][W] planes, read in place (mi355_tensor_describe_nchw)
    t = binding.Tensor(buf.ptr, x.shape[0], x.shape[2], x.shape[3], x.shape[1], 1, 0, 0)

    class Planar:
        pass
    p = Planar()
    p.t, p.buf = t, buf
    p.ref = lambda: C.byref(p.t)
    return p, buf


class Layer:
    """one case's operands; run(x, ...) returns (per-slot digests, {slot: outputs}, (kernel, geometry))"""

    def __init__(self, case, rng):
        self.case = case
        c, n, k = case.c, case.n, case.k
        self.wq, self.zp_w, self.bias, self.mv, self.sv = rand_layer(rng, n, c, k, case.gain)
        self.zp_in = 0 if c == 3 else 9
        self.zp_act = 128 if case.act == "linear" else 23
        self.s_act = np.float32(0.0625)
        self.act = binding.ACT[case.act]
        if case.fuse == "shortcut":
            self.Ka, self.Kb, self.zp_from, self.zp_out = 41000, 70000, 17, 131

    def device(self, x, res, plan, epilogue, store, flags=0):
        case = self.case
        xt, _keep = _input_tensor(case, x, self.zp_in)
        kw = dict(store=store, plan=plan, epilogue=epilogue)
        args = (self.wq, self.zp_w, case.k, self.bias, self.mv, self.sv, self.zp_in, self.zp_act, self.s_act, self.act)
        binding.shim().mi355_debug_flags(flags)
        try:
            if case.fuse in (None, "f32"):
                o = binding.conv_forward(xt, *args, want_acc=False, want_f32=case.fuse == "f32", stride=case.stride, **kw)
            elif flags and case.c != 3:
                # the generic route: the plain convolution on the row-image / implicit-GEMM kernel, the fused layer after it on the host
                # (the first layer keeps its fused call: debug bit 1024 sends it to the VALU kernels)
                o = binding.conv_forward(xt, *args, want_acc=False, want_f32=case.fuse == "yolo", **kw)
                o = dict(o, glue=True)
            else:
                fk = dict(res=res, Ka=getattr(self, "Ka", 0), Kb=getattr(self, "Kb", 0), zp_from=getattr(self, "zp_from", 0),
                          zp_out=getattr(self, "zp_out", 0), classes=80)
                o = binding.conv_fused_forward(xt, *args, case.fuse, **kw, **fk)
        finally:
            binding.shim().mi355_debug_flags(0)
        got = (binding.last_conv_kernel(), binding.last_conv_launch())
        return o, got


def _glue_host(case, L, u8, res_u8, f32):
    """the fused layer applied by the oracle to one slot's conv output"""
    if case.fuse == "pool2":
        return {"u8": oracle.maxpool_u8(u8, 2, 2, 1)}
    if case.fuse == "pool1":
        return {"u8": oracle.maxpool_u8(u8, 2, 1, 1)}
    if case.fuse == "upsample":
        return {"u8": oracle.upsample_u8(u8, 2)}
    if case.fuse == "shortcut":
        return {"u8": oracle.shortcut_u8(u8, res_u8, L.Ka, L.Kb, L.zp_act, L.zp_from, L.zp_out)}
    if case.fuse == "yolo":
        out = np.empty_like(f32)
        oracle.lib().orc_yolo_forward(f32.ctypes.data, case.n // 85, 80, case.H, case.W, out.ctypes.data)
        return {"u8": u8, "f32": f32, "yolo": out}
    if case.fuse == "f32":
        return {"u8": u8, "f32": f32}
    return {"u8": u8}


def _collect(case, L, o, res_nchw, slots):
    """device outputs -> (digests over every slot of every output tensor, {slot: {key: array}})"""
    B = case.B
    outs = {}
    if o.get("glue"):  # generic route: glue on the host, every slot
        u8 = o["u8"]
        f32 = o.get("f32")
        per = []
        for b in range(B):
            fb = None if f32 is None else f32[b].reshape(case.n, case.H, case.W)
            per.append(_glue_host(case, L, u8[b], None if res_nchw is None else res_nchw[b], fb))
        outs = {k: np.stack([p[k] for p in per]) for k in per[0]}
    else:
        outs["u8"] = o["u8"]
        for k in ("f32", "yolo"):
            if k in o:
                outs[k] = o[k].reshape(B, case.n, case.H, case.W)
    dig = {k: slot_digests(v) for k, v in outs.items()}
    picked = {b: {k: v[b].copy() for k, v in outs.items()} for b in slots}
    return dig, picked


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_layer_every_slot_both_plans(case):
    rng = np.random.default_rng(sum(map(ord, case.name)))
    B = case.B
    x = rng.integers(0, 256, (B, case.c, case.H, case.W), dtype=np.uint8)
    L = Layer(case, rng)
    res = res_nchw = None
    if case.fuse == "shortcut":
        res_nchw = rng.integers(0, 256, (B, case.n, case.H, case.W), dtype=np.uint8)
    slots = chosen_slots(B, seed=len(case.name))

    def run(xb, rb, plan, epi, store, flags=0):
        r_t = binding.DevTensor.from_nchw(rb, L.zp_from) if rb is not None else None
        o, got = L.device(xb, r_t, plan, epi, store, flags)
        return _collect(case, L, o, rb, slots), got

    # ---- oracle on the chosen slots (both stores: the weights must make wrap and saturate differ)
    want = {binding.STORE_WRAP: {}, binding.STORE_SATURATE: {}}
    pad = case.k // 2
    for b in slots:
        acc = oracle.conv_acc(x[b], L.wq, L.zp_w, case.k, case.stride, pad, L.zp_in)
        OH, OW = (case.H + 2 * pad - case.k) // case.stride + 1, (case.W + 2 * pad - case.k) // case.stride + 1
        for store in want:
            u8 = oracle.requant(acc, L.bias, L.mv, L.sv, L.zp_act, oracle.ACT[case.act], store).reshape(case.n, OH, OW)
            f32 = oracle.dequant(u8, L.zp_act, L.s_act) if case.fuse in ("f32", "yolo") else None
            want[store][b] = _glue_host(case, L, u8, None if res_nchw is None else res_nchw[b], f32)
    wrapped = sum(int((want[0][b]["u8"] != want[1][b]["u8"]).sum()) for b in slots)
    assert wrapped > 0, "wrap and saturate give the same bytes: the weights do not exercise the store modes"

    def check_oracle(picked, store, what):
        for b in slots:
            for k, v in want[store][b].items():
                g = picked[b][k].reshape(v.shape)
                if k == "yolo":
                    np.testing.assert_allclose(g, v, rtol=0, atol=2e-7, err_msg=f"{what} slot {b} {k}")
                else:
                    assert np.array_equal(g, v), f"{what}: slot {b} {k} differs from the oracle"

    # (plan, epilogue hint) per store: every combination with the wrap store, the host's pairing with the saturating one
    combos = {binding.STORE_WRAP: [(0, False), (0, True), (1, False), (1, True)], binding.STORE_SATURATE: [(0, False), (1, True)]}
    base = {}
    for store, runs in combos.items():
        ref = None
        for plan, epi in runs:
            what = f"plan {plan} epilogue {epi} store {store}"
            if plan == 1 and case.refused_plan1:
                with pytest.raises(binding.MI355Error, match="code -22"):
                    L.device(x, None, plan, epi, store)
                # what the host runs instead: the plain convolution under this plan, the pool apart
                o = binding.conv_forward(binding.DevTensor.from_nchw(x, L.zp_in), L.wq, L.zp_w, case.k, L.bias, L.mv, L.sv, L.zp_in,
                                         L.zp_act, L.s_act, L.act, store=store, want_acc=False, plan=plan, epilogue=epi)
                got = (binding.last_conv_kernel(), binding.last_conv_launch())
                dig, picked = _collect(case, L, dict(o, glue=True), res_nchw, slots)
            else:
                (dig, picked), got = run(x, res_nchw, plan, epi, store)
            kern_want = case.kern[plan]
            if case.c == 16 and case.n == 32 and case.fuse == "pool2" and epi:
                kern_want = 7  # the epilogue hint sends 16 -> 32 + maxpool to conv_pool16.hip under both plans
            assert got[0] == kern_want, f"{what}: served by kernel {got[0]}, meant for {kern_want}"
            expect_geom(case, plan, got)
            check_oracle(picked, store, what)
            if ref is None:
                ref = dig
                check_can_fail(x, slots, dig["u8"], what)
            else:
                assert dig == ref, f"{what}: differs from plan 0 (some slot of some tensor)"
            if store == binding.STORE_WRAP and epi:
                base[plan] = dig
        if store == binding.STORE_WRAP and not (case.c == 3 and case.planar):
            # (the VALU first-layer kernels of the generic route read 4-byte cells only: the cs = 4 cases cover them)
            (dig, picked), got = run(x, res_nchw, 0, False, store, flags=GENERIC)
            assert got[0] == (1 if case.c == 3 else 5), f"generic route served by kernel {got[0]}"
            check_oracle(picked, store, "generic route")
            assert dig == ref, "the generic route differs from the specialised kernels"
    # ---- roll check: the batch rolled by r, both plans, as the host runs them (epilogue table, wrap store)
    for plan in (0, 1):
        if plan == 1 and case.refused_plan1:
            continue
        for r in (1, 5):
            (dr, _), _ = run(np.roll(x, r, axis=0), None if res_nchw is None else np.roll(res_nchw, r, axis=0), plan, True,
                             binding.STORE_WRAP)
            for k in base[plan]:
                check_roll(base[plan][k], dr[k], r, f"plan {plan} {k}")


# ----------------------------------------------------------------------------------------------- net level, bench settings
TINY_KERNELS = {
    0: {0: 1, 2: 7, 4: 2, 6: 2, 8: 4, 10: 4, 12: 5, 13: 3, 14: 4, 15: 3, 18: 3, 21: 5, 22: 3},  # test_gpu_parity.py batch-64 map
    # throughput plan: conv_ws3 declines the one-round 128 / 256-channel layers (the fused pools of 8 and 10 with it: the host runs
    # them unfused); the row-image kernel's 128 x 128 tiles serve them
    1: {0: 1, 2: 7, 4: 2, 6: 2, 8: 5, 10: 5, 12: 5, 13: 3, 14: 5, 15: 3, 18: 3, 21: 5, 22: 3},
}


# YOLOv3 @608, batch 32: the same kernels under both plans (every launch needs several rounds; test_gpu_residual.py runs it with one image)
V3_KERNELS = {0: 1, 1: 2, 2: 3, 3: 2, 5: 2, 6: 3, 7: 2, 9: 3, 10: 2, 12: 4, 13: 3, 14: 4, 16: 3, 17: 4, 19: 3, 20: 4, 22: 3, 23: 4, 25: 3,
              26: 4, 28: 3, 29: 4, 31: 3, 32: 4, 34: 3, 35: 4, 37: 4, 38: 3, 39: 4, 41: 3, 42: 4, 44: 3, 45: 4, 47: 3, 48: 4, 50: 3, 51: 4,
              53: 3, 54: 4, 56: 3, 57: 4, 59: 3, 60: 4, 62: 5, 63: 3, 64: 5, 66: 3, 67: 5, 69: 3, 70: 5, 72: 3, 73: 5, 75: 3, 76: 5, 77: 3,
              78: 5, 79: 3, 80: 5, 81: 3, 84: 3, 87: 5, 88: 4, 89: 3, 90: 4, 91: 3, 92: 4, 93: 3, 96: 3, 99: 5, 100: 4, 101: 3, 102: 4,
              103: 3, 104: 4, 105: 3}


def _pull_light(net, i):
    """one layer's stored tensors (uint8 NCHW, float) without the int32 copy Net.pull makes"""
    H = net.H
    H.pull_layer_output(net.h, i)
    inf = net.info[i]
    cnt = net.batch * inf["outputs"]
    out = {}
    if inf["type"] != binding.T_YOLO and not net.is_fused(i):
        out["u8"] = binding._as(H.dnq_layer_u8(net.h, i), cnt, C.c_uint8).reshape(net.batch, -1)
    if inf["type"] == binding.T_YOLO or (inf["quant_stop"] and (net.keep_head_float or inf["type"] != binding.T_CONV or not net.fuses_next(i))):
        out["f32"] = binding._as(H.dnq_layer_f32(net.h, i), cnt, C.c_float).reshape(net.batch, -1)
    return out


def _net_run(nets, slots):
    """every stored tensor of every net: ({layer: {key: digests}}, {layer: {key: {slot: array}}}) per net (slots of nets[0] only)"""
    digs = [dict() for _ in nets]
    picked = {}
    for i in range(nets[0].n):
        for k, nk in enumerate(nets):
            o = _pull_light(nk, i)
            digs[k][i] = {key: slot_digests(v) for key, v in o.items()}
            if k == 0:
                picked[i] = {key: {b: v[b].copy() for b in slots} for key, v in o.items()}
    return digs, picked


def _oracle_slots(cfg, wts, x, slots):
    onet = oracle.OracleNet(cfg, wts)
    onet.prepare(np.float32(1.0 / 255.0), 0)
    return {b: onet.forward(x[b], accum=oracle.ACC_EXACT) for b in slots}


def _check_net_vs_oracle(info, picked, want, what):
    n_checked = 0
    for i, keys in picked.items():
        for key, per in keys.items():
            for b, got in per.items():
                w = want[b][i][key].ravel()
                if info[i]["type"] == binding.T_YOLO:
                    np.testing.assert_allclose(got, w, rtol=0, atol=2e-7, err_msg=f"{what}: layer {i} slot {b} yolo")
                else:
                    assert np.array_equal(got, w), f"{what}: layer {i} {key} slot {b} differs from the oracle"
                n_checked += 1
    return n_checked


def _bench_like(cfg, wts, x, B, slots, want, kernels=None):
    """plan 0 alone (eager), then plan 1 as bench.py runs it: parent + two replicas with their own batches (the parent's rolled by
    1 and by 5), hipGraph capture + replay, queued without synchronisation in between"""
    info = None
    digs = {}
    for plan in (0, 1):
        net = binding.Net(cfg, wts, batch=B, use_graph=plan == 1)
        net.prepare_fixed(1.0 / 255.0, 0)
        nets = [net]
        if plan == 1:
            nets += [net.replica(), net.replica()]
        for nk, r in zip(nets, (0, 1, 5)):
            nk.push_input(np.roll(x, r, axis=0))
            nk.sync()
        for _ in range(2):  # capture, then replay
            for nk in nets:
                nk.forward()
        for nk in nets:
            nk.sync()
        info = net.info
        kern = {i: net.conv_kernel(i) for i, inf in enumerate(info) if inf["type"] == binding.T_CONV}
        if kernels is not None:
            assert kern == kernels[plan], f"plan {plan}: per-layer kernel map {kern}"
        for nk in nets[1:]:
            assert {i: nk.conv_kernel(i) for i in kern} == kern
        d, picked = _net_run(nets, slots)
        n = _check_net_vs_oracle(info, picked, want, f"plan {plan}")
        assert n > 0
        for k, r in enumerate((0, 1, 5)[:len(nets)]):
            for i in d[k]:
                for key in d[k][i]:
                    if r:
                        check_roll(d[0][i][key], d[k][i][key], r, f"plan {plan} layer {i} {key}")
        digs[plan] = d[0]
        for nk in reversed(nets):
            nk.close()
    # (under plan 1 the host runs conv + pool apart where the fused call is refused: those convs' own tensors exist only there)
    common = [(i, k) for i in digs[0] for k in digs[0][i] if k in digs[1].get(i, {})]
    assert len(common) >= len(info) // 2
    bad = [(i, k) for i, k in common if digs[0][i][k] != digs[1][i][k]]
    assert not bad, f"the plans disagree on {bad[:8]}"
    return info, digs[0]


@pytest.mark.parametrize("cfg_name", ["yolov3-tiny_quant.cfg", "yolov3-tiny_quant_relu6.cfg"])
def test_yolov3_tiny_416_batch64_every_slot_both_plans(tmp_path, cfg_name):
    cfg = os.path.join(ROOT, "cfg", cfg_name)
    wts = str(tmp_path / "w.weights")
    synth.synth_weights(cfg, wts, seed=1234)
    B = 64
    x = synth.synth_image_u8(3, 416, 416, seed=4242, batch=B)
    slots = chosen_slots(B, seed=17)
    want = _oracle_slots(cfg, wts, x, slots)
    info, d = _bench_like(cfg, wts, x, B, slots, want, TINY_KERNELS)
    for i, keys in d.items():
        if "u8" in keys:
            check_can_fail(x, slots, keys["u8"], f"layer {i}")


def test_yolov3_608_batch32_every_slot_both_plans(tmp_path):
    cfg = os.path.join(ROOT, "cfg", "yolov3_quant.cfg")
    wts = str(tmp_path / "w.weights")
    synth.synth_weights(cfg, wts, seed=21)
    B = 32
    x = synth.synth_image_u8(3, 608, 608, seed=2323, batch=B)
    slots = [0, B // 2, B - 1]
    want = _oracle_slots(cfg, wts, x, slots)
    info, d = _bench_like(cfg, wts, x, B, slots, want, {0: V3_KERNELS, 1: V3_KERNELS})
    assert sum(inf["type"] == binding.T_CONV for inf in info) == 75 and sum(inf["type"] == binding.T_SHORTCUT for inf in info) == 23
    for i, keys in d.items():
        if "u8" in keys:
            check_can_fail(x, slots, keys["u8"], f"layer {i}")
