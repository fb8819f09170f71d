"""GPU suite (`-m gpu`) for the classifier tail (classify.hip): the fully connected layer (kernel id 14) against the
oracle's dense convolution of the flattened input, the global average pool against exact integers, the refusals of both calls, and
cfg/cls_unit.cfg through the host, teacher-forced layer by layer."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle
from yolo_quantization_amd import binding, synth

pytestmark = pytest.mark.gpu
S_ACT = np.float32(0.05)
ACTS = ("leaky", "relu6", "linear", "relu")


@pytest.fixture(scope="module", autouse=True)
def device():
    binding.init(0)


def _consts(rng, n):
    bias = rng.integers(-3000, 3000, n).astype(np.int32)
    M = rng.uniform(2.0 ** -12, 2.0 ** -8, n)
    shift = np.floor(-np.log2(M)).astype(int)
    return bias, np.round(M * 2.0 ** shift * 2 ** 31) * 2.0 ** -31, 2.0 ** -shift.astype(np.float64)


def connected_acc(x, wq, zp_w, zp_in):
    """The layer's definition: the oracle's dense 1x1 convolution of the input flattened in (c, y, x) order.  x: [C, H, W] -> [n]"""
    return oracle.conv_acc(x.reshape(-1, 1, 1), wq, zp_w, 1, 1, 0, zp_in)[:, 0]


def _cells_1x1(t, u8):
    """(flat byte indices, stored bytes) of a [B, n] result in the B x n x 1 x 1 tensor t's buffer"""
    b, ch = np.meshgrid(np.arange(u8.shape[0]), np.arange(u8.shape[1]), indexing="ij")
    return ((t.lead + (b * 2 + 1) * 2) * t.cs + ch).ravel(), (u8 ^ 0x80).ravel()


# (label, C, H, W, n, B, zp_in, zp_w, data, grid); zp_w None: random per filter; grid: (workgroups, threads) of the main launch, where
# the case states it.  A K-step is 64 bytes of the tensor's cells, an M tile 16 filters, an N tile 16 images, a workgroup up to four M
# tiles and 64 images; K is split into slices of at least 8 K-steps until 256 workgroups are reached (kargs.h fc_split).
CASES = (
    [("K%d" % K, K, 1, 1, 17, 3, 7, None, "rand", None) for K in (16, 48, 64, 80, 1040)]
    + [("n%d" % n, 80, 1, 1, n, 3, 7, None, "rand", None) for n in (1, 15, 16, 17, 100)]
    + [("B%d" % B, 48, 1, 1, 17, B, 7, None, "rand", None) for B in (1, 15, 16, 17, 33, 65)]
    # flattening: spare channels inside every cell of a non-square map; whole cells on a 7 x 7 map
    + [("flat_24_2x3", 24, 2, 3, 17, 3, 9, None, "rand", None), ("flat_16_7x7", 16, 7, 7, 17, 3, 9, None, "rand", None)]
    # split-K: 7 K-steps are one slice (workspace NULL); 128 K-steps under one filter block are 16 slices of 8; 244 packed K-steps
    # under 8 filter blocks and 2 image groups are 16 slices of 16, each staged in two chunks (15 K-steps of 64 images fill 64 KB)
    + [("S1", 448, 1, 1, 16, 3, 9, None, "rand", (1, 64)), ("S16", 8192, 1, 1, 16, 3, 9, None, "rand", (16, 64)),
       ("chunks", 964, 4, 4, 512, 65, 9, None, "rand", (8 * 16 * 2, 256))]
    + [("zi%d_zw%d" % (zi, zw), 24, 2, 3, 17, 3, zi, zw, "rand", None) for zi in (0, 128, 255) for zw in (0, 128, 255)]
    # the accumulators' extremes -K 255^2 and +K 255^2 at the largest K; shift values that are no powers of two
    + [("neg", 33024, 1, 1, 16, 3, 255, 255, "neg", None), ("pos", 33024, 1, 1, 16, 3, 255, 0, "pos", None),
       ("shift", 24, 2, 3, 17, 3, 13, None, "shift", None)])


@pytest.mark.parametrize("case", range(len(CASES)), ids=lambda i: CASES[i][0])
def test_connected_vs_oracle_convolution_of_the_flattened_input(case):
    label, Cc, H, W, n, B, zp_in, zw, data, grid = CASES[case]
    rng = np.random.default_rng(4000 + case)
    K = Cc * H * W
    x = rng.integers(0, 256, (B, Cc, H, W), dtype=np.uint8)
    wq = rng.integers(0, 256, (n, K), dtype=np.uint8)
    zp_w = rng.integers(0, 256, n, dtype=np.uint8) if zw is None else np.full(n, zw, np.uint8)
    if data in ("neg", "pos"):
        x[:] = 255
        wq[:] = 0 if data == "neg" else 255
    bias, mv, sv = _consts(rng, n)
    if data == "shift":
        sv = sv * rng.uniform(0.55, 0.95, n)
    zp_act = int(rng.integers(0, 200))
    act = ACTS[case % 4]
    acc = np.stack([connected_acc(x[b], wq, zp_w, zp_in) for b in range(B)])
    if data in ("neg", "pos"):
        assert acc.min() == acc.max() == (-1 if data == "neg" else 1) * K * 255 * 255
    xt = binding.DevTensor.from_nchw(x, zp_in ^ 0x5A)  # pad cells and spare channels hold a byte no sum may contain
    for store in (binding.STORE_WRAP, binding.STORE_SATURATE):
        u8 = np.stack([oracle.requant(acc[b][:, None], bias, mv, sv, zp_act, oracle.ACT[act], store)[:, 0] for b in range(B)])
        y = binding.DevTensor(B, 1, 1, n, 77)
        want_buf = y.buf.to_numpy(np.uint8, y.buf.nbytes)
        idx, val = _cells_1x1(y.t, u8)
        want_buf[idx] = val
        for plan in (0, 1):
            got = binding.connected_forward(xt, wq, zp_w, bias, mv, sv, zp_in, zp_act, S_ACT, binding.ACT[act], store, want_acc=True,
                                            want_f32=True, plan=plan, y=y, workspace=None if label == "S1" else True)
            assert binding.last_conv_kernel() == 14
            if grid:
                assert binding.last_conv_launch()[:2] == grid
            assert np.array_equal(got["int32"], acc), "int32 accumulators"
            assert np.array_equal(got["f32"], oracle.dequant(u8, zp_act, S_ACT)), "quant_stop float tail"
            assert np.array_equal(y.buf.to_numpy(np.uint8, y.buf.nbytes), want_buf), "output buffer, pad cells and spare channels included"


def test_connected_on_a_channel_window_of_a_wider_tensor():
    """x is channels 16..40 of a 48-channel tensor (cells of 48 bytes, data 16 bytes in): the blob packed for cells of 32 serves it"""
    rng = np.random.default_rng(77)
    B, n = 3, 17
    big = rng.integers(0, 256, (B, 48, 2, 3), dtype=np.uint8)
    wq, zp_w = rng.integers(0, 256, (n, 24 * 6), dtype=np.uint8), rng.integers(0, 256, n, dtype=np.uint8)
    bias, mv, sv = _consts(rng, n)
    acc = np.stack([connected_acc(big[b, 16:40], wq, zp_w, 5) for b in range(B)])
    keep = binding.DevTensor.from_nchw(big, 5)
    win = object.__new__(binding.DevTensor)
    win.buf, win.t = keep.buf, binding.Tensor.from_buffer_copy(keep.t)
    win.t.C, win.t.data = 24, keep.t.data + 16
    assert win.t.cs == 48
    got = binding.connected_forward(win, wq, zp_w, bias, mv, sv, 5, 30, S_ACT, binding.ACT["leaky"])
    assert np.array_equal(got["int32"], acc)


def _tie_image(Cc, H, W):
    """channel ch sums to HW m + HW // 2 + (-1, 0, +1): around the rounding tie 2 S + HW = 0 (mod 2 HW) of an even HW, the nearest
    sums either side of it for an odd one"""
    hw = H * W
    img = np.zeros((Cc, hw), np.uint8)
    for ch in range(Cc):
        s = hw * (1 + 7 * ch % 253) + hw // 2 + ch % 3 - 1
        img[ch] = s // hw
        img[ch, :s % hw] += 1
    return img.reshape(Cc, H, W)


@pytest.mark.parametrize("Cc", [16, 24, 64, 80])
@pytest.mark.parametrize("H,W", [(1, 1), (1, 5), (7, 7), (13, 13), (16, 17), (64, 63)])
def test_avgpool_vs_exact_integers(H, W, Cc):
    rng = np.random.default_rng(H * 100 + W + Cc)
    x = np.stack([rng.integers(0, 256, (Cc, H, W), dtype=np.uint8), np.zeros((Cc, H, W), np.uint8), np.full((Cc, H, W), 255, np.uint8),
                  _tie_image(Cc, H, W)])
    s = x.reshape(4, Cc, -1).astype(np.int64).sum(axis=2)
    want = ((2 * s + H * W) // (2 * H * W)).astype(np.uint8)
    for fill in (0, 255):  # the pad cells of x: either value would change every mean of one of the images if it were read
        y = binding.DevTensor(4, 1, 1, Cc, 77)
        want_buf = y.buf.to_numpy(np.uint8, y.buf.nbytes)
        idx, val = _cells_1x1(y.t, want)
        want_buf[idx] = val
        got = binding.avgpool_forward(binding.DevTensor.from_nchw(x, fill), y)
        assert np.array_equal(got["u8"].reshape(4, Cc), want)
        assert np.array_equal(y.buf.to_numpy(np.uint8, y.buf.nbytes), want_buf), "output buffer, pad cells and spare channels included"


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("call,what,msg", [
    ("connected", dict(ksize=3), "ksize 1, stride 1, pad 0"), ("connected", dict(accum=1), "MI355_ACC_EXACT only"),
    ("connected", dict(act=0), "activation must be"), ("connected", dict(xcs=8), "multiple of 16"),
    ("connected", dict(c=100), "desc.c != x.C x.H x.W"), ("connected", dict(xC=33040, c=33040), "<= 33024"),
    ("connected", dict(yH=2), "B x n x 1 x 1"), ("connected", dict(xC=8192, c=8192), "workspace"),
    ("avgpool", dict(yH=2), "1 x 1 map"), ("avgpool", dict(yC=32), "x's B and C"), ("avgpool", dict(xcs=8), "multiple of 16"),
    ("avgpool", dict(xH=2049, xW=2048), "2^22 cells")])
def test_refusals_write_nothing(call, what, msg):
    S = binding.shim()
    x = binding.DevTensor(2, 2, 3, 16, 0)   # (the refusals precede every read: the descriptors below may lie about the buffer)
    y = binding.DevTensor(2, 1, 1, 16, 33)
    before = y.buf.to_numpy(np.uint8, y.buf.nbytes)
    xt, yt = binding.Tensor.from_buffer_copy(x.t), binding.Tensor.from_buffer_copy(y.t)
    xt.cs, xt.C, xt.H, xt.W = what.get("xcs", xt.cs), what.get("xC", xt.C), what.get("xH", xt.H), what.get("xW", xt.W)
    if "xC" in what:
        xt.H = xt.W = 1
        xt.cs = what["xC"]
    yt.H, yt.C = what.get("yH", 1), what.get("yC", 16)
    if call == "avgpool":
        rc = S.mi355_avgpool_forward(C.byref(xt), C.byref(yt), None)
    else:
        d = binding.ConvDesc(16, what.get("c", 96), what.get("ksize", 1), 1, 0, what.get("act", 9), 0, what.get("accum", 0), 0, 33, 0.05)
        rc = S.mi355_connected_forward(C.byref(d), C.byref(xt), binding.DevBuf(1 << 16).ptr, C.byref(yt), None, None, None, None)
    err = S.mi355_last_error().decode()
    assert rc == -22 and err.startswith("invalid argument: %s_forward:" % call) and msg in err
    assert np.array_equal(y.buf.to_numpy(np.uint8, y.buf.nbytes), before)


# ------------------------------------------------------------------------------------------------ through the host
@pytest.mark.parametrize("mode", ["latency", "throughput", "graph"])
def test_cls_unit_through_the_host_teacher_forced(mode, cfg_dir, tmp_path):
    """every layer of the tail equals its definition applied to the tensor the host handed it (no oracle net)"""
    cfg, wts, B = os.path.join(cfg_dir, "cls_unit.cfg"), str(tmp_path / "cls_unit.weights"), 3
    recs = {r["i"]: r for r in synth.synth_weights(cfg, wts, seed=3)["layers"]}
    net = binding.Net(cfg, wts, batch=B, use_graph=mode == "graph")
    net.set("plan", int(mode == "throughput"))
    net.prepare_from_float(synth.image_u8_to_float(synth.synth_image_u8(3, 20, 24, seed=5, batch=B)))
    for _ in range(3 if mode == "graph" else 1):  # a captured graph: several replays
        net.forward()
    net.sync()
    u8 = [net.pull(i)["u8"] for i in range(net.n)]
    x = u8[3].reshape(B, 40, -1).astype(np.int64)
    assert np.array_equal(u8[4].reshape(B, 40), (2 * x.sum(axis=2) + x.shape[2]) // (2 * x.shape[2]))
    assert (net.prep(4)["s_act"], net.prep(4)["zp_act"]) == (net.prep(3)["s_act"], net.prep(3)["zp_act"]), "the pool inherits its input's record"
    assert (net.prep(5)["s_in"], net.prep(5)["zp_in"]) == (net.prep(3)["s_act"], net.prep(3)["zp_act"]), "... and hands it on"
    for i in (5, 6):
        p, act = net.prep(i), ("leaky", "linear")[i - 5]
        assert net.conv_kernel(i) == 14 and net.info[i]["type"] == binding.T_CONNECTED
        acc = np.stack([connected_acc(u8[i - 1].reshape(B, -1, 1, 1)[b], recs[i]["weights_uint8"], recs[i]["zp_w"], p["zp_in"]) for b in range(B)])
        want = np.stack([oracle.requant(acc[b][:, None], p["biases_int32"], p["M_value"], p["shift_value"], p["zp_act"], oracle.ACT[act])[:, 0]
                         for b in range(B)])
        assert np.array_equal(u8[i].reshape(B, -1), want)
    assert np.array_equal(net.pull(6)["f32"].reshape(B, -1), oracle.dequant(want, p["zp_act"], p["s_act"])), "the float logits"


def test_cls_route_unit_views_routes_replica_and_packed_import(cfg_dir, tmp_path):
    """the tail among routes: a [connected] whose input is a window of a concat's buffer, routes over both layers (copies), then the
    same tensors from a replica beside its parent and after a packed import"""
    cfg, wts, B = os.path.join(cfg_dir, "cls_route_unit.cfg"), str(tmp_path / "cls_route.weights"), 3
    recs = {r["i"]: r for r in synth.synth_weights(cfg, wts, seed=4)["layers"]}
    x = synth.synth_image_u8(3, 5, 6, seed=9, batch=B)

    def pull_all(net):
        net.sync()
        return [net.pull(i)["u8"] for i in range(net.n)]

    parent = binding.Net(cfg, wts, batch=B)
    parent.prepare_fixed(1.0 / 255.0, 0)
    parent.push_input(x); parent.forward()
    u8 = pull_all(parent)
    assert parent.plan(1)["out_view"] == 1 and not any(parent.plan(i)["out_view"] for i in (2, 4, 5, 7))
    assert np.array_equal(u8[3].reshape(B, 32, -1), np.concatenate([u8[1].reshape(B, 16, -1), u8[0].reshape(B, 16, -1)], 1))
    m = u8[3].reshape(B, 32, -1).astype(np.int64)
    assert np.array_equal(u8[4].reshape(B, 32), (2 * m.sum(axis=2) + 30) // 60)
    assert np.array_equal(u8[5], u8[4]) and np.array_equal(u8[7], u8[2])
    for i, src, act in ((2, 1, "leaky"), (6, 5, "relu"), (8, 7, "linear")):
        p = parent.prep(i)
        acc = np.stack([connected_acc(u8[src].reshape(B, -1, 1, 1)[b], recs[i]["weights_uint8"], recs[i]["zp_w"], p["zp_in"]) for b in range(B)])
        want = np.stack([oracle.requant(acc[b][:, None], p["biases_int32"], p["M_value"], p["shift_value"], p["zp_act"], oracle.ACT[act])[:, 0]
                         for b in range(B)])
        assert np.array_equal(u8[i].reshape(B, -1), want), i
    packed = parent.export_packed()
    rep = parent.replica()
    rep.push_input(x); rep.forward()
    assert all(np.array_equal(g, w) for g, w in zip(pull_all(rep), u8)), "replica"
    rep.close()
    parent.close()
    imp = binding.Net(cfg, None, batch=B)
    imp.import_packed(packed)
    imp.push_input(x); imp.forward()
    assert all(np.array_equal(g, w) for g, w in zip(pull_all(imp), u8)), "packed import"
    imp.close()
