"""GPU suite (`-m gpu`) for the depthwise convolution (conv_dw.hip, kernel id 10): the kernel against the per-channel oracle through
the C-ABI, the plain-C host against the dense twin of the same net, and the C-ABI's refusals."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle
from yolo_quantization_amd import binding, synth

pytestmark = pytest.mark.gpu
B = 3
S_ACT = np.float32(0.05)


@pytest.fixture(scope="module", autouse=True)
def device():
    binding.init(0)


def _consts(rng, c):
    bias = rng.integers(-3000, 3000, c).astype(np.int32)
    M = rng.uniform(2.0 ** -9, 2.0 ** -5, c)
    shift = np.floor(-np.log2(M)).astype(int)
    return bias, np.round(M * 2.0 ** shift * 2 ** 31) * 2.0 ** -31, 2.0 ** -shift.astype(np.float64)


# (C, H, W, k, stride, pad, zp_in, zp_w, act, plan, data); zp_w None: random per channel.  Tiles are 16 x 8, 8 x 16 or 4 x 32 output
# pixels (TH x TW, the one with the fewest tiles), channel chunks 64 wide.
CASES = [
    # channel counts: a ragged dword, cs above C, more than one chunk
    (16, 5, 7, 3, 1, 1, 7, None, "leaky", 0, "rand"), (17, 5, 7, 3, 1, 1, 7, None, "leaky", 1, "rand"),
    (64, 5, 7, 3, 1, 1, 7, None, "relu6", 0, "rand"), (65, 5, 7, 3, 1, 1, 7, None, "linear", 1, "rand"),
    (80, 5, 7, 5, 1, 2, 7, None, "leaky", 0, "rand"),
    # maps around every tile's edges
    (16, 1, 1, 3, 1, 1, 9, None, "leaky", 0, "rand"), (16, 2, 2, 3, 1, 1, 9, None, "leaky", 1, "rand"),
    (16, 15, 9, 3, 1, 1, 9, None, "leaky", 0, "rand"), (16, 16, 8, 3, 1, 1, 9, None, "relu6", 1, "rand"),
    (16, 17, 7, 3, 1, 1, 9, None, "linear", 0, "rand"), (16, 7, 17, 3, 1, 1, 9, None, "leaky", 1, "rand"),
    (16, 8, 16, 5, 1, 2, 9, None, "leaky", 0, "rand"), (16, 9, 15, 3, 1, 1, 9, None, "leaky", 0, "rand"),
    (16, 3, 33, 3, 1, 1, 9, None, "leaky", 1, "rand"), (16, 4, 32, 3, 1, 1, 9, None, "leaky", 0, "rand"),
    (16, 5, 31, 5, 1, 2, 9, None, "relu6", 1, "rand"), (16, 33, 17, 3, 1, 1, 9, None, "leaky", 0, "rand"),
    # sizes and paddings: 3x3 pad 0, 7x7 / 1x1 / 11x11 / 2x2 (the runtime-size path), padding above size / 2
    (17, 9, 10, 3, 1, 0, 11, None, "leaky", 0, "rand"), (17, 9, 10, 7, 1, 3, 11, None, "leaky", 1, "rand"),
    (17, 9, 10, 1, 1, 0, 11, None, "linear", 0, "rand"), (16, 6, 5, 11, 1, 5, 11, None, "leaky", 0, "rand"),
    (17, 9, 10, 3, 1, 2, 11, None, "relu6", 1, "rand"), (16, 9, 10, 2, 1, 1, 11, None, "leaky", 0, "rand"),
    (16, 3, 3, 5, 1, 4, 11, None, "leaky", 0, "rand"),
    # strides: 2 on odd and even maps, 3, stride 2 on the runtime-size path
    (17, 17, 19, 3, 2, 1, 13, None, "leaky", 0, "rand"), (64, 18, 20, 3, 2, 1, 13, None, "leaky", 1, "rand"),
    (16, 17, 18, 5, 2, 2, 13, None, "relu6", 0, "rand"), (16, 20, 19, 3, 3, 1, 13, None, "leaky", 1, "rand"),
    (16, 19, 20, 7, 2, 3, 13, None, "linear", 0, "rand"), (16, 35, 9, 3, 2, 0, 13, None, "leaky", 1, "rand"),
    # zero points at both ends
    (16, 6, 9, 3, 1, 1, 0, 0, "leaky", 0, "rand"), (16, 6, 9, 3, 1, 1, 0, 255, "leaky", 0, "rand"),
    (16, 6, 9, 3, 1, 1, 128, 0, "relu6", 1, "rand"), (16, 6, 9, 3, 1, 1, 128, 255, "linear", 0, "rand"),
    (16, 6, 9, 5, 1, 2, 255, 0, "leaky", 1, "rand"), (16, 6, 9, 5, 1, 2, 255, 255, "leaky", 0, "rand"),
    # the accumulators' extremes: -K 255^2 and +K 255^2
    (16, 6, 9, 3, 1, 1, 255, 255, "leaky", 0, "neg"), (16, 6, 9, 3, 1, 1, 255, 0, "leaky", 0, "pos"),
    (16, 13, 4, 11, 1, 5, 255, 255, "linear", 1, "neg"), (16, 13, 4, 11, 1, 5, 255, 0, "relu6", 0, "pos"),
]
REF_F32 = {7, 24}  # these two also in MI355_ACC_REF_F32: the same integers


def _cell_bytes(t, u8):
    """(flat byte indices, biased bytes) of a [B, C, OH, OW] result in tensor t's buffer"""
    Bn, Cn, H, W = u8.shape
    b, ch, y, x = np.meshgrid(np.arange(Bn), np.arange(Cn), np.arange(H), np.arange(W), indexing="ij")
    return ((t.lead + (b * (H + 1) + y + 1) * (W + 1) + x) * t.cs + ch).ravel(), (u8 ^ 0x80).ravel()


@pytest.mark.parametrize("case", range(len(CASES)), ids=lambda i: "C%d_%dx%d_k%d_s%d_p%d_zi%d_zw%s_%s_plan%d_%s" % CASES[i])
def test_kernel_vs_per_channel_oracle(case):
    Cn, H, W, k, s, pad, zp_in, zw, act, plan, data = CASES[case]
    rng = np.random.default_rng(1000 + case)
    x = rng.integers(0, 256, (B, Cn, H, W), dtype=np.uint8)
    wq = rng.integers(0, 256, (Cn, k * k), dtype=np.uint8)
    zp_w = rng.integers(0, 256, Cn, dtype=np.uint8) if zw is None else np.full(Cn, zw, np.uint8)
    if data != "rand":
        x[:] = 255
        wq[:] = 0 if data == "neg" else 255
    bias, mv, sv = _consts(rng, Cn)
    zp_act = int(rng.integers(0, 200))
    OH, OW = (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1
    acc = np.stack([np.concatenate([oracle.conv_acc(x[b, j:j + 1], wq[j:j + 1], zp_w[j:j + 1], k, s, pad, zp_in) for j in range(Cn)])
                    for b in range(B)])
    if data != "rand":
        assert acc.min() == acc.max() == (-1 if data == "neg" else 1) * k * k * 255 * 255
    xt = binding.DevTensor.from_nchw(x, zp_in)
    for store in (binding.STORE_WRAP, binding.STORE_SATURATE):
        u8 = np.stack([oracle.requant(acc[b], bias, mv, sv, zp_act, oracle.ACT[act], store) for b in range(B)])
        y = binding.DevTensor(B, OH, OW, Cn, 77)
        want_buf = y.buf.to_numpy(np.uint8, y.buf.nbytes)
        idx, val = _cell_bytes(y.t, u8.reshape(B, Cn, OH, OW))
        want_buf[idx] = val
        for accum in [binding.ACC_EXACT] + ([binding.ACC_REF_F32] if case in REF_F32 else []):
            got = binding.conv_dw_forward(xt, wq, zp_w, k, bias, mv, sv, zp_in, zp_act, S_ACT, binding.ACT[act], store, accum,
                                          want_acc=True, want_f32=True, stride=s, pad=pad, plan=plan, y=y)
            assert binding.last_conv_kernel() == 10
            assert np.array_equal(got["int32"], acc), "int32 accumulators"
            assert np.array_equal(got["f32"], oracle.dequant(u8, zp_act, S_ACT)), "quant_stop float tail"
            assert np.array_equal(y.buf.to_numpy(np.uint8, y.buf.nbytes), want_buf), "output buffer, pad cells and spare channels included"


def test_shift_value_not_a_power_of_two():
    """The two-step requant_u8 branch: shift_value that is no exact power of two (the reference's prep never makes one, a caller may)."""
    rng = np.random.default_rng(5)
    x = rng.integers(0, 256, (B, 17, 9, 10), dtype=np.uint8)
    wq = rng.integers(0, 256, (17, 9), dtype=np.uint8)
    zp_w = rng.integers(0, 256, 17, dtype=np.uint8)
    bias, mv, sv = _consts(rng, 17)
    sv = sv * rng.uniform(0.55, 0.95, 17)
    xt = binding.DevTensor.from_nchw(x, 11)
    for act in ("leaky", "relu6", "linear"):
        got = binding.conv_dw_forward(xt, wq, zp_w, 3, bias, mv, sv, 11, 23, S_ACT, binding.ACT[act], stride=1, pad=1)
        for b in range(B):
            acc = np.concatenate([oracle.conv_acc(x[b, j:j + 1], wq[j:j + 1], zp_w[j:j + 1], 3, 1, 1, 11) for j in range(17)])
            assert np.array_equal(got["u8"][b].reshape(17, -1), oracle.requant(acc, bias, mv, sv, 23, oracle.ACT[act])), act


# ------------------------------------------------------------------------------------------------ host against the dense twin
def _pull_all(net):
    net.sync()
    return [net.pull(i) for i in range(net.n)]


def _same(got, want, what, skip=()):
    for i, (g, w) in enumerate(zip(got, want)):
        for key in w:
            if key not in skip:
                assert np.array_equal(g[key], w[key]), (what, i, key)


def test_host_net_equals_its_dense_twin(cfg_dir, tmp_path):
    """dw_unit through the plain-C host equals the same net with `groups` removed and the weights expanded with the zero-point fill
    (DESIGN.md 7b): every tensor, as parity dump, latency plan, graph replay, throughput plan and a replica beside its parent; the
    detections; a packed export imported into a fresh net."""
    cfg = os.path.join(cfg_dir, "dw_unit.cfg")
    twin_cfg = str(tmp_path / "twin.cfg")
    with open(twin_cfg, "w") as f:
        f.write("".join(line for line in open(cfg) if not line.startswith("groups=")))
    wts, twin_wts = str(tmp_path / "dw.weights"), str(tmp_path / "twin.weights")
    synth.synth_weights(cfg, wts, seed=4)
    synth.synth_weights(cfg, twin_wts, seed=4, dense_twin=True)
    x = synth.synth_image_u8(3, 24, 24, seed=21, batch=B)
    x2 = synth.synth_image_u8(3, 24, 24, seed=22, batch=B)

    def run(c, w, xin, **kw):
        net = binding.Net(c, w, batch=B, **kw)
        net.prepare_fixed(1.0 / 255.0, 0)
        net.push_input(xin); net.forward()
        if kw.get("use_graph"):
            net.forward(); net.forward()
        return net, _pull_all(net)

    twin, want_dump = run(twin_cfg, twin_wts, x, dump_int32=True)
    twin.close()
    twin, want = run(twin_cfg, twin_wts, x)
    want_det = twin.detections_batch(24, 24, 0.0)
    twin.close()
    twin, want2 = run(twin_cfg, twin_wts, x2)
    twin.close()

    net, got = run(cfg, wts, x, dump_int32=True)
    _same(got, want_dump, "parity dump")
    dw = [1, 3, 5]  # the cfg's depthwise layers
    assert [net.conv_kernel(i) for i in dw] == [10, 10, 10]
    assert not any(net.plan(i)[key] for i in dw for key in binding.PLAN_KEYS[3:8]), "a depthwise layer is offered to no fusion"
    net.close()
    net, got = run(cfg, wts, x, use_graph=True)
    _same(got, want, "graph replay", skip=("int32",))
    net.close()
    parent, got = run(cfg, wts, x)
    _same(got, want, "latency plan", skip=("int32",))
    for a, b_ in zip(parent.detections_batch(24, 24, 0.0), want_det):
        assert np.array_equal(a, b_), "detections"
    packed = parent.export_packed()
    rep = parent.replica()  # switches the parent to the throughput plan
    rep.push_input(x2); parent.push_input(x)
    rep.sync(); parent.sync()
    for _ in range(3):
        rep.forward(); parent.forward()
    _same(_pull_all(parent), want, "throughput plan, parent", skip=("int32",))
    _same(_pull_all(rep), want2, "replica", skip=("int32",))
    rep.close()
    parent.close()
    imp = binding.Net(cfg, None, batch=B)
    imp.import_packed(packed)
    imp.push_input(x); imp.forward()
    _same(_pull_all(imp), want, "packed import", skip=("int32",))
    imp.close()


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("n,c,k,cs,msg", [(32, 16, 3, 16, "desc.n == desc.c"), (16, 16, 3, 4, "multiple of 16"), (16, 16, 12, 16, "1..11")])
def test_refusals_write_nothing(n, c, k, cs, msg):
    S = binding.shim()
    x = binding.DevTensor(1, 6, 6, 16, 0)
    y = binding.DevTensor(1, 6, 6, n, 33)
    before = y.buf.to_numpy(np.uint8, y.buf.nbytes)
    xt = binding.Tensor.from_buffer_copy(x.t)
    xt.cs = cs
    d = binding.ConvDesc(n, c, k, 1, k // 2, binding.ACT["leaky"], 0, 0, 0, 33, 0.05)
    blob = binding.DevBuf(1 << 16)
    assert S.mi355_conv_dw_forward(C.byref(d), C.byref(xt), blob.ptr, y.ref(), None, None, None) == -22
    assert msg in S.mi355_last_error().decode()
    assert np.array_equal(y.buf.to_numpy(np.uint8, y.buf.nbytes), before)
