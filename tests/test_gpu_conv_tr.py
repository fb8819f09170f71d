"""GPU suite (`-m gpu`) for the transposed convolution (conv_tr.hip, kernel id 11): the phase-split kernel through the C-ABI against
its stuffed dense twin built in numpy and run through the oracle, and the C-ABI's refusals."""
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


def _consts(rng, n):
    bias = rng.integers(-3000, 3000, n).astype(np.int32)
    M = rng.uniform(2.0 ** -12, 2.0 ** -8, n)
    shift = np.floor(-np.log2(M)).astype(int)
    return bias, np.round(M * 2.0 ** shift * 2 ** 31) * 2.0 ** -31, 2.0 ** -shift.astype(np.float64)


def twin_acc(x, w, zp_w, k, s, p, zp_in):
    """The layer's definition: the dense stride-1 convolution of the zero-point-stuffed map with the flipped weights.
    x: [c, H, W], w: [c, n, k, k] -> int32 [n, OH * OW]"""
    c, H, W = x.shape
    xh = np.full((c, (H - 1) * s + 1, (W - 1) * s + 1), zp_in, np.uint8)
    xh[:, ::s, ::s] = x
    wh = np.ascontiguousarray(w.transpose(1, 0, 2, 3)[:, :, ::-1, ::-1]).reshape(w.shape[1], -1)
    return oracle.conv_acc(xh, wh, zp_w, k, 1, k - 1 - p, zp_in)


# (c, n, H, W, k, s, p, zp_in, zp_w, act, data); zp_w None: random per filter.  A tile is 32 x 8, 16 x 16 or 8 x 32 quotients
# ((o + p) // s, one more than H for k4 s2 p1) by 32 or 64 filters; 64 quotients (8 x 8, 4 x 16 or 2 x 32 by the same width rule) by
# 128 filters when the channels of the larger tile do not fit in LDS, and 8 x 8 on chunks of 30 channel units when those do not either.
CASES = [
    # phases: one tap each; the usual x2 layer; 2 and 1 taps; the flipped dense layer; phases without a tap (the pure constant);
    # three phases per side; the largest size; padding at both ends of its range; the largest stride
    (16, 16, 5, 6, 2, 2, 0, 7, None, "leaky", "rand"), (17, 33, 5, 6, 4, 2, 1, 7, None, "leaky", "rand"),
    (16, 16, 5, 6, 3, 2, 1, 7, None, "relu6", "rand"), (16, 16, 5, 6, 3, 1, 1, 7, None, "linear", "rand"),
    (16, 16, 5, 6, 1, 2, 0, 7, None, "leaky", "rand"), (16, 16, 4, 5, 2, 3, 0, 7, None, "relu", "rand"),
    (16, 16, 4, 5, 5, 3, 2, 7, None, "leaky", "rand"), (16, 16, 3, 4, 11, 2, 5, 7, None, "leaky", "rand"),
    (16, 16, 5, 6, 3, 2, 0, 7, None, "leaky", "rand"), (16, 16, 5, 6, 4, 2, 3, 7, None, "relu6", "rand"),
    (16, 16, 3, 3, 3, 8, 1, 7, None, "leaky", "rand"),
    # channels and filters: unit pairs plus an odd unit, one filter; 3 filters (4-byte plain cells); more filters than the largest M
    # tile; the 128-filter tile on 64 quotients; channel chunks (30 units, then a pair and an odd unit)
    (80, 1, 5, 6, 4, 2, 1, 9, None, "leaky", "rand"), (17, 3, 5, 6, 3, 2, 1, 9, None, "leaky", "rand"),
    (32, 129, 5, 6, 2, 2, 0, 9, None, "leaky", "rand"), (240, 130, 3, 3, 11, 1, 5, 9, None, "linear", "rand"),
    (520, 1, 3, 3, 11, 1, 5, 9, None, "leaky", "rand"),
    # maps: single rows and columns, and each tile side at -1, 0, +1
    (16, 16, 1, 1, 4, 2, 1, 11, None, "leaky", "rand"), (16, 16, 1, 5, 4, 2, 1, 11, None, "leaky", "rand"),
    (16, 16, 5, 1, 4, 2, 1, 11, None, "leaky", "rand"), (16, 16, 14, 14, 4, 2, 1, 11, None, "leaky", "rand"),
    (16, 16, 15, 15, 4, 2, 1, 11, None, "relu6", "rand"), (16, 16, 16, 15, 4, 2, 1, 11, None, "leaky", "rand"),
    (16, 16, 15, 16, 4, 2, 1, 11, None, "leaky", "rand"), (16, 16, 7, 30, 4, 2, 1, 11, None, "leaky", "rand"),
    (16, 16, 8, 31, 4, 2, 1, 11, None, "linear", "rand"), (16, 16, 6, 32, 4, 2, 1, 11, None, "leaky", "rand"),
    (16, 16, 31, 6, 4, 2, 1, 11, None, "leaky", "rand"), (16, 16, 32, 7, 4, 2, 1, 11, None, "leaky", "rand"),
    (16, 16, 30, 7, 4, 2, 1, 11, None, "leaky", "rand"),
] + [
    # zero points at both ends and in the middle
    (16, 16, 4, 5, 3, 2, 1, zi, zw, "leaky", "rand") for zi in (0, 128, 255) for zw in (0, 128, 255)
] + [
    # the accumulators' extremes: -K 255^2 and +K 255^2 (K = c k k: the stuffed cells are 255 as well)
    (16, 16, 4, 5, 4, 2, 1, 255, 255, "leaky", "neg"), (16, 16, 4, 5, 4, 2, 1, 255, 0, "leaky", "pos"),
    # shift values that are no powers of two
    (17, 16, 4, 5, 4, 2, 1, 13, None, "leaky", "shift"),
]


def _cell_bytes(t, u8):
    """(flat byte indices, stored bytes) of a [B, n, OH, OW] result in tensor t's buffer (4-byte cells hold plain bytes)"""
    Bn, Cn, H, W = u8.shape
    b, ch, y, x = np.meshgrid(np.arange(Bn), np.arange(Cn), np.arange(H), np.arange(W), indexing="ij")
    return ((t.lead + (b * (H + 1) + y + 1) * (W + 1) + x) * t.cs + ch).ravel(), (u8 ^ (0 if t.cs == 4 else 0x80)).ravel()


@pytest.mark.parametrize("case", range(len(CASES)), ids=lambda i: "c%d_n%d_%dx%d_k%d_s%d_p%d_zi%d_zw%s_%s_%s" % CASES[i])
def test_kernel_vs_stuffed_twin(case):
    c, n, H, W, k, s, p, zp_in, zw, act, data = CASES[case]
    rng = np.random.default_rng(2000 + case)
    x = rng.integers(0, 256, (B, c, H, W), dtype=np.uint8)
    w = rng.integers(0, 256, (c, n, k, k), dtype=np.uint8)
    zp_w = rng.integers(0, 256, n, dtype=np.uint8) if zw is None else np.full(n, zw, np.uint8)
    if data in ("neg", "pos"):
        x[:] = 255
        w[:] = 0 if data == "neg" else 255
    bias, mv, sv = _consts(rng, n)
    if data == "shift":
        sv = sv * rng.uniform(0.55, 0.95, n)
    zp_act = int(rng.integers(0, 200))
    OH, OW = (H - 1) * s + k - 2 * p, (W - 1) * s + k - 2 * p
    acc = np.stack([twin_acc(x[b], w, zp_w, k, s, p, zp_in) for b in range(B)])
    assert acc.shape == (B, n, OH * OW)
    if data in ("neg", "pos"):
        assert acc.min() == acc.max() == (-1 if data == "neg" else 1) * c * k * k * 255 * 255
    xt = binding.DevTensor.from_nchw(x, zp_in)
    for store in (binding.STORE_WRAP, binding.STORE_SATURATE):
        u8 = np.stack([oracle.requant(acc[b], bias, mv, sv, zp_act, oracle.ACT[act], store) for b in range(B)])
        y = binding.DevTensor(B, OH, OW, n, 77)
        want_buf = y.buf.to_numpy(np.uint8, y.buf.nbytes)
        idx, val = _cell_bytes(y.t, u8.reshape(B, n, OH, OW))
        want_buf[idx] = val
        for plan in (0, 1):
            got = binding.conv_tr_forward(xt, w, zp_w, k, s, p, bias, mv, sv, zp_in, zp_act, S_ACT, binding.ACT[act], store,
                                          want_acc=True, want_f32=True, plan=plan, y=y)
            assert binding.last_conv_kernel() == 11
            assert np.array_equal(got["int32"], acc), "int32 accumulators"
            assert np.array_equal(got["f32"], oracle.dequant(u8, zp_act, S_ACT)), "quant_stop float tail"
            assert np.array_equal(y.buf.to_numpy(np.uint8, y.buf.nbytes), want_buf), "output buffer, pad cells and spare channels included"


# ------------------------------------------------------------------------------------------------ the host net
def _pull_all(net):
    net.sync()
    return [net.pull(i) for i in range(net.n)]


def _same(got, want, what, skip=()):
    for i, (g, w) in enumerate(zip(got, want)):
        for key in w:
            if key not in skip:
                assert np.array_equal(g[key], w[key]), (what, i, key)


def test_host_net_tr_unit(cfg_dir, tmp_path):
    """tr_unit through the plain-C host: in the parity dump each [deconvolutional] layer's int32 and bytes equal the stuffed twin computed
    from the pulled input and the host's prep; every tensor of the dump again under the latency plan, graph replay, the throughput plan
    with a replica beside its parent, and after a packed import."""
    cfg, wts = os.path.join(cfg_dir, "tr_unit.cfg"), str(tmp_path / "tr.weights")
    recs = {r["i"]: r for r in synth.synth_weights(cfg, wts, seed=6)["layers"]}
    x = synth.synth_image_u8(3, 24, 24, seed=31, batch=B)
    x2 = synth.synth_image_u8(3, 24, 24, seed=32, batch=B)

    def run(xin, **kw):
        net = binding.Net(cfg, wts, batch=B, **kw)
        net.prepare_fixed(1.0 / 255.0, 0)
        net.push_input(xin); net.forward()
        if kw.get("use_graph"):
            net.forward(); net.forward()
        return net, _pull_all(net)

    net, want2 = run(x2, dump_int32=True)
    net.close()
    net, want = run(x, dump_int32=True)
    for i in (1, 3):
        inf, pr = net.info[i], net.prep(i)
        assert inf["type"] == binding.T_DECONV and net.conv_kernel(i) == 11
        assert not any(net.plan(j)[key] for j in (i - 1, i) for key in binding.PLAN_KEYS[3:8]), "no fusion with or of a transposed layer"
        xin = want[i - 1]["u8"].reshape(B, inf["c"], inf["h"], inf["w"])
        acc = np.stack([twin_acc(xin[b], recs[i]["weights_uint8"], recs[i]["zp_w"], inf["size"], inf["stride"], inf["pad"], pr["zp_in"])
                        for b in range(B)])
        assert np.array_equal(want[i]["int32"], acc.ravel()), (i, "int32 against the twin")
        u8 = np.stack([oracle.requant(a, pr["biases_int32"], pr["M_value"], pr["shift_value"], pr["zp_act"], inf["activation"]) for a in acc])
        assert np.array_equal(want[i]["u8"], u8.ravel()), (i, "bytes against the twin")
    net.close()
    net, got = run(x, use_graph=True)
    _same(got, want, "graph replay", skip=("int32",))
    net.close()
    parent, got = run(x)
    _same(got, want, "latency plan", skip=("int32",))
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
@pytest.mark.parametrize("k,s,p,cs,accum,act,msg", [
    (3, 2, 3, 16, 0, "leaky", "0 <= pad <= size - 1"), (3, 9, 1, 16, 0, "leaky", "stride must be 1..8"),
    (12, 2, 1, 16, 0, "leaky", "size must be 1..11"), (3, 2, 1, 4, 0, "leaky", "multiple of 16"),
    (3, 2, 1, 16, 1, "leaky", "MI355_ACC_EXACT only"), (3, 2, 1, 16, 0, None, "activation must be"),
    (2, 1, 1, 16, 0, "leaky", "output map"), (3, 2, 1, 32, 0, "leaky", "x.C != desc.c")])  # 1 x 1 input: OH = 0; desc.c = 32 on 16 channels
def test_refusals_write_nothing(k, s, p, cs, accum, act, msg):
    S = binding.shim()
    hw = 1 if msg == "output map" else 4
    x = binding.DevTensor(1, hw, hw, 16, 0)
    OH = (hw - 1) * s + k - 2 * p
    y = binding.DevTensor(1, max(OH, 1), max(OH, 1), 16, 33)
    before = y.buf.to_numpy(np.uint8, y.buf.nbytes)
    xt = binding.Tensor.from_buffer_copy(x.t)
    xt.cs = cs
    d = binding.ConvDesc(16, cs if cs == 32 else 16, k, s, p, binding.ACT[act] if act else 0, 0, accum, 0, 33, 0.05)  # (0: logistic in the reference's enum)
    blob = binding.DevBuf(1 << 16)
    assert S.mi355_conv_tr_forward(C.byref(d), C.byref(xt), blob.ptr, y.ref(), None, None, None) == -22
    assert msg in S.mi355_last_error().decode()
    assert np.array_equal(y.buf.to_numpy(np.uint8, y.buf.nbytes), before)
