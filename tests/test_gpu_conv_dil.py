"""GPU suite (`-m gpu`) for the dilated convolution (conv_dil.hip, kernel id 13): the phase-gathered kernel through the C-ABI against
the numpy definition, its two identities against the dense call, the C-ABI's refusals, and cfg/dil_unit.cfg through
the plain-C host."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle
from test_conv_dil_cpu import BRANCHES, dil_acc, stuffed_twin
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


# (c, n, H, W, k, d, p, zp_in, zp_w, data); zp_w None: random per filter.  A workgroup takes 256 pixels (64 in the fallback) as G phase
# tiles of th x tw phase indices, tw = min(32, p2(ceil(OW / d))), by 32 | 64 (128) filters; LDS = 512 + G (th + k - 1)(tw + k - 1) unit.
WIDTHS = (63, 64, 65, 66)
CASES = (
    # phases of unequal size, pad below / no multiple of / above d; d beyond the map (every output its own phase)
    [(16, 16, 5, 6, 3, 2, p, 7, None, "lds9728" if p == 2 else "rand") for p in (0, 1, 2, 3)] + [(16, 16, 5, 6, 3, 7, 7, 7, None, "rand")]
    # sizes, and d = 1 (the dense layer)
    + [(16, 16, 5, 6, 2, 3, 1, 9, None, "rand"), (16, 16, 9, 9, 5, 2, 4, 9, None, "rand"), (16, 16, 3, 4, 11, 2, 10, 9, None, "rand"),
       (16, 16, 5, 6, 3, 1, 1, 9, None, "rand"), (8, 16, 7, 6, 4, 1, 2, 9, None, "rand")]
    # tile edges: phase images 31 | 32 | 33 wide (33: a second tile column) and as tall
    + [(16, 16, 5, w, 3, 2, 2, 11, None, "lds7040" if w == 66 else "rand") for w in WIDTHS]
    + [(16, 16, h, 5, 3, 2, 2, 11, None, "rand") for h in WIDTHS]
    # ASPP
    + [(32, 32, 33, 33, 3, d, d, 13, None, "rand") for d in (6, 12, 18)]
    # channels: units 4, 8, 16 and a one-channel last chunk; filters: the n % 4 store tail, more than one M group in both forms
    + [(c, 16, 5, 6, 3, 2, 2, 5, None, "rand") for c in (3, 8, 17, 40)]
    + [(16, n, 5, 6, 3, 2, 2, 5, None, "rand") for n in (5, 32, 33, 65, 130)]
    # the 64-pixel form: 512 + 64 * 121 * 16 bytes, where 256 pixels would need 496 128; 130 filters are two M groups of it
    + [(16, 16, 3, 3, 11, 20, 100, 9, None, "lds124416"), (16, 130, 3, 3, 11, 20, 100, 9, None, "lds124416")]
    # zero points at both ends and in the middle
    + [(16, 16, 4, 5, 3, 2, 2, zi, zw, "rand") for zi in (0, 128, 255) for zw in (0, 128, 255)]
    # the accumulators' extremes, -c k^2 255^2 and +c k^2 255^2; shift values that are no powers of two
    + [(16, 16, 4, 5, 3, 2, 2, 255, 255, "neg"), (16, 16, 4, 5, 3, 2, 2, 255, 0, "pos"), (24, 48, 4, 5, 3, 2, 2, 13, None, "shift")])
ACTS = ("leaky", "relu6", "linear", "relu")


def _cell_bytes(t, u8):
    """(flat byte indices, stored bytes) of a [B, n, OH, OW] result in tensor t's buffer"""
    Bn, Cn, H, W = u8.shape
    b, ch, y, x = np.meshgrid(np.arange(Bn), np.arange(Cn), np.arange(H), np.arange(W), indexing="ij")
    return ((t.lead + (b * (H + 1) + y + 1) * (W + 1) + x) * t.cs + ch).ravel(), (u8 ^ 0x80).ravel()


@pytest.mark.parametrize("case", range(len(CASES)), ids=lambda i: "c%d_n%d_%dx%d_k%d_d%d_p%d_zi%d_zw%s_%s" % CASES[i])
def test_kernel_vs_the_definition(case):
    c, n, H, W, k, d, p, zp_in, zw, data = CASES[case]
    act = ACTS[case % 4]
    rng = np.random.default_rng(4000 + case)
    x = rng.integers(0, 256, (B, c, H, W), dtype=np.uint8)
    wq = rng.integers(0, 256, (n, c * k * k), dtype=np.uint8)
    zp_w = rng.integers(0, 256, n, dtype=np.uint8) if zw is None else np.full(n, zw, np.uint8)
    if data in ("neg", "pos"):
        x[:] = 255
        wq[:] = 0 if data == "neg" else 255
    bias, mv, sv = _consts(rng, n)
    if data == "shift":
        sv = sv * rng.uniform(0.55, 0.95, n)
    zp_act = int(rng.integers(0, 200))
    OH, OW = H + 2 * p - d * (k - 1), W + 2 * p - d * (k - 1)
    acc = np.stack([dil_acc(x[b], wq, zp_w, k, d, p, zp_in) for b in range(B)])
    if data in ("neg", "pos"):
        assert acc.min() == acc.max() == (-1 if data == "neg" else 1) * c * k * k * 255 * 255
    # (c = 3 in 16-byte cells, not the image's 4-byte ones: a wider tensor seen as 3 channels, the 4th byte of the unit not zero)
    xt = binding.DevTensor.from_nchw(np.concatenate([x, 255 - x[:, :1]], 1) if c == 3 else x, zp_in)
    xt.t.C = c
    for store in (binding.STORE_WRAP, binding.STORE_SATURATE):
        u8 = np.stack([oracle.requant(acc[b], bias, mv, sv, zp_act, oracle.ACT[act], store) for b in range(B)]).reshape(B, n, OH, OW)
        y = binding.DevTensor(B, OH, OW, n, 77)
        want_buf = y.buf.to_numpy(np.uint8, y.buf.nbytes)
        idx, val = _cell_bytes(y.t, u8)
        want_buf[idx] = val
        args = (k, bias, mv, sv, zp_in, zp_act, S_ACT, binding.ACT[act], store)
        for plan in (0, 1):
            got = binding.conv_dil_forward(xt, wq, zp_w, d, *args, want_acc=True, want_f32=True, pad=p, plan=plan, y=y)
            assert binding.last_conv_kernel() == 13
            if data.startswith("lds"):
                assert binding.last_conv_launch()[1:] == (256, int(data[3:]))
            assert np.array_equal(got["int32"], acc), "int32 accumulators"
            assert np.array_equal(got["f32"], oracle.dequant(u8.reshape(B, n, -1), zp_act, S_ACT)), "quant_stop float tail"
            assert np.array_equal(y.buf.to_numpy(np.uint8, y.buf.nbytes), want_buf), "output buffer, pad cells and spare channels included"
        if d == 1:       # identity 1: the dense call defines the same layer
            assert np.array_equal(binding.conv_forward(xt, wq, zp_w, *args, pad=p)["int32"], acc)
        if case == 2:    # identity 2: and so does the dense D x D call on the stuffed twin
            wt, D = stuffed_twin(wq, zp_w, c, k, d)
            assert np.array_equal(binding.conv_forward(xt, wt, zp_w, D, *args[1:], pad=p)["int32"], acc)


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("d,k,s,p,cs,accum,act,hw,xoff,msg", [
    (0, 3, 1, 1, 0, 0, "leaky", 4, 0, "dilation >= 1"), (2, 1, 1, 0, 0, 0, "leaky", 4, 0, "size must be 2..11"),
    (2, 12, 1, 1, 0, 0, "leaky", 4, 0, "size must be 2..11"), (2, 3, 2, 2, 0, 0, "leaky", 4, 0, "stride must be 1"),
    (2, 3, 1, -1, 0, 0, "leaky", 4, 0, "pad >= 0"), (2, 3, 1, 2, 4, 0, "leaky", 4, 0, "multiple of 16"),
    (2, 3, 1, 2, 32, 0, "leaky", 4, 0, "x.C != desc.c"), (2, 3, 1, 2, 0, 1, "leaky", 4, 0, "MI355_ACC_EXACT only"),
    (2, 3, 1, 2, 0, 0, None, 4, 0, "activation must be"), (2, 3, 1, 0, 0, 0, "leaky", 4, 0, "output map is empty"),
    (2, 3, 1, 1, 0, 0, "leaky", 4, 0, "y shape"), (2, 3, 1, 2, 0, 0, "leaky", 4, 4, "aligned to 16")])
def test_refusals_write_nothing(d, k, s, p, cs, accum, act, hw, xoff, msg):
    S = binding.shim()
    c = 32 if msg == "x.C != desc.c" else 16  # desc.c = 32 on a 16-channel tensor
    x = binding.DevTensor(1, hw, hw, 16, 0)
    y = binding.DevTensor(1, hw, hw, 16, 33)  # the "same" map of pad = d (k // 2): pad 1 at d = 2 is the wrong shape
    before = y.buf.to_numpy(np.uint8, y.buf.nbytes)
    xt = binding.Tensor.from_buffer_copy(x.t)
    if cs:
        xt.cs = cs
    xt.data += xoff
    desc = binding.ConvDesc(16, c, k, s, p, binding.ACT[act] if act else 0, 0, accum, 0, 33, 0.05)  # (0: logistic in the reference's enum)
    blob = binding.DevBuf(1 << 16)
    assert S.mi355_conv_dil_forward(C.byref(desc), C.byref(xt), blob.ptr, d, y.ref(), None, None, None) == -22
    err = S.mi355_last_error().decode()
    assert err.startswith("invalid argument: conv_dil_forward:") and msg in err
    assert np.array_equal(y.buf.to_numpy(np.uint8, y.buf.nbytes), before)


# ------------------------------------------------------------------------------------------------ the plain-C host
def _pull_all(net):
    net.sync()
    return [net.pull(i) for i in range(net.n)]


def _same(got, want, what):
    for i, (g, w) in enumerate(zip(got, want)):
        for key in w:
            if key != "int32":
                assert np.array_equal(g[key], w[key]), (what, i, key)


def test_host_net_dil_unit(cfg_dir, tmp_path):
    """dil_unit through the plain-C host: in the parity dump each dilated branch's int32 and bytes equal the definition computed from the
    pulled stem tensor and the host's prep, and the route holds the three branches side by side; every tensor of the dump again under the
    latency plan, graph replay, the throughput plan with a replica beside its parent, and after a packed import."""
    cfg, wts = os.path.join(cfg_dir, "dil_unit.cfg"), str(tmp_path / "dil.weights")
    recs = {r["i"]: r for r in synth.synth_weights(cfg, wts, seed=6)["layers"]}
    x = synth.synth_image_u8(3, 20, 20, seed=31, batch=B)
    x2 = synth.synth_image_u8(3, 20, 20, seed=32, batch=B)

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
    stem = want[0]["u8"].reshape(B, 16, 20, 20)
    for i, d in BRANCHES.items():
        inf, pr = net.info[i], net.prep(i)
        assert (inf["dilation"], inf["pad"], net.conv_kernel(i)) == (d, d, 13)
        assert not any(net.plan(j)[key] for j in (i - 1, i) for key in binding.PLAN_KEYS[:2] + binding.PLAN_KEYS[3:8]), "no fusion, no view"
        acc = np.stack([dil_acc(stem[b], recs[i]["weights_uint8"], recs[i]["zp_w"], 3, d, d, pr["zp_in"]) for b in range(B)])
        assert np.array_equal(want[i]["int32"], acc.ravel()), (i, "int32 against the definition")
        u8 = np.stack([oracle.requant(a, pr["biases_int32"], pr["M_value"], pr["shift_value"], pr["zp_act"], inf["activation"]) for a in acc])
        assert np.array_equal(want[i]["u8"], u8.ravel()), (i, "bytes against the definition")
    cat = np.concatenate([want[i]["u8"].reshape(B, 16, 400) for i in BRANCHES], 1)
    assert np.array_equal(want[6]["u8"], cat.ravel()), "the route over the branches"
    net.close()
    net, got = run(x, use_graph=True)
    _same(got, want, "graph replay")
    net.close()
    parent, got = run(x)
    assert [parent.conv_kernel(i) for i in BRANCHES] == [13, 13, 13] and not any(parent.plan(i)["out_view"] for i in BRANCHES)
    _same(got, want, "latency plan")
    packed = parent.export_packed()
    rep = parent.replica()  # switches the parent to the throughput plan
    rep.push_input(x2); parent.push_input(x)
    rep.sync(); parent.sync()
    for _ in range(3):
        rep.forward(); parent.forward()
    _same(_pull_all(parent), want, "throughput plan, parent")
    _same(_pull_all(rep), want2, "replica")
    rep.close()
    parent.close()
    imp = binding.Net(cfg, None, batch=B)
    imp.import_packed(packed)
    imp.push_input(x); imp.forward()
    _same(_pull_all(imp), want, "packed import")
    imp.close()
