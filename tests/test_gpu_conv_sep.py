"""GPU suite (`-m gpu`) for the depthwise-separable block (conv_sep.hip, kernel id 15): one fused launch against the chained oracle
(per-channel depthwise layer, its requantised bytes, the dense 1x1 layer on them), the C-ABI's refusals, and the plain-C host's
opt-in pairs against the same net unfused."""
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


def _consts(rng, c, gain=1.0, np2=False):
    bias = rng.integers(-3000, 3000, c).astype(np.int32)
    M = rng.uniform(2.0 ** -9, 2.0 ** -5, c) * gain
    shift = np.floor(-np.log2(M)).astype(int)
    sv = 2.0 ** -shift.astype(np.float64)
    if np2:
        sv = sv * rng.uniform(0.55, 0.95, c)
    return bias, np.round(M * 2.0 ** shift * 2 ** 31) * 2.0 ** -31, sv


def case(c=16, n=16, H=5, W=7, k=3, s=1, pad=None, zi=7, zwd=None, zm=None, zwp=None, dact="leaky", pact="leaky", dstore=0, plan=0,
         data="rand", np2=False):
    return dict(c=c, n=n, H=H, W=W, k=k, s=s, pad=k // 2 if pad is None else pad, zi=zi, zwd=zwd, zm=zm, zwp=zwp, dact=dact, pact=pact,
                dstore=dstore, plan=plan, data=data, np2=np2)


# The kernel walks channels in chunks of 64 (K-steps of 16 or 32 channels: c % 16 != 0 reads the generic blob, else the row plane),
# tiles of 16 x 8 / 8 x 16 / 4 x 32 pixels, filter blocks of 128 (n <= 128) or 256.
CASES = (
    # channels: a ragged dword, the chunk edge, a 16-channel tail of the row plane, three chunks
    [case(c=c, n=33, plan=i & 1, dact=("leaky", "relu6", "linear")[i % 3]) for i, c in enumerate((16, 17, 64, 65, 80, 129))]
    + [case(c=96, n=40, pact="relu6"), case(c=32, n=16, pact="linear")]
    # filters: one, ragged dwords, the 32-row tile, and each side of both filter blocks
    + [case(n=n, plan=i & 1, pact=("leaky", "relu", "linear", "relu6")[i % 4]) for i, n in enumerate((1, 16, 30, 32, 33, 127, 128, 129, 255, 256, 257))]
    + [case(c=17, n=257, H=3, W=3)]
    # maps around every tile's edges
    + [case(H=h, W=w, n=32, plan=i & 1) for i, (h, w) in enumerate(((1, 1), (2, 2), (15, 9), (16, 8), (17, 7), (8, 16), (4, 32), (3, 33), (33, 17)))]
    # sizes and strides: the register paths on odd and even maps, the runtime path, pad 0, pad above size / 2
    + [case(c=65, H=17, W=19, k=3, s=2), case(c=64, H=18, W=20, k=3, s=2, plan=1), case(c=17, H=9, W=10, k=5, s=1, dact="relu6"),
       case(c=80, H=17, W=18, k=5, s=2), case(c=16, H=18, W=17, k=5, s=2, plan=1),
       case(c=65, H=9, W=10, k=7, pad=3), case(H=9, W=10, k=2, pad=1), case(c=17, H=9, W=10, k=1), case(H=20, W=19, k=3, s=3, plan=1),
       case(c=129, H=9, W=10, k=7, s=2, pad=3, n=40), case(c=17, H=9, W=10, pad=0), case(c=17, H=9, W=10, pad=2), case(H=3, W=3, k=5, pad=4)]
    # zero points at both ends of all four
    + [case(H=6, W=9, zi=zi, zwd=zwd, zm=zm, zwp=zwp, c=c)
       for zi, zwd, zm, zwp, c in ((0, 0, 0, 0, 16), (255, 255, 255, 255, 17), (0, 255, 0, 255, 64), (255, 0, 255, 0, 65), (128, 0, 255, 255, 16))]
    # the intermediate's store mode on data whose depthwise epilogue wraps
    + [case(c=65, H=6, W=9, data="wide", dstore=0), case(c=65, H=6, W=9, data="wide", dstore=1, dact="linear")]
    # extremes at three chunks: m = 255 everywhere, 1x1 accumulators +- c 255^2; all-0 depthwise weights
    + [case(c=129, n=33, H=4, W=5, zi=255, zwd=0, zwp=0, dact="linear", dstore=1, data="pos"),
       case(c=129, n=33, H=4, W=5, zi=255, zwd=0, zwp=255, dact="linear", dstore=1, data="neg"),
       case(c=129, n=33, H=4, W=5, zi=255, zwd=255, zwp=0, dact="linear", dstore=1, data="dneg")]
    # shift_value that is no power of two, in each stage and in both
    + [case(c=65, n=33, np2="dw"), case(c=65, n=33, np2="pw", pact="relu6"), case(c=64, n=33, np2="both", dact="linear")]
)


def _cell_bytes(t, u8):
    """(flat byte indices, biased bytes) of a [B, C, OH, OW] result in tensor t's buffer"""
    Bn, Cn, H, W = u8.shape
    b, ch, y, x = np.meshgrid(np.arange(Bn), np.arange(Cn), np.arange(H), np.arange(W), indexing="ij")
    return ((t.lead + (b * (H + 1) + y + 1) * (W + 1) + x) * t.cs + ch).ravel(), (u8 ^ 0x80).ravel()


def _id(i):
    q = CASES[i]
    return "c%d_n%d_%dx%d_k%d_s%d_p%d_%s_%s_plan%d_%s" % (q["c"], q["n"], q["H"], q["W"], q["k"], q["s"], q["pad"], q["dact"], q["pact"],
                                                        q["plan"], q["data"])


@pytest.mark.parametrize("i", range(len(CASES)), ids=_id)
def test_kernel_vs_chained_oracle(i):
    q = CASES[i]
    c, n, H, W, k, s, pad = (q[key] for key in ("c", "n", "H", "W", "k", "s", "pad"))
    rng = np.random.default_rng(3000 + i)
    x = rng.integers(0, 256, (B, c, H, W), dtype=np.uint8)
    wd = rng.integers(0, 256, (c, k * k), dtype=np.uint8)
    wp = rng.integers(0, 256, (n, c), dtype=np.uint8)
    zwd = rng.integers(0, 256, c, dtype=np.uint8) if q["zwd"] is None else np.full(c, q["zwd"], np.uint8)
    zwp = rng.integers(0, 256, n, dtype=np.uint8) if q["zwp"] is None else np.full(n, q["zwp"], np.uint8)
    zm = int(rng.integers(0, 200)) if q["zm"] is None else q["zm"]
    zp_act = int(rng.integers(0, 200))
    if q["data"] in ("pos", "neg", "dneg"):
        x[:] = 255
        wd[:] = 0 if q["data"] == "dneg" else 255
        wp[:] = 0 if q["data"] == "neg" else 255
    db, dM, dS = _consts(rng, c, gain=16.0 if q["data"] == "wide" else 1.0, np2=q["np2"] in ("dw", "both"))
    pb, pM, pS = _consts(rng, n, np2=q["np2"] in ("pw", "both"))
    OH, OW = (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1

    # the reference: per-channel depthwise accumulators, their requantised bytes m, the dense 1x1 layer on m
    dacc = [np.concatenate([oracle.conv_acc(x[b, j:j + 1], wd[j:j + 1], zwd[j:j + 1], k, s, pad, q["zi"]) for j in range(c)]) for b in range(B)]
    m = [oracle.requant(dacc[b], db, dM, dS, zm, oracle.ACT[q["dact"]], q["dstore"]).reshape(c, OH, OW) for b in range(B)]
    if q["data"] == "wide":
        other = [oracle.requant(dacc[b], db, dM, dS, zm, oracle.ACT[q["dact"]], 1 - q["dstore"]).reshape(c, OH, OW) for b in range(B)]
        assert any(not np.array_equal(u, v) for u, v in zip(m, other)), "the depthwise epilogue must wrap on this data"
    acc = np.stack([oracle.conv_acc(m[b], wp, zwp, 1, 1, 0, zm) for b in range(B)])
    if q["data"] in ("pos", "neg"):
        assert acc.min() == acc.max() == (1 if q["data"] == "pos" else -1) * c * 255 * 255

    xt = binding.DevTensor.from_nchw(x, q["zi"])
    dw = dict(wq=wd, zp_w=zwd, ksize=k, bias=db, M=dM, shift=dS, zp_in=q["zi"], zp_act=zm, activation=binding.ACT[q["dact"]], stride=s,
              pad=pad, store=q["dstore"])
    pw = dict(wq=wp, zp_w=zwp, bias=pb, M=pM, shift=pS, zp_act=zp_act, s_act=S_ACT, activation=binding.ACT[q["pact"]])
    for store in (binding.STORE_WRAP, binding.STORE_SATURATE):
        u8 = np.stack([oracle.requant(acc[b], pb, pM, pS, zp_act, oracle.ACT[q["pact"]], store) for b in range(B)])
        y = binding.DevTensor(B, OH, OW, n, 77)
        want_buf = y.buf.to_numpy(np.uint8, y.buf.nbytes)
        idx, val = _cell_bytes(y.t, u8.reshape(B, n, OH, OW))
        want_buf[idx] = val
        got = binding.conv_sep_forward(xt, dw, pw, store=store, want_acc=True, want_f32=True, plan=q["plan"], y=y)
        assert binding.last_conv_kernel() == 15
        assert np.array_equal(got["int32"], acc), "int32 accumulators of the 1x1 stage"
        assert np.array_equal(got["f32"], oracle.dequant(u8, zp_act, S_ACT)), "quant_stop float tail"
        assert np.array_equal(y.buf.to_numpy(np.uint8, y.buf.nbytes), want_buf), "output buffer, pad cells and spare channels included"


# ------------------------------------------------------------------------------------------------ refusals
def _blobs(c, k, n):
    rng = np.random.default_rng(9)
    db, dM, dS = _consts(rng, c)
    pb, pM, pS = _consts(rng, n)
    bd = binding.conv_dw_pack(rng.integers(0, 256, (c, k * k), dtype=np.uint8), np.zeros(c, np.uint8), k, db, dM, dS)
    bp = binding.conv_pack(rng.integers(0, 256, (n, c), dtype=np.uint8), np.zeros(n, np.uint8), c, 1, pb, pM, pS)
    return binding.DevBuf.from_numpy(bd), binding.DevBuf.from_numpy(bp)


@pytest.mark.parametrize("what,msg", [("ref_f32", "MI355_ACC_EXACT"), ("pw_size3", "ksize 1, stride 1, pad 0"), ("pw_stride2", "ksize 1, stride 1, pad 0"),
                                      ("pw_c", "pw.c != dw.n"), ("n3", "pw.n != 3"), ("cs4", "multiple of 16"),
                                      ("blob_dw", "blob_dw is not"), ("blob_pw", "blob_pw is not")])
def test_refusals_write_nothing(what, msg):
    S = binding.shim()
    n = 3 if what == "n3" else 32
    x = binding.DevTensor(1, 6, 6, 16, 0)
    y = binding.DevTensor(1, 6, 6, n, 33)
    before = y.buf.to_numpy(np.uint8, y.buf.nbytes)
    xt = binding.Tensor.from_buffer_copy(x.t)
    if what == "cs4":
        xt.cs = 4
    accum = binding.ACC_REF_F32 if what == "ref_f32" else binding.ACC_EXACT
    dd = binding.ConvDesc(16, 16, 3, 1, 1, binding.ACT["leaky"], 0, accum, 0, 33, 0.05)
    dp = binding.ConvDesc(n, 24 if what == "pw_c" else 16, 3 if what == "pw_size3" else 1, 2 if what == "pw_stride2" else 1, 0,
                          binding.ACT["leaky"], 0, accum, 33, 33, 0.05)
    # the blobs of this launch, or one of them from another layer (a 5x5 depthwise layer; a 1x1 layer of 48 filters)
    bd, bp = _blobs(16, 5 if what == "blob_dw" else 3, 48 if what == "blob_pw" else n)
    assert S.mi355_conv_sep_forward(C.byref(dd), C.byref(dp), C.byref(xt), bd.ptr, bp.ptr, y.ref(), None, None, None) == -22
    assert msg in S.mi355_last_error().decode()
    assert np.array_equal(y.buf.to_numpy(np.uint8, y.buf.nbytes), before)


# ------------------------------------------------------------------------------------------------ host: opt-in pairs
PAIRS, DW = [(1, 2), (3, 4), (5, 6)], [1, 3, 5, 7, 10]  # cfg/sep_unit.cfg: the blocks the planner takes; every depthwise layer


def _pull_stored(net):
    net.sync()
    return [None if net.is_fused(i) else net.pull(i) for i in range(net.n)]


def _same(got, want, what):
    for i, (g, w) in enumerate(zip(got, want)):
        for key in (w if g is not None else ()):
            if key != "int32":
                assert np.array_equal(g[key], w[key]), (what, i, key)


def test_host_pairs_fuse_only_when_asked(cfg_dir, tmp_path):
    """sep_unit with set_fuse_separable(True) equals the same net with it off -- every stored tensor and the detections -- under the
    latency plan, graph replay, the throughput plan with a replica and a packed import; kernel 15 exactly on the three pairs."""
    cfg = os.path.join(cfg_dir, "sep_unit.cfg")
    wts = str(tmp_path / "sep.weights")
    synth.synth_weights(cfg, wts, seed=4)
    x = synth.synth_image_u8(3, 24, 24, seed=21, batch=B)
    x2 = synth.synth_image_u8(3, 24, 24, seed=22, batch=B)

    def run(fuse, xin, weights=wts, packed=None, **kw):
        net = binding.Net(cfg, weights, batch=B, **kw)
        net.set_fuse_separable(fuse)
        if packed is not None:
            net.import_packed(packed)
        else:
            net.prepare_fixed(1.0 / 255.0, 0)
        net.push_input(xin); net.forward()
        if kw.get("use_graph"):
            net.forward(); net.forward()
        return net, _pull_stored(net)

    off, want = run(False, x)
    want_det = off.detections_batch(24, 24, 0.0)
    assert [off.conv_kernel(i) for i in DW] == [10] * 5 and 15 not in [off.conv_kernel(i) for i in range(off.n)]
    assert all(w is not None for w in want)
    off.close()
    off, want2 = run(False, x2)
    off.close()

    def check_ids(net):
        ids = [net.conv_kernel(i) for i in range(net.n)]
        assert [i for i, k in enumerate(ids) if k == 15] == [i for p in PAIRS for i in p], ids
        assert ids[7] == ids[10] == 10, "the refused pairs keep their kernels"
        assert [i for i in range(net.n) if net.is_fused(i)] == [p[0] for p in PAIRS]

    net, got = run(True, x, use_graph=True)
    _same(got, want, "graph replay"); check_ids(net)
    net.close()
    parent, got = run(True, x)
    _same(got, want, "latency plan"); check_ids(parent)
    for a, b_ in zip(parent.detections_batch(24, 24, 0.0), want_det):
        assert np.array_equal(a, b_), "detections"
    packed = parent.export_packed()
    rep = parent.replica()  # switches the parent to the throughput plan; inherits the flag
    rep.push_input(x2); parent.push_input(x)
    rep.sync(); parent.sync()
    for _ in range(3):
        rep.forward(); parent.forward()
    _same(_pull_stored(parent), want, "throughput plan, parent"); check_ids(parent)
    _same(_pull_stored(rep), want2, "replica"); check_ids(rep)
    rep.close()
    parent.set_fuse_separable(False)  # off again: the pair runs as two layers
    parent.forward()
    _same(_pull_stored(parent), want, "flag off again")
    assert [parent.conv_kernel(i) for i in DW] == [10] * 5
    parent.close()
    imp, got = run(True, x, weights=None, packed=packed)
    _same(got, want, "packed import"); check_ids(imp)
    imp.close()
