"""GPU suite (`-m gpu`) for the grouped convolution (conv_group.hip, kernel id 12): the block-diagonal kernel through the C-ABI against
one oracle convolution per group (identity 1), and the C-ABI's refusals."""
import ctypes as C

import numpy as np
import pytest

import oracle
from yolo_quantization_amd import binding

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


def group_acc(x, wq, zp_w, g, k, s, p, zp_in):
    """The layer's definition: group q is the oracle's dense convolution of its channel window.  x: [c, H, W], wq: [n, cg k k]"""
    cg, ng = x.shape[0] // g, wq.shape[0] // g
    return np.concatenate([oracle.conv_acc(x[q * cg:(q + 1) * cg], wq[q * ng:(q + 1) * ng], zp_w[q * ng:(q + 1) * ng], k, s, p, zp_in)
                           for q in range(g)])


# (c, n, g, H, W, k, s, p, zp_in, zp_w, act, data); zp_w None: random per filter.  An M tile is 16 filters, a piece 16 channels; a
# workgroup takes 256 pixels (32 x 8, 16 x 16 or 8 x 32 by the output width) or 64 (8 x 8, 4 x 16, 2 x 32) by up to 8 M tiles.
STRUCT = [(16, 16, 4), (16, 16, 2), (32, 32, 2), (64, 64, 2), (24, 48, 2), (16, 32, 16), (16, 16, 16), (16, 16, 1), (9, 15, 3),
          (128, 128, 32), (144, 272, 2)]
SIZES = [(5, 6, 1, 1, 0), (5, 6, 3, 2, 1), (5, 6, 3, 3, 0), (5, 6, 5, 1, 2), (5, 6, 4, 2, 0), (3, 4, 11, 1, 5), (15, 15, 7, 7, 3)]
MAPS = [(1, 1), (1, 5), (5, 1), (15, 15), (16, 15), (15, 16), (17, 16), (7, 31), (8, 32), (9, 33), (31, 7), (32, 8), (33, 9)]
ACTS = ("leaky", "relu6", "linear", "relu")
CASES = (
    # structure: groups per piece and tile, pieces per slot list, tiles per group, straddling groups, multipliers, depthwise, dense,
    # odd cg with pad channels and the n % 4 tail, blocks of more than one M tile, more than eight tiles with a ragged last one
    [(c, n, g, 5, 6, 3, 1, 1, 7, None, ACTS[i % 4], "rand") for i, (c, n, g) in enumerate(STRUCT)]
    + [(32, 32, 2, H, W, k, s, p, 9, None, ACTS[i % 4], "rand") for i, (H, W, k, s, p) in enumerate(SIZES)]
    # maps: single rows and columns, and each tile side at -1, 0, +1
    + [(32, 32, 2, H, W, 3, 1, 1, 11, None, ACTS[i % 4], "rand") for i, (H, W) in enumerate(MAPS)]
    # the 64-pixel fallback: the two groups' 16 pieces each, staged one group after the other
    + [(512, 2, 2, 3, 3, 11, 1, 5, 9, None, "leaky", "fallback")]
    # zero points at both ends and in the middle
    + [(16, 16, 4, 4, 5, 3, 1, 1, zi, zw, "leaky", "rand") for zi in (0, 128, 255) for zw in (0, 128, 255)]
    # the accumulators' extremes, -cg k^2 255^2 and +cg k^2 255^2; shift values that are no powers of two
    + [(16, 16, 4, 4, 5, 3, 1, 1, 255, 255, "leaky", "neg"), (16, 16, 4, 4, 5, 3, 1, 1, 255, 0, "leaky", "pos"),
       (24, 48, 2, 4, 5, 3, 1, 1, 13, None, "leaky", "shift")])


def _cell_bytes(t, u8):
    """(flat byte indices, stored bytes) of a [B, n, OH, OW] result in tensor t's buffer"""
    Bn, Cn, H, W = u8.shape
    b, ch, y, x = np.meshgrid(np.arange(Bn), np.arange(Cn), np.arange(H), np.arange(W), indexing="ij")
    return ((t.lead + (b * (H + 1) + y + 1) * (W + 1) + x) * t.cs + ch).ravel(), (u8 ^ 0x80).ravel()


@pytest.mark.parametrize("case", range(len(CASES)), ids=lambda i: "c%d_n%d_g%d_%dx%d_k%d_s%d_p%d_zi%d_zw%s_%s_%s" % CASES[i])
def test_kernel_vs_one_oracle_convolution_per_group(case):
    c, n, g, H, W, k, s, p, zp_in, zw, act, data = CASES[case]
    rng = np.random.default_rng(3000 + case)
    x = rng.integers(0, 256, (B, c, H, W), dtype=np.uint8)
    wq = rng.integers(0, 256, (n, c // g * k * k), dtype=np.uint8)
    zp_w = rng.integers(0, 256, n, dtype=np.uint8) if zw is None else np.full(n, zw, np.uint8)
    if data in ("neg", "pos"):
        x[:] = 255
        wq[:] = 0 if data == "neg" else 255
    bias, mv, sv = _consts(rng, n)
    if data == "shift":
        sv = sv * rng.uniform(0.55, 0.95, n)
    zp_act = int(rng.integers(0, 200))
    OH, OW = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    acc = np.stack([group_acc(x[b], wq, zp_w, g, k, s, p, zp_in) for b in range(B)])
    assert acc.shape == (B, n, OH * OW)
    if data in ("neg", "pos"):
        assert acc.min() == acc.max() == (-1 if data == "neg" else 1) * (c // g) * k * k * 255 * 255
    xt = binding.DevTensor.from_nchw(x, zp_in)
    for store in (binding.STORE_WRAP, binding.STORE_SATURATE):
        u8 = np.stack([oracle.requant(acc[b], bias, mv, sv, zp_act, oracle.ACT[act], store) for b in range(B)]).reshape(B, n, OH, OW)
        y = binding.DevTensor(B, OH, OW, n, 77)
        want_buf = y.buf.to_numpy(np.uint8, y.buf.nbytes)
        idx, val = _cell_bytes(y.t, u8)
        want_buf[idx] = val
        args = (k, bias, mv, sv, zp_in, zp_act, S_ACT, binding.ACT[act], store)
        for plan in (0, 1):
            got = binding.conv_group_forward(xt, wq, zp_w, g, *args, want_acc=True, want_f32=True, stride=s, pad=p, plan=plan, y=y)
            assert binding.last_conv_kernel() == 12
            if data == "fallback":  # 512 + 16 pieces of an 8 x 8 tile's 18 x 18 cells (plane pitch 325): the 32 x 8 tile needs 193 KB
                assert binding.last_conv_launch()[1:] == (256, 512 + 16 * 325 * 16)
            assert np.array_equal(got["int32"], acc), "int32 accumulators"
            assert np.array_equal(got["f32"], oracle.dequant(u8.reshape(B, n, -1), zp_act, S_ACT)), "quant_stop float tail"
            assert np.array_equal(y.buf.to_numpy(np.uint8, y.buf.nbytes), want_buf), "output buffer, pad cells and spare channels included"
        if g == c == n:  # the depthwise kernel defines the same layer
            assert np.array_equal(binding.conv_dw_forward(xt, wq, zp_w, *args, stride=s, pad=p)["u8"], u8)
        if g == 1:       # and so does the dense call
            assert np.array_equal(binding.conv_forward(xt, wq, zp_w, *args, stride=s, pad=p)["int32"], acc)


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("c,n,g,k,s,p,cs,accum,act,hw,msg", [
    (16, 16, 3, 3, 1, 1, 0, 0, "leaky", 4, "divide the channels"), (16, 20, 8, 3, 1, 1, 0, 0, "leaky", 4, "divide the filters"),
    (16, 16, 0, 3, 1, 1, 0, 0, "leaky", 4, "groups >= 1"), (16, 16, 4, 12, 1, 1, 0, 0, "leaky", 4, "size must be 1..11"),
    (16, 16, 4, 1, 2, 0, 0, 0, "leaky", 4, "1x1 layer needs stride 1"), (16, 16, 4, 3, 1, 1, 4, 0, "leaky", 4, "multiple of 16"),
    (32, 16, 4, 3, 1, 1, 32, 0, "leaky", 4, "x.C != desc.c"), (16, 16, 4, 3, 1, 1, 0, 1, "leaky", 4, "MI355_ACC_EXACT only"),
    (16, 16, 4, 3, 1, 1, 0, 0, None, 4, "activation must be"), (16, 16, 4, 3, 1, 0, 0, 0, "leaky", 1, "output map is empty"),
    (1024, 2, 2, 11, 1, 5, 0, 0, "leaky", 3, "no tile fits")])  # desc.c = 32 on a 16-channel tensor; a 1 x 1 map under a 3 x 3 kernel
def test_refusals_write_nothing(c, n, g, k, s, p, cs, accum, act, hw, msg):
    S = binding.shim()
    x = binding.DevTensor(1, hw, hw, 16 if msg == "x.C != desc.c" else c, 0)
    OH = max((hw + 2 * p - k) // s + 1, 1)
    y = binding.DevTensor(1, OH, OH, n, 33)
    before = y.buf.to_numpy(np.uint8, y.buf.nbytes)
    xt = binding.Tensor.from_buffer_copy(x.t)
    if cs:
        xt.cs = cs
    d = binding.ConvDesc(n, c, k, s, p, binding.ACT[act] if act else 0, 0, accum, 0, 33, 0.05)  # (0: logistic in the reference's enum)
    blob = binding.DevBuf(1 << 16)
    assert S.mi355_conv_group_forward(C.byref(d), C.byref(xt), blob.ptr, g, y.ref(), None, None, None) == -22
    err = S.mi355_last_error().decode()
    assert err.startswith("invalid argument: conv_group_forward:") and msg in err
    assert np.array_equal(y.buf.to_numpy(np.uint8, y.buf.nbytes), before)
