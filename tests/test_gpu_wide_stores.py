"""GPU suite (`-m gpu`): the one-store-per-lane epilogues of conv_pool16.hip (16 -> 32 + maxpool) and of the first layer's pooled MFMA kernel
(conv_aux.hip).  A lane's packed dwords are exchanged across the four k-group lanes (v_permlane16_swap / v_permlane32_swap) so that it holds 16
(8 for the 16-filter first layer) consecutive bytes of ONE pooled cell and stores them at once; offset and mask follow the row it stores.  What can
go wrong is a byte in the wrong cell, a masked lane that stores, or a store that reaches past its 16 bytes: every case compares the pooled bytes
with the oracle's conv -> requantise -> maxpool AND every other byte of the raw pooled buffer (pad cells, lead, tail, the channels of a wider cell
that this layer does not own) with the value the buffer was filled with."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle
from yolo_quantization_amd import binding
from test_gpu_parity import _rand_layer
from test_gpu_r2_kernels import _planar_tensor

pytestmark = pytest.mark.gpu

ACTS = ["leaky", "relu6", "linear"]
STORES = [(binding.STORE_WRAP, "wrap"), (binding.STORE_SATURATE, "saturate")]
GAINS = {"no-wrap": (2.0 ** -17, 2.0 ** -16), "much-wrap": (2.0 ** -11, 2.0 ** -7)}


@pytest.fixture(scope="module", autouse=True)
def device():
    binding.init(0)


def _check_outside_untouched(yp, n, fill):
    """every byte of the raw pooled buffer that is not one of channels 0 .. n - 1 of a cell inside the map still holds the fill value"""
    t = yp.t
    raw = yp.buf.to_numpy(np.uint8, yp.buf.nbytes)
    ncell = t.lead + t.B * (t.H + 1) * (t.W + 1) + t.tail
    assert raw.size == ncell * t.cs
    cells = raw.reshape(ncell, t.cs)
    inside = np.zeros((ncell, t.cs), bool)
    b, y, x = np.meshgrid(np.arange(t.B), np.arange(t.H), np.arange(t.W), indexing="ij")
    inside[(t.lead + (b * (t.H + 1) + y + 1) * (t.W + 1) + x).ravel(), :n] = True
    bad = ~inside & (cells != fill)
    assert not bad.any(), f"{int(bad.sum())} bytes outside the map were written, first at (cell, byte) {tuple(np.argwhere(bad)[0])}"


# ---------------------------------------------------------------------------------------------------------------- conv_pool16.hip
# (B, H, W): pooled maps 2 x 8 (smaller than a patch, mostly masked), 18 x 24 (a full and a half patch column, ragged rows), 10 x 26 (ten columns
# of the last patch), 17 x 40 (odd pooled height: the mask of a wave's SECOND row differs from its first), 35 x 16 (no ragged column)
P16_MAPS = [(3, 4, 16), (2, 36, 48), (2, 20, 52), (3, 34, 80), (1, 70, 32)]


@functools.lru_cache(maxsize=None)
def _p16_layer(B, H, W, gain):
    """input, layer parameters and the oracle's accumulators of a (map, gain): shared by the activation / store / table cases, never modified"""
    c, n = 16, 32
    rng = np.random.default_rng(H * 1000 + W + len(gain))
    x = rng.integers(0, 256, (B, c, H, W), dtype=np.uint8)
    wq, zp_w, bias, mv, sv = _rand_layer(rng, n, c, 3, *GAINS[gain])
    zp_w[0], zp_w[1], zp_w[2] = 0, 255, 1
    if gain != "much-wrap":
        bias = (bias // 16).astype(np.int32)
    zp_in = 9
    acc = [oracle.conv_acc(x[b], wq, zp_w, 3, 1, 1, zp_in) for b in range(B)]
    for a in (x, wq, zp_w, bias, mv, sv, *acc):
        a.setflags(write=False)
    return x, wq, zp_w, bias, mv, sv, zp_in, acc


def _p16_run(B, H, W, act, store, gain, table, cell_channels):
    c, n = 16, 32
    x, wq, zp_w, bias, mv, sv, zp_in, acc = _p16_layer(B, H, W, gain)
    zp_act = 23 if act != "linear" else 128
    want = np.stack([oracle.maxpool_u8(oracle.requant(acc[b], bias, mv, sv, zp_act, oracle.ACT[act], store).reshape(n, H, W), 2, 2, 1)
                     for b in range(B)])
    xt = binding.DevTensor.from_nchw(x, zp_in)
    blob = binding.DevBuf.from_numpy(binding.conv_pack(wq, zp_w, c, 3, bias, mv, sv, binding.ACT[act], zp_act + (table == "other-zero-point")))
    outs = []
    for hint, kernel in ((1, 7), (0, 2)):
        yp = binding.DevTensor(B, H // 2, W // 2, cell_channels, zp_act)
        yp.t.C = n  # (cell_channels > n: the layer owns the first n bytes of a wider cell)
        d = binding.ConvDesc(n, c, 3, 1, 1, binding.ACT[act], store, binding.ACC_EXACT, zp_in, zp_act, 1.0)
        d.epilogue_packed = hint
        binding.check(binding.shim().mi355_conv_pool_forward(C.byref(d), xt.ref(), blob.ptr, None, yp.ref(), None), "conv_pool")
        assert binding.shim().mi355_last_conv_kernel() == kernel
        got = yp.to_nchw()
        assert np.array_equal(got, want), f"kernel {kernel}: {int((got != want).sum())} of {got.size} pooled bytes differ"
        _check_outside_untouched(yp, n, zp_act ^ 0x80)
        outs.append(got)
    assert np.array_equal(outs[0], outs[1])


@pytest.mark.parametrize("B,H,W", P16_MAPS)
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("store", [s for s, _ in STORES], ids=[i for _, i in STORES])
@pytest.mark.parametrize("gain", list(GAINS))
@pytest.mark.parametrize("table", ["match", "other-zero-point"])
def test_conv_pool16_wide_stores(B, H, W, act, store, gain, table):
    """conv_pool16.hip (kernel 7): pooled bytes equal the oracle's, nothing outside the map is written, conv_small.hip (kernel 2, the same call
    without the hint) gives the same bytes.  "much-wrap" sends waves through the exact-path redo, a table made for another zero point sends every
    window through the general loop: both fill the registers that the exchange reads."""
    _p16_run(B, H, W, act, store, gain, table, 32)


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("store", [s for s, _ in STORES], ids=[i for _, i in STORES])
def test_conv_pool16_wide_stores_leave_the_rest_of_a_wider_cell(act, store):
    """The pooled tensor has 48-byte cells of which the layer owns 32: bytes 32 .. 47 of every cell keep the fill value."""
    _p16_run(2, 36, 48, act, store, "much-wrap", "match", 48)


# ---------------------------------------------------------------------------------------------------------------- first layer
# pooled 10 x 18 (ragged right and below: 8 x 16 patches) and 8 x 16 (exact)
L0_MAPS = [(2, 20, 36), (1, 16, 32)]


@functools.lru_cache(maxsize=None)
def _l0_layer(B, H, W, n):
    rng = np.random.default_rng(n + B + H + W)
    x = rng.integers(0, 256, (B, 3, H, W), dtype=np.uint8)
    wq, zp_w, bias, mv, sv = _rand_layer(rng, n, 3, 3, 2.0 ** -8, 2.0 ** -5)
    zp_in = 37
    acc = [oracle.conv_acc(x[b], wq, zp_w, 3, 1, 1, zp_in) for b in range(B)]
    for a in (x, wq, zp_w, bias, mv, sv, *acc):
        a.setflags(write=False)
    return x, wq, zp_w, bias, mv, sv, zp_in, acc


@pytest.mark.parametrize("B,H,W", L0_MAPS)
@pytest.mark.parametrize("n", [16, 32])
@pytest.mark.parametrize("layout", ["planar", "cell"])
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("store", [s for s, _ in STORES], ids=[i for _, i in STORES])
@pytest.mark.parametrize("ept", [False, True], ids=["derive", "table"])
def test_first_layer_pool_wide_stores(B, H, W, n, layout, act, store, ept):
    """conv_first_mfma_pool_kernel: one 8-byte (16 filters) / 16-byte (32 filters) store per lane and tile; bytes against the oracle, nothing
    outside the map written."""
    x, wq, zp_w, bias, mv, sv, zp_in, acc = _l0_layer(B, H, W, n)
    zp_act = 23
    want = np.stack([oracle.maxpool_u8(oracle.requant(acc[b], bias, mv, sv, zp_act, oracle.ACT[act], store).reshape(n, H, W), 2, 2, 1)
                     for b in range(B)])
    blob = binding.DevBuf.from_numpy(binding.conv_pack(wq, zp_w, 3, 3, bias, mv, sv, *((binding.ACT[act], zp_act) if ept else ())))
    if layout == "planar":
        xt, keep = _planar_tensor(x)
        xref = C.byref(xt)
    else:
        keep = binding.DevTensor.from_nchw(x, zp_in)
        xref = keep.ref()
    d = binding.ConvDesc(n, 3, 3, 1, 1, binding.ACT[act], store, binding.ACC_EXACT, zp_in, zp_act, 0.05)
    yp = binding.DevTensor(B, H // 2, W // 2, n, zp_act)
    binding.check(binding.shim().mi355_conv_pool_forward(C.byref(d), xref, blob.ptr, None, yp.ref(), None), "conv+pool (first layer)")
    assert binding.shim().mi355_last_conv_kernel() == 1
    assert binding.last_conv_launch()[2] == 0, "the MFMA kernel (no dynamic LDS; the VALU kernel has some) should have served the call"
    got = yp.to_nchw()
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {got.size} pooled bytes differ"
    _check_outside_untouched(yp, n, zp_act ^ 0x80)
