"""The general conv kernel's launcher and K layout at their switch points, on the device.

tests/kxk_geometry.py restates what conv_forward_impl, conv_generic_forward and conv_kxk_launch decide and lists one case on each side of
every labelled clause: the unit and chunk switches, the channel masks and tap-slot tails, ragged filter counts, every tile width of every
instantiation <U, MS, WM> (the 128-filter x 64-pixel configuration included), the fall-back widths, dynamic LDS on each side of 64 KiB, more
than one tile along x, y, the filters and the batch at once, and the refusals.  One test per case and store mode; each

  * runs through mi355_conv_forward with int32 and float dumps;
  * asserts mi355_last_conv_kernel() == 9 and that mi355_last_conv_launch() is the restatement's (grid, threads, lds) BEFORE it compares
    bytes: a case that slid to another tile fails for that reason;
  * compares every int32 accumulator, every uint8 and the float tail with the exact reference, bit for bit, and the bytes of the call
    without dumps with those of the call with them;
  * where x or y is a channel window of a wider tensor: the other channels of y keep their bytes;
  * a refusal: -22, its own message, and y still holds its fill;
  * a shape the dispatch keeps for the specialised launchers: served by another kernel, the same bytes.

Cases marked `twin` also run the ref-f32 twin (kernel 6): its grid, and the oracle's fp32-order accumulators and bytes.

Mutation check (made on the MI355X on scratch builds of conv_kxk.hip, not committed; both mutants compute wrong bytes inside their bounds).
Mutant 1, the patch origin one cell to the right for tiles with tx > 0 of the 256-pixel configurations: 8 cases red here (every first-
configuration case of more than one tile along x), 3 random nets red, all 66 grid tests of test_gpu_conv_kxk.py green.  Mutant 2, the
accumulator row groups of `<U, 1, 4>` swapped in pairs: all 16 cases of that configuration red here and the aimed net
kxk_stride7_wide_m_tile red in test_gpu_random_nets.py; every older test green."""
import ctypes as C

import numpy as np
import pytest

import kxk_geometry as kg
from yolo_quantization_amd import binding

pytestmark = pytest.mark.gpu

STORES = {"wrap": binding.STORE_WRAP, "sat": binding.STORE_SATURATE}


@pytest.fixture(scope="module", autouse=True)
def device():
    binding.init(0)


def _window(t, channels, offset):
    w = binding.Tensor.from_buffer_copy(t.t)
    w.C = channels
    w.data = C.c_void_p(t.t.data + offset)
    return w


def _call(ops, store, accum=binding.ACC_EXACT, dumps=True):
    """one mi355_conv_forward -> (rc, y of the whole output tensor before and after [B, channels, OH, OW], int32, f32)"""
    cs, S = ops.cs, binding.shim()
    xt = binding.DevTensor.from_nchw(ops.wide, ops.zp_in)
    x = _window(xt, cs.c, cs.xwin[1]) if cs.xwin else xt.t
    blob = binding.DevBuf.from_numpy(binding.conv_pack(ops.wq, ops.zp_w, cs.c, cs.k, ops.bias, ops.mv, ops.sv))
    wraw, zraw = binding.DevBuf.from_numpy(ops.wq), binding.DevBuf.from_numpy(ops.zp_w)
    OH, OW = (max(v, 1) for v in cs.out_hw())
    yt = binding.DevTensor(cs.B, OH, OW, cs.ywin[0] if cs.ywin else cs.n, kg.ZP_ACT)
    y = _window(yt, cs.n, cs.ywin[1]) if cs.ywin else yt.t
    before = yt.to_nchw()
    cnt = cs.B * cs.n * OH * OW
    acc, f32 = (binding.DevBuf(cnt * 4), binding.DevBuf(cnt * 4)) if dumps else (None, None)
    d = binding.ConvDesc(cs.n, cs.c, cs.k, cs.stride, cs.pad, binding.ACT[cs.act], STORES[store], accum, ops.zp_in, kg.ZP_ACT, float(kg.S_ACT), 0, 0)
    rc = S.mi355_conv_forward(C.byref(d), C.byref(x), blob.ptr, wraw.ptr, zraw.ptr, C.byref(y), acc.ptr if dumps else None,
                              f32.ptr if dumps else None, None)
    binding.check(S.mi355_stream_sync(None), "sync")
    out = dict(rc=rc, before=before, y=yt.to_nchw())
    if dumps and rc == 0:
        out["int32"] = acc.to_numpy(np.int32, cnt).reshape(cs.B, cs.n, OH * OW)
        out["f32"] = f32.to_numpy(np.float32, cnt).reshape(cs.B, cs.n, OH * OW)
    return out


def _assert_bytes(cs, out, want_u8, what):
    off = cs.ywin[1] if cs.ywin else 0
    got = out["y"][:, off:off + cs.n]
    bad = np.argwhere(got != want_u8)
    assert not len(bad), f"{what}: {len(bad)} bytes differ from the reference, first at (b, ch, y, x) = {bad[:4].tolist()}"
    keep = np.ones(out["y"].shape[1], bool)
    keep[off:off + cs.n] = False
    assert np.array_equal(out["y"][:, keep], out["before"][:, keep]), f"{what}: channels outside the window changed"


def _assert_dumps(out, want_acc, want_f32, what):
    bad = np.argwhere(out["int32"] != want_acc)
    assert not len(bad), f"{what}: {len(bad)} int32 accumulators differ, first at (b, ch, pixel) = {bad[:4].tolist()}"
    assert np.array_equal(out["f32"], want_f32), f"{what}: the float tail"


_OPS = {}


def _operands(cs):
    """the case's operands and references, shared by its two store modes"""
    if cs.name not in _OPS:
        _OPS.clear()
        _OPS[cs.name] = kg.Operands(cs)
    return _OPS[cs.name]


@pytest.mark.parametrize("store", ["wrap", "sat"])
@pytest.mark.parametrize("cs", kg.CASES, ids=repr)
def test_launch_geometry_and_bytes(cs, store):
    _, g = kg.trace_case(cs)
    ops = _operands(cs)
    S = binding.shim()
    if g != "specialised" and g["refused"]:  # nothing launched: -22, the clause's own message, y untouched
        out = _call(ops, store)
        assert out["rc"] == -22 and g["refused"] in S.mi355_last_error().decode(), (out["rc"], S.mi355_last_error().decode())
        assert np.array_equal(out["y"], out["before"]), "a refused call wrote to y"
        return
    exact = cs.accum == "exact"
    what = f"{cs.name} store {store}"
    out = _call(ops, store, binding.ACC_EXACT if exact else binding.ACC_REF_F32)
    assert out["rc"] == 0, (what, out["rc"], S.mi355_last_error().decode())
    kern, launch = binding.last_conv_kernel(), binding.last_conv_launch()
    if g == "specialised":
        assert kern not in (6, 9), f"{what}: the dispatch keeps this shape for the specialised launchers, kernel {kern} served it"
    else:
        assert kern == g["kernel"], f"{what}: served by kernel {kern}, the restatement says {g['kernel']}"
        assert launch == (g["grid"], g["threads"], g["lds"]), f"{what}: launched (grid, threads, lds) = {launch}, the restatement says {g}"
    if exact:
        want_acc, want_u8 = ops.want["int32"], ops.want[store]
    else:
        want_acc, want_u8 = ops.want_ref_f32(store)
    _assert_bytes(cs, out, want_u8, what)
    _assert_dumps(out, want_acc, kg.oracle_dequant(want_u8), what)
    if exact:  # without dumps the same bytes, the same launch
        fast = _call(ops, store, dumps=False)
        assert fast["rc"] == 0 and np.array_equal(fast["y"], out["y"]), f"{what}: the call without dumps stores other bytes"
        if g != "specialised":
            assert (binding.last_conv_kernel(), binding.last_conv_launch()) == (9, launch)
    if cs.twin:  # the ref-f32 twin of the same call: one thread per output element
        OH, OW = cs.out_hw()
        t = kg.ref_f32_launch(cs.B, cs.n, OH, OW)
        out = _call(ops, store, binding.ACC_REF_F32)
        assert out["rc"] == 0 and binding.last_conv_kernel() == 6
        assert binding.last_conv_launch() == (t["grid"], t["threads"], t["lds"]) == (kg.cdiv(cs.B * cs.n * OH * OW, 256), 256, 0)
        want_acc, want_u8 = ops.want_ref_f32(store)
        _assert_bytes(cs, out, want_u8, f"{cs.name} ref-f32 twin")
        _assert_dumps(out, want_acc, kg.oracle_dequant(want_u8), f"{cs.name} ref-f32 twin")
