"""Every conv launcher's tile geometry at its switch points, on the device.

tests/launch_geometry.py restates what each launcher decides and lists one case on each side of every labelled clause (many tiny
images wherever a clause depends on a tile or pixel count: tile counts scale with B, not with the map).  Each case here

  * runs the layer through the C-ABI entry the host uses (mi355_conv_forward, mi355_conv_pool_forward with a pooled-size or a
    conv-size ypool, the per-image forms) under the plan and the debug flags the case names;
  * asserts that mi355_last_conv_kernel() and mi355_last_conv_launch() are the restatement's family and (grid, threads, lds): a case
    that drifted off its clause fails instead of passing quietly;
  * compares every output byte with the exact reference (launch_geometry.conv_ref), under both store modes, bit for bit;
  * where the case names a second route (a debug switch that sends the same call to another family), does the same there.

One clause is not pinned on the device: conv_small.hip's persistent grid is clamped once more by the workgroups per CU that the kernel's
registers allow, which only the code object knows, so a launch of min(ntiles, 256 k) workgroups is accepted for every k up to the restated
per_cu.  A launcher whose per_cu dropped from 3 to 2 would pass here; the LDS arithmetic behind per_cu is held by the CPU sweep.

No knob that changes the geometry behind the restatement's back may be set."""
import ctypes as C
import os

import numpy as np
import pytest

import launch_geometry as lg
import oracle
from yolo_quantization_amd import binding

pytestmark = pytest.mark.gpu

KNOBS = ("MI355_MID_TP", "MI355_MID_FULL", "MI355_SMALL_PER_CU", "MI355_S32_PER_CU", "MI355_P16_GRID", "MI355_L0_GRID")
_set = [k for k in KNOBS if k in os.environ]
assert not _set, f"{_set} would silently change the launch geometry these tests pin: unset them"


@pytest.fixture(scope="module", autouse=True)
def device():
    binding.init(0)


class _Planar:
    """the reference's [B][3][H][W] planes, read in place"""

    def __init__(self, x):
        self.buf = binding.DevBuf.from_numpy(x)
        self.t = binding.Tensor(self.buf.ptr, x.shape[0], x.shape[2], x.shape[3], x.shape[1], 1, 0, 0)

    def ref(self):
        return C.byref(self.t)


class Operands:
    """one case's image batch and layer, and the exact reference under both store modes (computed once)"""

    def __init__(self, cs):
        rng = np.random.default_rng(sum(map(ord, cs.name)))
        self.cs = cs
        self.x = rng.integers(0, 256, (cs.B, cs.c, cs.H, cs.W), dtype=np.uint8)
        self.wq, self.zp_w = lg.rand_layer(rng, cs.n, cs.c, cs.k)[:2]
        self.zp_act, self.s_act, self.act = 23, np.float32(0.0625), binding.ACT[cs.act]
        if cs.per_image:  # two bank entries (the same weights packed for two input scales) and every image's own zero point
            self.entry_of = rng.integers(0, 2, cs.B).astype(np.int32)
            self.zp_in = rng.integers(0, 256, cs.B).astype(np.uint8)
        else:
            self.zp_in = 0 if cs.c == 3 else 9
        acc, OH, OW = lg.conv_acc_ref(self.x, self.wq, self.zp_w, cs.k, cs.stride, self.zp_in)
        # "some-wrap" multipliers; maps of a few pixels are mostly padding and their small accumulators do not leave the byte under them:
        # there the stronger regime, so that the two store modes differ in every case that is large enough to tell
        for gain in ("some-wrap", "much-wrap"):
            self.entries = [lg.rand_layer(rng, cs.n, cs.c, cs.k, gain)[2:] for _ in range(2 if cs.per_image else 1)]
            self.bias, self.mv, self.sv = self.entries[0]
            self.want = self._reference(acc, OH, OW)
            if self.stores_differ():
                break

    def stores_differ(self):
        return bool((self.want["wrap"] != self.want["sat"]).any())

    def _reference(self, acc, OH, OW):
        cs = self.cs
        want = {}
        for name, store in (("wrap", binding.STORE_WRAP), ("sat", binding.STORE_SATURATE)):
            if cs.per_image:
                u8 = np.empty(acc.shape, np.uint8)
                col_entry = np.repeat(self.entry_of, OH * OW)
                for e, (b, m, s) in enumerate(self.entries):
                    sel = col_entry == e
                    u8[:, sel] = oracle.requant(np.ascontiguousarray(acc[:, sel]), b, m, s, self.zp_act, oracle.ACT[cs.act], store)
            else:
                u8 = oracle.requant(acc, self.bias, self.mv, self.sv, self.zp_act, oracle.ACT[cs.act], store)
            u8 = u8.reshape(cs.n, cs.B, OH, OW).transpose(1, 0, 2, 3)
            if cs.fuse == "pool2":
                u8 = lg.maxpool2(u8)
            elif cs.fuse == "pool1":
                u8 = lg.maxpool1(u8)
            want[name] = np.ascontiguousarray(u8)
        return want

    def run(self, store, flags):
        """-> (output bytes [B, n, OH, OW], (kernel id, (grid, threads, lds)))"""
        cs = self.cs
        S = binding.shim()
        st = binding.STORE_WRAP if store == "wrap" else binding.STORE_SATURATE
        xt = _Planar(self.x) if cs.planar else binding.DevTensor.from_nchw(self.x, 0 if cs.per_image else self.zp_in)
        args = (self.wq, self.zp_w, cs.k, self.bias, self.mv, self.sv, 0 if cs.per_image else self.zp_in, self.zp_act, self.s_act, self.act)
        S.mi355_debug_flags(flags)
        try:
            if cs.per_image:
                out = self._run_per_image(xt, st)
            elif cs.fuse:
                out = binding.conv_fused_forward(xt, *args, cs.fuse, store=st, plan=cs.plan, epilogue=cs.epilogue)["u8"]
            else:
                out = binding.conv_forward(xt, *args, store=st, want_acc=False, stride=cs.stride, plan=cs.plan, epilogue=cs.epilogue)["u8"]
        finally:
            S.mi355_debug_flags(0)
        return out, (binding.last_conv_kernel(), binding.last_conv_launch())

    def _run_per_image(self, xt, st):
        cs = self.cs
        S = binding.shim()
        ept = (self.act, self.zp_act) if cs.epilogue else ()
        blobs = [binding.conv_pack(self.wq, self.zp_w, cs.c, cs.k, b, m, s, *ept) for b, m, s in self.entries]
        eb = (len(blobs[0]) + 15) & ~15
        bank = np.zeros(2 * eb, np.uint8)
        for e, bl in enumerate(blobs):
            bank[e * eb:e * eb + len(bl)] = bl
        bank_d, ent_d, zp_d = binding.DevBuf.from_numpy(bank), binding.DevBuf.from_numpy(self.entry_of), binding.DevBuf.from_numpy(self.zp_in)
        d = binding.ConvDesc(cs.n, cs.c, cs.k, 1, 1, self.act, st, binding.ACC_EXACT, 0, self.zp_act, float(self.s_act), cs.plan, int(cs.epilogue))
        if cs.fuse == "pool2":
            y = binding.DevTensor(cs.B, cs.H // 2, cs.W // 2, cs.n, self.zp_act)
            binding.check(S.mi355_conv_pool_forward_per_image(C.byref(d), xt.ref(), bank_d.ptr, eb, ent_d.ptr, zp_d.ptr, None, y.ref(), None),
                          "conv_pool_forward_per_image")
        else:
            y = binding.DevTensor(cs.B, cs.H, cs.W, cs.n, self.zp_act)
            binding.check(S.mi355_conv_forward_per_image(C.byref(d), xt.ref(), bank_d.ptr, eb, ent_d.ptr, zp_d.ptr, None, None, y.ref(), None,
                                                         None, None), "conv_forward_per_image")
        binding.check(S.mi355_stream_sync(None), "sync")
        return y.to_nchw()


def assert_launch(cs, flags, got, what):
    """the launch is the one the restatement names under these flags"""
    import copy
    c2 = copy.copy(cs)
    c2.flags = flags
    _, g, refusals = lg.trace_case(c2)
    assert g is not None
    kern, (grid, threads, lds) = got
    refused = [r["family"] + ":" + r["refused"] for r in refusals]
    assert kern == g["kernel"], f"{what}: served by kernel {kern}, the restatement says {g['family']} ({g['kernel']}) after {refused}"
    grids = [g["grid"]]
    if g["family"] == "conv_small":  # the launch clamps a persistent grid to what the kernel's registers allow per CU (the code object decides)
        grids = sorted({min(g["ntiles"], 256 * k) for k in range(1, g["per_cu"] + 1)})
    assert grid in grids and (threads, lds) == (g["threads"], g["lds"]), \
        f"{what}: launched (grid, threads, lds) = {(grid, threads, lds)}, the restatement says {grids} x {(g['threads'], g['lds'])} ({g['family']} after {refused}: {g})"


@pytest.mark.parametrize("cs", lg.CASES, ids=repr)
def test_launch_geometry_and_bytes(cs):
    _, g, refusals = lg.trace_case(cs)
    ops = Operands(cs)
    if ops.want["wrap"].size >= 4096:
        assert ops.stores_differ(), "wrap and saturate give the same bytes: the weights do not exercise the store modes"
    if g is None:  # the fused call is refused outright: the host runs the two layers apart
        with pytest.raises(binding.MI355Error, match="code -22"):
            ops.run(cs.store, cs.flags)
        return
    other = "sat" if cs.store == "wrap" else "wrap"
    for store in (cs.store, other):
        out, got = ops.run(store, cs.flags)
        assert_launch(cs, cs.flags, got, f"store {store}")
        bad = np.argwhere(out != ops.want[store])
        assert not len(bad), f"store {store}: {len(bad)} bytes differ from the reference, first at (b, ch, y, x) = {bad[:4].tolist()} ({g})"
    if cs.alt is not None:
        out, got = ops.run(cs.store, cs.alt)
        assert_launch(cs, cs.alt, got, f"route under flags {cs.alt:#x}")
        assert got[0] != g["kernel"] or cs.alt == lg.F_SMALL and cs.c == 3, "the second route is the same family"
        bad = np.argwhere(out != ops.want[cs.store])
        assert not len(bad), f"route under flags {cs.alt:#x}: {len(bad)} bytes differ from the reference, first at {bad[:4].tolist()}"
