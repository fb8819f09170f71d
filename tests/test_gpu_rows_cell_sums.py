"""The row-image 3x3 kernels' sums of x' (conv_rows.hip, conv_rows16.hip), on the device.

The epilogue adds dz * sum(x') over each pixel's receptive field to its accumulator; the sums are built per cell of the LDS row image, one
64-channel chunk at a time.  conv_rows16.hip keeps a cell's running sum in a register of the thread that owns it for the whole K loop
(where a thread owns one cell) and hands the S plane to the epilogue once; the other instantiations add into the S plane per chunk.  The
int32 accumulator dump carries dz * sum(x') undisguised, so a wrong, stale or lost sum is a wrong integer here.

Every case goes through binding.conv_forward with and without the accumulator dump, under both stores and both plans, the tile forced
with mi355_conv_set_tile, and asserts

  * kernel id 5 and the (grid, threads, lds) that tests/launch_geometry.py restates for that tile (a case that drifted to another
    launcher fails instead of passing quietly), and the cell count rows_cap * RS the case is there for;
  * every int32 accumulator and every byte against launch_geometry.conv_acc_ref / conv_ref.

Operands that expose the sums: image 0 is all 0, image 1 all 255, the others random; zp_in 0, 255 and values in between; zp_w 0 and 255
on the first two filters (dz = 128 and -127), the rest 90 .. 165 (launch_geometry.rand_layer)."""
import numpy as np
import pytest

import launch_geometry as lg
import oracle
from yolo_quantization_amd import binding

pytestmark = pytest.mark.gpu

ZP_ACT, S_ACT = 23, np.float32(0.0625)


@pytest.fixture(scope="module", autouse=True)
def device():
    binding.init(0)


class Case:
    def __init__(self, name, c, n, B, H, W, bm, bn, zp_in, rows16, RS, cells=None, nt=0, act="leaky", tiles_min=1):
        self.name, self.c, self.n, self.B, self.H, self.W, self.bm, self.bn, self.zp_in = name, c, n, B, H, W, bm, bn, zp_in
        self.rows16, self.RS, self.cells, self.nt, self.act, self.tiles_min = rows16, RS, cells, nt, act, tiles_min

    def __repr__(self):
        return self.name

    def geom(self):
        return lg._conv_rows(lg.Trace(), self.B, self.H, self.W, self.c, self.n, 3, self.bm, self.bn, self.nt)


# threads of a workgroup: 256 (four waves) except the 128 x 256 / 128 x 384 tiles (512).  cells = rows_cap * RS of the plan.
CASES = [
    # ---- conv_rows16.hip, 16-slot rows, one cell per thread (sums in registers): 128 x 128, 64 x 128, 128 x 256
    # channel chunks: 1 (only the LAST body), 2, 3 (odd: both buffers, last chunk in buffer 0), 8
    Case("r16-128x128-c64-W12-cells=threads", 64, 128, 5, 2, 12, 128, 128, 0, True, 16, cells=256),  # one tile over five images: the bound
    Case("r16-128x128-c128-W12-cells<threads", 128, 128, 7, 7, 12, 128, 128, 255, True, 16, cells=240, tiles_min=5),
    Case("r16-128x128-c192-W13", 192, 128, 3, 13, 13, 128, 128, 9, True, 16, tiles_min=4),
    Case("r16-128x128-c512-W14", 512, 128, 4, 13, 14, 128, 128, 255, True, 16, tiles_min=6),
    Case("r16-128x128-c192-W13-more-tiles", 192, 256, 5, 13, 13, 128, 128, 0, True, 16, nt=9, tiles_min=9),
    Case("r16-64x128-c64-W12-cells=threads", 64, 64, 5, 2, 12, 64, 128, 255, True, 16, cells=256),
    Case("r16-64x128-c192-W13", 192, 64, 7, 7, 13, 64, 128, 0, True, 16, tiles_min=3),
    Case("r16-128x256-c128-W13", 128, 128, 6, 13, 13, 128, 256, 0, True, 16, tiles_min=4),
    Case("r16-128x256-c64-W14", 64, 128, 3, 13, 14, 128, 256, 255, True, 16, tiles_min=3),
    # ---- conv_rows16.hip, two cells per thread (sums in the S plane per chunk): below, at and above the thread count
    Case("r16-128x192-c128-W12-cells<threads", 128, 128, 3, 13, 12, 128, 192, 255, True, 16, cells=240, tiles_min=3),
    Case("r16-128x192-c64-W12-cells=threads", 64, 128, 5, 2, 12, 128, 192, 0, True, 16, cells=256),
    Case("r16-128x192-c192-W12-cells>threads", 192, 128, 4, 3, 12, 128, 192, 9, True, 16, cells=272),
    Case("r16-64x256-c128-W14-cells<threads", 128, 64, 3, 13, 14, 64, 256, 0, True, 16, cells=240, tiles_min=3),
    Case("r16-64x256-c192-W12-cells>threads", 192, 64, 4, 3, 12, 64, 256, 255, True, 16, cells=272),
    Case("r16-128x384-c128-W12-cells<threads", 128, 128, 6, 4, 12, 128, 384, 0, True, 16, cells=496),
    Case("r16-128x384-c192-W12-cells>threads", 192, 128, 4, 7, 12, 128, 384, 255, True, 16, cells=528),
    Case("r16-128x384-c64-W19-extra-slots", 64, 128, 3, 19, 19, 128, 384, 9, True, 32, tiles_min=3),
    # ---- conv_rows.hip (sums in the S plane per chunk): 32-filter tiles on 16-slot rows, 32- and 64-slot rows
    Case("rows-32x128-c128-W13", 128, 32, 3, 13, 13, 32, 128, 255, False, 16, tiles_min=4),
    Case("rows-128x128-c128-W24", 128, 128, 3, 6, 24, 128, 128, 0, False, 32, tiles_min=4),
    Case("rows-128x128-c192-W26", 192, 128, 3, 5, 26, 128, 128, 255, False, 32, tiles_min=4),
    Case("rows-128x192-c64-W30", 64, 128, 3, 7, 30, 128, 192, 9, False, 32, tiles_min=4),
    Case("rows-64x256-c128-W26", 128, 64, 3, 6, 26, 64, 256, 0, False, 32, tiles_min=2),
    Case("rows-128x128-c128-W48", 128, 128, 3, 4, 48, 128, 128, 255, False, 64, tiles_min=5),
    Case("rows-128x128-c64-W62", 64, 128, 3, 3, 62, 128, 128, 0, False, 64, tiles_min=5),
]


def operands(cs):
    rng = np.random.default_rng(sum(map(ord, cs.name)))
    x = rng.integers(0, 256, (cs.B, cs.c, cs.H, cs.W), dtype=np.uint8)
    x[0], x[1] = 0, 255
    wq, zp_w, bias, mv, sv = lg.rand_layer(rng, cs.n, cs.c, 3, "much-wrap")
    assert zp_w[0] == 0 and zp_w[1] == 255
    return x, wq, zp_w, bias, mv, sv


def force_tile(cs):
    binding.shim().mi355_conv_set_tile(cs.bm | (cs.nt << 16), cs.bn)


def release():
    S = binding.shim()
    S.mi355_conv_set_tile(0, 0)
    S.mi355_debug_flags(0)


def assert_launch(cs, g, what, extra_lds=0):
    got = (binding.last_conv_kernel(), binding.last_conv_launch())
    assert got == (5, (g["grid"], g["threads"], g["lds"] + extra_lds)), f"{what}: launched {got}, the restatement says {g}"


@pytest.mark.parametrize("cs", CASES, ids=repr)
def test_accumulators_and_bytes(cs):
    g = cs.geom()
    assert g["refused"] is None and g["rows16"] == cs.rows16 and g["RS"] == cs.RS and (g["bm"], g["bn"]) == (cs.bm, cs.bn), g
    assert g["ntiles"] >= cs.tiles_min, g
    threads = g["threads"]
    if cs.cells is not None:
        assert g["rows_cap"] * cs.RS == cs.cells, (g["rows_cap"], cs.RS, cs.cells)
    print(f"{cs.name}: rows_cap {g['rows_cap']} x {cs.RS} = {g['rows_cap'] * cs.RS} cells, {threads} threads, {g['ntiles']} x {g['mtiles']} tiles of <= "
          f"{-(-g['total'] // g['ntiles'])} pixels, {cs.c // 64} chunks")
    x, wq, zp_w, bias, mv, sv = operands(cs)
    acc, OH, OW = lg.conv_acc_ref(x, wq, zp_w, 3, 1, cs.zp_in)
    want_acc = np.ascontiguousarray(acc.reshape(cs.n, cs.B, OH * OW).transpose(1, 0, 2))
    act = binding.ACT[cs.act]
    S = binding.shim()
    try:
        for store_name, store, ostore in (("wrap", binding.STORE_WRAP, oracle.STORE_WRAP), ("sat", binding.STORE_SATURATE, oracle.STORE_SATURATE)):
            u8 = oracle.requant(acc, bias, mv, sv, ZP_ACT, oracle.ACT[cs.act], ostore)
            want_u8 = np.ascontiguousarray(u8.reshape(cs.n, cs.B, OH, OW).transpose(1, 0, 2, 3))
            for plan in (0, 1):
                for want in (True, False):
                    what = f"{cs.name} store {store_name} plan {plan} dump {want}"
                    S.mi355_debug_flags(lg.GEN)
                    force_tile(cs)
                    xt = binding.DevTensor.from_nchw(x, cs.zp_in)
                    out = binding.conv_forward(xt, wq, zp_w, 3, bias, mv, sv, cs.zp_in, ZP_ACT, S_ACT, act, store=store, want_acc=want, plan=plan)
                    assert_launch(cs, g, what)
                    if want:
                        bad = np.argwhere(out["int32"] != want_acc)
                        assert not len(bad), f"{what}: {len(bad)} int32 accumulators differ, first at (b, ch, pixel) = {bad[:4].tolist()}"
                    bad = np.argwhere(out["u8"] != want_u8)
                    assert not len(bad), f"{what}: {len(bad)} bytes differ, first at (b, ch, y, x) = {bad[:4].tolist()}"
    finally:
        release()


def _fused_case():
    return Case("r16-128x128-c128-W13-fused", 128, 128, 3, 13, 13, 128, 128, 255, True, 16, act="leaky")


@pytest.mark.parametrize("store_name", ["wrap", "sat"])
def test_fused_upsample_behind_the_handover(store_name):
    """the untouched epilogue's upsample store behind the new hand-over of S: every pixel 2 x 2 times"""
    cs = _fused_case()
    g = cs.geom()
    x, wq, zp_w, bias, mv, sv = operands(cs)
    store, ostore = (binding.STORE_WRAP, oracle.STORE_WRAP) if store_name == "wrap" else (binding.STORE_SATURATE, oracle.STORE_SATURATE)
    want = lg.conv_ref(x, wq, zp_w, 3, 1, cs.zp_in, bias, mv, sv, ZP_ACT, oracle.ACT[cs.act], ostore)
    want = want.repeat(2, axis=2).repeat(2, axis=3)
    S = binding.shim()
    try:
        for plan in (0, 1):
            S.mi355_debug_flags(lg.GEN)
            force_tile(cs)
            xt = binding.DevTensor.from_nchw(x, cs.zp_in)
            out = binding.conv_fused_forward(xt, wq, zp_w, 3, bias, mv, sv, cs.zp_in, ZP_ACT, S_ACT, binding.ACT[cs.act], "upsample", store=store, plan=plan)
            assert_launch(cs, g, f"upsample plan {plan}")
            bad = np.argwhere(out["u8"] != want)
            assert not len(bad), f"plan {plan}: {len(bad)} bytes differ, first at (b, ch, y, x) = {bad[:4].tolist()}"
    finally:
        release()


@pytest.mark.parametrize("store_name", ["wrap", "sat"])
def test_fused_yolo_head_behind_the_handover(store_name):
    """a 3x3 yolo head (linear, 3 x (5 + 80) filters: two filter tiles, the second one short) through the row-image kernel: bytes, the float tail, the yolo activations"""
    classes = 80
    cs = Case("r16-128x128-c128-W13-yolo", 128, 3 * (5 + classes), 3, 13, 13, 128, 128, 0, True, 16, act="linear")
    g = cs.geom()
    x, wq, zp_w, bias, mv, sv = operands(cs)
    store, ostore = (binding.STORE_WRAP, oracle.STORE_WRAP) if store_name == "wrap" else (binding.STORE_SATURATE, oracle.STORE_SATURATE)
    want = lg.conv_ref(x, wq, zp_w, 3, 1, cs.zp_in, bias, mv, sv, ZP_ACT, oracle.ACT[cs.act], ostore)
    f = ((want.astype(np.int32) - ZP_ACT).astype(np.float32) * S_ACT).reshape(cs.B, cs.n, -1)
    S = binding.shim()
    try:
        for plan in (0, 1):
            S.mi355_debug_flags(lg.GEN)
            force_tile(cs)
            xt = binding.DevTensor.from_nchw(x, cs.zp_in)
            out = binding.conv_fused_forward(xt, wq, zp_w, 3, bias, mv, sv, cs.zp_in, ZP_ACT, S_ACT, binding.ACT[cs.act], "yolo", store=store, plan=plan,
                                             classes=classes)
            assert_launch(cs, g, f"yolo plan {plan}", extra_lds=1024)  # + the logistic table of a fused head
            assert np.array_equal(out["u8"], want), f"plan {plan}: bytes"
            assert np.array_equal(out["f32"], f), f"plan {plan}: the float tail"
            e = np.arange(cs.n) % (5 + classes)
            raw = (e == 2) | (e == 3)
            assert np.array_equal(out["yolo"][:, raw], f[:, raw]), f"plan {plan}: w / h entries pass through"
            # logistic of 256 possible values in float: a few ulp of a number in (0, 1)
            logi = 1.0 / (1.0 + np.exp(-f[:, ~raw].astype(np.float64)))
            assert np.abs(out["yolo"][:, ~raw] - logi).max() <= 1e-6, f"plan {plan}: logistic entries"
    finally:
        release()
