"""The kernels between the convs at their edges, on the device: every case of tests/glue_edges.py through the C-ABI entry points.

One helper holds the invariant the conv kernels rely on.  Every output tensor (`Out`) lives inside a larger buffer of sentinel bytes, is filled
with mi355_tensor_fill (which is checked on the way) and photographed; after the call the WHOLE buffer is compared with the photograph plus the
bytes the reference says the call owns.  So a store into a pad cell (column W, the lead row, lead, tail), into a neighbouring channel window or
outside the tensor fails the case that makes it, wherever it lands; the message says which kind of byte was hit.  Flat outputs (float tensors,
quantised bytes, min / max pairs, checksums) sit between sentinel guards in the same way (`Flat`).  Inputs (`In`) carry uint8 0xff in all their
pad cells, the byte that would win a max pool, and random bytes in every channel the call must not read.

Refusals return MI355_EINVAL with their message and leave every byte as it was."""
import ctypes as C

import numpy as np
import pytest

import glue_edges as ge
import oracle
from yolo_quantization_amd import binding

pytestmark = pytest.mark.gpu

G = ge.GUARD


@pytest.fixture(scope="module", autouse=True)
def device():
    binding.init(0)
    binding.shim().mi355_checksum_u32.argtypes = [C.c_void_p, C.c_long, C.c_void_p, C.c_void_p]


def S():
    return binding.shim()


def refused(rc, message):
    assert rc == ge.EINVAL, f"code {rc} instead of MI355_EINVAL"
    assert S().mi355_last_error().decode() == "invalid argument: " + message


def _tensor(base, cells, Cc, off, over):
    d = dict(B=cells.B, H=cells.H, W=cells.W, C=Cc, cs=cells.cs, lead=cells.lead, tail=cells.tail)
    d.update(over)
    return binding.Tensor(base + off if base is not None else None, d["B"], d["H"], d["W"], d["C"], d["cs"], d["lead"], d["tail"])


class In:
    """an input operand: `full` [B][cs][H][W] are the plain bytes of every interior cell, the pad cells hold uint8 0xff"""

    def __init__(self, B, H, W, t, full):
        self.cells, self.t = ge.Cells(B, H, W, t.cs, t.lead), t
        raw = np.full(self.cells.nbytes, 0xff ^ self.cells.bias, np.uint8)
        self.cells.put(raw, full)
        self.buf = binding.DevBuf.from_numpy(raw)

    def tensor(self, Cc, off=None, **over):
        return _tensor(self.buf.ptr.value, self.cells, Cc, self.t.off if off is None else off, over)


class Out:
    """an output tensor inside a sentinel buffer: filled through mi355_tensor_fill, photographed, compared whole"""
    KIND = ("an interior byte of the written channels", "a byte of a neighbouring channel window / pad channel", "a byte of a pad cell")

    def __init__(self, B, H, W, t, zp):
        assert zp in ge.ZERO_POINTS
        self.cells, self.t, self.zp = ge.Cells(B, H, W, t.cs, t.lead), t, zp
        n = self.cells.nbytes
        host = np.full(2 * G + n, ge.SENTINEL, np.uint8)
        self.buf = binding.DevBuf.from_numpy(host)
        binding.check(S().mi355_tensor_fill(C.byref(self.tensor(t.wide, 0)), zp, None), "tensor_fill")
        self.snap = self.read()
        body = host[G:G + n].reshape(self.cells.ncells, t.cs)
        if t.cs == 4:  # (zp, zp, zp, 0) cells, plain
            body[:, :3], body[:, 3] = zp, 0
        else:
            body[:] = zp ^ 0x80
        assert np.array_equal(self.snap, host), "mi355_tensor_fill: every byte of the tensor, pads included, and nothing around it"

    def tensor(self, Cc, off=None, **over):
        return _tensor(self.buf.ptr.value + G, self.cells, Cc, self.t.off if off is None else off, over)

    def read(self):
        return self.buf.to_numpy(np.uint8, self.buf.nbytes)

    def check(self, writes, Cc=0, what=""):
        """writes: [(first byte in the cell, plain [B][n][H][W] bytes)], applied in order to the photograph; everything else must equal it"""
        want = self.snap.copy()
        for off, x in writes:
            self.cells.put(want[G:G + self.cells.nbytes], x, off)
        got = self.read()
        if np.array_equal(got, want):
            return got
        bad = np.flatnonzero(got != want)
        inside = bad[(bad >= G) & (bad < G + self.cells.nbytes)] - G
        kinds = self.cells.kinds(self.t.off, Cc)[inside]
        msg = [f"{what}: {bad.size} bytes differ"]
        if inside.size < bad.size:
            msg.append(f"{bad.size - inside.size} of them OUTSIDE the tensor")
        for k in range(3):
            if (kinds == k).any():
                at = int(inside[kinds == k][0])
                msg.append(f"{int((kinds == k).sum())} x {self.KIND[k]} (first: cell {at // self.cells.cs} byte {at % self.cells.cs}: "
                           f"{got[G + at]:#x}, want {want[G + at]:#x})")
        raise AssertionError("; ".join(msg))


class Flat:
    """nbytes of output between two guards, `off` bytes past an aligned address; everything starts as `init`"""

    def __init__(self, nbytes, off=0, init=ge.SENTINEL):
        self.n, self.off = nbytes, off
        host = np.full(2 * G + off + nbytes, ge.SENTINEL, np.uint8)
        host[G + off:G + off + nbytes] = init
        self.snap = host
        self.buf = binding.DevBuf.from_numpy(host)
        self.ptr = self.buf.ptr.value + G + off

    def check(self, want=None, what=""):
        """the payload (the photograph when want is None) and both guards, byte for byte"""
        exp = self.snap.copy()
        if want is not None:
            exp[G + self.off:G + self.off + self.n] = np.ascontiguousarray(want).view(np.uint8).ravel()
        got = self.buf.to_numpy(np.uint8, self.buf.nbytes)
        bad = np.flatnonzero(got != exp)
        if bad.size:
            lo, hi = G + self.off, G + self.off + self.n
            guard = int(((bad < lo) | (bad >= hi)).sum())
            raise AssertionError(f"{what}: {bad.size} bytes differ, {guard} of them in the guards; first at payload byte {int(bad[0]) - lo}: "
                                 f"{got[bad[0]]:#x}, want {exp[bad[0]]:#x}")
        return got[G + self.off:G + self.off + self.n]


def owned(ref, full, off, Cc, *args):
    """the writes of a group kernel: the reference on the logical channels, then on the pad channels behind them up to the 16-byte group"""
    w = [ref(full[:, off:off + Cc], *args)]
    if Cc % 16:
        w.append(ref(full[:, off + Cc:off + ge.up16(Cc)], *args))
    return w


# ------------------------------------------------------------------------------------------------------------------------------- max pool
@pytest.mark.parametrize("cs", ge.POOL_CASES, ids=lambda c: c.name)
def test_maxpool(cs):
    full, _ = ge.pool_inputs(cs)
    x = In(cs.B, cs.H, cs.W, cs.x, full)
    OH, OW = ge.pool_out(cs.H, cs.size, cs.stride, cs.pad), ge.pool_out(cs.W, cs.size, cs.stride, cs.pad)
    y = Out(cs.B, OH, OW, cs.y, 23)
    binding.check(S().mi355_maxpool_forward(C.byref(x.tensor(cs.C)), C.byref(y.tensor(cs.C)), cs.size, cs.stride, cs.pad, None), cs.name)
    want = owned(ge.maxpool_ref, full, cs.x.off, cs.C, cs.size, cs.stride, cs.pad)
    if ge.pool_has_outside_window(cs):
        assert (want[0] == 0).any(), "a window that lies wholly outside the image stores exactly 0"
    y.check([(cs.y.off, want[0])] + [(cs.y.off + cs.C, w) for w in want[1:]], cs.C, cs.name)


def test_maxpool_refusals():
    x = In(3, 6, 6, ge.plain(16), ge.operand_bytes("refuse", 3, 6, 6, ge.plain(16)))
    y = Out(3, 3, 3, ge.plain(16), 23)
    binding.check(S().mi355_maxpool_forward(C.byref(x.tensor(16)), C.byref(y.tensor(16)), 2, 2, 0, None), "the legal call")
    y = Out(3, 3, 3, ge.plain(16), 23)
    for label, message, ch in ge.POOL_REFUSALS:
        xt = x.tensor(16, **({"cs": ch["xcs"]} if "xcs" in ch else {}))
        over = {k[1:] if k != "ycs" else "cs": v for k, v in ch.items() if k in ("yC", "yB", "yH", "yW", "ycs")}
        yt = y.tensor(over.pop("C", 16), **over)
        rc = S().mi355_maxpool_forward(C.byref(xt), C.byref(yt), ch.get("size", 2), ch.get("stride", 2), ch.get("pad", 0), None)
        refused(rc, message)
        y.check([], 16, label)
    null = binding.Tensor(None, 3, 3, 3, 16, 16, 2, 6)
    refused(S().mi355_maxpool_forward(C.byref(x.tensor(16)), C.byref(null), 2, 2, 0, None), "maxpool: null")
    refused(S().mi355_maxpool_forward(None, C.byref(y.tensor(16)), 2, 2, 0, None), "maxpool: null")
    y.check([], 16, "null")


# ------------------------------------------------------------------------------------------------------------------- upsample and route
@pytest.mark.parametrize("cs", ge.UP_CASES, ids=lambda c: c.name)
def test_upsample(cs):
    full = ge.operand_bytes(cs.name, cs.B, cs.H, cs.W, cs.x, lo=0)
    x = In(cs.B, cs.H, cs.W, cs.x, full)
    y = Out(cs.B, cs.H * cs.stride, cs.W * cs.stride, cs.y, 77)
    binding.check(S().mi355_upsample_forward(C.byref(x.tensor(cs.C)), C.byref(y.tensor(cs.C)), cs.stride, None), cs.name)
    want = owned(ge.upsample_ref, full, cs.x.off, cs.C, cs.stride)
    y.check([(cs.y.off, want[0])] + [(cs.y.off + cs.C, w) for w in want[1:]], cs.C, cs.name)


def test_upsample_refusals():
    x = In(3, 3, 4, ge.plain(16), ge.operand_bytes("refuse", 3, 3, 4, ge.plain(16)))
    y = Out(3, 6, 8, ge.plain(16), 77)
    for label, xo, yo, stride in (("stride does not match", {}, {}, 3), ("stride 0", {}, {}, 0), ("C mismatch", {}, {"C": 15}, 2),
                                  ("B mismatch", {}, {"B": 2}, 2), ("x is the 4-byte image", {"cs": 4}, {}, 2), ("y is the 4-byte image", {}, {"cs": 4}, 2)):
        yo = dict(yo)
        rc = S().mi355_upsample_forward(C.byref(x.tensor(16, **xo)), C.byref(y.tensor(yo.pop("C", 16), **yo)), stride, None)
        refused(rc, "upsample: shape")
        y.check([], 16, label)
    refused(S().mi355_upsample_forward(None, C.byref(y.tensor(16)), 2, None), "upsample: null")


def _route_call(tensors, yt):
    arr = (C.POINTER(binding.Tensor) * len(tensors))(*[C.pointer(t) for t in tensors])
    return S().mi355_route_forward(arr, len(tensors), C.byref(yt), None)


@pytest.mark.parametrize("cs", ge.ROUTE_CASES, ids=lambda c: c.name)
def test_route(cs):
    bufs, tensors, logical, last = {}, [], [], None
    for i, (c, t) in enumerate(zip(cs.Cs, cs.xs)):
        key = (t.cs, t.lead, t.wide) if ge.is_window(t, c) else i  # windows of one wide tensor share its buffer
        if key not in bufs:
            full = ge.operand_bytes(f"{cs.name}/{key}", cs.B, cs.H, cs.W, t, lo=0)
            bufs[key] = (full, In(cs.B, cs.H, cs.W, t, full))
        full, x = bufs[key]
        tensors.append(x.tensor(c, t.off))
        logical.append(full[:, t.off:t.off + c])
        last = full[:, t.off + c:t.off + ge.up16(c)]
    total = sum(cs.Cs)
    y = Out(cs.B, cs.H, cs.W, cs.y, 77)
    binding.check(_route_call(tensors, y.tensor(total)), cs.name)
    writes = [(cs.y.off, ge.route_ref(logical))]
    if ge.route_aligned(cs.Cs) and cs.Cs[-1] % 16:  # the group path: the last input's pad bytes land in y's own padding
        writes.append((cs.y.off + total, last))
    y.check(writes, total, cs.name)


def test_route_refusals():
    fulls = [ge.operand_bytes(f"r{i}", 3, 3, 5, ge.plain(16)) for i in range(2)]
    xs = [In(3, 3, 5, ge.plain(16), f) for f in fulls]
    y = Out(3, 3, 5, ge.plain(32), 77)
    ok = [x.tensor(16) for x in xs]
    for label, tensors, yt, message in (
            ("channel sum", ok, y.tensor(31), "route: channel sum != y.C"), ("channel sum, one input", ok[:1], y.tensor(32), "route: channel sum != y.C"),
            ("map", [ok[0], xs[1].tensor(16, W=4)], y.tensor(32), "route: input layout"), ("rows", [xs[0].tensor(16, H=2), ok[1]], y.tensor(32), "route: input layout"),
            ("batch", [ok[0], xs[1].tensor(16, B=2)], y.tensor(32), "route: input layout"),
            ("a 4-byte image input", [ok[0], xs[1].tensor(16, cs=4)], y.tensor(32), "route: input layout"),
            ("a null input", [ok[0], binding.Tensor(None, 3, 3, 5, 16, 16, 2, 8)], y.tensor(32), "route: input layout")):
        refused(_route_call(tensors, yt), message)
        y.check([], 32, label)
    refused(S().mi355_route_forward(None, 2, C.byref(y.tensor(32)), None), "route: null")
    arr = (C.POINTER(binding.Tensor) * 2)(*[C.pointer(t) for t in ok])
    refused(S().mi355_route_forward(arr, 0, C.byref(y.tensor(32)), None), "route: null")
    y.check([], 32, "null")


# --------------------------------------------------------------------------------------------------------------------------------- shortcut
@pytest.fixture(scope="module")
def pairs():
    a, b = ge.shortcut_pairs()
    t = ge.plain(16)
    return a, b, In(1, 256, 256, t, a), In(1, 256, 256, t, b)


def _shortcut(a, b, y, s, Cc=16):
    return S().mi355_shortcut_forward(C.byref(a), C.byref(b), C.byref(y), s.Ka, s.Kb, s.za, s.zb, s.zo, None)


@pytest.mark.parametrize("s", ge.SC_SETS, ids=lambda s: s.name)
def test_shortcut_all_byte_pairs(pairs, s):
    """all 65 536 (a, b) pairs in every lane of the group, one launch per parameter set"""
    a, b, ta, tb = pairs
    y = Out(1, 256, 256, ge.plain(16), 23)
    binding.check(_shortcut(ta.tensor(16), tb.tensor(16), y.tensor(16), s), s.name)
    y.check([(0, ge.shortcut_ref(a, b, s))], 16, s.name)


def test_shortcut_ragged_channels_three_layouts():
    r = ge.SC_RAGGED
    fa, fb = (ge.operand_bytes(n, r.B, r.H, r.W, t, lo=0) for n, t in (("sa", r.a), ("sb", r.b)))
    a, b = In(r.B, r.H, r.W, r.a, fa), In(r.B, r.H, r.W, r.b, fb)
    y = Out(r.B, r.H, r.W, r.y, 23)
    binding.check(_shortcut(a.tensor(r.C), b.tensor(r.C), y.tensor(r.C), r.s), "ragged")
    n = ge.up16(r.C)
    pa, pb = fa[:, r.a.off:r.a.off + n], fb[:, r.b.off:r.b.off + n]
    y.check([(r.y.off, ge.shortcut_ref(pa[:, :r.C], pb[:, :r.C], r.s)), (r.y.off + r.C, ge.shortcut_ref(pa[:, r.C:], pb[:, r.C:], r.s))], r.C, "ragged")


def test_shortcut_refusals():
    t = ge.plain(16)
    a, b = (In(3, 4, 5, t, ge.operand_bytes(n, 3, 4, 5, t)) for n in "ab")
    y = Out(3, 4, 5, t, 23)
    s = ge.Sc("ok", 40000, 70000, 3, 200, 100, "corners")
    share = "shortcut: both inputs and the output must share batch, map size and channels"
    mult = "shortcut: multipliers must be in [1, 2^21)"
    for label, ao, bo, yo, so, message in (
            ("y one column wider", {}, {}, {"W": 6}, {}, share), ("b one row short", {}, {"H": 3}, {}, {}, share), ("a other batch", {"B": 2}, {}, {}, {}, share),
            ("b other channels", {}, {"C": 15}, {}, {}, share), ("y other channels", {}, {}, {"C": 17}, {}, share),
            ("Ka 0", {}, {}, {}, {"Ka": 0}, mult), ("Ka 2^21", {}, {}, {}, {"Ka": 1 << 21}, mult), ("Kb 0", {}, {}, {}, {"Kb": 0}, mult),
            ("Kb 2^21", {}, {}, {}, {"Kb": 1 << 21}, mult), ("Ka negative", {}, {}, {}, {"Ka": -5}, mult),
            ("a is the 4-byte image", {"cs": 4}, {}, {}, {}, "shortcut: layout"), ("b is the 4-byte image", {}, {"cs": 4}, {}, {}, "shortcut: layout"),
            ("y is the 4-byte image", {}, {}, {"cs": 4}, {}, "shortcut: layout")):
        ao, bo, yo = dict(ao), dict(bo), dict(yo)
        rc = _shortcut(a.tensor(ao.pop("C", 16), **ao), b.tensor(bo.pop("C", 16), **bo), y.tensor(yo.pop("C", 16), **yo), s._replace(**so))
        refused(rc, message)
        y.check([], 16, label)
    refused(S().mi355_shortcut_forward(None, C.byref(b.tensor(16)), C.byref(y.tensor(16)), 1, 1, 0, 0, 0, None), "shortcut: null")


# ------------------------------------------------------------------------------------------------------------ layout converters and fill
def _nchw_to_tensor(cs, x):
    src = binding.DevBuf.from_numpy(np.concatenate([np.zeros(cs.src_off, np.uint8), x.ravel(), np.zeros(16, np.uint8)]))
    y = Out(cs.B, cs.H, cs.W, ge.plain(cs.C), cs.zp)
    binding.check(S().mi355_nchw_to_tensor(src.ptr.value + cs.src_off, C.byref(y.tensor(cs.C)), None), cs.name)
    return y, y.check([(0, ge.nchw_to_cells_ref(x, y.cells.cs))], cs.C, cs.name)


def _lay_bytes(cs):
    return np.random.default_rng(cs.C * 100 + cs.W).integers(0, 256, (cs.B, cs.C, cs.H, cs.W), dtype=np.uint8)


@pytest.mark.parametrize("cs", ge.LAY_CASES, ids=lambda c: c.name)
def test_nchw_to_tensor(cs):
    x = _lay_bytes(cs)
    y, got = _nchw_to_tensor(cs, x)
    body = got[G:G + y.cells.nbytes].reshape(y.cells.ncells, y.cells.cs)
    if cs.C == 3:
        assert (body[:, 3] == 0).all(), "the fourth byte of every 4-byte cell, pad cells included"
    else:
        inner, n4 = body[y.cells.interior()], (cs.C + 3) // 4 * 4
        assert (inner[:, cs.C:n4] == 0x80).all(), "the pad channels the converter stores hold uint8 0"
        assert (inner[:, n4:] == (cs.zp ^ 0x80)).all(), "behind the last 4-byte group the fill stays"
    # and back: the plain bytes again
    back = Flat(x.size)
    binding.check(S().mi355_tensor_to_nchw(C.byref(y.tensor(cs.C)), back.ptr, None), "tensor_to_nchw")
    back.check(x, cs.name + ": round trip")


def test_nchw3_both_converters_agree_byte_for_byte():
    """W = 8, C = 3: the four-pixel kernel (aligned source) and the generic one (source one byte further) leave the same buffer"""
    a, b = (next(c for c in ge.LAY_CASES if c.name == n) for n in ("c3w8", "c3w8_src+1"))
    assert ge.layout_fast_path(a) and not ge.layout_fast_path(b) and (a.B, a.H, a.W, a.zp) == (b.B, b.H, b.W, b.zp)
    x = _lay_bytes(a)
    assert np.array_equal(_nchw_to_tensor(a, x)[1], _nchw_to_tensor(b, x)[1])


@pytest.mark.parametrize("name,B,Cc,H,W,t", ge.UNLAY_CASES, ids=[c[0] for c in ge.UNLAY_CASES])
def test_tensor_to_nchw(name, B, Cc, H, W, t):
    full = ge.operand_bytes(name, B, H, W, t, lo=0)
    x = In(B, H, W, t, full)
    out = Flat(B * Cc * H * W)
    binding.check(S().mi355_tensor_to_nchw(C.byref(x.tensor(Cc)), out.ptr, None), name)
    out.check(full[:, t.off:t.off + Cc], name)


def test_tensor_fill_both_cell_sizes_and_the_planar_refusal():
    for Cc, zp in ((3, 77), (3, 0), (16, 0), (17, 255), (48, 1), (1, 128)):
        Out(3, 3, 5, ge.plain(Cc), zp)  # asserts the fill
    y = Out(2, 3, 5, ge.plain(16), 23)
    refused(S().mi355_tensor_fill(C.byref(y.tensor(16, cs=1, lead=0, tail=0)), 5, None), "tensor_fill: a planar tensor has no pad cells")
    refused(S().mi355_tensor_fill(C.byref(binding.Tensor(None, 2, 3, 5, 16, 16, 2, 8)), 5, None), "tensor")
    y.check([], 16, "refused fills")


# ------------------------------------------------------------------------------------------------------------------------------- dequant
def _dequant(x, c0, nc, zp, scale, out, out_C, out_c0):
    return S().mi355_dequant_forward(x, c0, nc, zp, scale, out, out_C, out_c0, None)


@pytest.mark.parametrize("cs", ge.DQ_CASES, ids=lambda c: c.name)
def test_dequant(cs):
    B, H, W = ge.DQ_B, ge.DQ_H, ge.DQ_W
    t = ge.plain(cs.C)
    full = ge.operand_bytes(cs.name, B, H, W, t, lo=0)
    x = In(B, H, W, t, full)
    out = Flat(B * cs.out_C * H * W * 4)
    binding.check(_dequant(C.byref(x.tensor(cs.C)), cs.c0, cs.nc, cs.zp, cs.scale, out.ptr, cs.out_C, cs.out_c0), cs.name)
    want = np.full(B * cs.out_C * H * W * 4, ge.SENTINEL, np.uint8).view(np.float32).reshape(B, cs.out_C, H, W).copy()
    want[:, cs.out_c0:cs.out_c0 + cs.nc] = ge.dequant_ref(full[:, cs.c0:cs.c0 + cs.nc], cs.zp, cs.scale)
    out.check(want, cs.name)  # the other planes keep their sentinel


def test_dequant_refusals():
    B, H, W = ge.DQ_B, ge.DQ_H, ge.DQ_W
    t = ge.plain(37)
    x = In(B, H, W, t, ge.operand_bytes("dq", B, H, W, t, lo=0))
    out = Flat(B * 24 * H * W * 4)
    binding.check(_dequant(C.byref(x.tensor(37)), 5, 20, 3, 0.5, out.ptr, 24, 2), "the legal call")
    out = Flat(B * 24 * H * W * 4)
    for label, ch, message in ge.DQ_REFUSALS:
        xt = x.tensor(37, **({"cs": ch["cs"]} if "cs" in ch else {}))
        if "data" in ch:
            xt.data = None
        xr = None if "x" in ch else C.byref(xt)
        rc = _dequant(xr, ch.get("c0", 5), ch.get("nc", 20), 3, 0.5, None if "out" in ch else out.ptr, 24, ch.get("out_c0", 2))
        refused(rc, message)
        out.check(None, label)


# ----------------------------------------------------------------------------------------------------------------- float input quantiser
def _src(x, off):
    """the floats `off` bytes past an aligned address (device allocations are at least 256-byte aligned)"""
    buf = binding.DevBuf.from_numpy(np.concatenate([np.zeros(off // 4, np.float32), x, np.zeros(8, np.float32)]))
    assert buf.ptr.value % 16 == 0
    return buf, buf.ptr.value + off


def test_image_quantize_counts_and_addresses():
    """every count at every source and output address: the vector / scalar loads, the dword / byte stores, the tail of the last thread"""
    for i, (count, so, oo) in enumerate(ge.q_launches()):
        scale, zp = ge.Q_PARAMS[i % len(ge.Q_PARAMS)]
        x = ge.q_data(count, "mixed", scale, seed=i)
        buf, ptr = _src(x, so)
        out = Flat(count, off=oo)
        assert out.ptr % 4 == oo
        binding.check(S().mi355_image_quantize(ptr, count, scale, zp, out.ptr, None), "image_quantize")
        out.check(ge.quantize_ref(x, scale, zp), f"count {count} source +{so} output +{oo} scale {scale} zp {zp}")


@pytest.mark.parametrize("kind", ge.Q_KINDS)
def test_image_quantize_data(kind):
    """ties on k + 0.5 of both signs, both clamps, denormals, zeros of both signs, one-signed images, under every (scale, zero point)"""
    for count in (5, 257, 1025):
        for scale, zp in ge.Q_PARAMS:
            x = ge.q_data(count, kind, scale)
            want = ge.quantize_ref(x, scale, zp)
            if kind == "mixed" and count > 5 and scale in (0.25, 0.5):
                q = (x / np.float32(scale)).astype(np.float64)
                assert ((q - np.floor(q) == 0.5) & (q > 0)).any() and ((q - np.floor(q) == 0.5) & (q < 0)).any(), "ties of both signs"
                assert (want == 0).any() and (want == 255).any()
            buf, ptr = _src(x, 0)
            out = Flat(count)
            binding.check(S().mi355_image_quantize(ptr, count, scale, zp, out.ptr, None), "image_quantize")
            out.check(want, f"{kind} count {count} scale {scale} zp {zp}")


@pytest.mark.parametrize("kind", ge.Q_KINDS)
def test_image_minmax_bit_patterns(kind):
    """the returned max / min as BIT PATTERNS (-0.0f for an image without a negative element), NaNs skipped, at every count and both addresses"""
    for count in ge.Q_COUNTS:
        if count == ge.Q_COUNTS[-1] and kind not in ("mixed", "negative"):
            continue
        for so in ge.Q_SRC_OFFSETS:
            for nans in (False, True):
                x = ge.q_data(count, kind, seed=so)
                if nans:
                    x = ge.with_nans(x)
                buf, ptr = _src(x, so)
                mm = Flat(8)
                binding.check(S().mi355_image_minmax(ptr, count, mm.ptr, None), "image_minmax")
                want = ge.minmax_ref(x)
                got = mm.check(want, f"{kind} count {count} source +{so} nans {nans}: want bits {want[0]:#x} {want[1]:#x}")
                assert got.view(np.uint32).tolist() == want.tolist()


@pytest.mark.parametrize("B,count", ge.Q_BATCHED, ids=[f"B{b}x{n}" for b, n in ge.Q_BATCHED])
def test_image_batched_minmax_and_per_image_quantize(B, count):
    """images of 5 and 7 floats: odd images start off the 16-byte and the 4-byte grids; B = 2049: the per-image workgroup cap 2048 / B is lifted to 1"""
    imgs = [ge.q_data(count, ge.Q_KINDS[b % len(ge.Q_KINDS)], ge.Q_PARAMS[b % 4][0], seed=b) for b in range(B)]
    x = np.concatenate(imgs)
    buf, ptr = _src(ge.with_nans(x) if B > 1 else x, 0)
    xn = ge.with_nans(x) if B > 1 else x
    mm = Flat(8 * B)
    binding.check(S().mi355_image_minmax_batched(ptr, B, count, mm.ptr, None), "image_minmax_batched")
    mm.check(np.concatenate([ge.minmax_ref(xn[b * count:(b + 1) * count]) for b in range(B)]), f"min / max of {B} images")
    scales = np.array([ge.Q_PARAMS[b % 4][0] for b in range(B)], np.float32)
    zps = np.array([ge.Q_PARAMS[b % 4][1] for b in range(B)], np.uint8)
    buf2, ptr2 = _src(x, 0)
    sd, zd = binding.DevBuf.from_numpy(scales), binding.DevBuf.from_numpy(zps)
    out = Flat(B * count)
    binding.check(S().mi355_image_quantize_per_image(ptr2, B, count, sd.ptr, zd.ptr, out.ptr, None), "image_quantize_per_image")
    out.check(np.concatenate([ge.quantize_ref(imgs[b], scales[b], int(zps[b])) for b in range(B)]), f"{B} images quantised")


def test_image_quantiser_refusals():
    x = ge.q_data(16, "mixed")
    buf, ptr = _src(x, 0)
    mm, out = Flat(64), Flat(64)
    sd, zd = binding.DevBuf.from_numpy(np.ones(4, np.float32)), binding.DevBuf.from_numpy(np.zeros(4, np.uint8))
    B = ge.Q_B_REFUSED
    refused(S().mi355_image_minmax_batched(ptr, B, 5, mm.ptr, None), "image_minmax_batched: null / empty / B > 65535")
    refused(S().mi355_image_quantize_per_image(ptr, B, 5, sd.ptr, zd.ptr, out.ptr, None), "image_quantize_per_image: null / empty / B > 65535")
    refused(S().mi355_image_minmax_batched(ptr, 0, 5, mm.ptr, None), "image_minmax_batched: null / empty / B > 65535")
    refused(S().mi355_image_minmax_batched(ptr, 2, 0, mm.ptr, None), "image_minmax_batched: null / empty / B > 65535")
    refused(S().mi355_image_minmax(ptr, 0, mm.ptr, None), "image_minmax: null / empty")
    refused(S().mi355_image_minmax(None, 4, mm.ptr, None), "image_minmax: null / empty")
    refused(S().mi355_image_quantize(ptr, 0, 0.5, 3, out.ptr, None), "image_quantize: null / empty")
    for scale, zp in ((0.0, 3), (-1.0, 3), (float("nan"), 3), (0.5, -1), (0.5, 256)):
        refused(S().mi355_image_quantize(ptr, 4, scale, zp, out.ptr, None), "image_quantize: need scale > 0 and 0 <= zero_point <= 255")
    mm.check(None, "min / max untouched")
    out.check(None, "bytes untouched")


# ------------------------------------------------------------------------------------------------------------------------------ letterbox
@pytest.mark.parametrize("cs", ge.LB_CASES, ids=lambda c: c.name)
def test_letterbox(cs):
    im = ge.letterbox_source(cs)
    want = oracle.letterbox_image(im, cs.h, cs.w)
    src = binding.DevBuf.from_numpy(im)
    out = Flat(want.nbytes)
    binding.check(S().mi355_letterbox_forward(src.ptr, cs.imw, cs.imh, cs.c, out.ptr, cs.w, cs.h, None), cs.name)
    got = out.check(want, cs.name).view(np.float32).reshape(want.shape)  # bit for bit
    # outside the kernel's own statement: the last column and row of the embedded image come from the source's last column and row alone
    new_w, new_h, ox, oy = ge.letterbox_geometry(cs.imw, cs.imh, cs.w, cs.h)
    col = ge.letterbox_last_column(im, new_h)
    assert np.array_equal(got[:, oy:oy + new_h, ox + new_w - 1].view(np.uint32), col.view(np.uint32)), "last column"
    row, iy, dy = ge.letterbox_last_row(im, new_w, new_h)
    assert np.array_equal(got[:, oy + new_h - 1, ox:ox + new_w].view(np.uint32), row.view(np.uint32)), "last row"
    if iy == cs.imh - 1 and dy == 0:
        assert got[:, oy + new_h - 1, ox + new_w - 1].tolist() == im[:, -1, -1].tolist(), "the corner is the source's last pixel"
    bars = np.ones(want.shape, bool)
    bars[:, oy:oy + new_h, ox:ox + new_w] = False
    assert (got[bars] == 0.5).all()


def test_letterbox_refusals():
    src = binding.DevBuf.from_numpy(np.zeros(4 * 40 * 20, np.float32))
    out = Flat(4 * 32 * 32 * 4)
    for cs, message in ge.LB_REFUSED:
        refused(S().mi355_letterbox_forward(src.ptr, cs.imw, cs.imh, cs.c, out.ptr, cs.w, cs.h, None), message)
        out.check(None, cs.name)
    refused(S().mi355_letterbox_forward(None, 4, 4, 1, out.ptr, 8, 8, None), ge.LB_BAD_SIZE)


# ------------------------------------------------------------------------------------------------------------------------ yolo activation
@pytest.mark.parametrize("HW", ge.YOLO_MAPS, ids=lambda m: f"hw{m[0] * m[1]}")
@pytest.mark.parametrize("classes", ge.YOLO_CLASSES)
@pytest.mark.parametrize("n", ge.YOLO_N)
def test_yolo_forward(n, classes, HW):
    H, W = HW
    B, per = ge.YOLO_B, classes + 5
    x = ge.yolo_input(B, n, classes, H * W, seed=n * 1000 + classes * 10 + H)
    src = binding.DevBuf.from_numpy(x)
    out = Flat(x.nbytes)
    binding.check(S().mi355_yolo_forward(src.ptr, out.ptr, B, n, classes, H, W, None), "yolo")
    raw = out.buf.to_numpy(np.uint8, out.buf.nbytes)
    assert (raw[:G] == ge.SENTINEL).all() and (raw[G + x.nbytes:] == ge.SENTINEL).all(), "the guards around the output"
    got = raw[G:G + x.nbytes].view(np.float32).reshape(x.shape)
    want = ge.yolo_ref(x)
    # entries 2 and 3 of every anchor: bit for bit, NaN payloads, infinities, -0.0f and denormals included
    assert np.array_equal(got[:, :, 2:4].view(np.uint32), x[:, :, 2:4].view(np.uint32))
    act = np.ones(per, bool)
    act[2:4] = False
    g, w, v = got[:, :, act], want[:, :, act], x[:, :, act]
    assert np.isfinite(g).all()
    d = ge.ulps_apart(g, w)
    assert d.max() <= 1, f"{int((d > 1).sum())} activations more than one float32 ulp from the double-precision logistic (worst {int(d.max())})"
    exact = np.isin(v, np.array(ge.YOLO_EXACT, np.float32))
    assert exact.sum() >= min(len(ge.YOLO_EXACT), 3) and np.array_equal(g[exact].view(np.uint32), w[exact].view(np.uint32)), "the exact points"


def test_yolo_refusals():
    x = ge.yolo_input(2, 3, 1, 4, seed=1)
    src = binding.DevBuf.from_numpy(x)
    out = Flat(x.nbytes)
    for label, ch in ge.YOLO_REFUSALS:
        a = dict(B=2, n=3, classes=1, H=2, W=2)
        a.update(ch)
        refused(S().mi355_yolo_forward(src.ptr, out.ptr, a["B"], a["n"], a["classes"], a["H"], a["W"], None), ge.YOLO_REFUSAL_MESSAGE)
        out.check(None, label)
    refused(S().mi355_yolo_forward(None, out.ptr, 2, 3, 1, 2, 2, None), "yolo: null")
    refused(S().mi355_yolo_forward(src.ptr, None, 2, 3, 1, 2, 2, None), "yolo: null")
    binding.check(S().mi355_yolo_forward(src.ptr, out.ptr, 2, 3, 0, 2, 2, None), "classes == 0 is legal: five entries an anchor")


# ------------------------------------------------------------------------------------------------------------------------------- checksum
def _checksum(words, start=0):
    buf = binding.DevBuf.from_numpy(words) if words.size else binding.DevBuf(16)
    s = Flat(8, init=0)
    if start:
        binding.check(S().mi355_h2d(s.ptr, np.array([start], np.uint64).ctypes.data, 8, None), "h2d")
        s.snap[G:G + 8] = np.array([start], np.uint64).view(np.uint8)
    binding.check(S().mi355_checksum_u32(buf.ptr, words.size, s.ptr, None), "checksum")
    return s


@pytest.mark.parametrize("n", ge.CK_COUNTS)
def test_checksum_u32(n):
    words = ge.checksum_words(n)
    want = ge.checksum_ref(words)
    _checksum(words).check(np.array([want], np.uint64), f"{n} words")
    start = 0xFFFFFFFFFFFFFF00  # *sum_dev += ..., modulo 2^64
    _checksum(words, start).check(np.array([(want + start) & ((1 << 64) - 1)], np.uint64), f"{n} words on top of a sum")


def test_checksum_tells_permutations_apart():
    words = ge.checksum_words(1000, seed=3)
    perms = [words, words[::-1].copy(), np.roll(words, 1), np.concatenate([words[1:2], words[0:1], words[2:]])]
    sums = []
    for p in perms:
        want = ge.checksum_ref(p)
        _checksum(p).check(np.array([want], np.uint64), "permutation")
        sums.append(want)
    assert len(set(sums)) == len(perms)
    refused(S().mi355_checksum_u32(None, 4, _checksum(words).ptr, None), "checksum: null")
