"""The batched frame input path at the switch points of its letterbox geometry, on the device: every case of tests/frame_geometry.py through the
two C-ABI calls of the u8 kind, the geometry cases through the float letterbox (one table, two kernels), the sizes where geometry meets a
source's own addressing through the five other kinds, and a few host-level batches.

Both outputs of a launch live between guards of sentinel bytes and are compared WHOLE with their photograph plus the bytes the case owns (the
min / max words of every slot, every byte of every slot's three planes): a store into a neighbouring plane, row or slot, in front of an
unaligned output or past its end fails the case that makes it.  Source rows are padded with 0xEE to an odd pitch.  Every comparison is exact.
One case per test; the whole file, 577 tests, takes 1.6 s on an MI355X (profiles/frame_geometry_gpu_tests.log)."""
import ctypes as C
import os

import numpy as np
import pytest

import frame_geometry as fg
import frames_bayer_util as fb
import frames_packed_util as fp
import frames_util
from frames_util import CFG, ROOT, _bits, _wts
from yolo_quantization_amd import binding

pytestmark = pytest.mark.gpu

G = fg.GUARD


@pytest.fixture(scope="module", autouse=True)
def _dev():
    binding.init(0)


def S():
    return binding.shim()


class Guarded:
    """nbytes of device output `off` bytes past an aligned address, between two guards; the payload starts as `init` (bytes)"""

    def __init__(self, nbytes, off=0, init=None):
        self.n, self.lo = nbytes, G + off
        host = np.full(2 * G + off + nbytes, fg.SENTINEL, np.uint8)
        if init is not None:
            host[self.lo:self.lo + nbytes] = init
        self.snap = host
        self.buf = binding.DevBuf.from_numpy(host)
        assert self.buf.ptr.value % 16 == 0
        self.ptr = C.c_void_p(self.buf.ptr.value + self.lo)

    def check(self, want, what, unit=1):
        """want: the payload (None: the photograph's).  The whole buffer, byte for byte."""
        exp = self.snap.copy()
        if want is not None:
            exp[self.lo:self.lo + self.n] = np.ascontiguousarray(want).view(np.uint8).ravel()
        got = self.buf.to_numpy(np.uint8, self.buf.nbytes)
        bad = np.flatnonzero(got != exp)
        if bad.size:
            guard = int(((bad < self.lo) | (bad >= self.lo + self.n)).sum())
            at = int(bad[0]) - self.lo
            raise AssertionError(f"{what}: {bad.size} bytes differ, {guard} of them in the guards; first at payload byte {at} (element {at // unit}): "
                                 f"{got[bad[0]]:#x}, want {exp[bad[0]]:#x}")

    def free(self):
        self.buf.free()


class Run:
    """One batch through the two C-ABI calls of a kind.  lays: (planes, entry) of every DISTINCT frame, as frames_util's _lay_* give them; slots:
    which distinct frame each slot of the batch holds (the table entries share the device frames)."""

    def __init__(self, kind, struct, lays, slots, w, h, out_off=0):
        self.kind, self.B, self.w, self.h = kind, len(slots), w, h
        self.bufs, entries = [], []
        for planes, entry in lays:
            ptrs, pitches = [], []
            for p in planes:
                pitch = (p.shape[1] + 4) | 1  # odd, at least 4 bytes of 0xEE behind every row
                self.bufs.append(binding.DevBuf.from_numpy(frames_util._padded(p, pitch)))
                ptrs.append(self.bufs[-1].ptr.value)
                pitches.append(pitch)
            entries.append(np.frombuffer(bytes(entry(ptrs, pitches)), np.uint8))
        raw = np.ascontiguousarray(np.stack(entries)[np.asarray(slots)])
        self.table = (struct * self.B)()
        assert raw.nbytes == C.sizeof(self.table)
        C.memmove(self.table, raw.ctypes.data, raw.nbytes)
        self.table_dev = binding.DevBuf.from_numpy(raw)
        self.bufs.append(self.table_dev)
        self.mm = Guarded(8 * self.B, init=np.full(2 * self.B, 7.0, np.float32).view(np.uint8))
        self.out = Guarded(self.B * 3 * h * w, off=out_off)

    def minmax(self):
        call = getattr(S(), f"mi355_frames_{self.kind}_letterbox_minmax")
        return call(self.table_dev.ptr, self.table, self.B, self.w, self.h, self.mm.ptr, None)

    def quantize(self, scales, zps):
        pairs = [binding.DevBuf.from_numpy(np.asarray(scales, np.float32)), binding.DevBuf.from_numpy(np.asarray(zps, np.uint8))]
        self.bufs += pairs
        call = getattr(S(), f"mi355_frames_{self.kind}_letterbox_quantize")
        return call(self.table_dev.ptr, self.table, self.B, self.w, self.h, pairs[0].ptr, pairs[1].ptr, self.out.ptr, None)

    def free(self):
        for b in self.bufs + [self.mm, self.out]:
            b.free()


def _both_passes(run, wants, slots, what):
    """wants: fg.Want per distinct frame.  The min / max words of every slot first, then every byte of every slot."""
    slots = np.asarray(slots)
    binding.check(run.minmax(), what + ": minmax")
    run.mm.check(np.stack([x.mm for x in wants])[slots], what + ": min / max words", unit=4)
    run.out.check(None, what + ": the min / max pass stores no byte")
    binding.check(run.quantize(np.array([x.scale for x in wants], np.float32)[slots], np.array([x.zp for x in wants], np.uint8)[slots]),
                  what + ": quantize")
    run.out.check(np.stack([x.q for x in wants])[slots], what + ": bytes")
    run.mm.check(np.stack([x.mm for x in wants])[slots], what + ": the quantiser stores no min / max word", unit=4)
    run.free()


# ------------------------------------------------------------------------------------------------------------------- u8: the full table
@pytest.mark.parametrize("c", fg.CASES, ids=lambda c: c.name)
def test_u8(c):
    """slot b holds distinct frame b % 3; distinct frame 1 is stored as BGR, so the byte offsets inside a pixel are exercised by every batch"""
    n = min(c.B, fg.FRAMES_DISTINCT)
    lays = []
    for s in range(n):
        f, order = fg.frame(c, s), "bgr" if s == 1 else "rgb"
        lays.append(frames_util._lay_u8(np.ascontiguousarray(f[:, :, ::-1]) if s == 1 else f, s, order))
    slots = np.arange(c.B) % n
    _both_passes(Run("u8", binding.FrameU8, lays, slots, c.w, c.h, c.out_off), fg.expected(c.name), slots, c.name)


# ------------------------------------------------------------------------------------------- the float kernel: the same geometry cases
@pytest.mark.parametrize("c", fg.GEO_CASES, ids=lambda c: c.name)
def test_float_letterbox(c):
    want = fg.expected(c.name)[0].lb
    src = binding.DevBuf.from_numpy(fg.planes(fg.frame(c, 0)))
    out = Guarded(want.nbytes)
    binding.check(S().mi355_letterbox_forward(src.ptr, c.imw, c.imh, 3, out.ptr, c.w, c.h, None), c.name)
    out.check(want, c.name, unit=4)
    src.free(); out.free()


# -------------------------------------------------------------------------------------------------------------- the five other sources
def _lay_packed(frame, w, fmt, matrix):
    m = 0 if fmt in fp.RGBX else binding.YUV_MATRIX[matrix]
    return [frame], lambda p, q: binding.FramePacked(p[0], w, frame.shape[0], q[0], binding.PACKED_FORMAT[fmt], m, 0)


def _lay_p010(y16, uv16, matrix):
    h, w = y16.shape
    planes = [np.ascontiguousarray(p).astype("<u2").view(np.uint8).reshape(p.shape[0], -1) for p in (y16, uv16)]
    return planes, lambda p, q: binding.FrameP010(p[0], p[1], w, h, q[0], q[1], 0, binding.YUV_MATRIX[matrix], (C.c_int * 2)(0, 0))


def _lay_bayer(data, w, h, pattern, sample, shift, tone):
    planes = [data] + ([np.ascontiguousarray(tone, np.uint8).reshape(1, 768)] if tone is not None else [])
    return planes, lambda p, q: binding.FrameBayer(p[0], p[1] if tone is not None else None, w, h, q[0], binding.BAYER_PATTERN[pattern],
                                                   binding.RAW_SAMPLE[sample], shift, (C.c_int * 2)(0, 0))


def _bytes(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def _source(variant, w, h, seed):
    """(kind, struct, lay, the RGB frame the source stands for) of one frame of `variant`, through the converters of the util modules"""
    kind, a, b = variant
    if kind == "yuv":  # a: layout, b: matrix
        y, uv = _bytes((h, w), seed), _bytes(((h + 1) // 2, (w + 1) // 2, 2), seed + 1)
        rows, cols = (np.arange(h) >> 1)[:, None], (np.arange(w) >> 1)[None, :]
        iu = 1 if a == "nv21" else 0
        rgb = frames_util.yuv_to_rgb(y, uv[rows, cols, iu], uv[rows, cols, 1 - iu], binding.YUV_MATRIX[b])
        return kind, binding.FrameYUV, frames_util._lay_yuv((y, uv), 0, a, b), rgb
    if kind == "planar":  # a: format, b: matrix
        planes = tuple(_bytes(s, seed + k) for k, s in enumerate(frames_util.plane_shapes(a, w, h)))
        if a in ("rgb", "bgr"):
            rgb = np.stack(planes if a == "rgb" else planes[::-1], axis=-1)
        else:
            sx, sy = frames_util.SHIFTS[a]
            rows, cols = (np.arange(h) >> sy)[:, None], (np.arange(w) >> sx)[None, :]
            u, v = (planes[2], planes[1]) if a == "yv12" else (planes[1], planes[2])
            rgb = frames_util.yuv_to_rgb(planes[0], u[rows, cols], v[rows, cols], binding.YUV_MATRIX[b])
        return kind, binding.FramePlanar, frames_util._lay_planar(planes, 0, a, b), rgb
    if kind == "packed":  # a: format, b: matrix
        f = fp.packed_frame(a, w, h, seed)
        return kind, binding.FramePacked, _lay_packed(f, w, a, b), fp.packed_to_rgb(f, w, a, b)
    if kind == "p010":  # a: bits, b: matrix
        y16, uv16 = fp.p010_frame(w, h, seed, bits=a)
        y16, uv16 = y16 | np.uint16(seed % 61), uv16 | np.uint16(seed % 59)  # low bits that a rounding reader would use
        return kind, binding.FrameP010, _lay_p010(y16, uv16, b), fp.p010_to_rgb(y16, uv16, b)
    assert kind == "bayer"  # a: pattern, b: (sample, shift, toned)
    sample, shift, toned = b
    tone = (np.random.default_rng(seed + 5).permutation(768) % 256).astype(np.uint8).reshape(3, 256) if toned else None
    f = fb.pack(_bytes((h, w), seed), sample, shift)
    data = np.ascontiguousarray(f).astype("<u2").view(np.uint8).reshape(h, -1) if sample == "u16" else f
    assert data.shape[1] == fb.row_bytes(sample, w)
    rgb = fb.demosaic(f, a, sample, shift, tone, w if sample.startswith("mipi") else None)
    return kind, binding.FrameBayer, _lay_bayer(data, w, h, a, sample, shift, tone), rgb


VARIANTS = ([("yuv", "nv12", "bt601"), ("yuv", "nv21", "bt709f")]
            + [("planar", f, m) for f, m in (("i420", "bt601"), ("yv12", "bt709"), ("i422", "bt601f"), ("i444", "bt709f"), ("rgb", "bt601"), ("bgr", "bt601"))]
            + [("packed", f, m) for f, m in (("rgba", "bt601"), ("abgr", "bt601"), ("yuyv", "bt601"), ("uyvy", "bt709"), ("yvyu", "bt601f"))]
            + [("p010", 10, "bt601"), ("p010", 16, "bt709")]
            + [("bayer", p, x) for p, x in (("rggb", ("u8", 0, False)), ("bggr", ("u16", 2, True)), ("grbg", ("mipi10", 0, False)),
                                           ("gbrg", ("mipi12", 0, True)), ("mono", ("u8", 0, True)), ("mono", ("u16", 8, False)),
                                           ("mono", ("mipi10", 0, False)), ("mono", ("mipi12", 0, False)))])


def _allowed(variant, s):
    return variant[0] != "bayer" or variant[1] == "mono" or (s.imw >= 2 and s.imh >= 2)  # a Bayer pattern needs 2 x 2


SOURCE_RUNS = [(v, s) for v in VARIANTS for s in fg.SOURCE_SIZES if _allowed(v, s)]


def _vid(v):
    return "-".join(str(x) for x in ((v[0], v[1]) + (tuple(v[2]) if isinstance(v[2], tuple) else (v[2],))))


@pytest.mark.parametrize("variant,s", SOURCE_RUNS, ids=[f"{_vid(v)}-{s.imw}x{s.imh}_into_{s.w}x{s.h}" for v, s in SOURCE_RUNS])
def test_other_sources(variant, s):
    """two slots: the frame, and a second frame of the same size, so that slot 1's addressing meets the same geometry"""
    made = [_source(variant, s.imw, s.imh, 100 * k + s.imw + 7 * s.imh) for k in range(2)]
    wants = [fg.expected_rgb(np.ascontiguousarray(m[3]), s.w, s.h) for m in made]
    assert made[0][3].shape == (s.imh, s.imw, 3)
    _both_passes(Run(made[0][0], made[0][1], [m[2] for m in made], [0, 1], s.w, s.h), wants, [0, 1], _vid(variant))


def test_every_kind_allows_the_one_pixel_sizes_it_should():
    one = [s for s in fg.SOURCE_SIZES if s.imw == 1 or s.imh == 1]
    assert len(one) == 5
    ran = {(v[0], v[1], s) for v, s in SOURCE_RUNS if s in one}
    assert all((v[0], v[1], s) in ran for v in VARIANTS for s in one if v[0] != "bayer" or v[1] == "mono")
    assert not any(k == "bayer" and p != "mono" for k, p, _ in ran)


# ------------------------------------------------------------------------------------------------------------------------- host level
GOLDEN = os.path.join(ROOT, "tests", "golden")
HOST_SIZES = [(1, 5), (5, 1), (3, 14)]  # w x h into the 12 x 12 network: one column, one row, new_w == 2 with the short last row


def _pair_of_nets(tmp_path, per_image):
    wts = _wts(tmp_path)
    a, b = binding.Net(CFG, wts, batch=3), binding.Net(CFG, wts, batch=3)
    for n in (a, b):
        n.set_input_per_image(per_image)
    return a, b


def _same_input(a, b, what):
    assert np.array_equal(a._pull_input(), b._pull_input()), f"{what}: input bytes"
    (sa, za), (sb, zb) = a.input_quantization(), b.input_quantization()
    assert sa.shape == (3,) and np.array_equal(_bits(sa), _bits(sb)) and np.array_equal(za, zb), f"{what}: scales / zero points"
    return sa, za


@pytest.mark.parametrize("per_image", [False, True], ids=["shared_scale", "per_image"])
def test_host_one_pixel_wide_frames_equal_the_float_path(tmp_path, per_image):
    assert fg.GEO_CLAUSES["geo.last_row_short"](fg.Case("", 3, 14, 12, 12))
    a, b = _pair_of_nets(tmp_path, per_image)
    frames = [_bytes((h, w, 3), 40 + k) | np.uint8(1) for k, (w, h) in enumerate(HOST_SIZES)]
    for rot in range(3):  # every frame is image 0, which defines the shared scale, once
        fr = frames[rot:] + frames[:rot]
        a.prepare_from_frames_u8(fr)
        b.prepare_from_images_gpu([fg.planes(f) for f in fr])
        s, z = _same_input(a, b, f"rotation {rot}")
        x = a._pull_input().reshape(3, 3, 12, 12)
        for slot in range(3 if per_image else 1):
            want = fg.expected_rgb(fr[slot], 12, 12)
            assert _bits(s[slot]) == _bits(want.scale) and z[slot] == want.zp and np.array_equal(x[slot], want.q), f"rotation {rot} slot {slot}"
    a.close(); b.close()


@pytest.mark.parametrize("per_image", [False, True], ids=["shared_scale", "per_image"])
@pytest.mark.parametrize("kind,names", [("png", ["rgb8_adam7_1x1", "pal4_adam7_1x1", "grey16_plain_1x1"]), ("jpeg", ["420_1x1", "444_1x1", "422_1x1"])])
def test_host_one_pixel_fixtures_go_through_the_coded_inputs(tmp_path, kind, names, per_image):
    with np.load(os.path.join(GOLDEN, kind + "_expected.npz")) as z:
        want = [z[n] for n in names]
    assert all(w.shape == (1, 1, 3) for w in want)
    files = []
    for n in names:
        with open(os.path.join(GOLDEN, kind, n + (".jpg" if kind == "jpeg" else ".png")), "rb") as f:
            files.append(f.read())
    a, b = _pair_of_nets(tmp_path, per_image)
    sizes = a.prepare_from_png(files) if kind == "png" else a.prepare_from_jpeg(files)
    assert sizes == [(1, 1)] * 3
    b.prepare_from_frames_u8(want)
    _same_input(a, b, kind)
    x = a._pull_input().reshape(3, 3, 12 * 12)
    assert (x == x[:, :, :1]).all(), "a 1 x 1 frame fills its whole slot: equal aspects, no bars"
    a.close(); b.close()
