"""What the tests of the frame input path share (test_frames_*_cpu.py, test_gpu_frames_*.py): the expected result of an RGB frame
from the oracle, the numpy restatement of the integer YUV -> RGB formulas, one batch through the two C-ABI calls of any kind of
frames, and the host- and CLI-level helpers.  Importing it touches no device."""
import ctypes as C
import os

import numpy as np

import oracle
from yolo_quantization_amd import binding, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "cfg", "tiny_unit.cfg")
CLASSES = 5
EINVAL = -22

# (yoff, cy, crv, cgu, cgv, cbu): round(x * 65536) of the standards' coefficients, by matrix id
COEF = {0: (16, 76309, 104597, 25675, 53279, 132201), 1: (0, 65536, 91881, 22553, 46802, 116130),
        2: (16, 76309, 117489, 13975, 34925, 138438), 3: (0, 65536, 103206, 12276, 30679, 121609)}
SHIFTS = {"i420": (1, 1), "yv12": (1, 1), "i422": (1, 0), "i444": (0, 0)}  # (sx, sy) of the planar YUV formats


def yuv_to_rgb(Y, U, V, matrix):
    """the specified integer conversion: int32, floor shift, clamp"""
    yoff, cy, crv, cgu, cgv, cbu = COEF[matrix]
    Y, U, V = (np.asarray(a).astype(np.int32) for a in (Y, U, V))
    yy = cy * (Y - yoff)
    r = (yy + crv * (V - 128) + 32768) >> 16
    g = (yy - cgu * (U - 128) - cgv * (V - 128) + 32768) >> 16
    b = (yy + cbu * (U - 128) + 32768) >> 16
    return np.stack([np.clip(c, 0, 255).astype(np.uint8) for c in (r, g, b)], axis=-1)


def plane_shapes(fmt, w, h):
    """[(rows, columns)] of the three planes of a planar frame"""
    if fmt in ("rgb", "bgr"):
        return [(h, w)] * 3
    sx, sy = SHIFTS[fmt]
    c = ((h + sy) >> sy, (w + sx) >> sx)
    return [(h, w), c, c]


def _planes(frame):
    """load_image_color's planar floats of an RGB frame (ref: src/image.c:1386)"""
    return np.ascontiguousarray(frame.transpose(2, 0, 1)).astype(np.float32) / np.float32(255)


def _expected(frame, netw, neth):
    lb = oracle.letterbox_image(_planes(frame), neth, netw)
    q, s, z = oracle.quantize_image(lb)
    return lb, q, s, z


def _pair_from_minmax(mx, mn):
    """the host's own scale / zero-point expressions (quant_image_with_min_max) on a two-element image with that max / min"""
    x = np.array([mx, mn + np.float32(0)], np.float32)
    out = np.zeros(2, np.uint8)
    s, z = C.c_float(), C.c_uint8()
    binding.host().quant_image_with_min_max(2, x.ctypes.data, out.ctypes.data, C.byref(s), C.byref(z))
    return np.float32(s.value), z.value


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _padded(plane2d, pitch):
    rows = np.full((plane2d.shape[0], pitch), 0xEE, np.uint8)
    rows[:, :plane2d.shape[1]] = plane2d
    return rows


def _per_frame(x, b):
    return x if isinstance(x, str) else x[b]


# How a frame of each kind is laid out for the C-ABI: (its planes as 2-D byte arrays, entry(device addresses, pitches) -> the table
# entry).  b: the slot; the names after it are one for the batch or one per frame.
def _lay_u8(f, b, order="rgb"):
    h, w, _ = f.shape
    return [f.reshape(h, 3 * w)], lambda p, q: binding.FrameU8(p[0], w, h, q[0], binding.FRAME_ORDER[_per_frame(order, b)], (C.c_int * 2)(0, 0))


def _lay_yuv(f, b, layout="nv12", matrix="bt601"):
    y, uv = f
    h, w = y.shape
    lay, mat = binding.YUV_LAYOUT[_per_frame(layout, b)], binding.YUV_MATRIX[_per_frame(matrix, b)]
    return ([y, uv.reshape(uv.shape[0], 2 * ((w + 1) // 2))],
            lambda p, q: binding.FrameYUV(p[0], p[1], w, h, q[0], q[1], lay, mat, (C.c_int * 2)(0, 0)))


def _lay_planar(f, b, fmt="i420", matrix="bt601"):
    h, w = f[0].shape
    fm = _per_frame(fmt, b)
    assert [p.shape for p in f] == plane_shapes(fm, w, h)
    m = 0 if fm in ("rgb", "bgr") else binding.YUV_MATRIX[_per_frame(matrix, b)]  # matrix is passed as 0 for rgb / bgr frames
    return list(f), lambda p, q: binding.FramePlanar((C.c_void_p * 3)(*p), w, h, (C.c_int * 3)(*q), binding.PLANAR_FORMAT[fm], m,
                                                     (C.c_int * 3)(0, 0, 0))


KINDS = {"u8": (binding.FrameU8, _lay_u8), "yuv": (binding.FrameYUV, _lay_yuv), "planar": (binding.FramePlanar, _lay_planar)}


class _Launch:
    """One batch through the two C-ABI calls of a kind of frames: "u8" (frames: uint8 [h][w][3] arrays; order), "yuv" (frames: (y, uv)
    pairs; layout, matrix) or "planar" (frames: tuples of three planes; fmt, matrix).  pitch[b]: the pitch of every plane of frame b
    (one number for a u8 frame), rows are then padded with 0xEE bytes."""

    def __init__(self, kind, frames, netw, neth, *how, pitch=None, **named):
        B = len(frames)
        struct, lay = KINDS[kind]
        self.kind, self.B, self.netw, self.neth = kind, B, netw, neth
        self.bufs = []
        self.table = (struct * B)()
        for b, f in enumerate(frames):
            planes, entry = lay(f, b, *how, **named)
            ps = [p.shape[1] for p in planes] if not pitch else ([pitch[b]] if kind == "u8" else list(pitch[b]))
            bufs = [binding.DevBuf.from_numpy(_padded(p, q)) for p, q in zip(planes, ps)]
            self.bufs += bufs
            self.table[b] = entry([x.ptr.value for x in bufs], ps)
        self.out = binding.DevBuf.from_numpy(np.full(B * 3 * neth * netw, 0xA5, np.uint8))
        self.mm = binding.DevBuf.from_numpy(np.full(2 * B, 7.0, np.float32))
        self.pairs = None

    def upload_table(self):
        self.table_dev = binding.DevBuf(C.sizeof(self.table))
        binding.check(binding.shim().mi355_h2d(self.table_dev.ptr, C.addressof(self.table), C.sizeof(self.table), None), "h2d")
        binding.check(binding.shim().mi355_stream_sync(None), "sync")

    def minmax_rc(self):
        call = getattr(binding.shim(), f"mi355_frames_{self.kind}_letterbox_minmax")
        return call(self.table_dev.ptr, self.table, self.B, self.netw, self.neth, self.mm.ptr, None)

    def quantize_rc(self, scales, zps):
        self.pairs = (binding.DevBuf.from_numpy(np.asarray(scales, np.float32)), binding.DevBuf.from_numpy(np.asarray(zps, np.uint8)))
        call = getattr(binding.shim(), f"mi355_frames_{self.kind}_letterbox_quantize")
        return call(self.table_dev.ptr, self.table, self.B, self.netw, self.neth, self.pairs[0].ptr, self.pairs[1].ptr, self.out.ptr, None)

    def run(self):
        """(minmax [B][2], scale [B], zero point [B], bytes [B][3][h][w])"""
        self.upload_table()
        binding.check(self.minmax_rc(), "minmax")
        mm = self.mm.to_numpy(np.float32, 2 * self.B).reshape(self.B, 2)
        pairs = [_pair_from_minmax(mm[b, 0], mm[b, 1]) for b in range(self.B)]
        s = np.array([p[0] for p in pairs], np.float32)
        z = np.array([p[1] for p in pairs], np.uint8)
        binding.check(self.quantize_rc(s, z), "quantize")
        q = self.out.to_numpy(np.uint8, self.B * 3 * self.neth * self.netw).reshape(self.B, 3, self.neth, self.netw)
        return mm, s, z, q

    def out_bytes(self):
        return self.out.to_numpy(np.uint8, self.B * 3 * self.neth * self.netw)

    def free(self):
        for b in self.bufs + [self.out, self.mm] + list(self.pairs or ()):
            b.free()
        if hasattr(self, "table_dev"):
            self.table_dev.free()


def _assert_frame(got, b, frame, netw, neth, what):
    mm, s, z, q = got
    lb, want_q, want_s, want_z = _expected(frame, netw, neth)
    want_max, want_min = max(lb.max(), np.float32(0)), min(lb.min(), np.float32(0))
    assert _bits(mm[b, 0]) == _bits(want_max), f"{what}: max"
    assert mm[b, 1] == want_min, f"{what}: min"  # -0.0f (the seed) == 0.0f
    assert _bits(s[b]) == _bits(want_s) and z[b] == want_z, f"{what}: scale / zero point"
    assert np.array_equal(q[b], want_q), f"{what}: bytes"


# ------------------------------------------------------------------------------------------------------------ host level
def _wts(tmp_path, seed=3):
    p = str(tmp_path / f"tiny_unit_{seed}.weights")
    synth.synth_weights(CFG, p, seed=seed)
    return p


def _layers_and_dets(net, frames):
    net.forward()
    net.sync()
    outs = [net.pull(i) for i in range(net.n)]
    heads = [i for i, inf in enumerate(net.info) if inf["type"] == binding.T_YOLO]
    dets = [net.detections_sizes(i, CLASSES, [f.shape[1] for f in frames], [f.shape[0] for f in frames], 0.005, 1, 512) for i in heads]
    return outs, dets


def _assert_same_run(got, want, what):
    (outs_a, dets_a), (outs_b, dets_b) = got, want
    for i, (a, b) in enumerate(zip(outs_a, outs_b)):
        assert a.keys() == b.keys()
        for k in a:
            assert np.array_equal(a[k], b[k]), f"{what}: layer {i} {k}"
    assert len(dets_a) == len(dets_b) > 0
    for (ca, ra), (cb, rb) in zip(dets_a, dets_b):
        assert np.array_equal(ca, cb) and np.array_equal(ra, rb), f"{what}: detections"
        assert ca.sum() > 0


# ------------------------------------------------------------------------------------------------------------------- CLI
def _write_ppm(path, rgb_hwc):
    with open(path, "wb") as f:
        f.write(f"P6\n{rgb_hwc.shape[1]} {rgb_hwc.shape[0]}\n255\n".encode())
        f.write(np.ascontiguousarray(rgb_hwc, np.uint8).tobytes())


def _blocks(stdout):
    """per-image blocks of `detector test` output, the timing line reduced to the file name"""
    out, cur = [], None
    for line in stdout.splitlines():
        if ": Predicted in " in line:
            cur = [line.split(": Predicted in ")[0]]
            out.append(cur)
        elif cur is not None:
            cur.append(line)
    return out
