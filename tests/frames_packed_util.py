"""What the tests of the packed (RGBA .. ABGR, YUYV .. YVYU) and P010 frame sources share (test_frames_packed_cpu.py,
test_gpu_frames_packed.py).  The specification of both sources is the three numpy converters below: each turns a frame of a new kind
into a frame of a kind the project already serves -- interleaved RGB, planar I422, NV12 -- and the new source must give, bit for bit,
what the old one gives for the converted frame.  Importing this file touches no device."""
import ctypes as C

import numpy as np

import frames_util
from frames_util import _per_frame
from yolo_quantization_amd import binding

RGBX = {"rgba": (0, 1, 2), "bgra": (2, 1, 0), "argb": (1, 2, 3), "abgr": (3, 2, 1)}  # the bytes of a pixel that hold R, G, B
UNUSED = {"rgba": 3, "bgra": 3, "argb": 0, "abgr": 0}                                # and the one that holds neither
YUV422 = {"yuyv": (0, 2, 1, 3), "uyvy": (1, 3, 0, 2), "yvyu": (0, 2, 3, 1)}          # the bytes of a macropixel that hold Y0, Y1, U, V
MATRICES = ["bt601", "bt601f", "bt709", "bt709f"]


def rgbx_to_rgb(frame, format):
    """uint8 [h][w][4] -> the interleaved RGB frame [h][w][3]: the fourth byte dropped, the others in R, G, B order"""
    return np.ascontiguousarray(frame[:, :, list(RGBX[format])])


def yuv422_to_planes(frame, w, format):
    """uint8 [h][>= 4 * ((w + 1) // 2)] rows of macropixels -> the I422 frame (Y [h][w], U [h][(w + 1) // 2], V the same)"""
    h, cw = frame.shape[0], (w + 1) // 2
    g = frame[:, :4 * cw].reshape(h, cw, 4)
    y0, y1, u, v = YUV422[format]
    Y = np.stack([g[:, :, y0], g[:, :, y1]], axis=-1).reshape(h, 2 * cw)[:, :w]
    return np.ascontiguousarray(Y), np.ascontiguousarray(g[:, :, u]), np.ascontiguousarray(g[:, :, v])


def p010_to_nv12(y16, uv16):
    """uint16 planes -> the NV12 frame of their high bytes: truncation, not rounding"""
    return (y16 >> 8).astype(np.uint8), (uv16 >> 8).astype(np.uint8)


def packed_to_rgb(frame, w, format, matrix="bt601"):
    """the interleaved RGB frame of a packed frame given as bytes [h][row_bytes], through the converters and frames_util.yuv_to_rgb"""
    if format in RGBX:
        return rgbx_to_rgb(frame[:, :4 * w].reshape(frame.shape[0], w, 4), format)
    Y, U, V = yuv422_to_planes(frame, w, format)
    cols = np.arange(w) >> 1
    return np.ascontiguousarray(frames_util.yuv_to_rgb(Y, U[:, cols], V[:, cols], MATRICES.index(matrix)))


def p010_to_rgb(y16, uv16, matrix="bt601"):
    y, uv = p010_to_nv12(y16, uv16)
    h, w = y.shape
    rows, cols = (np.arange(h) >> 1)[:, None], (np.arange(w) >> 1)[None, :]
    return np.ascontiguousarray(frames_util.yuv_to_rgb(y, uv[rows, cols, 0], uv[rows, cols, 1], MATRICES.index(matrix)))


def packed_row_bytes(format, w):
    return 4 * w if format in RGBX else 4 * ((w + 1) // 2)


def packed_frame(format, w, h, seed):
    """random bytes [h][row_bytes] of a packed frame"""
    return np.random.default_rng(seed).integers(0, 256, (h, packed_row_bytes(format, w)), dtype=np.uint8)


def p010_frame(w, h, seed, bits=10):
    """(y [h][w], uv [(h + 1) // 2][(w + 1) // 2][2]) uint16, random samples of `bits` bits at the top, the low bits zero"""
    rng = np.random.default_rng(seed)
    shift = 16 - bits
    return tuple((rng.integers(0, 1 << bits, s, dtype=np.uint16) << shift).astype(np.uint16) for s in ((h, w), ((h + 1) // 2, (w + 1) // 2, 2)))


def geometry_accepts(imw, imh, w, h):
    """frame_geometry's rule (csrc/frames.hip) for an imw x imh frame into a w x h input, in float32 as there"""
    f = np.float32
    if f(w) / f(imw) < f(h) / f(imh):
        new_w, new_h = w, (imh * w) // imw
    else:
        new_h, new_w = h, (imw * h) // imh
    if new_w < 2 or new_h < 2:
        return False
    ws, hs = f(imw - 1) / f(new_w - 1), f(imh - 1) / f(new_h - 1)
    # row iy + 1 / column ix + 1 are never read from a frame of one row / one column
    return not (int(f(new_h - 1) * hs) > imh - 1 or (imh > 1 and int(f(new_h - 2) * hs) + 1 > imh - 1) or
                (imw > 1 and int(f(new_w - 2) * ws) + 1 > imw - 1))


class Launch(frames_util._Launch):
    """One batch through the two C-ABI calls of the "packed" or the "p010" kind.  frames: for "packed" (bytes [h][row_bytes], w) pairs
    and format / matrix names, one for the batch or one per frame; for "p010" (y16, uv16) pairs and matrix.  extra: bytes added to
    every plane's tight pitch; offset: bytes between the device allocation (aligned) and the first byte of each plane, so 1
    gives an odd address; pad: what the row padding and the bytes before the plane hold -- None: 0xEE, a number: that byte, a numpy
    Generator: random bytes."""

    def __init__(self, kind, frames, netw, neth, format=None, matrix="bt601", extra=0, offset=0, pad=None):
        B = len(frames)
        self.kind, self.B, self.netw, self.neth = kind, B, netw, neth
        self.bufs = []
        self.table = ((binding.FramePacked if kind == "packed" else binding.FrameP010) * B)()
        for b, f in enumerate(frames):
            m = binding.YUV_MATRIX[_per_frame(matrix, b)]
            if kind == "packed":
                planes, (h, w) = [f[0]], (f[0].shape[0], f[1])
            else:
                planes, (h, w) = [np.ascontiguousarray(p).astype("<u2").view(np.uint8).reshape(p.shape[0], -1) for p in f], f[0].shape
            ptr, pitch = [], []
            for p in planes:
                q = p.shape[1] + extra
                n = offset + p.shape[0] * q
                raw = pad.integers(0, 256, n, dtype=np.uint8) if hasattr(pad, "integers") else np.full(n, 0xEE if pad is None else pad, np.uint8)
                raw[offset:].reshape(p.shape[0], q)[:, :p.shape[1]] = p
                self.bufs.append(binding.DevBuf.from_numpy(raw))
                assert self.bufs[-1].ptr.value % 4 == 0
                ptr.append(self.bufs[-1].ptr.value + offset)
                pitch.append(q)
            if kind == "packed":
                fm = _per_frame(format, b)
                self.table[b] = binding.FramePacked(ptr[0], w, h, pitch[0], binding.PACKED_FORMAT[fm], 0 if fm in RGBX else m, 0)
            else:
                self.table[b] = binding.FrameP010(ptr[0], ptr[1], w, h, pitch[0], pitch[1], 0, m, (C.c_int * 2)(0, 0))
        self.out = binding.DevBuf.from_numpy(np.full(B * 3 * neth * netw, 0xA5, np.uint8))
        self.mm = binding.DevBuf.from_numpy(np.full(2 * B, 7.0, np.float32))
        self.pairs = None


def run(cls, *a, **kw):
    """(minmax, scale, zero point, bytes) of one launch, its buffers freed"""
    L = cls(*a, **kw)
    got = L.run()
    L.free()
    return got


def assert_same(got, want, what):
    """min / max words, scale bits, zero points and bytes of two launches"""
    for name, a, b in zip(("min / max", "scale", "zero point", "bytes"), got, want):
        a, b = (frames_util._bits(a), frames_util._bits(b)) if a.dtype == np.float32 else (a, b)
        assert a.shape == b.shape and np.array_equal(a, b), f"{what}: {name}"
