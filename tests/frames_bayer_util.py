"""The raw sensor frame source (mi355_frame_bayer) restated in numpy: D(frame), the interleaved RGB frame the Bayer input path stands
for, as include/mi355_yolo_int8.h defines it, and packers for the four sample layouts.  The GPU tests compare the Bayer calls with the
u8 calls on demosaic(...); tests/test_frames_bayer_cpu.py checks demosaic itself against a literal per-pixel loop."""
import numpy as np

PATTERNS = ["rggb", "bggr", "grbg", "gbrg", "mono"]  # MI355_BAYER_RGGB .. MI355_BAYER_MONO
BAYER = PATTERNS[:4]
SAMPLES = ["u8", "u16", "mipi10", "mipi12"]  # MI355_RAW_U8 .. MI355_RAW_MIPI12
# P[y & 1][x & 1] as plane indices (R, G, B = 0, 1, 2)
TILE = {"rggb": ((0, 1), (1, 2)), "bggr": ((2, 1), (1, 0)), "grbg": ((1, 0), (2, 1)), "gbrg": ((1, 2), (0, 1))}


def row_bytes(sample, w):
    """the bytes of a tightly packed row of w samples"""
    return {"u8": w, "u16": 2 * w, "mipi10": 5 * ((w + 3) // 4), "mipi12": 3 * ((w + 1) // 2)}[sample]


def raw8(frame, sample, shift=0, w=None):
    """uint8 [h][w]: the 8-bit samples of a frame -- uint8 [h][w] (u8), uint16 [h][w] (u16) or uint8 [h][>= row_bytes] with w (MIPI)"""
    frame = np.asarray(frame)
    if sample == "u8":
        assert frame.dtype == np.uint8
        return frame.copy()
    if sample == "u16":
        assert frame.dtype == np.uint16
        return np.minimum(frame.astype(np.int32) >> shift, 255).astype(np.uint8)
    assert frame.dtype == np.uint8 and w is not None
    x = np.arange(w)
    col = 5 * (x >> 2) + (x & 3) if sample == "mipi10" else 3 * (x >> 1) + (x & 1)
    return frame[:, col].copy()


def colours(pattern, h, w):
    """int [h][w]: c(x, y), the plane of every site; MONO: all 0 (its tone table)"""
    if pattern == "mono":
        return np.zeros((h, w), np.int64)
    t = np.array(TILE[pattern])
    return t[np.arange(h)[:, None] & 1, np.arange(w)[None, :] & 1]


def _reflect(i, n):
    return np.where(i < 0, -i, np.where(i >= n, 2 * (n - 1) - i, i))


def demosaic(frame, pattern, sample="u8", shift=0, tone=None, w=None):
    """D(frame): uint8 [h][w][3]"""
    r8 = raw8(frame, sample, shift, w).astype(np.int64)
    h, w = r8.shape
    c = colours(pattern, h, w)
    s = r8 if tone is None else np.asarray(tone, np.uint8).astype(np.int64)[c, r8]
    if pattern == "mono":
        return np.repeat(s[:, :, None], 3, axis=2).astype(np.uint8)
    assert h >= 2 and w >= 2
    ys, xs = np.arange(h), np.arange(w)

    def at(dy, dx):
        return s[_reflect(ys + dy, h)[:, None], _reflect(xs + dx, w)[None, :]]
    horizontal = (at(0, -1) + at(0, 1) + 1) >> 1
    vertical = (at(-1, 0) + at(1, 0) + 1) >> 1
    cross = (at(0, -1) + at(0, 1) + at(-1, 0) + at(1, 0) + 2) >> 2
    diagonal = (at(-1, -1) + at(-1, 1) + at(1, -1) + at(1, 1) + 2) >> 2
    hc = np.array(TILE[pattern])[ys[:, None] & 1, (xs[None, :] ^ 1) & 1]  # c(x ^ 1, y): the colour of a site's row neighbours
    out = np.zeros((h, w, 3), np.int64)
    g = c == 1
    for k in (0, 2):
        out[:, :, k] = np.where(c == k, s, np.where(g, np.where(hc == k, horizontal, vertical), diagonal))
    out[:, :, 1] = np.where(g, s, cross)
    return out.astype(np.uint8)


def mosaic(rgb, pattern):
    """uint8 [h][w]: the mosaic a sensor behind `pattern` samples from an RGB image (MONO: plane 0)"""
    rgb = np.asarray(rgb)
    h, w = rgb.shape[:2]
    c = colours(pattern, h, w)
    return np.take_along_axis(rgb, c[:, :, None], axis=2)[:, :, 0].astype(np.uint8)


def pack(samples, sample, shift=0, low=None):
    """A frame of layout `sample` whose raw8 is `samples` (uint8 [h][w]); low: the bits below the 8 kept ones (default: a pattern that
    is not zero, so that a reader which used them would be found out).  u16: uint16 [h][w] = samples << shift | low bits; MIPI:
    uint8 [h][row_bytes] with the low bits in the group's last byte."""
    samples = np.asarray(samples, np.uint8)
    h, w = samples.shape
    if sample == "u8":
        return samples.copy()
    if low is None:
        low = (np.arange(h * w).reshape(h, w) * 7 + 3)
    if sample == "u16":
        return ((samples.astype(np.uint16) << shift) | (np.asarray(low) & ((1 << shift) - 1)).astype(np.uint16)).astype(np.uint16)
    n = 4 if sample == "mipi10" else 2  # pixels of a group; a group is n + 1 bytes
    out = np.zeros((h, row_bytes(sample, w)), np.uint8)
    x = np.arange(w)
    out[:, (n + 1) * (x // n) + x % n] = samples
    bits = 2 if sample == "mipi10" else 4
    for xx in range(w):
        out[:, (n + 1) * (xx // n) + n] |= ((np.asarray(low)[:, xx] & ((1 << bits) - 1)) << (bits * (xx % n))).astype(np.uint8)
    return out


def padded(frame, pad, fill=0xA5):
    """the frame inside rows `pad` elements longer: a view whose row stride is the padded pitch"""
    frame = np.asarray(frame)
    big = np.full((frame.shape[0], frame.shape[1] + pad), fill, frame.dtype)
    big[:, :frame.shape[1]] = frame
    return big[:, :frame.shape[1]]
