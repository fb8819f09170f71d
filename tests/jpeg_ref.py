"""numpy restatement of the device half of the JPEG decoder (yolo_quantization_amd/csrc/jpeg.hip), written from the lines of
stb_image v2.19 the reference compiles (ref: src/stb_image.h): dequantisation with the 16-bit store (:1969-1999), the two-pass
inverse DCT (:2163-2261), the resamplers as functions of the output pixel (:3173-3235, :3354-3363, the row walk :3611-3644) and the
colour modes (:3367-3391, :3646-3687).

Everything is computed in int64.  stb computes in 32-bit ints, where an overflow is undefined; OverflowError is raised when an
intermediate leaves int32, so a test input that passes here keeps stb's own arithmetic defined (the device wraps instead).
"""
import numpy as np


def _f2f(x):  # ref :2163 -- the literal is a float, the product with 4096 exact, + 0.5 in double, truncation
    return int(float(np.float32(x)) * 4096 + 0.5)


C_0_541, C_N1_847, C_0_765, C_1_175 = _f2f(0.5411961), _f2f(-1.847759065), _f2f(0.765366865), _f2f(1.175875602)
C_0_298, C_2_053, C_3_072, C_1_501 = _f2f(0.298631336), _f2f(2.053119869), _f2f(3.072711026), _f2f(1.501321110)
C_N0_899, C_N2_562, C_N1_961, C_N0_390 = _f2f(-0.899976223), _f2f(-2.562915447), _f2f(-1.961570560), _f2f(-0.390180644)


def _chk(*arrays):
    for a in arrays:
        if np.any(a > 2**31 - 1) or np.any(a < -2**31):
            raise OverflowError("an intermediate of the inverse DCT leaves int32")
    return arrays[0]


def _idct_1d(s, bias):
    """s: int64 [..., 8] along the last axis -> the 8 outputs before the shift (x + bias +- t), ref :2167-2202"""
    s0, s1, s2, s3, s4, s5, s6, s7 = (s[..., k] for k in range(8))
    p1 = _chk((s2 + s6) * C_0_541)
    t2 = _chk(p1 + _chk(s6 * C_N1_847))
    t3 = _chk(p1 + _chk(s2 * C_0_765))
    t0 = _chk((s0 + s4) * 4096)
    t1 = _chk((s0 - s4) * 4096)
    x0, x3, x1, x2 = _chk(t0 + t3), _chk(t0 - t3), _chk(t1 + t2), _chk(t1 - t2)
    t0, t1, t2, t3 = s7, s5, s3, s1
    p3, p4, p1, p2 = t0 + t2, t1 + t3, t0 + t3, t1 + t2
    p5 = _chk((p3 + p4) * C_1_175)
    t0, t1, t2, t3 = _chk(t0 * C_0_298), _chk(t1 * C_2_053), _chk(t2 * C_3_072), _chk(t3 * C_1_501)
    p1 = _chk(p5 + _chk(p1 * C_N0_899))
    p2 = _chk(p5 + _chk(p2 * C_N2_562))
    p3 = _chk(p3 * C_N1_961)
    p4 = _chk(p4 * C_N0_390)
    t3 = _chk(t3 + _chk(p1 + p4))
    t2 = _chk(t2 + _chk(p2 + p3))
    t1 = _chk(t1 + _chk(p2 + p4))
    t0 = _chk(t0 + _chk(p1 + p3))
    x0, x1, x2, x3 = _chk(x0 + bias), _chk(x1 + bias), _chk(x2 + bias), _chk(x3 + bias)
    out = np.stack([x0 + t3, x1 + t2, x2 + t1, x3 + t0, x3 - t0, x2 - t1, x1 - t2, x0 - t3], axis=-1)
    return _chk(out)


def dequantise(coef, quant):
    """(short)(coefficient * quantiser): the low 16 bits of the product, signed (ref :1969, :1986, :1999)"""
    prod = np.asarray(coef, np.int64) * np.asarray(quant, np.int64)
    return ((prod + 32768) % 65536) - 32768


def idct_blocks(coef, quant):
    """coef int16 [..., 64] (natural order), quant uint16 [64] -> uint8 [..., 8, 8]; OverflowError where stb's ints would overflow"""
    d = dequantise(coef, quant).reshape(np.shape(coef)[:-1] + (8, 8))
    # columns first: the 1-D pass runs down every column (ref :2211-2235); the all-zero shortcut gives the same numbers
    v = _idct_1d(np.swapaxes(d, -1, -2), 512) >> 10  # [..., column, k]
    v = np.swapaxes(v, -1, -2)  # [..., row k, column]
    o = _idct_1d(v, 65536 + (128 << 17)) >> 17
    return np.clip(o, 0, 255).astype(np.uint8)


def idct_plane(coef, quant):
    """coef int16 [blocks_h][blocks_w][64] -> the plane uint8 [8 blocks_h][8 blocks_w]"""
    bh, bw = coef.shape[:2]
    t = idct_blocks(coef, quant)  # [bh][bw][8][8]
    return t.transpose(0, 2, 1, 3).reshape(8 * bh, 8 * bw)


def _rows_v2(y, rows):
    """near / far rows of output row y for vs == 2: the walk of ref :3611-3644"""
    near = y >> 1
    far = np.where(y & 1, np.minimum(near + 1, rows - 1), np.maximum(near - 1, 0))
    return near, far


def resample(plane, rows, hs, vs, w, h):
    """Component plane (uint8 [>= rows][>= ceil(w / hs)]) -> int64 [h][w]: the sample stb's resampler gives output pixel (x, y)."""
    p = np.asarray(plane, np.int64)
    wl = (w + hs - 1) // hs
    y = np.arange(h)[:, None]
    x = np.arange(w)[None, :]
    if hs == 1 and vs == 1:
        return p[:h, :w]
    if vs == 2 and hs <= 2:
        ny, fy = _rows_v2(y, rows)
        if hs == 1:  # ref :3173
            return (3 * p[ny, x] + p[fy, x] + 2) >> 2
        t = 3 * p[ny[:, 0], :wl] + p[fy[:, 0], :wl]  # [h][wl], ref :3213-3235
        if wl == 1:
            return np.broadcast_to((t[:, :1] + 2) >> 2, (h, w)).copy()
        i = (x + 1) >> 1
        ic = np.clip(i, 1, wl - 1)
        t0, t1 = t[:, ic[0] - 1], t[:, ic[0]]
        mid = np.where(x & 1, (3 * t0 + t1 + 8) >> 4, (3 * t1 + t0 + 8) >> 4)
        out = np.where(x == 0, (t[:, :1] + 2) >> 2, mid)
        return np.where(x == 2 * wl - 1, (t[:, wl - 1:wl] + 2) >> 2, out)
    if hs == 2 and vs == 1:  # ref :3183-3209
        r = p[:h, :wl]
        if wl == 1:
            return np.broadcast_to(r[:, :1], (h, w)).copy()
        i = x >> 1
        left, right = r[:, np.clip(i[0] - 1, 0, wl - 1)], r[:, np.clip(i[0] + 1, 0, wl - 1)]
        mid = np.where(x & 1, (3 * r[:, i[0]] + right + 2) >> 2, (3 * r[:, i[0]] + left + 2) >> 2)
        out = np.where(x == 0, r[:, :1], mid)
        out = np.where(x == 2 * wl - 2, (3 * r[:, wl - 2:wl - 1] + r[:, wl - 1:wl] + 2) >> 2, out)  # :3202
        return np.where(x == 2 * wl - 1, r[:, wl - 1:wl], out)
    return p[y // vs, x // hs]  # ref :3354, the walk reduces to y // vs


def _f2fix(x):  # ref :3367, all in float
    return int(np.float32(x) * np.float32(4096.0) + np.float32(0.5)) << 8


def ycbcr_to_rgb(yy, cb, cr):
    """ref :3368-3391 on int64 arrays of one shape -> uint8 [..., 3]"""
    yf = (yy << 20) + (1 << 19)
    cr = cr - 128
    cb = cb - 128
    r = yf + cr * _f2fix(1.40200)
    g = yf + cr * -_f2fix(0.71414) + (((cb * -_f2fix(0.34414)) & 0xffffffff & 0xffff0000) ^ 0x80000000) - 0x80000000
    b = yf + cb * _f2fix(1.77200)
    _chk(r, g, b)
    return np.clip(np.stack([r >> 20, g >> 20, b >> 20], axis=-1), 0, 255).astype(np.uint8)


def to_rgb(w, h, mode, comps):
    """comps: [{"plane", "rows", "hs", "vs"}] -> uint8 [h][w][3]; mode "ycbcr" | "rgb" | "grey" """
    s = [resample(c["plane"], c.get("rows", np.shape(c["plane"])[0]), c["hs"], c["vs"], w, h) for c in comps[:1 if mode == "grey" else 3]]
    if mode == "ycbcr":
        return ycbcr_to_rgb(s[0], s[1], s[2])
    if mode == "rgb":
        return np.stack(s, axis=-1).astype(np.uint8)
    return np.stack([s[0]] * 3, axis=-1).astype(np.uint8)


def decode(d):
    """jpeg_coefficients' dict -> uint8 [h][w][3]"""
    comps = [{"plane": idct_plane(c["coef"], c["quant"]), "rows": c["rows"], "hs": c["hs"], "vs": c["vs"]} for c in d["components"]]
    return to_rgb(d["w"], d["h"], d["mode"], comps)
