"""PNG after the inflate, restated in numpy: what mi355_png_unfilter and mi355_png_to_rgb compute, and the encoder side (filtering
chosen rows with chosen per-row filters, packing samples, splitting an image into its Adam7 passes) that builds their inputs.  The
rules are stb_image v2.19's (the reference's src/stb_image.h:4307-4931); tests/test_png_cpu.py pins unfilter() to a per-byte loop of
the definition and the whole to the pixels the compiled reference loads (tests/golden/png_expected.npz)."""
import numpy as np

# (xorig, yorig, xspc, yspc) of the seven passes
ADAM7 = ((0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2))
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
PAIRS = [(0, 1), (0, 2), (0, 4), (0, 8), (0, 16), (2, 8), (2, 16), (3, 1), (3, 2), (3, 4), (3, 8), (4, 8), (4, 16), (6, 8), (6, 16)]
GREY_SCALE = {1: 0xFF, 2: 0x55, 4: 0x11, 8: 1}


def filter_unit(depth, color):
    return 1 if depth < 8 else CHANNELS[color] * depth // 8


def row_bytes(w, depth, color):
    return (w * CHANNELS[color] * depth + 7) // 8


def pass_size(w, h, index):
    xo, yo, xs, ys = ADAM7[index]
    return max(0, (w - xo + xs - 1) // xs), max(0, (h - yo + ys - 1) // ys)


def paeth(a, b, c):
    a, b, c = (np.asarray(v, np.int32) for v in (a, b, c))
    pa, pb, pc = np.abs(b - c), np.abs(a - c), np.abs(a + b - 2 * c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def _predict(f, a, b, c):
    f = np.asarray(f)
    return np.select([f == 1, f == 2, f == 3, f == 4], [a, b, (a + b) >> 1, paeth(a, b, c)], 0)


def unfilter(filtered, bpp):
    """filtered: uint8 [rows][1 + row_bytes], every row led by its filter byte (above 4: as None) -> uint8 [rows][row_bytes].
    Walks the anti-diagonals of the (row, unit) grid, the only order in which everything a unit needs is known."""
    filtered = np.asarray(filtered, np.uint8)
    rows, rb = filtered.shape[0], filtered.shape[1] - 1
    assert rb % bpp == 0
    W = rb // bpp
    f = filtered[:, 0].astype(np.int32)
    raw = filtered[:, 1:].astype(np.int32).reshape(rows, W, bpp)
    P = np.zeros((rows + 1, W + 1, bpp), np.int32)  # P[y + 1][x + 1]: unit x of row y; row 0 and column 0 are the zeros outside
    for d in range(rows + W - 1):
        ys = np.arange(max(0, d - W + 1), min(rows - 1, d) + 1)
        xs = d - ys
        a, b, c = P[ys + 1, xs], P[ys, xs + 1], P[ys, xs]
        P[ys + 1, xs + 1] = (raw[ys, xs] + _predict(f[ys][:, None], a, b, c)) & 255
    return P[1:, 1:].reshape(rows, rb).astype(np.uint8)


def unfilter_bytewise(filtered, bpp):
    """the definition, one byte at a time (small inputs only)"""
    rows, rb = len(filtered), len(filtered[0]) - 1
    out = [[0] * rb for _ in range(rows)]
    for y in range(rows):
        f = int(filtered[y][0])
        for i in range(rb):
            a = out[y][i - bpp] if i >= bpp else 0
            b = out[y - 1][i] if y else 0
            c = out[y - 1][i - bpp] if y and i >= bpp else 0
            if f == 1:
                p = a
            elif f == 2:
                p = b
            elif f == 3:
                p = (a + b) // 2
            elif f == 4:
                q = a + b - c
                pa, pb, pc = abs(q - a), abs(q - b), abs(q - c)
                p = a if pa <= pb and pa <= pc else (b if pb <= pc else c)
            else:
                p = 0
            out[y][i] = (int(filtered[y][1 + i]) + p) & 255
    return np.array(out, np.uint8).reshape(rows, rb)


def filter_rows(recon, filters, bpp):
    """The encoder: recon uint8 [rows][row_bytes], filters[y] in 0..4 -> uint8 [rows][1 + row_bytes]."""
    recon = np.asarray(recon, np.uint8).astype(np.int32)
    rows, rb = recon.shape
    a = np.zeros_like(recon)
    a[:, bpp:] = recon[:, :rb - bpp]
    b = np.zeros_like(recon)
    b[1:] = recon[:-1]
    c = np.zeros_like(recon)
    c[1:, bpp:] = recon[:-1, :rb - bpp]
    f = np.asarray(filters, np.int32).reshape(rows, 1)
    out = np.empty((rows, rb + 1), np.uint8)
    out[:, 0] = f[:, 0]
    out[:, 1:] = (recon - _predict(f, a, b, c)) & 255
    return out


def pack_samples(samples, depth):
    """samples: int [rows][w][channels], each below 2 ** depth -> uint8 [rows][row_bytes] (MSB first, 16 bits big-endian)"""
    s = np.asarray(samples)
    rows, w, n = s.shape
    if depth == 8:
        return s.astype(np.uint8).reshape(rows, w * n)
    if depth == 16:
        return np.stack([s >> 8, s & 255], -1).astype(np.uint8).reshape(rows, w * n * 2)
    bits = ((s.reshape(rows, w * n, 1) >> np.arange(depth - 1, -1, -1)) & 1).astype(np.uint8).reshape(rows, w * n * depth)
    return np.packbits(bits, axis=1)


def unpack_samples(rows_u8, w, depth, color):
    """reconstructed rows -> uint8 [rows][w][channels] as stb holds them before the channel change: depth 16 keeps the high byte,
    depths below 8 are unpacked MSB first and grey is scaled"""
    r = np.asarray(rows_u8, np.uint8)
    n = CHANNELS[color]
    if depth == 8:
        return r[:, :w * n].reshape(-1, w, n)
    if depth == 16:
        return r[:, :w * n * 2].reshape(-1, w, n, 2)[..., 0]
    bits = np.unpackbits(r, axis=1)[:, :w * depth].reshape(-1, w, depth).astype(np.int32)
    v = (bits << np.arange(depth - 1, -1, -1)).sum(-1)
    if color == 0:
        v = v * GREY_SCALE[depth]
    return v.astype(np.uint8).reshape(-1, w, 1)


def adam7_split(samples):
    """[h][w][n] -> {pass index: [rows][pw][n]} for the passes that hold pixels"""
    s = np.asarray(samples)
    out = {}
    for k, (xo, yo, xs, ys) in enumerate(ADAM7):
        p = s[yo::ys, xo::xs]
        if p.shape[0] and p.shape[1]:
            out[k] = p
    return out


def to_rgb(w, h, depth, color, interlace, passes, palette=None, pal_len=None):
    """passes: {index: reconstructed uint8 [rows][row_bytes]} (plain: {0: ..}) -> uint8 [h][w][3], stbi_load(.., 3)'s pixels"""
    out = np.zeros((h, w, 3), np.uint8)
    for k, rows in passes.items():
        xo, yo, xs, ys = ADAM7[k] if interlace else (0, 0, 1, 1)
        pw = pass_size(w, h, k)[0] if interlace else w
        s = unpack_samples(rows, pw, depth, color)
        if color == 3:
            pal = np.zeros((256, 3), np.uint8)
            src = np.asarray(palette, np.uint8).reshape(-1, 3)
            n = len(src) if pal_len is None else pal_len
            pal[:n] = src[:n]
            rgb = pal[s[..., 0]]
        elif color in (0, 4):
            rgb = np.repeat(s[..., :1], 3, axis=-1)
        else:
            rgb = s[..., :3]
        out[yo::ys, xo::xs] = rgb
    return out


def decode_scanlines(d):
    """png_scanlines' dict (yolo_quantization_amd.binding) -> uint8 [h][w][3]: both kernels' restatements on a file's inflated bytes"""
    passes = {}
    for q in d["passes"]:
        n = q["rows"] * (q["row_bytes"] + 1)
        passes[q["index"]] = unfilter(d["filtered"][q["offset"]:q["offset"] + n].reshape(q["rows"], q["row_bytes"] + 1), d["bpp"])
    return to_rgb(d["w"], d["h"], d["depth"], d["color"], d["interlace"], passes, d["palette"], d["pal_len"])
