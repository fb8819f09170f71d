"""Writes tests/golden/jpeg/*.jpg and tests/golden/jpeg_expected.npz: small baseline JPEG files and, per file, the RGB bytes the
compiled reference loads from it (refdrv.load_image_color -> stbi_load(.., 3); rint(255 * float), after asserting that the floats
are exactly float32(byte / 255.)).  Needs Pillow and the built oracle/_ref; run by hand, the results are committed.

Three kinds of files:
  * written by Pillow (libjpeg): 4:4:4 / 4:2:2 / 4:2:0 at MCU multiples and odd sizes, tiny sizes, greyscale, restart intervals,
    optimised Huffman tables, quality 30 / 100, custom quantiser tables;
  * Pillow files with header bytes rewritten: 4:4:0 and 4:1:1 (SOF sampling factors and dimensions changed so that the MCU count and
    the blocks per MCU stay what the stream holds -- the picture is scrambled, the stream decodes), Adobe transform 0 and component
    ids 'R','G','B' (RGB pass-through), a 16-bit quantiser table, SOF1;
  * written by the small baseline encoder below from random coefficients, for what Pillow cannot request: one component per scan
    (non-interleaved), a quantiser table redefined between scans, 4:1:0, a 3x1 sampling factor.
Every file must be one the reference decodes: the generator fails otherwise.  progressive.jpg and cmyk.jpg are for the refusal
tests and have no expectation.
"""
import os
import struct
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
import refdrv  # noqa: E402

OUT = os.path.join(HERE, "jpeg")

ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42,
          49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]


def picture(w, h, seed, grey=False):
    """smooth gradients plus noise: every DCT frequency is present, both clamps are reached"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([(x * 255) // max(w - 1, 1), (y * 255) // max(h - 1, 1), ((x + y) * 255) // max(w + h - 2, 1)], axis=-1)
    a = np.clip(base + rng.integers(-70, 71, (h, w, 3)), 0, 255).astype(np.uint8)
    return a[:, :, 0] if grey else a


# ---- marker segments -------------------------------------------------------------------------------------------------------------
def segments(data):
    """[(marker, start, end)] of the segments in front of the first scan; start is the 0xFF, end is behind the payload"""
    out, pos = [], 2
    while True:
        assert data[pos] == 0xFF
        m = data[pos + 1]
        n = struct.unpack(">H", data[pos + 2:pos + 4])[0]
        out.append((m, pos, pos + 2 + n))
        if m == 0xDA:
            return out
        pos += 2 + n


def rewrite_sof(data, w, h, sampling):
    """the frame header's size and the components' sampling bytes replaced"""
    b = bytearray(data)
    for m, s, _ in segments(data):
        if m in (0xC0, 0xC1):
            b[s + 5:s + 9] = struct.pack(">HH", h, w)
            for i, (hh, vv) in enumerate(sampling):
                b[s + 11 + 3 * i] = hh << 4 | vv
    return bytes(b)


def adobe_rgb(data):
    """the JFIF segment replaced by an Adobe APP14 segment with colour transform 0: the components are R, G, B as they are"""
    (m, s, e) = segments(data)[0]
    assert m == 0xE0
    app14 = b"\xff\xee" + struct.pack(">H", 14) + b"Adobe\x00" + b"\x64\x00\x00\x00\x00" + b"\x00"
    return data[:s] + app14 + data[e:]


def rgb_ids(data):
    """component ids 'R', 'G', 'B' in the frame and scan headers"""
    b = bytearray(data)
    for m, s, _ in segments(data):
        for i in range(3):
            if m in (0xC0, 0xC1):
                b[s + 10 + 3 * i] = b"RGB"[i]
            if m == 0xDA:
                b[s + 5 + 2 * i] = b"RGB"[i]
    return bytes(b)


def dqt16(data):
    """the first quantiser table rewritten with 16-bit entries, one of them above 255"""
    for m, s, e in segments(data):
        if m == 0xDB:
            assert data[s + 4] >> 4 == 0
            vals = list(data[s + 5:s + 69])
            vals[5] = 300
            seg = b"\xff\xdb" + struct.pack(">H", 2 + 129) + bytes([0x10 | (data[s + 4] & 15)]) + struct.pack(">64H", *vals)
            rest = data[s + 69:e]  # further tables of the same segment
            if rest:
                seg += b"\xff\xdb" + struct.pack(">H", 2 + len(rest)) + rest
            return data[:s] + seg + data[e:]
    raise AssertionError("no DQT")


def sof1(data):
    b = bytearray(data)
    for m, s, _ in segments(data):
        if m == 0xC0:
            b[s + 1] = 0xC1
    return bytes(b)


# ---- a small baseline encoder (T.81 annex F.1.2) for coefficient-level files -------------------------------------------------------
def huff_tables_of(data):
    """{(class, id): (counts[16], values)} of a file's DHT segments"""
    out = {}
    for m, s, e in segments(data):
        if m != 0xC4:
            continue
        pos = s + 4
        while pos < e:
            tc_th = data[pos]
            counts = list(data[pos + 1:pos + 17])
            n = sum(counts)
            out[(tc_th >> 4, tc_th & 15)] = (counts, list(data[pos + 17:pos + 17 + n]))
            pos += 17 + n
    return out


def code_map(counts, values):
    codes, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            codes[values[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return codes


class BitWriter:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, value, length):
        self.acc = self.acc << length | (value & ((1 << length) - 1))
        self.n += length
        while self.n >= 8:
            byte = self.acc >> (self.n - 8) & 255
            self.out.append(byte)
            if byte == 0xFF:
                self.out.append(0)
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)


def magnitude(v):
    size = int(abs(v)).bit_length()
    return size, (v if v >= 0 else v + (1 << size) - 1)


def encode_block(bw, blk, pred, dc, ac):
    diff = int(blk[0]) - pred
    size, bits = magnitude(diff)
    bw.put(*dc[size])
    if size:
        bw.put(bits, size)
    run = 0
    zz = [int(blk[ZIGZAG[k]]) for k in range(64)]
    last = max([k for k in range(1, 64) if zz[k]], default=0)
    for k in range(1, last + 1):
        if zz[k] == 0:
            run += 1
            continue
        while run > 15:
            bw.put(*ac[0xF0])
            run -= 16
        size, bits = magnitude(zz[k])
        bw.put(*ac[run << 4 | size])
        bw.put(bits, size)
        run = 0
    if last < 63:
        bw.put(*ac[0x00])
    return int(blk[0])


def write_coefficient_jpeg(w, h, comps, qtables, scans, seed, tables, requant=None):
    """comps: [(id, h, v, tq)]; qtables: {tq: [64] natural order}; scans: lists of component indices; requant: {scan index: {tq:
    table}}, DQT segments written in front of that scan.  Coefficients are random: a DC walk and a few low frequencies per block."""
    rng = np.random.default_rng(seed)
    hmax, vmax = max(c[1] for c in comps), max(c[2] for c in comps)
    mx, my = -(-w // (8 * hmax)), -(-h // (8 * vmax))
    dcmap, acmap = code_map(*tables[(0, 0)]), code_map(*tables[(1, 0)])

    def dqt(tabs):
        seg = b""
        for tq, t in tabs.items():
            seg += b"\xff\xdb" + struct.pack(">H", 67) + bytes([tq]) + bytes(int(t[ZIGZAG[k]]) for k in range(64))
        return seg

    def dht(tc, key):
        counts, values = tables[key]
        return b"\xff\xc4" + struct.pack(">H", 19 + len(values)) + bytes([tc << 4]) + bytes(counts) + bytes(values)

    coef = []
    for (_, ch, cv, _) in comps:
        bwid, bhei = mx * ch, my * cv
        c = np.zeros((bhei, bwid, 64), np.int16)
        c[:, :, 0] = np.clip(np.cumsum(rng.integers(-12, 13, bhei * bwid)).reshape(bhei, bwid), -200, 200)
        for k in (1, 8, 9, 2, 16, 10, 27, 63):
            c[:, :, k] = rng.integers(-6, 7, (bhei, bwid)) * (rng.random((bhei, bwid)) < 0.4)
        coef.append(c)
    out = bytearray(b"\xff\xd8\xff\xe0" + struct.pack(">H", 16) + b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    out += dqt(qtables)
    out += b"\xff\xc0" + struct.pack(">HBHHB", 8 + 3 * len(comps), 8, h, w, len(comps))
    for (cid, ch, cv, tq) in comps:
        out += bytes([cid, ch << 4 | cv, tq])
    out += dht(0, (0, 0)) + dht(1, (1, 0))
    for si, scan in enumerate(scans):
        if requant and si in requant:
            out += dqt(requant[si])
        out += b"\xff\xda" + struct.pack(">HB", 6 + 2 * len(scan), len(scan))
        for ci in scan:
            out += bytes([comps[ci][0], 0x00])
        out += b"\x00\x3f\x00"
        bw = BitWriter()
        pred = [0] * len(comps)
        if len(scan) == 1:  # the component's own blocks in raster order, over its real size
            ci = scan[0]
            cw = -(-(w * comps[ci][1]) // hmax)
            chh = -(-(h * comps[ci][2]) // vmax)
            for by in range(-(-chh // 8)):
                for bx in range(-(-cw // 8)):
                    pred[ci] = encode_block(bw, coef[ci][by, bx], pred[ci], dcmap, acmap)
        else:
            for uy in range(my):
                for ux in range(mx):
                    for ci in scan:
                        for yy in range(comps[ci][2]):
                            for xx in range(comps[ci][1]):
                                blk = coef[ci][uy * comps[ci][2] + yy, ux * comps[ci][1] + xx]
                                pred[ci] = encode_block(bw, blk, pred[ci], dcmap, acmap)
        bw.flush()
        out += bw.out
    out += b"\xff\xd9"
    return bytes(out)


# ---- the fixtures ----------------------------------------------------------------------------------------------------------------
def pillow(name, w, h, seed, grey=False, **kw):
    path = os.path.join(OUT, name + ".jpg")
    Image.fromarray(picture(w, h, seed, grey)).save(path, "JPEG", **kw)
    return path


def raw(name, data):
    path = os.path.join(OUT, name + ".jpg")
    with open(path, "wb") as f:
        f.write(data)
    return path


def read(path):
    with open(path, "rb") as f:
        return f.read()


def expectation(path):
    f = refdrv.load_image_color(path)  # float32 [3][h][w]; exits the process on a file stb refuses
    by = np.rint(f * 255).astype(np.uint8)
    assert np.array_equal(f, (by / 255.).astype(np.float32)), path
    return np.ascontiguousarray(by.transpose(1, 2, 0))


def main():
    os.makedirs(OUT, exist_ok=True)
    paths, seed = [], 0
    for ss, tag in ((0, "444"), (1, "422"), (2, "420")):
        for (w, h) in ((48, 32), (51, 37)):
            seed += 1
            paths.append(pillow(f"{tag}_{w}x{h}", w, h, seed, subsampling=ss, quality=85))
        for (w, h) in ((1, 1), (17, 1), (1, 13), (2, 5), (3, 4), (4, 3)):  # one pixel / row / column; w_lores 1 (w 1, 2) and 2 (w 3, 4)
            seed += 1
            paths.append(pillow(f"{tag}_{w}x{h}", w, h, seed, subsampling=ss, quality=90))
    paths.append(pillow("grey_51x37", 51, 37, 40, grey=True, quality=85))
    paths.append(pillow("grey_8x8", 8, 8, 41, grey=True, quality=85))
    paths.append(pillow("420_restart1_51x37", 51, 37, 42, subsampling=2, quality=85, restart_marker_blocks=1))
    paths.append(pillow("422_restart2_51x37", 51, 37, 43, subsampling=1, quality=85, restart_marker_blocks=2))
    paths.append(pillow("420_optimised_51x37", 51, 37, 44, subsampling=2, quality=85, optimize=True))
    paths.append(pillow("420_q30_51x37", 51, 37, 45, subsampling=2, quality=30))
    paths.append(pillow("444_q100_51x37", 51, 37, 46, subsampling=0, quality=100))
    luma = [3 + (k % 8) + 2 * (k // 8) for k in range(64)]
    chroma = [40 - (k % 8) - 3 * (k // 8) for k in range(64)]
    paths.append(pillow("420_two_tables_51x37", 51, 37, 47, subsampling=2, qtables=[luma, chroma]))
    # header rewrites: the stream of a 48x32 4:2:2 file (3 x 4 MCUs of 2 + 1 + 1 blocks) read as 4:4:0, that of a 48x32 4:2:0 file
    # (3 x 2 MCUs of 4 + 1 + 1 blocks) as 4:1:1
    s422, s420, s444 = (read(os.path.join(OUT, f"{t}_48x32.jpg")) for t in ("422", "420", "444"))
    paths.append(raw("440_23x61", rewrite_sof(s422, 23, 61, [(1, 2), (1, 1), (1, 1)])))
    paths.append(raw("440_24x64", rewrite_sof(s422, 24, 64, [(1, 2), (1, 1), (1, 1)])))
    paths.append(raw("411_61x23", rewrite_sof(s420, 61, 23, [(4, 1), (1, 1), (1, 1)])))
    paths.append(raw("411_64x24", rewrite_sof(s420, 64, 24, [(4, 1), (1, 1), (1, 1)])))
    paths.append(raw("rgb_adobe0_48x32", adobe_rgb(s444)))
    paths.append(raw("rgb_ids_48x32", rgb_ids(s444)))
    paths.append(raw("444_dqt16_48x32", dqt16(s444)))
    paths.append(raw("420_sof1_48x32", sof1(s420)))
    # coefficient-level files
    tables = huff_tables_of(s444)
    qa, qb = [6 + (k % 8) + (k // 8) for k in range(64)], [14 + 2 * (k % 8) for k in range(64)]
    ycc = [(1, 1, 1, 0), (2, 1, 1, 1), (3, 1, 1, 1)]
    paths.append(raw("444_noninterleaved_29x19", write_coefficient_jpeg(29, 19, ycc, {0: qa, 1: qb}, [[0], [1], [2]], 60, tables)))
    paths.append(raw("420_noninterleaved_37x27",
                     write_coefficient_jpeg(37, 27, [(1, 2, 2, 0), (2, 1, 1, 1), (3, 1, 1, 1)], {0: qa, 1: qb}, [[0], [1], [2]], 61, tables)))
    # table 1 is redefined between the Cb and the Cr scan: Cb keeps the first definition
    paths.append(raw("444_requant_29x19", write_coefficient_jpeg(29, 19, ycc, {0: qa, 1: qb}, [[0], [1], [2]], 62, tables, requant={2: {1: qa}})))
    paths.append(raw("410_61x27", write_coefficient_jpeg(61, 27, [(1, 4, 2, 0), (2, 1, 1, 1), (3, 1, 1, 1)], {0: qa, 1: qb}, [[0, 1, 2]], 63, tables)))
    paths.append(raw("h3v1_43x11", write_coefficient_jpeg(43, 11, [(1, 3, 1, 0), (2, 1, 1, 1), (3, 1, 1, 1)], {0: qa, 1: qb}, [[0, 1, 2]], 64, tables)))
    paths.append(raw("h1v4_11x43", write_coefficient_jpeg(11, 43, [(1, 1, 4, 0), (2, 1, 1, 1), (3, 1, 2, 1)], {0: qa, 1: qb}, [[0, 1, 2]], 65, tables)))
    paths.append(raw("h1v3_11x29", write_coefficient_jpeg(11, 29, [(1, 1, 3, 0), (2, 1, 1, 1), (3, 1, 1, 1)], {0: qa, 1: qb}, [[0, 1, 2]], 67, tables)))
    paths.append(raw("h2v2_chroma_h2v1_37x27",
                     write_coefficient_jpeg(37, 27, [(1, 2, 2, 0), (2, 2, 1, 1), (3, 1, 2, 1)], {0: qa, 1: qb}, [[0, 1, 2]], 66, tables)))

    expected = {os.path.splitext(os.path.basename(p))[0]: expectation(p) for p in paths}
    np.savez_compressed(os.path.join(HERE, "jpeg_expected.npz"), **expected)
    # for the refusal tests only
    Image.fromarray(picture(32, 24, 70)).save(os.path.join(OUT, "progressive.jpg"), "JPEG", progressive=True)
    Image.fromarray(picture(32, 24, 71)).convert("CMYK").save(os.path.join(OUT, "cmyk.jpg"), "JPEG")
    total = sum(os.path.getsize(os.path.join(OUT, f)) for f in os.listdir(OUT))
    print(f"{len(paths)} fixtures + 2 refused files, {total} bytes of .jpg, "
          f"{os.path.getsize(os.path.join(HERE, 'jpeg_expected.npz'))} bytes of expectations")


if __name__ == "__main__":
    main()
