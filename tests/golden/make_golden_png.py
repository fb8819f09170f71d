"""Writes tests/golden/png/*.png and tests/golden/png_expected.npz: small PNG files and, per file, the RGB bytes the compiled
reference loads from it (refdrv.load_image_color -> stbi_load(.., 3); rint(255 * float), after asserting that the floats are exactly
float32(byte / 255.)).  The files come from the PNG writer of tests/png_streams.py, which chooses the filter of every row, the
interlace flag, the chunking and the deflate stream.  The files named refuse_* are the ones the decoder refuses; they have no
expectation.  Run by hand from the repository root, with oracle/_ref built:

    python tests/golden/make_golden_png.py
"""
import os
import struct
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import png_ref  # noqa: E402
import png_streams as ps  # noqa: E402
import refdrv  # noqa: E402

OUT = os.path.join(HERE, "png")
NAMES = {0: "grey", 2: "rgb", 3: "pal", 4: "ga", 6: "rgba"}


def picture(w, h, depth, color, seed):
    """int [h][w][channels] below 2 ** depth: gradients with a little coarse noise, in cells, so that the files stay small and every filter
    has something to predict"""
    rng = np.random.RandomState(seed)
    n = png_ref.CHANNELS[color]
    y, x = np.mgrid[0:h, 0:w]
    noise = np.repeat(np.repeat(rng.randint(0, 3, (h // 6 + 1, w // 6 + 1)), 6, 0), 6, 1)[:h, :w]  # coarse: 6 x 6 cells
    v = np.stack([(x * (3 + k) + y * (5 - k) + 17 * k + 8 * noise) % 256 for k in range(n)], -1)
    if depth == 16:
        return v * 256 + (x * 7 + y * 13)[..., None] % 256
    return v >> (8 - depth)


def palette(n, seed):
    return np.random.RandomState(seed).randint(0, 256, (n, 3)).astype(np.uint8)


def cycle(k, y):
    return (y + k) % 5


def fixed_only(raw):
    c = zlib.compressobj(9, zlib.DEFLATED, 15, 9, zlib.Z_FIXED)
    return c.compress(raw) + c.flush()


def window_file():
    """255 x 140 grey: rows of 256 filtered bytes, so that row y + 128 lies 32768 bytes behind row y; everything beyond the first
    32 KiB is coded as matches at distance 32768"""
    w, h = 255, 140
    rows = np.zeros((h, w + 1), np.uint8)
    rows[0, 1:] = (np.arange(w) * 5) % 256
    rows[1, 1:] = (np.arange(w) * 11 + 3) % 256
    for y in range(2, 128):
        rows[y] = rows[y - 2]
    rows[128:] = rows[:h - 128]
    raw = rows.tobytes()
    d = ps.Deflate()
    tokens = list(raw[:512])
    at = 512
    while at < 32768:
        n = min(258, 32768 - at)
        tokens.append((n, 512))
        at += n
    while at < len(raw):
        n = min(258, len(raw) - at)
        if len(raw) - at - n in (1, 2):
            n -= 3
        tokens.append((n, 32768))
        at += n
    d.fixed(tokens, final=True)
    assert bytes(d.raw) == raw and zlib.decompress(d.zlib()) == raw
    return ps.SIG + ps.ihdr(w, h, 8, 0) + ps.chunk(b"IDAT", d.zlib()) + ps.chunk(b"IEND")


def build_files():
    files = {}

    def add(name, w, h, depth, color, interlace=0, filters=cycle, seed=1, **kw):
        if color == 3 and "palette" not in kw:
            kw["palette"] = palette(1 << depth, seed + 100)
        files[name] = ps.write_png(picture(w, h, depth, color, seed), depth, color, interlace, filters, **kw)

    for color, depth in png_ref.PAIRS:  # every colour type / depth pair, plain and Adam7, the filters cycling row by row
        for il in (0, 1):
            add(f"{NAMES[color]}{depth}_{'adam7' if il else 'plain'}_51x37", 51, 37, depth, color, il, seed=color * 16 + depth)
    for w, h in ((1, 1), (1, 13), (17, 1), (2, 5), (3, 4), (4, 3)):  # Adam7 passes that are empty
        add(f"rgb8_adam7_{w}x{h}", w, h, 8, 2, 1, seed=w * 7 + h)
        add(f"pal4_adam7_{w}x{h}", w, h, 4, 3, 1, seed=w * 5 + h)
        add(f"grey16_plain_{w}x{h}", w, h, 16, 0, 0, seed=w * 3 + h)
    add("rgb8_plain_64x61", 64, 61, 8, 2, 0, seed=3)
    add("rgb8_adam7_64x61", 64, 61, 8, 2, 1, seed=4)
    add("grey1_adam7_64x61", 64, 61, 1, 0, 1, seed=5)
    for w, h in ((9, 131), (131, 9)):  # rows cross two band edges; widths below and above 64
        add(f"rgb8_plain_{w}x{h}", w, h, 8, 2, 0, seed=w)
        add(f"rgba8_adam7_{w}x{h}", w, h, 8, 6, 1, seed=w + 1)
        add(f"grey2_plain_{w}x{h}", w, h, 2, 0, 0, seed=w + 2)
    for f, fname in enumerate(("none", "sub", "up", "average", "paeth")):  # one filter on every row, the first included
        add(f"rgb8_plain_{fname}_51x37", 51, 37, 8, 2, 0, filters=lambda k, y, f=f: f, seed=20 + f)
        add(f"rgba16_adam7_{fname}_19x23", 19, 23, 16, 6, 1, filters=lambda k, y, f=f: f, seed=30 + f)
        add(f"grey4_plain_{fname}_33x17", 33, 17, 4, 0, 0, filters=lambda k, y, f=f: f, seed=40 + f)
    # tRNS: validated, without effect on RGB
    add("pal8_trns_23x19", 23, 19, 8, 3, 0, seed=50, trns=bytes(range(0, 200, 2)))
    add("grey8_trns_23x19", 23, 19, 8, 0, 0, seed=51, trns=struct.pack(">H", 40))
    add("grey16_trns_23x19", 23, 19, 16, 0, 1, seed=52, trns=struct.pack(">H", 0x2a15))
    add("rgb8_trns_23x19", 23, 19, 8, 2, 1, seed=53, trns=struct.pack(">HHH", 10, 20, 30))
    add("rgb16_trns_23x19", 23, 19, 16, 2, 0, seed=54, trns=struct.pack(">HHH", 0x1234, 0x5678, 0x9abc))
    add("pal4_short_palette_23x19", 23, 19, 4, 3, 0, seed=55, palette=palette(16, 155))
    # chunk layout
    gama, text = ps.chunk(b"gAMA", struct.pack(">I", 45455)), ps.chunk(b"tEXt", b"Comment\x00chunks in odd places")
    add("rgb8_idat_1byte_17x9", 17, 9, 8, 2, 0, seed=60, idat_sizes=[1])
    add("rgb8_idat_uneven_51x37", 51, 37, 8, 2, 1, seed=61, idat_sizes=[1, 7, 300, 2, 0, 64])
    add("rgb8_ancillary_51x37", 51, 37, 8, 2, 0, seed=62, idat_sizes=[100], before=[gama, ps.chunk(b"sRGB", b"\x00"), text],
        between=[text, ps.chunk(b"tIME", bytes(7))])
    add("rgb8_trailing_51x37", 51, 37, 8, 2, 0, seed=63, trailing=bytes(range(200)))
    add("grey8_adam7_trailing_51x37", 51, 37, 8, 0, 1, seed=64, trailing=bytes(5))
    # deflate
    add("rgb8_stored_33x17", 33, 17, 8, 2, 0, seed=70, deflate=lambda raw: zlib.compress(raw, 0))
    add("rgb8_fixed_51x37", 51, 37, 8, 2, 0, seed=71, deflate=fixed_only)
    add("rgb8_dynamic_51x37", 51, 37, 8, 2, 1, seed=72, deflate=lambda raw: zlib.compress(raw, 6))
    files["grey8_window_255x140"] = window_file()
    return files


def main():
    os.makedirs(OUT, exist_ok=True)
    files = build_files()
    expected = {}
    for name, data in sorted(files.items()):
        path = os.path.join(OUT, name + ".png")
        with open(path, "wb") as f:
            f.write(data)
        assert len(data) <= 8192, (name, len(data))
        im = refdrv.load_image_color(path)  # asserts that the reference loaded the file
        assert im.shape[0] == 3
        b = np.rint(im * np.float32(255)).astype(np.uint8)
        assert np.array_equal(b.astype(np.float32) / np.float32(255.), im), name
        expected[name] = np.ascontiguousarray(b.transpose(1, 2, 0))
    for name, (data, _) in sorted(ps.refusal_files().items()):
        with open(os.path.join(OUT, "refuse_" + name + ".png"), "wb") as f:
            f.write(data)
    np.savez_compressed(os.path.join(HERE, "png_expected.npz"), **expected)
    print(f"{len(expected)} files with expectations, {len(ps.refusal_files())} refusal files")


if __name__ == "__main__":
    main()
