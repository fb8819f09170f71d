"""Frame views (mi355_frame_view: a rectangle of a frame under an EXIF orientation) restated in numpy, and the case tables of
tests/test_frame_views_cpu.py and tests/test_gpu_frame_views.py.  No device code, no ctypes here.

The view of a frame is V = O_orient(RGB(frame)[y0 : y0 + h, x0 : x0 + w]); what the view calls must give is what the u8 calls' contract gives
for V as an interleaved RGB frame (frame_geometry.expected_rgb: the oracle's letterbox, the quantiser line, the min / max words)."""
from collections import namedtuple

import numpy as np

import frame_geometry as fg

ORIENTS = tuple(range(1, 9))
View = namedtuple("View", "x0 y0 w h orient")


def oriented(a, orient):
    """O_orient of an [h][w][3] array: the header's table, the transforms that make a file with that EXIF value upright"""
    return {1: lambda: a, 2: lambda: a[:, ::-1], 3: lambda: a[::-1, ::-1], 4: lambda: a[::-1], 5: lambda: a.transpose(1, 0, 2),
            6: lambda: np.rot90(a, -1), 7: lambda: a[::-1, ::-1].transpose(1, 0, 2), 8: lambda: np.rot90(a, 1)}[orient]()


def apply_view(rgb, view):
    """V as a contiguous uint8 [vh][vw][3] frame"""
    v = View(*view)
    assert 0 <= v.x0 and 0 <= v.y0 and v.w >= 1 and v.h >= 1 and v.x0 + v.w <= rgb.shape[1] and v.y0 + v.h <= rgb.shape[0]
    return np.ascontiguousarray(oriented(rgb[v.y0:v.y0 + v.h, v.x0:v.x0 + v.w], v.orient))


def view_size(view):
    v = View(*view)
    return (v.h, v.w) if v.orient >= 5 else (v.w, v.h)


def tap_to_frame(view, u, t):
    """the index maps of the kernels' Viewed source: the frame coordinates of view pixel (u, t)"""
    v = View(*view)
    cw, ch = v.w, v.h
    x, y = {1: (u, t), 2: (cw - 1 - u, t), 3: (cw - 1 - u, ch - 1 - t), 4: (u, ch - 1 - t), 5: (t, u), 6: (t, ch - 1 - u),
            7: (cw - 1 - t, ch - 1 - u), 8: (cw - 1 - t, u)}[v.orient]
    return v.x0 + x, v.y0 + y


def apply_view_by_loop(rgb, view):
    """apply_view pixel by pixel through the index maps"""
    vw, vh = view_size(view)
    out = np.zeros((vh, vw, 3), np.uint8)
    for t in range(vh):
        for u in range(vw):
            x, y = tap_to_frame(view, u, t)
            out[t, u] = rgb[y, x]
    return out


def accepted(view, w, h):
    vw, vh = view_size(view)
    return bool(fg.geometry1(vw, vh, w, h).accepted)


# ------------------------------------------------------------------------------------------------------------------------------ cases
FRAMES = ((13, 9), (8, 6), (2, 2))          # (w, h) of the frames
NETS = ((12, 12), (16, 12), (7, 5))         # the network inputs; 7 x 5: a width that is no multiple of 4
OUT_OFF = {(12, 12): 0, (16, 12): 1, (7, 5): 3}  # bytes between an aligned address and the output


def rects(fw, fh):
    """{label: (x0, y0, w, h)} of a frame: one label per clause of the view's addressing"""
    r = {"whole": (0, 0, fw, fh), "last_column": (fw - 1, 0, 1, fh), "last_row": (0, fh - 1, fw, 1),
         "right_bottom": (fw // 2, fh // 2, fw - fw // 2, fh - fh // 2), "corner_2x2_far": (fw - 2, fh - 2, 2, 2), "corner_2x2_near": (0, 0, 2, 2),
         "one_pixel": (fw - 1, fh - 1, 1, 1)}
    if fw >= 5 and fh >= 5:
        r["odd_offset_odd_size"] = (1, 1, fw // 2 | 1, fh // 2 | 1)
        r["odd_offset_to_the_edges"] = (3, 1, fw - 3, fh - 1)
    return r


RECT_CLAUSES = {
    "whole": lambda f, r: r == (0, 0) + f,
    "odd_x0_y0_w_h": lambda f, r: all(v % 2 == 1 for v in r),
    "last_column_alone": lambda f, r: r[0] == f[0] - 1 and r[2] == 1 and r[3] > 1,
    "last_row_alone": lambda f, r: r[1] == f[1] - 1 and r[3] == 1 and r[2] > 1,
    "touches_right_and_bottom": lambda f, r: r[0] + r[2] == f[0] and r[1] + r[3] == f[1] and r[0] > 0 and r[1] > 0,
    "strictly_inside": lambda f, r: r[0] > 0 and r[1] > 0 and r[0] + r[2] < f[0] and r[1] + r[3] < f[1],
    "2x2_in_a_corner": lambda f, r: r[2:] == (2, 2) and r[0] in (0, f[0] - 2) and r[1] in (0, f[1] - 2),
    "1x1": lambda f, r: r[2:] == (1, 1),
}

# (frame, label, rect, net): every orient is a slot of one launch; the orients the letterbox geometry refuses are refused, not launched
U8_CASES = [(f, label, r, n) for f in FRAMES for label, r in rects(*f).items() for n in NETS]

# Per kind, the offsets its addressing cares about, on the 13 x 9 frame: x0 in 0..3 (the four positions inside a MIPI10 group, both
# halves of a 4:2:2 macropixel and of a MIPI12 group, both columns of a 4:2:0 chroma sample), y0 in {0, 1}; 6 wide, so that a view from an odd x0
# starts and ends inside a macropixel; the last two touch the right and bottom edges, where a Bayer window reflects at the FRAME's border
KIND_FRAME = (13, 9)
KIND_RECTS = [(x0, y0, 6, 5) for y0 in (0, 1) for x0 in (0, 1, 2, 3)] + [(7, 4, 6, 5), (3, 3, 10, 6), (0, 0, 13, 9)]
KIND_NETS = ((12, 12), (7, 5))
KIND_VIEWS = [View(*r, o) for r in KIND_RECTS for o in ORIENTS]

# Bayer: a view strictly inside the frame at odd (x0, y0) and one touching the far edges
BAYER_INSIDE = (3, 1, 7, 5)
BAYER_EDGE = (7, 3, 6, 6)

# refusals of a view: (name, view, message after "view: ") against a 13 x 9 frame into 12 x 12
FRAME_W, FRAME_H = 13, 9
M_ORIENT, M_RESERVED, M_SIZE, M_RECT = ("view: orient outside 1..8", "view: reserved must be 0", "view: need w, h >= 1",
                                        "view: rectangle outside the frame")
INT_MAX = 2 ** 31 - 1
REFUSED_VIEWS = (
    ("orient_0", (0, 0, 13, 9, 0), M_ORIENT), ("orient_9", (0, 0, 13, 9, 9), M_ORIENT), ("orient_negative", (0, 0, 13, 9, -1), M_ORIENT),
    ("w_0", (0, 0, 0, 9, 1), M_SIZE), ("h_0", (0, 0, 13, 0, 1), M_SIZE), ("w_negative", (5, 0, -3, 9, 1), M_SIZE),
    ("x0_negative", (-1, 0, 5, 5, 1), M_RECT), ("y0_negative", (0, -1, 5, 5, 1), M_RECT), ("too_wide", (1, 0, 13, 9, 1), M_RECT),
    ("too_high", (0, 1, 13, 9, 1), M_RECT), ("x0_behind", (13, 0, 1, 1, 1), M_RECT), ("y0_behind", (0, 9, 1, 1, 1), M_RECT),
    ("sum_overflows_w", (1, 0, INT_MAX, 1, 1), M_RECT), ("sum_overflows_h", (0, 1, 1, INT_MAX, 6), M_RECT),
    ("x0_int_max", (INT_MAX, 0, 1, 1, 1), M_RECT),
    # the order among the view's own refusals: orient, reserved (see the CPU file), size, rectangle
    ("orient_before_size", (0, 0, 0, 0, 0), M_ORIENT), ("size_before_rectangle", (-1, -1, 0, 1, 1), M_SIZE),
    # then the geometry of the ORIENTED size: 1 x 9 gives a resized side of 1, and so does 9 x 1
    ("degenerate_column", (12, 0, 1, 9, 1), fg.DEGENERATE), ("degenerate_column_turned", (12, 0, 1, 9, 6), fg.DEGENERATE),
    ("degenerate_row", (0, 8, 13, 1, 1), fg.DEGENERATE),
)


def rgb_frame(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def expected_view(rgb, view, w, h):
    """fg.Want of the view: the u8 contract on the materialised view"""
    return fg.expected_rgb(apply_view(rgb, view), w, h)


# ------------------------------------------------------------------------------------------------------------- boxes, restated
def box_to_frame(view, frame_w, frame_h, box):
    """network_view_box_to_frame in float64 numpy, rounded to float32 at the end: box = (x, y, w, h) float32, relative to the view"""
    v = View(*view)
    x, y, bw, bh = (np.float64(np.float32(t)) for t in box)
    cw, ch = np.float64(v.w), np.float64(v.h)
    vw, vh = (ch, cw) if v.orient >= 5 else (cw, ch)
    u, t, pw, ph = x * vw, y * vh, bw * vw, bh * vh
    cx, cy = {1: (u, t), 2: (cw - u, t), 3: (cw - u, ch - t), 4: (u, ch - t), 5: (t, u), 6: (t, ch - u), 7: (cw - t, ch - u),
              8: (cw - t, u)}[v.orient]
    if v.orient >= 5:
        pw, ph = ph, pw
    return np.array([(v.x0 + cx) / frame_w, (v.y0 + cy) / frame_h, pw / frame_w, ph / frame_h], np.float64).astype(np.float32)


def tiles(frame, count, overlap):
    """one axis of network_tile_views: (size, [starts]) or None when refused"""
    if frame < 1 or count < 1 or overlap < 0:
        return None
    size = -((frame + (count - 1) * overlap) // -count)
    if size > frame or overlap >= size:
        return None
    return size, [frame - size if i == count - 1 else min(i * (size - overlap), frame - size) for i in range(count)]


# ------------------------------------------------------------------------------------------------------------------------- EXIF, built
def exif_app1(orientation, big_endian=False, where="only", typ=3, count=1, ifd_offset=8, tag=0x0112):
    """an APP1 Exif segment whose IFD0 holds the orientation tag (`where`: only | first | last | absent among other tags)"""
    e = ">" if big_endian else "<"
    import struct

    def entry(tg, ty, cn, val):
        return struct.pack(e + "HHI", tg, ty, cn) + (struct.pack(e + "H", val) + b"\0\0" if ty == 3 else struct.pack(e + "I", val))
    others = [entry(0x0100, 3, 1, 640), entry(0x011A, 5, 1, 200)]
    mine = entry(tag, typ, count, orientation)
    entries = {"only": [mine], "first": [mine] + others, "last": others + [mine], "absent": others}[where]
    pad = b"\0" * (ifd_offset - 8) if ifd_offset >= 8 else b""
    tiff = (b"MM\0*" if big_endian else b"II*\0") + struct.pack(e + "I", ifd_offset) + pad + struct.pack(e + "H", len(entries)) + b"".join(entries) \
        + struct.pack(e + "I", 0)
    body = b"Exif\0\0" + tiff
    return b"\xff\xe1" + struct.pack(">H", len(body) + 2) + body


def jpeg_with(segments, tail=b"\xff\xda\x00\x02\xff\xd9"):
    """SOI, an APP0 JFIF stub, the segments, then a scan marker and the end"""
    app0 = b"\xff\xe0\x00\x10JFIF\0\x01\x01\0\0\x01\0\x01\0\0"
    return b"\xff\xd8" + app0 + b"".join(segments) + tail
