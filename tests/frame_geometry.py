"""The batched frame input path (csrc/frames.hip: frame_geometry, letterbox_px3, the two kernel bodies, frames_check) at the points where its
letterbox geometry changes form: restatements, the case tables, one label per clause.

Shared by tests/test_frame_geometry_cpu.py (the restatements against tests/oracle.py, both sides of every label, invariants over a sweep, the
refusals through the shim's host-side check) and tests/test_gpu_frame_geometry.py (every case on the device).  No device code, no ctypes here.

Expected results: the floats are oracle.letterbox_image on the planes byte / 255, the bytes glue_edges.quantize_ref (the quantiser line:
float32 quotient, C round in double, + zp in double, to float, to int, clamp), the min / max glue_edges.minmax_ref (max(x, +0), min(x, -0) as
bit patterns).  Every comparison is exact.  q < 0 cannot occur in this path: every letterboxed float is >= 0 (bytes / 255 and 0.5 under
non-negative weights) and zp >= 0, so only the clamp at 255 is aimed at."""
import functools
from collections import namedtuple

import numpy as np

import oracle
from glue_edges import Reach, minmax_ref, quantize_ref  # noqa: F401  (Reach is used by the tests)

f32 = np.float32
SIDE_MAX = 32768      # frames_check: the largest side of a frame and of the network input
B_MAX = 65535         # frames_check: the largest batch (the grid's y extent)
SENTINEL = 0xA5       # around and between the outputs
PAD = 0xEE            # behind every source row
GUARD = 4096

# ------------------------------------------------------------------------------------------------------------- frame_geometry, restated
# width_bound: the float comparison (float)w / imw < (float)h / imh.  sized: both resized sides >= 2.  The three float clauses, each on its
# own and WITHOUT its guard: row_last = (int)((new_h - 1) h_scale) > imh - 1, row_next = (int)((new_h - 2) h_scale) + 1 > imh - 1,
# col_next = (int)((new_w - 2) w_scale) + 1 > imw - 1.  row_next counts only when imh > 1, col_next only when imw > 1 (the kernels never read
# row iy + 1 of a one-row frame or column ix + 1 of a one-column frame).  All fields are arrays when the arguments are.
Geo = namedtuple("Geo", "width_bound new_w new_h ox oy w_scale h_scale sized row_last row_next col_next accepted")


def geometry(imw, imh, w, h, guarded=True):
    """frame_geometry(imw, imh, w, h): int arithmetic in int32's range (imh * w <= 2^30), the comparison, both scales and the clauses in float32.
    guarded=False: the rule before the imh > 1 / imw > 1 guards."""
    imw, imh, w, h = np.broadcast_arrays(*(np.asarray(a, np.int64) for a in (imw, imh, w, h)))
    assert (imw >= 1).all() and (imh >= 1).all() and (imw * h < 2 ** 31).all() and (imh * w < 2 ** 31).all()
    wb = w.astype(f32) / imw.astype(f32) < h.astype(f32) / imh.astype(f32)
    new_w = np.where(wb, w, (imw * h) // imh)
    new_h = np.where(wb, (imh * w) // imw, h)
    sized = (new_w >= 2) & (new_h >= 2)
    dw, dh = np.where(sized, new_w - 1, 1).astype(f32), np.where(sized, new_h - 1, 1).astype(f32)  # unsized: never divided in C either
    ws, hs = (imw - 1).astype(f32) / dw, (imh - 1).astype(f32) / dh
    assert ws.dtype == f32 and hs.dtype == f32
    row_last = ((new_h - 1).astype(f32) * hs).astype(np.int64) > imh - 1
    row_next = ((new_h - 2).astype(f32) * hs).astype(np.int64) + 1 > imh - 1
    col_next = ((new_w - 2).astype(f32) * ws).astype(np.int64) + 1 > imw - 1
    bad = row_last | (row_next & ((imh > 1) | (not guarded))) | (col_next & ((imw > 1) | (not guarded)))
    return Geo(wb, new_w, new_h, (w - new_w) // 2, (h - new_h) // 2, ws, hs, sized, row_last & sized, row_next & sized, col_next & sized,
               sized & ~bad)


def geometry1(imw, imh, w, h, guarded=True):
    """the same for one (source, network) pair, as Python scalars"""
    return Geo(*(v.item() if v.dtype != f32 else f32(v) for v in geometry(imw, imh, w, h, guarded)))


Taps = namedtuple("Taps", "ix dx two_x iy dy two_y")


def taps(imw, imh, g):
    """letterbox_px3: per column xx of the resized image (ix, dx, whether column ix + 1 is read), per row r (iy, dy, whether row iy + 1 is)"""
    xx, r = np.arange(g.new_w), np.arange(g.new_h)
    last_x = (xx == g.new_w - 1) | (imw == 1)
    sx = xx.astype(f32) * f32(g.w_scale)
    ix = np.where(last_x, imw - 1, sx.astype(np.int64))
    dx = np.where(last_x, f32(0), sx - ix.astype(f32)).astype(f32)
    last_y = (r == g.new_h - 1) | (imh == 1)
    sy = r.astype(f32) * f32(g.h_scale)
    iy = sy.astype(np.int64)
    dy = (sy - iy.astype(f32)).astype(f32)
    return Taps(ix, dx, ~last_x, iy, dy, ~last_y)


def letterbox_restated(planes, w, h):
    """the floats of letterbox_px3 for float32 planes [c][imh][imw]: each product and sum rounded on its own, 0.5 outside the resized image"""
    planes = np.ascontiguousarray(planes, f32)
    c, imh, imw = planes.shape
    g = geometry1(imw, imh, w, h)
    assert g.accepted
    t = taps(imw, imh, g)
    ix1, iy1 = np.where(t.two_x, t.ix + 1, t.ix), np.where(t.two_y, t.iy + 1, t.iy)  # the taps not read are replaced, never out of range
    one = f32(1)

    def row(iy):
        a, b = planes[:, iy[:, None], t.ix[None, :]], planes[:, iy[:, None], ix1[None, :]]
        return np.where(t.two_x[None, None, :], (one - t.dx) * a + t.dx * b, a).astype(f32)
    val = (one - t.dy)[None, :, None] * row(t.iy)
    val = np.where(t.two_y[None, :, None], val + t.dy[None, :, None] * row(iy1), val).astype(f32)
    out = np.full((c, h, w), f32(.5), f32)
    out[:, g.oy:g.oy + g.new_h, g.ox:g.ox + g.new_w] = val
    return out


# ---------------------------------------------------------------------------------------------------------------- frames_check, restated
DEGENERATE = "degenerate aspect (resized side < 2)"
BAD_BATCH = "null table / need 1 <= B <= 65535"
BAD_NET = "need 2 <= w, h <= 32768 for the network input"
BAD_FRAME = "need 1 <= w, h <= 32768 for every frame"


def frames_check(B, w, h, sizes, guarded=True):
    """the conditions every kind shares, in their order: None, or the refusal without its "<kind>: " prefix.  sizes: (imw, imh) per frame"""
    if B <= 0 or B > B_MAX:
        return BAD_BATCH
    if w < 2 or h < 2 or w > SIDE_MAX or h > SIDE_MAX:
        return BAD_NET
    for imw, imh in sizes:
        if imw < 1 or imh < 1 or imw > SIDE_MAX or imh > SIDE_MAX:
            return BAD_FRAME
        if not geometry1(imw, imh, w, h, guarded).accepted:
            return DEGENERATE
    return None


# ------------------------------------------------------------------------------------------------------------- the two launch sizings
def minmax_grid_x(B, w, h):
    want = (h * w + 255) // 256
    cap = 2048 // B if 2048 // B > 0 else 1
    return min(want, cap)


def quantize_grid_x(w, h):
    return (h * ((w + 3) // 4) + 255) // 256


def minmax_trips(B, w, h):
    """iterations of the grid-stride loop of the busiest thread"""
    per_trip = minmax_grid_x(B, w, h) * 256
    return (h * w + per_trip - 1) // per_trip


def store_paths(B, w, h, out_off):
    """letterbox_quantize_body's store decision over every (slot, plane, row, thread): how many take the 4-byte store ("wide"), how many store
    four single bytes because the position is not 4-byte aligned ("bytes"), how many serve a row's tail of 1..3 pixels ("tail")"""
    b, k, y, q = np.ogrid[:B, :3, :h, :(w + 3) // 4]
    o = out_off + ((b * 3 + k) * h + y) * w + 4 * q
    full = 4 * q + 3 < w + 0 * o
    wide = full & (o % 4 == 0)
    return {"wide": int(wide.sum()), "bytes": int((full & ~wide).sum()), "tail": int((~full).sum())}


# ------------------------------------------------------------------------------------------------------------------------------- cases
# One table for the u8 kernels and the float kernel.  B slots hold frames of the case's size, slot b the frame of seed b % FRAMES_DISTINCT (the
# large batches share three device frames).  out_off: bytes between an aligned address and the output.  pair: the (scale, zero point) every slot
# is quantised with; None: the oracle's own pair of each slot's letterboxed image.  data: "rand" | "ramp" (every byte value in every plane) |
# "zero".
Case = namedtuple("Case", "name imw imh w h B out_off pair data", defaults=(1, 0, None, "rand"))
FRAMES_DISTINCT = 3
V1 = f32(1) / f32(255)   # the float of byte 1


def _geo_cases():
    c = [
        # the branch taken
        Case("width_bound_down", 40, 25, 16, 12),      # 16 x 10, a one-pixel bar above and below, scale 2.6
        Case("height_bound_odd_bars", 12, 20, 12, 12),  # 7 x 12, bars of 2 and 3
        Case("equal_aspects_up", 6, 4, 12, 8),         # w * imh == h * imw: the else branch, no bars
        Case("equal_aspects_down", 39, 27, 13, 9),
        Case("identity", 12, 12, 12, 12),
        Case("identity_odd", 13, 11, 13, 11),
        Case("identity_with_far_bar", 12, 11, 12, 12),  # new == im, h - new_h == 1: no bar above, one row below
        Case("identity_bars_both_1", 10, 12, 12, 12),   # w - new_w == 2: a one-pixel bar on either side
        Case("bars_1_and_2", 9, 13, 12, 13),            # w - new_w == 3
        # resized side 2
        Case("new_w_2_short_row", 3, 14, 12, 12),
        Case("new_h_2", 14, 3, 12, 12),
        Case("new_2x2", 5, 5, 2, 2),
        Case("new_w_2_wide_net", 5, 9, 17, 4),
        # the last row
        Case("short_row_4x14", 4, 14, 12, 12),
        Case("short_row_5x27", 5, 27, 12, 12),
        Case("short_row_7x27", 7, 27, 12, 12),
        Case("exact_row_down", 53, 37, 12, 12),
        # scale
        Case("upscale_2x2", 2, 2, 12, 12),
        Case("upscale_3x2", 3, 2, 13, 11),
        Case("upscale_tall", 5, 7, 12, 31),
        Case("downscale_5", 61, 47, 12, 12),
        # one-pixel sources
        Case("1x5", 1, 5, 12, 12),                      # 2 x 12
        Case("5x1", 5, 1, 12, 12),                      # 12 x 2
        Case("1x7_into_16", 1, 7, 16, 16),
        Case("7x1_into_16", 7, 1, 16, 16),
        Case("1x2", 1, 2, 13, 11),
        Case("2x1", 2, 1, 13, 11),
        Case("1x1", 1, 1, 12, 12),
        Case("1x1_into_2x2", 1, 1, 2, 2),
        Case("1x1_into_13x4", 1, 1, 13, 4),
        # side limits
        Case("source_w_32768", 32768, 158, 416, 416),   # new_h == 2
        Case("source_h_32768", 158, 32768, 416, 416),
        Case("net_w_32768", 5, 3, 32768, 2),
        Case("net_h_32768", 3, 5, 2, 32768),
    ]
    return c


def _store_cases():
    c = [Case(f"store_w{w}_h{h}_out+{o}", 2 * w, 2 * h, w, h, B=2, out_off=o) for w in range(2, 10) for h in (2, 3) for o in range(4)]
    # h * ((w + 3) / 4) threads: one below, on and one above a workgroup
    c += [Case("threads_255", 10, 85, 10, 85, B=2), Case("threads_256", 8, 128, 8, 128, B=2), Case("threads_257", 4, 257, 4, 257, B=2),
          Case("threads_257_out+1", 3, 257, 3, 257, B=2, out_off=1)]
    return c


def _minmax_cases():
    return [Case("pixels_255", 15, 17, 15, 17), Case("pixels_256", 16, 16, 16, 16),
            Case("pixels_258", 6, 2, 129, 2),           # 257 is prime and both sides are >= 2: the nearest count above a workgroup
            Case("second_trip", 5, 3, 1024, 513),        # 525 312 pixels > 2048 * 256
            Case("B_3_slots", 3, 3, 2, 2, B=3), Case("B_2048", 3, 3, 2, 2, B=2048), Case("B_2049", 3, 3, 2, 2, B=2049),
            Case("B_65535", 2, 2, 2, 2, B=B_MAX)]


def _quant_cases():
    two = f32(2) * V1
    pairs = [("tie", two, 0), ("tie_scale_below", np.nextafter(two, f32(0)), 0), ("tie_scale_above", np.nextafter(two, f32(1)), 0),
             ("tie_zp255", two, 255), ("tie3", f32(2) * f32(f32(3) / f32(255)), 7),
             ("unit_zp0", V1, 0),                       # q = byte: 255 is reached and not clamped
             ("unit_zp1", V1, 1),                       # q = byte + 1: 256 clamps, 255 does not
             ("unit_zp255", V1, 255)]
    c = [Case("quant_" + n, 16, 16, 16, 16, B=2, pair=(s, z), data="ramp") for n, s, z in pairs]
    c.append(Case("quant_zero_frame", 12, 12, 12, 12, B=2, pair=(V1, 23), data="zero"))  # max stays +0.0, min -0.0
    return c


GEO_CASES, STORE_CASES, MINMAX_CASES, QUANT_CASES = _geo_cases(), _store_cases(), _minmax_cases(), _quant_cases()
CASES = GEO_CASES + STORE_CASES + MINMAX_CASES + QUANT_CASES
ONE_PIXEL = [c.name for c in GEO_CASES if c.imw == 1 or c.imh == 1]  # refused before the imw > 1 / imh > 1 guards

# Refused: (name, B, w, h, [(imw, imh)], message).  Frames in front of the bad one are good ones.
REFUSED = (
    ("resized_w_1", 2, 12, 12, [(5, 7), (1, 7)], DEGENERATE), ("resized_h_1", 2, 12, 12, [(5, 7), (7, 1)], DEGENERATE),
    ("resized_h_1_wide", 1, 32, 32, [(40, 2)], DEGENERATE), ("resized_w_0", 1, 16, 16, [(1, 20)], DEGENERATE),
    ("resized_h_0", 2, 16, 16, [(5, 7), (20, 1)], DEGENERATE), ("resized_w_1_2x13", 1, 12, 12, [(2, 13)], DEGENERATE),
    ("source_w_32769", 2, 416, 416, [(5, 7), (32769, 158)], BAD_FRAME), ("source_h_32769", 1, 416, 416, [(158, 32769)], BAD_FRAME),
    ("source_w_0", 1, 12, 12, [(0, 5)], BAD_FRAME), ("source_h_0", 1, 12, 12, [(5, 0)], BAD_FRAME),
    ("net_w_32769", 1, 32769, 2, [(5, 3)], BAD_NET), ("net_h_32769", 1, 2, 32769, [(3, 5)], BAD_NET),
    ("net_w_1", 1, 1, 12, [(5, 7)], BAD_NET), ("net_h_1", 1, 12, 1, [(5, 7)], BAD_NET),
    ("B_65536", 65536, 2, 2, [(2, 2)], BAD_BATCH), ("B_0", 0, 2, 2, [(2, 2)], BAD_BATCH),
)


def _g(c):
    return geometry1(c.imw, c.imh, c.w, c.h)


def _last_row(c):
    g = _g(c)
    t = taps(c.imw, c.imh, g)
    return int(t.iy[-1]), float(t.dy[-1])


def _bars(c):
    """the widths of the four bars: left, right, top, bottom"""
    g = _g(c)
    return g.ox, c.w - g.new_w - g.ox, g.oy, c.h - g.new_h - g.oy


GEO_CLAUSES = {
    "geo.width_bound": lambda c: _g(c).width_bound,
    "geo.height_bound": lambda c: not _g(c).width_bound and c.w * c.imh != c.h * c.imw,
    "geo.equal_aspects": lambda c: c.w * c.imh == c.h * c.imw,       # the else branch
    "geo.new_w_2": lambda c: _g(c).new_w == 2, "geo.new_h_2": lambda c: _g(c).new_h == 2,
    "geo.bars_none": lambda c: _bars(c) == (0, 0, 0, 0),
    "geo.bars_left_right": lambda c: _g(c).new_w < c.w, "geo.bars_top_bottom": lambda c: _g(c).new_h < c.h,
    "geo.far_bar_one_wider": lambda c: (c.w - _g(c).new_w) % 2 == 1 or (c.h - _g(c).new_h) % 2 == 1,
    "geo.bars_equal": lambda c: max(_bars(c)) > 0 and (c.w - _g(c).new_w) % 2 == 0 and (c.h - _g(c).new_h) % 2 == 0,
    "geo.bar_one_pixel": lambda c: 1 in _bars(c),
    "geo.near_bar_0_far_bar_1": lambda c: _bars(c)[:2] == (0, 1) or _bars(c)[2:] == (0, 1),
    "geo.identity": lambda c: (_g(c).new_w, _g(c).new_h) == (c.imw, c.imh),   # both scales exactly 1, every dx and dy exactly 0
    "geo.upscale": lambda c: 0 < _g(c).w_scale < 1 or 0 < _g(c).h_scale < 1,
    "geo.downscale_gt_2": lambda c: _g(c).w_scale > 2 or _g(c).h_scale > 2,
    "geo.last_row_exact": lambda c: _last_row(c) == (c.imh - 1, 0.0),
    "geo.last_row_short": lambda c: c.imh > 1 and _last_row(c)[0] == c.imh - 2,
    "geo.imw_1": lambda c: c.imw == 1, "geo.imh_1": lambda c: c.imh == 1, "geo.1x1": lambda c: (c.imw, c.imh) == (1, 1),
    "geo.source_side_32768": lambda c: max(c.imw, c.imh) == SIDE_MAX, "geo.net_side_32768": lambda c: max(c.w, c.h) == SIDE_MAX,
    "geo.net_side_2": lambda c: min(c.w, c.h) == 2,
}
_threads = lambda c: c.h * ((c.w + 3) // 4)  # noqa: E731
LAUNCH_CLAUSES = dict(
    [(f"store.w_{w}", (lambda w: lambda c: c.w == w)(w)) for w in range(2, 10)]
    + [(f"store.out+{o}", (lambda o: lambda c: c.out_off == o)(o)) for o in range(4)]
    + [(f"store.threads_{n}", (lambda n: lambda c: _threads(c) == n)(n)) for n in (255, 256, 257)]
    + [(f"mm.pixels_{n}", (lambda n: lambda c: c.h * c.w == n)(n)) for n in (255, 256, 258)]
    + [(f"mm.B_{n}", (lambda n: lambda c: c.B == n)(n)) for n in (1, 2048, 2049, B_MAX)])
LAUNCH_CLAUSES.update({
    "store.h_odd": lambda c: c.h % 2 == 1,
    "store.wide": lambda c: store_paths(min(c.B, 2), c.w, c.h, c.out_off)["wide"] > 0,
    "store.bytes": lambda c: store_paths(min(c.B, 2), c.w, c.h, c.out_off)["bytes"] > 0,
    "store.tail": lambda c: c.w % 4 != 0,
    "store.wide_and_bytes_in_one_launch": lambda c: min(store_paths(min(c.B, 2), c.w, c.h, c.out_off)[k] for k in ("wide", "bytes")) > 0,
    "store.blocks>1": lambda c: quantize_grid_x(c.w, c.h) > 1,
    "mm.blocks>1": lambda c: minmax_grid_x(c.B, c.w, c.h) > 1,
    "mm.cap_2048/B_binds": lambda c: minmax_grid_x(c.B, c.w, c.h) < (c.h * c.w + 255) // 256,
    "mm.cap_floors_to_0": lambda c: 2048 // c.B == 0,
    "mm.second_trip": lambda c: minmax_trips(c.B, c.w, c.h) > 1,
})


def quant_edges(scale, zp):
    """over the 256 floats byte / 255 (what an identity frame holds): how many quotients sit exactly on k + 0.5, within two float32 steps below
    and above such a point, and how many results are 254, 255 (the largest unclamped) and 256 (clamped by one) before the clamp"""
    v = np.arange(256, dtype=f32) / f32(255)
    q = v / f32(scale)
    assert q.dtype == f32
    half = np.floor(q) + f32(.5)
    step = np.spacing(half)
    d = q.astype(np.float64)
    r = np.copysign(np.floor(np.abs(d) + 0.5), d) + zp
    return {"tie": int((q == half).sum()), "below": int(((q < half) & (half - q <= 2 * step)).sum()),
            "above": int(((q > half) & (q - half <= 2 * step)).sum()),
            "254": int((r == 254).sum()), "255": int((r == 255).sum()), "256": int((r == 256).sum()), "far": int((r > 256).sum())}


def _qe(c):
    return quant_edges(*c.pair) if c.pair else dict.fromkeys(("tie", "below", "above", "254", "255", "256", "far"), 0)


QUANT_CLAUSES = {
    "q.tie": lambda c: _qe(c)["tie"] > 0, "q.step_below_tie": lambda c: _qe(c)["below"] > 0, "q.step_above_tie": lambda c: _qe(c)["above"] > 0,
    "q.clamp_hit_by_one": lambda c: _qe(c)["256"] > 0, "q.clamp_missed_by_one": lambda c: _qe(c)["255"] > 0 and _qe(c)["256"] == 0,
    "q.clamp_far": lambda c: _qe(c)["far"] > 0,
    "q.zp_0": lambda c: c.pair is not None and c.pair[1] == 0, "q.zp_255": lambda c: c.pair is not None and c.pair[1] == 255,
    "q.zero_frame": lambda c: c.data == "zero", "q.every_byte_value": lambda c: c.data == "ramp",
}

# Listed, not reached: (name, why)
UNREACHED = (
    ("byte_offsets_above_2^31", "needs iy * pitch beyond 2 GiB, a frame no test can hold; every such product in frames.hip (rows of every source, the "
     "output position) carries a (size_t) cast on its first factor: read, not run"),
    ("float_and_exact_aspects_disagree", "the float comparison and w * imh < h * imw differ only for sources of about 5e8 pixels (smallest found: "
     "23403 x 23233 into 413 x 410, where new_w is w either way); the CPU file states the invariants there"),
    ("mm.pixels_257", "h * w == 257 needs a network side of 1: 257 is prime; 258 = 129 x 2 stands in"),
    ("clause.row_last", "(int)((new_h - 1) * h_scale) > imh - 1: fired by no accepted-size source of the sweep"),
    ("clause.row_next", "(int)((new_h - 2) * h_scale) + 1 > imh - 1 with imh > 1: fired by none; without the guard exactly by imh == 1"),
    ("clause.col_next", "(int)((new_w - 2) * w_scale) + 1 > imw - 1 with imw > 1: fired by none; without the guard exactly by imw == 1"),
)
DEAD_CLAUSES = ("clause.row_last", "clause.row_next", "clause.col_next")
DISAGREEMENT = (23403, 23233, 413, 410)  # (imw, imh, w, h): float comparison false, exact comparison true


# ------------------------------------------------------------------------------------------- where geometry meets a source's own addressing
# (imw, imh, w, h) for the five other sources: each is run by every layout of every kind that allows the size (a Bayer pattern needs 2 x 2)
Size = namedtuple("Size", "imw imh w h")
SOURCE_SIZES = (Size(13, 9, 12, 12), Size(9, 5, 12, 12), Size(10, 5, 12, 12), Size(11, 5, 12, 12), Size(7, 5, 12, 12), Size(3, 2, 13, 11),
                Size(5, 7, 12, 31), Size(3, 14, 12, 12), Size(14, 3, 12, 12), Size(5, 27, 12, 12), Size(4, 14, 12, 12), Size(2, 2, 12, 12),
                Size(61, 47, 12, 12), Size(9, 13, 9, 13),
                Size(1, 5, 12, 12), Size(5, 1, 12, 12), Size(1, 1, 12, 12), Size(1, 2, 13, 11), Size(2, 1, 13, 11))


def _t(s):
    return taps(s.imw, s.imh, _g(s))


SOURCE_CLAUSES = {
    # the last column and row at odd w and h: the chroma sample at ((w - 1) >> 1, (h - 1) >> 1) serves one pixel, the last 4:2:2 macropixel is half used
    "src.odd_w_and_h": lambda s: s.imw % 2 == 1 and s.imh % 2 == 1 and s.imw > 1 and s.imh > 1,
    "src.last_mipi10_group_of_1": lambda s: s.imw % 4 == 1 and s.imw > 1, "src.last_mipi10_group_of_2": lambda s: s.imw % 4 == 2 and s.imw > 2,
    "src.last_mipi10_group_of_3": lambda s: s.imw % 4 == 3, "src.last_mipi12_group_of_1": lambda s: s.imw % 2 == 1 and s.imw > 1,
    # Bayer reflection: a tap in the last column / row whose window reaches w, h (reflected to w - 2, h - 2), and one at column / row 0
    "src.taps_in_last_column_and_row": lambda s: s.imw > 1 and s.imh > 1 and _t(s).ix.max() == s.imw - 1 and (_t(s).iy + _t(s).two_y).max() == s.imh - 1,
    "src.new_side_2": lambda s: min(_g(s).new_w, _g(s).new_h) == 2,
    "src.short_last_row": lambda s: s.imh > 1 and _t(s).iy[-1] == s.imh - 2,
    # an upscale where both taps fall into one chroma sample / macropixel (even ix, ix + 1 read) and one where they straddle two (odd ix)
    "src.two_taps_in_one_chroma_sample": lambda s: bool((_t(s).two_x & (_t(s).ix % 2 == 0)).any()) and _g(s).w_scale < 1,
    "src.two_taps_across_chroma_samples": lambda s: bool((_t(s).two_x & (_t(s).ix % 2 == 1)).any()),
    "src.two_rows_in_one_chroma_row": lambda s: bool((_t(s).two_y & (_t(s).iy % 2 == 0)).any()) and _g(s).h_scale < 1,
    "src.downscale_gt_2": lambda s: _g(s).w_scale > 2 and _g(s).h_scale > 2,
    "src.identity": lambda s: (s.imw, s.imh) == (s.w, s.h),
    "src.one_column": lambda s: s.imw == 1, "src.one_row": lambda s: s.imh == 1, "src.one_pixel": lambda s: s.imw == 1 and s.imh == 1,
}


# ---------------------------------------------------------------------------------------------------------------- frames and expectations
def _seed(name, slot):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(name)) * 8 + slot


def frame(c, slot):
    """uint8 [imh][imw][3]: the frame of distinct slot `slot` (< FRAMES_DISTINCT)"""
    if c.data == "zero":
        return np.zeros((c.imh, c.imw, 3), np.uint8)
    rng = np.random.default_rng(_seed(c.name, slot))
    if c.data == "ramp":
        assert c.imw * c.imh == 256
        return np.stack([rng.permutation(256).astype(np.uint8).reshape(c.imh, c.imw) for _ in range(3)], axis=-1)
    return rng.integers(0, 256, (c.imh, c.imw, 3), dtype=np.uint8)


def planes(rgb):
    """load_image_color's planar floats of an RGB frame (ref: src/image.c:1386)"""
    return np.ascontiguousarray(rgb.transpose(2, 0, 1)).astype(f32) / f32(255)


Want = namedtuple("Want", "lb mm scale zp q")


def expected_rgb(rgb, w, h, pair=None):
    """what both passes must give for one RGB frame: the floats, the min / max words, the pair used, the bytes [3][h][w]"""
    lb = oracle.letterbox_image(planes(rgb), h, w)
    if pair is None:
        _, s, z = oracle.quantize_image(lb)
        pair = (f32(s), int(z))
    return Want(lb, minmax_ref(lb), f32(pair[0]), int(pair[1]), quantize_ref(lb, pair[0], pair[1]))


@functools.lru_cache(maxsize=None)
def expected(name):
    """[Want] of the case's distinct frames, computed once and shared by the tests; callers leave it unchanged"""
    c = BY_NAME[name]
    return [expected_rgb(frame(c, s), c.w, c.h, c.pair) for s in range(min(c.B, FRAMES_DISTINCT))]


BY_NAME = {c.name: c for c in CASES}
