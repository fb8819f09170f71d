"""The kernels between the convs (csrc/glue.hip behind the C-ABI entry points of csrc/shim.hip) at their edges: the case tables, one label per
clause, and plain numpy references.

Shared by tests/test_gpu_glue_edges.py (runs every case on the device through one helper that holds the invariant "no pad cell, no byte of a
neighbouring channel window, no byte outside the tensor is written") and tests/test_glue_edges_cpu.py (every reference against tests/oracle.py,
every label reached on both sides, every shortcut parameter set on its aimed edge by count, the tables' sizes).  No device, no ctypes here.

References work on plain [B][C][H][W] arrays (int64 for integers, np.float32 step by step where a kernel rounds to float) and know nothing
about cells, groups or threads.  The device layout is restated once, in `Cells`, from the header's formula.

What a call may write (the ownership rule of the group kernels, shim.hip: "bytes of a cell this layer owns"): maxpool, upsample, shortcut and the
aligned route path store whole 16-byte groups, so a tensor (or window) of C channels at byte offset `off` of its cells owns bytes
[off, off + up16(C)).  Bytes off + C .. off + up16(C) are pad channels; the tables only place a ragged C where those bytes are pad bytes
C..cs of the wider tensor's own cells (checked by the CPU file), the header documents them as writable, and every case states what they become:
the same operation applied to the inputs' bytes at the same positions.  Everything else must come back as the snapshot."""
from collections import namedtuple

import numpy as np

EINVAL = -22
SENTINEL = 0xA5   # the bytes around and between the tensors; differs from zp and zp ^ 0x80 for every zero point a case fills with
GUARD = 4096      # sentinel bytes in front of and behind every output tensor
ZERO_POINTS = (0, 1, 23, 77, 128, 255)  # the zero points the cases may fill with (SENTINEL is none of them, plain or biased)
MAX_TENSOR_BYTES = 8 << 20


def cdiv(a, b):
    """C's truncating division"""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def up16(c):
    return (c + 15) // 16 * 16


# --------------------------------------------------------------------------------------------------------- the device layout, restated once
class Cells:
    """include/mi355_yolo_int8.h: cell(b, y, x) = lead + (b * (H + 1) + (y + 1)) * (W + 1) + x, cells of cs bytes, bytes stored ^ 0x80
    (plain bytes in the cs == 4 image)."""

    def __init__(self, B, H, W, cs, lead=2, tail=None):
        self.B, self.H, self.W, self.cs, self.lead = B, H, W, cs, lead
        self.tail = W + 3 if tail is None else tail
        self.ncells = lead + B * (H + 1) * (W + 1) + self.tail
        self.nbytes = self.ncells * cs
        self.bias = 0 if cs == 4 else 0x80

    def interior(self):
        b, y, x = np.ogrid[:self.B, :self.H, :self.W]
        return (self.lead + (b * (self.H + 1) + (y + 1)) * (self.W + 1) + x).ravel()

    def put(self, raw, x, off=0):
        """x: plain [B][n][H][W] bytes into bytes off .. off + n of every interior cell of raw (flat uint8 of nbytes)"""
        assert x.shape[0] == self.B and x.shape[2:] == (self.H, self.W) and off + x.shape[1] <= self.cs
        body = raw.reshape(self.ncells, self.cs)
        body[self.interior(), off:off + x.shape[1]] = x.transpose(0, 2, 3, 1).reshape(-1, x.shape[1]).astype(np.uint8) ^ self.bias

    def get(self, raw, off, n):
        body = raw.reshape(self.ncells, self.cs)
        return (body[self.interior(), off:off + n] ^ self.bias).reshape(self.B, self.H, self.W, n).transpose(0, 3, 1, 2)

    def kinds(self, off, n):
        """per byte of the buffer: 0 interior byte of channels [off, off + n), 1 other byte of an interior cell, 2 byte of a pad cell"""
        k = np.full((self.ncells, self.cs), 2, np.uint8)
        k[self.interior()] = 1
        k[self.interior(), off:off + n] = 0
        return k.ravel()


# an operand: cells of cs bytes with `lead` pad cells in front; the tensor the call sees is the window of C channels at byte `off` of a tensor of
# `wide` channels (plain tensor: off 0, wide == C)
T = namedtuple("T", "cs lead off wide")


def plain(C, lead=2):
    return T(4 if C == 3 else up16(C), lead, 0, C)


def is_window(t, C):
    return t.off != 0 or t.wide != C


def owned_ok(t, C):
    """the group kernels' stores [off, off + up16(C)) stay in the cell, and what lies behind channel C are pad bytes of the wide tensor's own"""
    end = t.off + up16(C)
    return t.off % 16 == 0 and t.cs % 16 == 0 and end <= t.cs and t.off + C <= t.wide and (C % 16 == 0 or t.off + C == t.wide)


def readable_ok(t, C):
    """the group kernels' loads [off, off + up16(C)) stay in the cell"""
    return t.off % 16 == 0 and t.cs % 16 == 0 and t.off + up16(C) <= t.cs


def operand_bytes(name, B, H, W, t, lo=1):
    """every byte of every interior cell of one operand, plain, [B][cs][H][W], drawn from lo..255 and seeded by the name"""
    rng = np.random.default_rng(sum(map(ord, name)) + 7919 * t.cs + t.off)
    return rng.integers(lo, 256, (B, t.cs, H, W), dtype=np.uint8)


class Reach:
    """label -> the sides (True / False) a table's cases reach"""

    def __init__(self, clauses, cases):
        self.clauses, self.hits = clauses, {k: set() for k in clauses}
        for cs in cases:
            for k, f in clauses.items():
                self.hits[k].add(bool(f(cs)))

    def missing(self):
        return [(k, side) for k, h in self.hits.items() for side in (True, False) if side not in h]


# ------------------------------------------------------------------------------------------------------------------------------- max pool
Pool = namedtuple("Pool", "name B C H W size stride pad x y data")
PLANT = (0x00, 0x7f, 0x80, 0xff)


def pool_out(n, size, stride, pad):
    """(n + pad - size) / stride + 1 the C way (ref: src/maxpool_layer.c:31-32): truncation, not floor"""
    return cdiv(n + pad - size, stride) + 1


def maxpool_ref(x, size, stride, pad):
    B, Cc, H, W = x.shape
    OH, OW = pool_out(H, size, stride, pad), pool_out(W, size, stride, pad)
    first = -(pad // 2)  # C's -pad / 2 for pad >= 0
    xi = x.astype(np.int64)
    out = np.zeros((B, Cc, OH, OW), np.int64)  # `max` starts at 0 and a tap outside the image is 0
    for oy in range(OH):
        for ox in range(OW):
            for n in range(size):
                for m in range(size):
                    iy, ix = first + oy * stride + n, first + ox * stride + m
                    if 0 <= iy < H and 0 <= ix < W:
                        out[:, :, oy, ox] = np.maximum(out[:, :, oy, ox], xi[:, :, iy, ix])
    return out.astype(np.uint8)


def pool_has_outside_window(cs):
    first = -(cs.pad // 2)
    for n, o in ((cs.H, pool_out(cs.H, cs.size, cs.stride, cs.pad)), (cs.W, pool_out(cs.W, cs.size, cs.stride, cs.pad))):
        for i in range(o):
            lo = first + i * cs.stride
            if lo + cs.size <= 0 or lo >= n:
                return True
    return False


def pool_threads(cs):
    return cs.B * pool_out(cs.H, cs.size, cs.stride, cs.pad) * pool_out(cs.W, cs.size, cs.stride, cs.pad) * (up16(cs.C) // 16)


POOL_CLAUSES = {
    "pool.size_1": lambda c: c.size == 1, "pool.size_2": lambda c: c.size == 2, "pool.size_3": lambda c: c.size == 3, "pool.size_5": lambda c: c.size == 5,
    "pool.stride_1": lambda c: c.stride == 1, "pool.stride_2": lambda c: c.stride == 2, "pool.stride_3": lambda c: c.stride == 3,
    "pool.stride_gt_size": lambda c: c.stride > c.size,
    "pool.pad_0": lambda c: c.pad == 0, "pool.pad_1": lambda c: c.pad == 1, "pool.pad_size-1": lambda c: c.pad == c.size - 1,
    "pool.pad_odd": lambda c: c.pad % 2 == 1,                       # -pad / 2 truncates
    "pool.window_all_outside": pool_has_outside_window,           # must store exactly 0: the bytes are drawn from 1..255
    "pool.H+pad<size": lambda c: c.H + c.pad < c.size,              # where C's division and Python's // disagree
    "pool.map_1x1": lambda c: c.H == 1 and c.W == 1,
    "pool.ragged_C": lambda c: c.C % 16 != 0, "pool.groups>1": lambda c: c.C > 16,
    "pool.x_window": lambda c: is_window(c.x, c.C), "pool.y_window": lambda c: is_window(c.y, c.C),
    "pool.cs_and_lead_differ": lambda c: c.x.cs != c.y.cs and c.x.lead != c.y.lead,
    "pool.planted": lambda c: c.data == "planted",
    "pool.threads%256==255": lambda c: pool_threads(c) % 256 == 255, "pool.threads%256==0": lambda c: pool_threads(c) % 256 == 0,
    "pool.threads%256==1": lambda c: pool_threads(c) % 256 == 1 and pool_threads(c) > 256,
}
CHANNELS = (1, 15, 16, 17, 33, 48)


def _pool_cases():
    out = []

    def add(name, C, H, W, size, stride, pad, x=None, y=None, data="rand", B=3):
        out.append(Pool(name, B, C, H, W, size, stride, pad, x or plain(C), y or plain(C), data))

    for size in (1, 2, 3, 5):          # window and padding: every size with every stride and pad, on an odd 7 x 6 map
        for stride in sorted({1, 2, 3, size + 1}):
            for pad in sorted({0, 1, size - 1, 2 * size + 1}):  # 2 * size + 1: odd, and the first window lies wholly outside the image
                H, W = 7, 6
                if pool_out(H, size, stride, pad) < 1 or pool_out(W, size, stride, pad) < 1:
                    continue
                add(f"k{size}s{stride}p{pad}", 16, H, W, size, stride, pad)
    for C in CHANNELS:                 # channels: one ragged group, one full, ragged second and third groups
        add(f"c{C}_k2s2p1", C, 5, 7, 2, 2, 1)
        add(f"c{C}_k3s1p2", C, 4, 3, 3, 1, 2)
    for size, stride, pad in ((2, 1, 1), (2, 2, 0), (3, 2, 1), (5, 1, 4), (3, 1, 7)):  # planted bytes: lanes, column W, the next image
        add(f"planted_k{size}s{stride}p{pad}", 16, 6, 5, size, stride, pad, data="planted")
        add(f"planted33_k{size}s{stride}p{pad}", 33, 3, 4, size, stride, pad, data="planted")
    # windows: x a window of a wider tensor; y a 16-aligned window; both, with other cs and lead; a ragged y window in front of the wide tensor's pad
    add("xwin", 16, 5, 7, 2, 2, 1, x=T(64, 2, 16, 64))
    add("xwin_ragged", 17, 5, 7, 3, 2, 1, x=T(64, 2, 16, 40))
    add("ywin", 32, 5, 7, 2, 2, 1, y=T(80, 2, 32, 80))
    add("ywin_first", 16, 5, 7, 2, 1, 1, y=T(48, 2, 0, 48))
    add("ywin_ragged", 17, 6, 6, 3, 2, 1, y=T(80, 3, 16, 33))
    add("xywin", 48, 6, 5, 2, 2, 0, x=T(96, 5, 32, 96), y=T(64, 2, 16, 64))
    add("xywin_ragged", 33, 4, 5, 2, 1, 1, x=T(64, 4, 0, 64), y=T(112, 1, 48, 81))
    # map sizes
    add("H+pad<size", 16, 2, 2, 5, 3, 1)          # (2 + 1 - 5) / 3 + 1 = 1 the C way, 0 with a floor
    add("H+pad<size_c33", 33, 1, 3, 4, 3, 1)
    add("map1x1", 16, 1, 1, 2, 2, 1)
    add("map1x1_k1", 17, 1, 1, 1, 1, 0)
    # thread counts: one below, on and one above a multiple of 256
    add("threads255", 16, 5, 17, 1, 1, 0)           # 3 * 5 * 17
    add("threads256", 16, 8, 8, 1, 1, 0, B=4)
    add("threads512", 32, 8, 8, 2, 1, 1, B=4)
    add("threads257", 16, 1, 257, 1, 1, 0, B=1)
    add("threads511", 16, 7, 73, 2, 1, 1, B=1)      # 7 * 73
    return out


POOL_CASES = _pool_cases()


def pool_inputs(cs):
    """(every byte of x's cells [B][cs][H][W], the logical x [B][C][H][W])"""
    full = operand_bytes(cs.name, cs.B, cs.H, cs.W, cs.x)
    if cs.data == "planted":  # image 1: channel c holds PLANT[c % 4] everywhere, its neighbours are full of 0xff
        full[:] = 0xff
        for c in range(cs.C):
            full[1 % cs.B, cs.x.off + c] = PLANT[c % 4]
    return full, full[:, cs.x.off:cs.x.off + cs.C]


# POOL_REFUSALS: (label, the message mi355_last_error() must hold, what to change on a legal call: C 16, 3 x 6 x 6 -> 3 x 3, size 2, stride 2, pad 0)
POOL_REFUSALS = (
    ("stride 0", "maxpool: need size >= 1, stride >= 1 and pad >= 0", dict(stride=0)),
    ("stride -1", "maxpool: need size >= 1, stride >= 1 and pad >= 0", dict(stride=-1)),
    ("size 0", "maxpool: need size >= 1, stride >= 1 and pad >= 0", dict(size=0)),
    ("size -2", "maxpool: need size >= 1, stride >= 1 and pad >= 0", dict(size=-2)),
    ("pad -1", "maxpool: need size >= 1, stride >= 1 and pad >= 0", dict(pad=-1)),
    ("C mismatch", "maxpool: layout", dict(yC=15)),
    ("B mismatch", "maxpool: layout", dict(yB=2)),
    ("output one row short", "maxpool: output dims", dict(yH=2)),
    ("output one column wide", "maxpool: output dims", dict(yW=4)),
    ("floor-sized output", "maxpool: output dims", dict(size=9, stride=4, yH=0, yW=0)),  # (6 - 9) / 4 + 1 = 1 the C way
    ("x is the 4-byte image", "maxpool: layout", dict(xcs=4)),
    ("y is the 4-byte image", "maxpool: layout", dict(ycs=4)),
)


# ------------------------------------------------------------------------------------------------------------------- upsample and route
Up = namedtuple("Up", "name B C H W stride x y")
Route = namedtuple("Route", "name B H W Cs xs y")   # xs: one T per input; inputs with the same (cs, lead) and disjoint channels share one wide tensor


def upsample_ref(x, stride):
    return np.repeat(np.repeat(x, stride, axis=2), stride, axis=3)


def route_ref(xs):
    return np.concatenate(xs, axis=1)


def route_aligned(Cs):
    """the shim's rule: 16-byte groups when every input but the last has a multiple of 16 channels, else byte by byte"""
    return all(c % 16 == 0 for c in Cs[:-1])


UP_CLAUSES = {
    "up.stride_1": lambda c: c.stride == 1, "up.stride_2": lambda c: c.stride == 2, "up.stride_3": lambda c: c.stride == 3,
    "up.stride_4": lambda c: c.stride == 4, "up.ragged_C": lambda c: c.C % 16 != 0, "up.groups>1": lambda c: c.C > 16,
    "up.x_window": lambda c: is_window(c.x, c.C), "up.y_window": lambda c: is_window(c.y, c.C),
    "up.cs_and_lead_differ": lambda c: c.x.cs != c.y.cs and c.x.lead != c.y.lead,
}
ROUTE_CLAUSES = {
    "route.copy_cells": lambda c: route_aligned(c.Cs), "route.copy_cell_bytes": lambda c: not route_aligned(c.Cs),
    "route.n_1": lambda c: len(c.Cs) == 1, "route.n_2": lambda c: len(c.Cs) == 2, "route.n_4": lambda c: len(c.Cs) == 4,
    "route.n_16": lambda c: len(c.Cs) == 16,
    "route.aligned_ragged_last": lambda c: route_aligned(c.Cs) and c.Cs[-1] % 16 != 0,
    "route.inputs_are_windows": lambda c: any(is_window(t, n) for t, n in zip(c.xs, c.Cs)),
    "route.y_window": lambda c: is_window(c.y, sum(c.Cs)),
}


def _up_cases():
    out = []
    for stride in (1, 2, 3, 4):
        for C in CHANNELS:
            out.append(Up(f"s{stride}c{C}", 3, C, 3, 5, stride, plain(C), plain(C)))
        out.append(Up(f"s{stride}_xwin", 3, 16, 3, 4, stride, T(64, 2, 32, 64), plain(16)))
        out.append(Up(f"s{stride}_ywin", 3, 32, 2, 5, stride, plain(32), T(96, 2, 16, 96)))
        out.append(Up(f"s{stride}_xywin_ragged", 3, 17, 3, 3, stride, T(64, 5, 16, 64), T(80, 3, 32, 49)))
    return out


def _route_cases():
    out = []

    def add(name, Cs, xs=None, y=None, H=3, W=5):
        out.append(Route(name, 3, H, W, tuple(Cs), tuple(xs or [plain(c) if c != 3 else T(16, 2, 0, 3) for c in Cs]), y or plain(sum(Cs))))

    add("n1", [16])
    add("n1_ragged", [17])
    add("n2", [32, 48])
    add("n4", [16, 16, 32, 16])
    add("n16", [16] * 16)
    add("aligned_last17", [16, 17])                       # the last input ends inside a group: its pad bytes land in y's own padding
    add("aligned_last40", [32, 16, 40])
    for c in (1, 15, 17, 24):                             # a non-last input that ends inside a group: every later offset is unaligned
        add(f"bytes_first{c}", [c, 16])
        add(f"bytes_mid{c}", [16, c, 33])
    add("bytes_n4", [1, 15, 17, 24])
    add("bytes_n16", [3] * 16)
    add("xs_windows", [16, 32], xs=[T(64, 2, 0, 64), T(64, 2, 32, 64)])        # two windows of one wide tensor
    add("xs_windows_bytes", [7, 20, 5], xs=[T(48, 3, 5, 48), T(48, 3, 12, 48), T(48, 3, 40, 48)])  # ... off the 16-byte grid: byte path only
    add("y_window", [16, 32], y=T(96, 4, 16, 96))
    add("y_window_ragged_last", [16, 17], y=T(96, 2, 48, 81))
    add("y_window_bytes", [15, 17], xs=[plain(15), T(64, 2, 16, 64)], y=T(64, 3, 9, 64))
    return out


UP_CASES, ROUTE_CASES = _up_cases(), _route_cases()


def route_writes(cs):
    """per input: (first byte of y's cell, bytes stored): whole groups on the aligned path, the input's channels byte by byte otherwise"""
    al, off, w = route_aligned(cs.Cs), cs.y.off, []
    for c in cs.Cs:
        w.append((off, up16(c) if al else c))
        off += c
    return w


# --------------------------------------------------------------------------------------------------------------------------------- shortcut
Sc = namedtuple("Sc", "name Ka Kb za zb zo aim")
K_MAX = (1 << 21) - 1


def shortcut_terms(a, b, s):
    """(t, q): t = Ka (a - za) + Kb (b - zb), q = zo + floor((t + 2^15) / 2^16), both int64 and unclamped"""
    t = np.int64(s.Ka) * (a.astype(np.int64) - s.za) + np.int64(s.Kb) * (b.astype(np.int64) - s.zb)
    return t, s.zo + ((t + 32768) >> 16)  # numpy's >> on int64 is the arithmetic (floor) shift


def shortcut_ref(a, b, s):
    return np.clip(shortcut_terms(a, b, s)[1], 0, 255).astype(np.uint8)


def shortcut_pairs():
    """all 65 536 byte pairs as one 256 x 256 map of 16 channels: channel 0 holds (a, b) = (row, column), channel k a permutation of the rows
    and another of the columns (an odd multiplier and an offset modulo 256), so every lane of the group sees every pair somewhere"""
    i, j = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    a = np.stack([(i * (2 * k + 1) + 17 * k) % 256 for k in range(16)])[None].astype(np.uint8)
    b = np.stack([(j * (2 * ((5 * k) % 16) + 1) + 31 * k) % 256 for k in range(16)])[None].astype(np.uint8)
    return a, b


def shortcut_edge_counts(a, b, s):
    """how many elements sit on each part of the edge a parameter set aims at: every figure must be positive.
    corners: the four pairs of extreme bytes (the largest products of either sign the multipliers see); tie: t mod 2^16 == 0x8000 with t > 0 and
    with t < 0; clamp_lo / clamp_hi: q one step inside, on and outside the clamp; clamp_both: -1 | 0 and 255 | 256; clamp_far: far outside both"""
    t, q = shortcut_terms(a, b, s)
    tie = (t & 0xFFFF) == 0x8000
    return {"corners": tuple(int(((a == u) & (b == v)).sum()) for u in (0, 255) for v in (0, 255)),
            "tie": (int((tie & (t > 0)).sum()), int((tie & (t < 0)).sum())),
            "clamp_lo": tuple(int((q == v).sum()) for v in (-1, 0, 1)), "clamp_hi": tuple(int((q == v).sum()) for v in (254, 255, 256)),
            "clamp_both": tuple(int((q == v).sum()) for v in (-1, 0, 255, 256)),
            "clamp_far": (int((q < -1000).sum()), int((q > 1256).sum()))}[s.aim]


def _sc_sets():
    out, zps = [], (0, 1, 128, 255)
    n = 0
    for Ka in (1, 65536, K_MAX):      # the multiplier limits, crossed, the zero points walking through {0, 1, 128, 255}^3
        for Kb in (1, 65536, K_MAX):
            out.append(Sc(f"K{Ka}x{Kb}", Ka, Kb, zps[n % 4], zps[(n // 4 + n) % 4], zps[(n + 2) % 4], "corners"))
            n += 1
    # the rounding tie: t mod 2^16 == 0x8000 whenever (a - za) is odd (first set) or (a - za) + (b - zb) is odd (second), both signs of t
    out.append(Sc("tie_a", 32768, 65536, 128, 128, 128, "tie"))
    out.append(Sc("tie_ab", 32768, 32768, 1, 255, 128, "tie"))
    out.append(Sc("tie_3", 3 * 32768, 5 * 32768, 128, 0, 0, "tie"))
    # the clamps: q = zo + (a - za) + (b - zb) walks over -1 | 0 | 1 and 254 | 255 | 256
    out.append(Sc("clamp_lo", 65536, 65536, 128, 128, 0, "clamp_lo"))
    out.append(Sc("clamp_hi", 65536, 65536, 128, 128, 255, "clamp_hi"))
    out.append(Sc("clamp_both_zp0", 65536, 65536, 255, 0, 1, "clamp_both"))
    out.append(Sc("clamp_lo_half", 32768, 32768, 128, 128, 127, "clamp_lo"))   # ties next to the clamp: q = 127 + floor((a + b - 255) / 2)
    out.append(Sc("clamp_hi_half", 32768, 32768, 0, 0, 2, "clamp_hi"))         # q = 2 + floor((a + b + 1) / 2)
    out.append(Sc("clamp_far_kmax", K_MAX, K_MAX, 1, 255, 128, "clamp_far"))   # q = 128 + about 32 (a + b - 256): thousands beyond either clamp
    return out


SC_SETS = _sc_sets()
# the second launch: ragged channels, three different cell sizes and leads, b and y windows
ScRagged = namedtuple("ScRagged", "B C H W a b y s")
SC_RAGGED = ScRagged(3, 17, 5, 7, T(32, 2, 0, 17), T(48, 4, 16, 48), T(64, 3, 32, 49), Sc("ragged", 40000, 70000, 3, 200, 100, "corners"))


def shortcut_int32_intermediates(Ka, Kb, za, zb, zo, a, b):
    """every intermediate of the kernel's int arithmetic (shim.hip's k0, common.h's shortcut4_biased), left to right, as Python integers"""
    k0_steps = [32768 + (zo << 16), 32768 + (zo << 16) - Ka * za, 32768 + (zo << 16) - Ka * za - Kb * zb, Ka * za, Kb * zb]
    k0 = k0_steps[2]
    return k0_steps + [Ka * a, Kb * b, Ka * a + Kb * b, Ka * a + Kb * b + k0]


# ------------------------------------------------------------------------------------------------------------ layout converters and fill
Lay = namedtuple("Lay", "name B C H W src_off zp")


def layout_fast_path(cs):
    """nchw_to_phwc_launch's rule for the four-pixel kernel"""
    return cs.C == 3 and cs.W % 4 == 0 and cs.src_off % 4 == 0


LAY_CLAUSES = {
    "lay.four_pixel_kernel": layout_fast_path,
    "lay.C3_W%4": lambda c: c.C == 3 and c.W % 4 == 0,
    "lay.C3_unaligned_source": lambda c: c.C == 3 and c.src_off % 4 != 0,
    "lay.cs_4": lambda c: c.C == 3,
    "lay.ragged_4_group": lambda c: c.C % 4 != 0 and c.C != 3,
    "lay.ragged_16_group": lambda c: c.C % 16 != 0 and c.C != 3,
    "lay.groups>1": lambda c: c.C > 16,
}
LAY_CASES = ([Lay(f"c{C}", 3, C, 3, 5, 0, zp) for C, zp in zip((1, 2, 3, 4, 5, 15, 16, 17), (0, 23, 77, 128, 255, 1, 23, 77))]
             + [Lay(f"c3w{W}", 3, 3, 3, W, 0, 23) for W in (4, 8, 12, 5, 6, 7)]
             + [Lay("c3w8_src+1", 3, 3, 3, 8, 1, 23), Lay("c3w4_src+2", 3, 3, 5, 4, 2, 0), Lay("c3w8h67", 2, 3, 67, 8, 0, 1),  # 2 * 67 * 2 = 268 threads
                Lay("c33_blocks", 3, 33, 5, 7, 0, 128)])                                                                      # 3 * 9 * 35 = 945 threads
# mi355_tensor_to_nchw: (name, B, C, H, W, T)
UNLAY_CASES = (("plain16", 3, 16, 3, 5, plain(16)), ("plain17", 3, 17, 2, 3, plain(17)), ("plain1", 3, 1, 4, 4, plain(1)), ("image3", 3, 3, 3, 5, plain(3)),
               ("window", 3, 16, 3, 5, T(64, 2, 32, 64)), ("window_off_grid", 3, 7, 3, 5, T(48, 4, 21, 48)), ("window_ragged", 2, 33, 5, 3, T(96, 3, 16, 49)))


def nchw_to_cells_ref(x, cs):
    """what mi355_nchw_to_tensor stores in every interior cell: (bytes as they are stored, how many).  The converter writes whole 4-byte
    groups: channels as x ^ 0x80 (plain in the 4-byte image), the pad channels of the last group as uint8 0 (stored 0x80; 0 in the image).
    Bytes behind the last 4-byte group keep what mi355_tensor_fill left there."""
    B, Cc, H, W = x.shape
    n = (Cc + 3) // 4 * 4
    full = np.zeros((B, n, H, W), np.uint8)  # plain 0: stored as 0x80 in 16-byte cells, as 0 in the image
    full[:, :Cc] = x
    return full


# ------------------------------------------------------------------------------------------------------------------------------- dequant
Dq = namedtuple("Dq", "name C c0 nc out_C out_c0 zp scale")
DQ_SCALES = (1.0, 2.0 ** -7, 0.3)
DQ_CLAUSES = {
    "dq.first_channel": lambda c: c.c0 == 0, "dq.last_channel": lambda c: c.c0 + c.nc == c.C, "dq.ragged_C": lambda c: c.C % 16 != 0,
    "dq.out_first_plane": lambda c: c.out_c0 == 0, "dq.out_last_plane": lambda c: c.out_c0 + c.nc == c.out_C,
    "dq.out_middle": lambda c: c.out_c0 > 0 and c.out_c0 + c.nc < c.out_C,
    "dq.zp_0": lambda c: c.zp == 0, "dq.zp_255": lambda c: c.zp == 255,
    "dq.scale_1": lambda c: c.scale == 1.0, "dq.scale_pow2": lambda c: c.scale == 2.0 ** -7, "dq.scale_other": lambda c: c.scale == 0.3,
}
DQ_CASES = (Dq("all", 37, 0, 37, 37, 0, 0, 1.0), Dq("first", 37, 0, 1, 1, 0, 255, 2.0 ** -7), Dq("last", 37, 36, 1, 3, 2, 77, 0.3),
            Dq("middle_of_wider", 37, 5, 20, 24, 2, 255, 0.3), Dq("middle_zp0", 48, 16, 16, 40, 13, 0, 2.0 ** -7), Dq("into_first", 16, 15, 1, 4, 0, 128, 1.0),
            Dq("group_edge", 33, 15, 18, 19, 1, 1, 0.3), Dq("c1", 1, 0, 1, 2, 1, 255, 1.0))
DQ_B, DQ_H, DQ_W = 3, 3, 5
# what to change on the legal call (C 37 in cs 48, c0 5, nc 20, out_C 24, out_c0 2) -> the message
DQ_REFUSALS = (("x null", dict(x=None), "dequant: null / layout"), ("x data null", dict(data=None), "dequant: null / layout"),
               ("out null", dict(out=None), "dequant: null / layout"), ("the 4-byte image", dict(cs=4), "dequant: null / layout"),
               ("c0 < 0", dict(c0=-1), "dequant: channel range"), ("nc == 0", dict(nc=0), "dequant: channel range"),
               ("nc < 0", dict(nc=-3), "dequant: channel range"), ("c0 + nc > C", dict(c0=18), "dequant: channel range"),
               ("out_c0 < 0", dict(out_c0=-1), "dequant: channel range"), ("out_c0 + nc > out_C", dict(out_c0=5), "dequant: channel range"))


def dequant_ref(u, zp, scale):
    """(float)(u - zp) * scale: the int -> float conversion is exact, the product one float32 rounding"""
    return (u.astype(np.int64) - int(zp)).astype(np.float32) * np.float32(scale)


# ----------------------------------------------------------------------------------------------------------------- float input quantiser
# A quotient x / scale outside int32 range (and a NaN input to the quantiser) is outside the contract: C leaves the float -> int conversion
# undefined there, and hosts (x86: INT_MIN) and the device (saturation) differ.  No case asserts on it; quantize_ref refuses such an input.
Q_COUNTS = (1, 2, 3, 4, 5, 255, 256, 257, 1023, 1025, 2048 * 256 + 1)  # the last one makes the min / max grid-stride loop iterate
Q_SRC_OFFSETS = (0, 4)         # bytes: the 16-byte vector load and the scalar path
Q_OUT_OFFSETS = (0, 1, 2, 3)   # bytes: the dword store and the byte stores
Q_PARAMS = ((0.25, 3), (0.0123, 128), (1.0 / 255.0, 0), (0.5, 255))   # (scale, zero point): powers of two make the planted ties exact
Q_KINDS = ("mixed", "positive", "negative", "zero", "negzero", "denormal")
Q_BATCHED = ((1, 5), (2, 5), (3, 5), (1, 7), (2, 7), (3, 7), (2049, 5))   # (B, count_per_image); 2049: the workgroup cap 2048 / B floors to 0
Q_B_REFUSED = 65536


def q_path_labels(count, src_off, out_off):
    """which of image_quantize_kernel's paths a launch takes somewhere (restated from its two conditions)"""
    full, tail = count >= 4, count % 4 != 0
    return {("q.vector_load", full and src_off % 16 == 0), ("q.scalar_load", tail or src_off % 16 != 0),
            ("q.dword_store", full and out_off % 4 == 0), ("q.byte_store", tail or out_off % 4 != 0),
            ("q.blocks>1", count > 1024), ("q.minmax_loop_iterates", count > 2048 * 256)}


Q_LABELS = ("q.vector_load", "q.scalar_load", "q.dword_store", "q.byte_store", "q.blocks>1", "q.minmax_loop_iterates")


def q_launches():
    """(count, source offset, output offset): every small count at every address; the large one at the two ends"""
    out = [(n, s, o) for n in Q_COUNTS[:-1] for s in Q_SRC_OFFSETS for o in Q_OUT_OFFSETS]
    return out + [(Q_COUNTS[-1], 0, 0), (Q_COUNTS[-1], 4, 3)]


def q_data(count, kind, scale=0.25, seed=0):
    """float32 images.  mixed: plain values, quotients exactly on k + 0.5 for both signs (scale is a power of two in those launches), values that
    clamp at 0 and 255, denormals, +-0."""
    rng = np.random.default_rng(count * 31 + seed + len(kind))
    x = (rng.standard_normal(count) * 20).astype(np.float32)
    if kind == "mixed":
        k = rng.integers(-300, 300, count)
        ties = ((k + 0.5) * scale).astype(np.float32)
        pick = rng.integers(0, 6, count)
        x = np.where(pick == 0, ties, x)
        x = np.where(pick == 1, np.float32(1e4) * np.sign(x), x)               # clamps at both ends
        x = np.where(pick == 2, np.float32(1e-40) * np.sign(x), x)             # denormals
        x = np.where(pick == 3, np.float32(0.0) * np.sign(x), x).astype(np.float32)  # +-0
    elif kind == "positive":
        x = np.abs(x) + np.float32(0.5)
    elif kind == "negative":
        x = -np.abs(x) - np.float32(0.5)
    elif kind == "zero":
        x = np.zeros(count, np.float32)
    elif kind == "negzero":
        x = np.full(count, -0.0, np.float32)
    elif kind == "denormal":
        x = (rng.integers(1, 1 << 23, count).astype(np.uint32) | (rng.integers(0, 2, count).astype(np.uint32) << 31)).view(np.float32)
    return np.ascontiguousarray(x, np.float32)


def with_nans(x, seed=0):
    """a copy with NaNs of both signs planted, the first and the last element included (the min / max must skip them)"""
    rng = np.random.default_rng(x.size + seed)
    y = x.copy().view(np.uint32)
    at = np.unique(np.concatenate([[0, x.size - 1], rng.integers(0, x.size, max(1, x.size // 7))]))
    y[at] = np.where(at % 2 == 0, 0x7fc00000, 0xffc00001).astype(np.uint32)
    return y.view(np.float32)


def minmax_ref(x):
    """the BIT PATTERNS (uint32) of max(x, +0.0f) and min(x, -0.0f): the reference's 0.0f seeds, strict comparisons, so NaNs and zeros of either
    sign never replace a seed; the minimum of an image without a negative element is -0.0f (include/mi355_yolo_int8.h)"""
    x = np.asarray(x, np.float32).ravel()
    pos, neg = x[x > 0], x[x < 0]
    mx = pos.max() if pos.size else np.float32(0.0)
    mn = neg.min() if neg.size else np.float32(-0.0)
    return np.array([mx, mn], np.float32).view(np.uint32)


def quantize_ref(x, scale, zp):
    x = np.asarray(x, np.float32)
    q = x / np.float32(scale)                                   # float32 division
    assert q.dtype == np.float32 and np.isfinite(q).all() and (np.abs(q) < 2.0 ** 31 - 256).all(), "outside the contract (see above)"
    d = q.astype(np.float64)
    r = np.copysign(np.floor(np.abs(d) + 0.5), d)               # round(): half away from zero, in double
    t = (r + np.float64(zp)).astype(np.float32)                 # the sum in double, stored to float
    return np.clip(np.trunc(t).astype(np.int64), 0, 255).astype(np.uint8)


# ------------------------------------------------------------------------------------------------------------------------------ letterbox
Lb = namedtuple("Lb", "name imw imh c w h")
LB_CASES = (Lb("1xN", 1, 7, 1, 16, 16), Lb("Nx1", 7, 1, 3, 16, 16), Lb("2x2", 2, 2, 4, 16, 16), Lb("larger", 40, 25, 3, 16, 12),
            Lb("smaller", 5, 3, 3, 32, 20), Lb("wider_shorter", 40, 3, 1, 32, 32), Lb("narrower_taller", 3, 37, 4, 24, 32),
            Lb("side_exactly_2", 40, 3, 3, 32, 32), Lb("same_size", 9, 9, 1, 9, 9), Lb("1xN_tall_target", 1, 5, 3, 6, 31), Lb("portrait", 11, 30, 3, 32, 17))
LB_DEGENERATE, LB_BAD_SIZE = "letterbox: degenerate aspect (resized side < 2)", "letterbox: null / bad size"
LB_REFUSED = ((Lb("side_would_be_1", 40, 2, 3, 32, 32), LB_DEGENERATE), (Lb("1xN_side_0", 1, 20, 1, 16, 16), LB_DEGENERATE),
              (Lb("target_1_wide", 5, 5, 1, 1, 8), LB_BAD_SIZE), (Lb("no_channels", 5, 5, 0, 8, 8), LB_BAD_SIZE),
              (Lb("source_0_wide", 0, 5, 1, 8, 8), LB_BAD_SIZE))
LB_CLAUSES = {
    "lb.imw_1": lambda c: c.imw == 1, "lb.imh_1": lambda c: c.imh == 1,
    "lb.source_wider_than_target": lambda c: c.imw > c.w, "lb.source_taller_than_target": lambda c: c.imh > c.h,
    "lb.resized_side_2": lambda c: min(letterbox_geometry(c.imw, c.imh, c.w, c.h)[:2]) == 2,
    "lb.bars_left_right": lambda c: letterbox_geometry(c.imw, c.imh, c.w, c.h)[2] > 0,
    "lb.bars_top_bottom": lambda c: letterbox_geometry(c.imw, c.imh, c.w, c.h)[3] > 0,
    "lb.c_1": lambda c: c.c == 1, "lb.c_3": lambda c: c.c == 3, "lb.c_4": lambda c: c.c == 4,
}


def letterbox_geometry(imw, imh, w, h):
    """(new_w, new_h, ox, oy) of letterbox_image (ref: src/image.c:812-831): the comparison in float, the sizes in int"""
    if np.float32(w) / np.float32(imw) < np.float32(h) / np.float32(imh):
        new_w, new_h = w, (imh * w) // imw
    else:
        new_h, new_w = h, (imw * h) // imh
    return new_w, new_h, (w - new_w) // 2, (h - new_h) // 2


def letterbox_last_column(im, new_h):
    """column new_w - 1 of the resized image: the source's last column alone, combined vertically (each product and the sum one float32 rounding)"""
    c, imh, imw = im.shape
    col = im[:, :, imw - 1].astype(np.float32)
    out = np.empty((c, new_h), np.float32)
    h_scale = np.float32(imh - 1) / np.float32(new_h - 1)
    for r in range(new_h):
        sy = np.float32(r) * h_scale
        iy = int(sy)
        dy = np.float32(sy - np.float32(iy))
        v = np.float32(1 - dy) * col[:, iy]
        if not (r == new_h - 1 or imh == 1):
            v = v + dy * col[:, iy + 1]
        out[:, r] = v
    return out


def letterbox_last_row(im, new_w, new_h):
    """row new_h - 1 of the resized image: the first vertical term only, of the horizontally resized source row (int)((new_h - 1) * h_scale) --
    the source's last row, weight 1, whenever that float product is exactly imh - 1 (returned as iy, dy for the caller to tell)"""
    c, imh, imw = im.shape
    sy = np.float32(new_h - 1) * (np.float32(imh - 1) / np.float32(new_h - 1))
    iy = int(sy)
    dy = np.float32(sy - np.float32(iy))
    row = im[:, iy, :].astype(np.float32)
    out = np.empty((c, new_w), np.float32)
    w_scale = np.float32(imw - 1) / np.float32(new_w - 1)
    for x in range(new_w):
        if x == new_w - 1 or imw == 1:
            v = row[:, imw - 1]
        else:
            sx = np.float32(x) * w_scale
            ix = int(sx)
            dx = np.float32(sx - np.float32(ix))
            v = np.float32(1 - dx) * row[:, ix] + dx * row[:, ix + 1]
        out[:, x] = np.float32(1 - dy) * v
    return out, iy, dy


def letterbox_source(cs):
    rng = np.random.default_rng(cs.imw * 131 + cs.imh * 17 + cs.c)
    return rng.random((cs.c, cs.imh, cs.imw), dtype=np.float32)


# ------------------------------------------------------------------------------------------------------------------------ yolo activation
YOLO_N, YOLO_CLASSES = (1, 3, 5), (1, 80)
YOLO_MAPS = ((1, 1), (7, 9), (8, 8), (5, 13), (1, 257))   # hw = 1, 63, 64, 65, 257
YOLO_B = 2
YOLO_EXACT = (88.0, -88.0, 104.0, -104.0, 745.0, -745.0, np.inf, -np.inf)   # the rounding to float leaves the device's exp no say here
YOLO_PASSTHROUGH_BITS = (0x7fc00000, 0xffc00001, 0x7f800001, 0x7f800000, 0xff800000, 0x80000000, 0x00000001, 0x807fffff)  # NaNs, +-inf, -0, denormals
YOLO_REFUSALS = (("B 0", dict(B=0)), ("B -1", dict(B=-1)), ("n 0", dict(n=0)), ("H 0", dict(H=0)), ("W 0", dict(W=0)), ("W -4", dict(W=-4)),
                 ("classes -1", dict(classes=-1)), ("classes -5", dict(classes=-5)))
YOLO_REFUSAL_MESSAGE = "yolo: need B, n, H, W >= 1 and classes >= 0"


def yolo_input(B, n, classes, hw, seed):
    """[B][n][classes + 5][hw] floats: plain values everywhere; the bit patterns above planted in entries 2 and 3, the exact points in the others"""
    rng = np.random.default_rng(seed)
    per = classes + 5
    x = (rng.standard_normal((B, n, per, hw)) * 6).astype(np.float32)
    flat = x.reshape(B * n, per, hw)
    for i, bits in enumerate(YOLO_PASSTHROUGH_BITS):
        flat[i % (B * n), 2 + i % 2, (i * 7) % hw] = np.array([bits], np.uint32).view(np.float32)[0]
    for i, v in enumerate(YOLO_EXACT):
        flat[(i + 1) % (B * n), (0, 1, 4, per - 1)[i % 4], (i * 5 + 1) % hw] = np.float32(v)
    return x


def yolo_ref(x):
    """entries 2, 3 untouched; the others np.float32(1 / (1 + exp(-float64(v))))"""
    with np.errstate(over="ignore", invalid="ignore"):  # (the NaNs planted in entries 2 and 3 pass through the cast)
        out = (1.0 / (1.0 + np.exp(-x.astype(np.float64)))).astype(np.float32)
    out[:, :, 2:4] = x[:, :, 2:4]
    return out


def ulps_apart(a, b):
    """distance in float32 steps between finite floats of one sign region (denormals included)"""
    def key(v):
        i = np.ascontiguousarray(v, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(key(a) - key(b))


# ------------------------------------------------------------------------------------------------------------------------------- checksum
CK_COUNTS = (0, 1, 255, 256, 257, 1024 * 256 + 1)   # the last one makes the grid-stride loop iterate (1024 workgroups of 256 at the most)


def checksum_ref(words):
    """sum of word[i] * (2 i + 1) modulo 2^64, in Python integers"""
    return sum(int(w) * (2 * i + 1) for i, w in enumerate(words.tolist())) & ((1 << 64) - 1)


def checksum_words(n, seed=0):
    return np.random.default_rng(n + seed).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
