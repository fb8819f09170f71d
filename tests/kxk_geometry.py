"""The general conv kernel's launcher and K layout, restated clause by clause, and the case table built from it (no GPU needed).

conv_kxk.hip serves every [convolutional] shape the specialised kernels refuse.  Restated here, from the sources' text:

  * kxk_unit / kxk_geom (kargs.h): unit bytes per tap, channel chunks, K-steps per chunk, padded filter rows;
  * the part of conv_forward_impl / conv_generic_forward (shim.hip) that decides a call goes to the general kernel: specialised_shape,
    legacy_geom / legacy_exact, cell4_out, and the refusals in front of the launch (a 1x1 with stride or padding, a padded map smaller than
    the kernel, an input window that does not start on the kernel's unit);
  * conv_kxk_launch (conv_kxk.hip): the two tile configurations (32 | 64 filters x 256 pixels, then 128 filters x 64 pixels, four waves
    along M), the preferred tile width and its two fall-backs {pref, 8, 16}, the LDS test of each, the grid, or "no tile fits";
  * conv_ref_f32_general_launch: the ref-f32 twin's grid.

Every decision goes through a Trace (launch_geometry.Trace on this module's own labels), so that tests/test_kxk_geometry_cpu.py can demand
that the case table reaches both sides of every clause, and tests/test_gpu_kxk_geometry.py that a launch on the device is the
instantiation's (grid, threads, lds) named here before it compares bytes.

Labels not reached on both sides, each by name with its reason: SIZE_GUARDS (need 2^31 workgroups) and DEAD (cannot be true given the
clauses in front; the CPU sweep checks that).

Also here: the exact vectorised reference for any (k, stride, pad) -- zero-point-padded windows, one float64 matrix product (exact:
|acc| < 2^53), wrapped to int32 as oracle.conv_acc wraps, ONE oracle.requant call -- and the K layout of the packed A fragments
(lane, half, tap slot, channel) for the packing test."""
import numpy as np

import launch_geometry as lg

KB = 1024
LDS_MAX = 160 * KB
THREADS = 256
MAX_SLOTS = 128          # KXK_MAX_SLOTS: tap slots per channel chunk (the tap table in front of the patch: 128 ints)
cdiv = lg.cdiv

LABELS = {
    "dispatch": ("d.specialised_shape", "d.ref_f32", "d.legacy_geom", "d.legacy_exact_s2", "d.cell4_out", "d.to_general", "d.k1_stride_or_pad",
                 "d.map_smaller_than_kernel", "d.no_general_fragments", "d.unaligned_window"),
    "geom": ("g.unit4", "g.unit8", "g.chunks>1", "g.last_chunk_partial", "g.tail_slots_masked", "g.slot_table_full", "g.in_plain_cells",
             "g.out_plain_cells"),
    "launch": ("l.slots>128", "l.in_cs4_needs_unit4", "l.ms2", "l.cfg2_tried", "l.pref8", "l.pref16", "l.tw>npx", "l.pref_fits", "l.fall8_fits",
               "l.fall16_fits", "l.grid_2^31", "l.tiles_x>1", "l.tiles_y>1", "l.mgroups>1", "l.lds>64K", "l.ragged_x", "l.ragged_y", "l.ragged_n32",
               "l.ragged_n4"),
}
ALL_LABELS = {l: k for k, ls in LABELS.items() for l in ls}

SIZE_GUARDS = {
    "l.grid_2^31": "grid > 2^31 - 1: 2^31 workgroups of at least one output pixel and 4-byte cell each, an 8 GiB output",
}
# label -> (the side that cannot happen, why)
DEAD = {
    "l.slots>128": (True, "spc * 2 * (16 / U) is k * k rounded up to whole K-steps of 32 / U taps: at most 128 (U = 4, 16 x 8), 124 (U = 8), 122 (U = 16) "
                          "for k <= 11, and conv_forward refuses k > 11"),
    "l.tw>npx": (True, "the widths are 8, 16 and 32; the smaller tile holds 64 pixels"),
    "l.in_cs4_needs_unit4": (True, "4-byte cells belong to 3-channel tensors (mi355_tensor_describe), conv_forward refuses x.C != c, and c = 3 has unit 4"),
    "d.no_general_fragments": (True, "a blob lacks the general section only for a specialised 1x1 with n != 3; such a layer reaches the general kernel "
                                     "only with a stride or a padding, which is refused first"),
}


class Trace(lg.Trace):
    """launch_geometry.Trace over this module's labels"""

    def __call__(self, label, cond):
        assert label in ALL_LABELS, label
        cond = bool(cond)
        self.hits.setdefault(label, set()).add(cond)
        return cond


# ------------------------------------------------------------------------------------------------------------ kargs.h
def kxk_unit(c):
    return 4 if c <= 4 else (8 if c <= 8 else 16)


def kxk_geom(n, c, k, tr=None):
    """kxk_geom: K = (channel chunk, tap slot, channel in the chunk), `unit` channel bytes per tap"""
    tr = tr or Trace()
    unit = 4 if tr("g.unit4", c <= 4) else (8 if tr("g.unit8", c <= 8) else 16)
    tpl = 16 // unit                       # taps per 16-byte lane fragment
    nchunks = cdiv(c, 16) if unit == 16 else 1
    tr("g.chunks>1", nchunks > 1)
    tr("g.last_chunk_partial", c - (nchunks - 1) * unit < unit)
    spc = cdiv(k * k, 2 * tpl)             # K-steps per chunk: two lane halves of tpl taps
    tr("g.tail_slots_masked", spc * 2 * tpl > k * k)
    tr("g.slot_table_full", spc * 2 * tpl == MAX_SLOTS)
    return dict(unit=unit, tpl=tpl, nchunks=nchunks, spc=spc, ksteps=nchunks * spc, mpad=cdiv(n, 128) * 128)


def frag_index(g, k):
    """where byte e of lane `lane` of K-step `st` of chunk `ch` comes from: arrays [ksteps, 64, 16] of (tap, channel), -1 where the slot or the
    channel is padding.  Lane = (row lane % 32, half kh = lane / 32); byte e = tap slot (2 st + kh) tpl + e / U, channel ch U + e % U."""
    U, tpl = g["unit"], g["tpl"]
    step = np.arange(g["ksteps"])[:, None, None]
    lane = np.arange(64)[None, :, None]
    e = np.arange(16)[None, None, :]
    ch, st = step // g["spc"], step % g["spc"]
    tap = (2 * st + lane // 32) * tpl + e // U
    chan = ch * U + e % U + 0 * lane
    return np.where(tap < k * k, tap, -1), chan


# ------------------------------------------------------------------------------------------------------------ shim.hip
def specialised_shape(c, k):
    return k in (1, 3) and ((c == 3 and k == 3) or c % 16 == 0)


def out_size(H, W, k, s, pad):
    return (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1


def _refuse(why, **kw):
    return dict(kernel=None, refused=why, grid=None, threads=None, lds=None, **kw)


def dispatch(tr, cs):
    """conv_forward_impl / conv_generic_forward up to the launch -> None: the general kernels take the call; "specialised": the other
    launchers do; or the refusal"""
    c, n, k, s, pad = cs.c, cs.n, cs.k, cs.stride, cs.pad
    assert 1 <= k <= 11 and s >= 1 and pad >= 0
    spec = tr("d.specialised_shape", specialised_shape(c, k))
    legacy_geom = tr("d.legacy_geom", s == 1 and ((k == 3 and pad == 1) or (k == 1 and pad == 0)))
    legacy = legacy_geom
    if not tr("d.ref_f32", cs.accum == "ref_f32"):
        legacy = legacy_geom or tr("d.legacy_exact_s2", s == 2 and k == 3 and pad == 1 and c % 16 == 0)
    cell4_out = tr("d.cell4_out", cs.out_cs() == 4)
    if not tr("d.to_general", not spec or not legacy or cell4_out):
        return "specialised"
    if tr("d.k1_stride_or_pad", k == 1 and (s != 1 or pad != 0)):
        return _refuse("1x1")
    if tr("d.map_smaller_than_kernel", cs.H + 2 * pad < k or cs.W + 2 * pad < k):
        return _refuse("the padded map is smaller than the kernel")
    if cs.accum == "ref_f32":
        return None
    # blob_layout: a specialised 3x3 blob and every 3-filter blob carry the general section behind their own
    if tr("d.no_general_fragments", spec and not (k == 3 or n == 3)):
        return _refuse("no general-kernel fragments")
    if tr("d.unaligned_window", cs.x_offset() % kxk_unit(c)):
        return _refuse("aligned")
    return None


# ------------------------------------------------------------------------------------------------------------ conv_kxk.hip
def tile_fits(U, npx, tw, k, s):
    th = npx // tw
    ph, pw = (th - 1) * s + k, (tw - 1) * s + k
    lds = MAX_SLOTS * 4 + ph * pw * U
    return lds <= LDS_MAX, th, ph, pw, lds


def conv_kxk_launch(tr, B, H, W, c, n, k, s, pad, in_cs=None):
    """conv_kxk_launch: the first tile that fits of {(ms, 1), (1, 4)} x {pref, 8, 16}"""
    g = kxk_geom(n, c, k, tr)
    U = g["unit"]
    OH, OW = out_size(H, W, k, s, pad)
    assert OH >= 1 and OW >= 1
    in_cs = in_cs or lg.cell_bytes(c)
    if tr("l.slots>128", g["spc"] * 2 * (16 // U) > MAX_SLOTS):
        return _refuse("slots")
    if tr("l.in_cs4_needs_unit4", in_cs == 4 and U != 4):
        return _refuse("in_cs")
    tr("g.in_plain_cells", in_cs == 4)
    cfgs = ((2 if tr("l.ms2", n > 32) else 1, 1), (1, 4))
    for ci, (ms, wm) in enumerate(cfgs):
        if ci:
            tr("l.cfg2_tried", True)
        npx = (4 // wm) * 64
        pref = 8 if tr("l.pref8", OW <= 8) else (16 if tr("l.pref16", OW <= 16) else 32)
        for ti, (tw, label) in enumerate(((pref, "l.pref_fits"), (8, "l.fall8_fits"), (16, "l.fall16_fits"))):
            if tr("l.tw>npx", tw > npx):
                continue
            fits, th, ph, pw, lds = tile_fits(U, npx, tw, k, s)
            if not tr(label, fits):
                continue
            if not ci:
                tr("l.cfg2_tried", False)
            tiles_x, tiles_y = cdiv(OW, tw), cdiv(OH, th)
            mgroups = cdiv(n, 32 * ms * wm)
            grid = mgroups * B * tiles_x * tiles_y
            if tr("l.grid_2^31", grid > 0x7FFFFFFF):
                return _refuse("grid")
            tr("l.tiles_x>1", tiles_x > 1)
            tr("l.tiles_y>1", tiles_y > 1)
            tr("l.mgroups>1", mgroups > 1)
            tr("l.lds>64K", lds > 64 * KB)
            tr("l.ragged_x", OW % tw != 0)
            tr("l.ragged_y", OH % th != 0)
            tr("l.ragged_n32", n % 32 != 0)   # a wave's last 32-row tile ends early: the `row0 >= n` skip
            tr("l.ragged_n4", n % 4 != 0)     # the last dword of a cell is stored byte by byte
            return dict(kernel=9, refused=None, inst=(U, ms, wm), tw=tw, th=th, ph=ph, pw=pw, tiles_x=tiles_x, tiles_y=tiles_y, mgroups=mgroups,
                        grid=grid, threads=THREADS, lds=lds, OH=OH, OW=OW, cfg=ci, choice=("pref", "fall8", "fall16")[ti], geom=g)
    return _refuse("no tile of the general kernel fits", geom=g, choice="refused", unit=U)


def ref_f32_launch(B, n, OH, OW):
    """conv_ref_f32_general_launch: one thread per output element"""
    return dict(kernel=6, refused=None, grid=cdiv(B * n * OH * OW, 256), threads=256, lds=0)


def route(tr, cs):
    """what mi355_conv_forward does with the case -> "specialised" | the general launch | the refusal"""
    d = dispatch(tr, cs)
    if d is not None:
        return d
    OH, OW = out_size(cs.H, cs.W, cs.k, cs.stride, cs.pad)
    tr("g.out_plain_cells", cs.out_cs() == 4)
    if cs.accum == "ref_f32":
        return ref_f32_launch(cs.B, cs.n, OH, OW)
    return conv_kxk_launch(tr, cs.B, cs.H, cs.W, cs.c, cs.n, cs.k, cs.stride, cs.pad, cs.in_cs())


# ------------------------------------------------------------------------------------------------------------ invariants (CPU)
def check_launch(g, B, H, W, c, n, k, s, pad, in_cs=None):
    """what the kernel relies on, for an accepted launch (the kernel's own index arithmetic, restated)"""
    U, ms, wm = g["inst"]
    tw, th, ph, pw = g["tw"], g["th"], g["ph"], g["pw"]
    wn = 4 // wm
    assert g["lds"] <= LDS_MAX and g["lds"] == MAX_SLOTS * 4 + ph * pw * U
    assert tw * th == wn * 64 and th == (wn * 64) >> {8: 3, 16: 4, 32: 5}[tw], "TH as the kernel derives it from tw_sh"
    # tiles cover every output pixel exactly once: tile (ty, tx) holds pixels oy0 + p / TW, ox0 + p % TW below (OH, OW)
    seen = np.zeros((g["OH"], g["OW"]), np.int32)
    p = np.arange(wn * 64)
    for ty in range(g["tiles_y"]):
        for tx in range(g["tiles_x"]):
            oy, ox = ty * th + p // tw, tx * tw + p % tw
            ok = (oy < g["OH"]) & (ox < g["OW"])
            assert ok.any(), "an empty tile"
            np.add.at(seen, (oy[ok], ox[ok]), 1)
    assert (seen == 1).all()
    # the largest patch cell a lane reads: its window origin plus the last tap's offset
    cbase = (p // tw) * s * pw + (p % tw) * s
    tapoff = np.array([(t // k) * pw + t % k if t < k * k else 0 for t in range(MAX_SLOTS)])
    assert int(cbase.max() + tapoff.max()) == ph * pw - 1
    slots = g["geom"]["spc"] * 2 * g["geom"]["tpl"]
    assert k * k <= slots <= MAX_SLOTS
    # every staged in-image cell lies inside the tensor: the last image's last pixel, the last chunk's bytes
    in_cs = in_cs or lg.cell_bytes(c)
    last_cell = 2 + ((B - 1) * (H + 1) + H) * (W + 1) + (W - 1)
    assert last_cell * in_cs + (g["geom"]["nchunks"] - 1) * U + U <= lg.in_cells(B, H, W) * in_cs
    assert (g["geom"]["nchunks"] - 1) * U + U <= in_cs
    # no wave reads fragments past the packed blob, and the filters are covered
    assert g["mgroups"] * 32 * ms * wm <= g["geom"]["mpad"] and g["mgroups"] * 32 * ms * wm >= n
    assert g["grid"] == g["mgroups"] * B * g["tiles_x"] * g["tiles_y"]


def nothing_fits(U, k, s, OW):
    """no configuration of the launcher's list fits"""
    pref = 8 if OW <= 8 else (16 if OW <= 16 else 32)
    return not any(tile_fits(U, npx, tw, k, s)[0] for npx in (256, 64) for tw in (pref, 8, 16))


# ------------------------------------------------------------------------------------------------------------ reference
def conv_windows(x, k, stride, pad, zp_in):
    """x [B, c, H, W] u8 -> float64 [c * k * k, B * OH * OW]: the windows in im2col order (channel, ky, kx), every tap outside the image the
    image's input zero point, for any pad >= 0 (whole windows in the padding included)"""
    B, c, H, W = x.shape
    OH, OW = out_size(H, W, k, stride, pad)
    zp = np.broadcast_to(np.asarray(zp_in, np.uint8).reshape(-1, 1, 1, 1), (B, 1, 1, 1))
    xp = np.empty((B, c, H + 2 * pad, W + 2 * pad), np.uint8)
    xp[:] = zp
    xp[:, :, pad:pad + H, pad:pad + W] = x
    col = np.empty((c, k, k, B, OH, OW), np.float64)
    for ky in range(k):
        for kx in range(k):
            col[:, ky, kx] = xp[:, :, ky:ky + stride * (OH - 1) + 1:stride, kx:kx + stride * (OW - 1) + 1:stride].transpose(1, 0, 2, 3)
    return col.reshape(c * k * k, B * OH * OW), OH, OW


def conv_acc_ref(x, wq, zp_w, k, stride, pad, zp_in):
    """exact accumulators [n, B * OH * OW] int32, wrapped as oracle.conv_acc wraps them.  zp_in: a scalar, or one per image"""
    wd = wq.astype(np.float64) - zp_w.astype(np.float64)[:, None]
    col, OH, OW = conv_windows(x, k, stride, pad, zp_in)
    acc = wd @ col
    assert np.abs(acc).max() < 2.0 ** 53
    return acc.astype(np.int64).astype(np.int32), OH, OW  # (int64 -> int32: the low 32 bits, as the C cast)


def conv_ref(x, wq, zp_w, k, stride, pad, zp_in, bias, mv, sv, zp_act, act, store):
    """-> (int32 [B, n, OH * OW], u8 [B, n, OH, OW]): conv_acc_ref + ONE oracle.requant call on [n, B * OH * OW]"""
    import oracle
    acc, OH, OW = conv_acc_ref(x, wq, zp_w, k, stride, pad, zp_in)
    u8 = oracle.requant(acc, bias, mv, sv, zp_act, act, store)
    n, B = wq.shape[0], x.shape[0]
    return (np.ascontiguousarray(acc.reshape(n, B, OH * OW).transpose(1, 0, 2)),
            np.ascontiguousarray(u8.reshape(n, B, OH, OW).transpose(1, 0, 2, 3)))


# ------------------------------------------------------------------------------------------------------------ the case table
class Case:
    """one mi355_conv_forward call.  xwin / ywin: (channels of the wider tensor, channel offset) when x / y is a channel window of a wider
    tensor.  twin: the ref-f32 twin runs as well.  accum: 'exact' | 'ref_f32' (dispatch probes)."""

    def __init__(self, name, c, n, H, W, B, k, stride, pad, act="leaky", xwin=None, ywin=None, twin=False, accum="exact"):
        self.name, self.c, self.n, self.H, self.W, self.B, self.k, self.stride, self.pad = name, c, n, H, W, B, k, stride, pad
        self.act, self.xwin, self.ywin, self.twin, self.accum = act, xwin, ywin, twin, accum

    def __repr__(self):
        return self.name

    def in_cs(self):
        return lg.cell_bytes(self.xwin[0] if self.xwin else self.c)

    def out_cs(self):
        return lg.cell_bytes(self.ywin[0] if self.ywin else self.n)

    def x_offset(self):
        """x.data modulo 16 (device allocations are aligned far beyond that)"""
        return self.xwin[1] if self.xwin else 0

    def out_hw(self):
        return out_size(self.H, self.W, self.k, self.stride, self.pad)


def trace_case(cs):
    tr = Trace()
    return tr, route(tr, cs)


def macs(cs):
    OH, OW = cs.out_hw()
    return cs.B * max(OH, 0) * max(OW, 0) * cs.n * cs.c * cs.k * cs.k


def device_tensors(cs):
    """bytes of every device tensor the case's call touches"""
    OH, OW = (max(v, 1) for v in cs.out_hw())
    cx, cy = (cs.xwin[0] if cs.xwin else cs.c), (cs.ywin[0] if cs.ywin else cs.n)
    return {"x": lg.tensor_bytes(cs.B, cs.H, cs.W, cx), "x_nchw": cs.B * cx * cs.H * cs.W, "y": lg.tensor_bytes(cs.B, OH, OW, cy),
            "y_nchw": cs.B * cy * OH * OW, "acc": 4 * cs.B * cs.n * OH * OW, "f32": 4 * cs.B * cs.n * OH * OW}


def _c(*a, **kw):
    return Case(*a, **kw)


CASES = []


def _add(*cases):
    CASES.extend(cases)


def _k(tag, c, n, OH, OW, B, k, s, pad, ey=0, ex=0, **kw):
    """a case by its OUTPUT map: H = (OH - 1) s + k - 2 pad + ey (ey, ex < s: rows / columns behind the last window that no window reads)"""
    assert 0 <= ey < s and 0 <= ex < s
    H, W = (OH - 1) * s + k - 2 * pad + ey, (OW - 1) * s + k - 2 * pad + ex
    assert H >= 1 and W >= 1 and out_size(H, W, k, s, pad) == (OH, OW)
    return Case(f"{tag}_c{c}_n{n}_{H}x{W}_B{B}_k{k}s{s}p{pad}", c, n, H, W, B, k, s, pad, **kw)


# ---- the dispatch (shim.hip): shapes the specialised launchers keep, shapes handed to the general kernels, the refusals in front of a launch
_add(
    _c("d_kept_3x3_c16", 16, 16, 6, 6, 2, 3, 1, 1),
    _c("d_kept_3x3_s2_c16", 16, 16, 8, 8, 2, 3, 2, 1),
    _c("d_kept_1x1_c16", 16, 16, 5, 5, 2, 1, 1, 0),
    _c("d_kept_first_layer", 3, 16, 6, 6, 2, 3, 1, 1),
    _c("d_general_c3_3x3_s2", 3, 16, 9, 11, 2, 3, 2, 1),
    _c("d_general_c16_3x3_s2_ref_f32_only", 16, 16, 8, 8, 2, 3, 2, 1, accum="ref_f32"),
    _c("d_general_c16_3x3_p0", 16, 16, 7, 7, 2, 3, 1, 0),
    _c("d_general_n3_3x3_c16_cell4_out", 16, 3, 6, 6, 2, 3, 1, 1, twin=True),
    _c("d_general_n3_1x1_c32_cell4_out", 32, 3, 5, 7, 2, 1, 1, 0),
    _c("d_refused_1x1_s2", 8, 16, 6, 6, 1, 1, 2, 0),
    _c("d_refused_1x1_p1_c32", 32, 16, 6, 6, 1, 1, 1, 1),
    _c("d_refused_map_2x9_below_k5", 8, 16, 2, 9, 1, 5, 1, 1),
    _c("d_refused_map_9x1_below_k4", 24, 16, 9, 1, 1, 4, 1, 1),
    _c("d_window_c24_at_16_of_64", 24, 20, 9, 7, 2, 5, 2, 2, xwin=(64, 16)),
    _c("d_window_c24_at_4_of_64_refused", 24, 20, 9, 7, 2, 5, 2, 2, xwin=(64, 4)),
    _c("d_window_c8_at_8_of_32", 8, 20, 9, 7, 2, 3, 1, 0, xwin=(32, 8)),
    _c("d_window_c8_at_4_of_32_refused", 8, 20, 9, 7, 2, 3, 1, 0, xwin=(32, 4)),
    _c("d_window_c4_at_4_of_16", 4, 20, 9, 7, 2, 3, 1, 2, xwin=(16, 4)),
    _c("d_window_c2_at_6_of_16_refused", 2, 20, 9, 7, 2, 3, 1, 2, xwin=(16, 6)),
)

# ---- the K layout: the unit at c = 4 | 5 and 8 | 9, chunks at c = 16 | 17, the last chunk's channel mask on, under and over each dword edge,
# plain 4-byte image cells (c = 3) against 16-byte biased cells (c = 1, 2, 4), the 3-filter layer's plain output cells
_add(
    _k("k_u4_biased_cell", 1, 8, 5, 6, 2, 3, 1, 1),
    _k("k_u4_biased_cell", 2, 8, 4, 7, 2, 5, 2, 2, act="relu"),
    _k("k_u4_plain_cell", 3, 8, 5, 6, 2, 3, 1, 0, twin=True),
    _k("k_u4_biased_cell", 4, 8, 5, 6, 2, 3, 2, 1, ey=1, ex=1),
    _k("k_u4_plain_in_plain_out", 3, 3, 6, 5, 2, 5, 1, 2),
    _k("k_u8", 5, 8, 5, 6, 2, 3, 1, 1, twin=True),
    _k("k_u8", 7, 8, 4, 7, 2, 4, 2, 3, act="relu6"),
    _k("k_u8", 8, 8, 5, 6, 2, 3, 1, 2),
    _k("k_u16_one_chunk", 9, 8, 5, 6, 2, 3, 1, 1),
    _k("k_u16_one_chunk", 12, 8, 4, 7, 2, 2, 1, 0),
    _k("k_u16_one_chunk", 13, 8, 5, 6, 2, 3, 2, 1),
    _k("k_u16_one_chunk", 15, 8, 5, 6, 2, 4, 1, 3),
    _k("k_u16_one_chunk", 16, 8, 5, 6, 2, 5, 1, 2, twin=True),
    _k("k_u16_two_chunks", 17, 8, 5, 6, 2, 3, 1, 0),
    _k("k_u16_two_chunks", 19, 8, 4, 7, 2, 2, 1, 1, act="linear"),
    _k("k_u16_two_chunks", 20, 8, 5, 6, 2, 3, 3, 1, ey=2, ex=1),
    _k("k_u16_two_chunks", 21, 8, 5, 6, 2, 5, 2, 4),
    _k("k_u16_two_chunks", 28, 8, 4, 7, 2, 3, 1, 1),
    _k("k_u16_two_chunks", 29, 8, 5, 6, 2, 4, 2, 0),
    _k("k_u16_two_chunks", 31, 8, 5, 6, 2, 3, 1, 2),
    _k("k_u16_three_chunks", 33, 8, 5, 6, 2, 1, 1, 0),
)

# ---- the tap slots of the last K-step: U = 16 even k (none masked) | odd k (one), U = 8 k = 2 (exact) | 3, U = 4 k = 1 (seven masked),
# 4 (exact), 11 (128 slots: the table full); paddings 0, k / 2, k - 1 and beyond k (whole windows in the zero-point fill)
_add(
    _k("t_u16_even", 24, 12, 6, 5, 1, 6, 1, 3),
    _k("t_u16_odd", 24, 12, 6, 5, 1, 7, 2, 6),
    _k("t_u16_k11", 10, 12, 3, 4, 1, 11, 3, 5),
    _k("t_u8_exact", 6, 12, 6, 5, 1, 2, 1, 1),
    _k("t_u8_masked_pad_beyond_k", 6, 12, 8, 7, 1, 3, 1, 4),
    _k("t_u8_k11", 8, 12, 7, 8, 1, 11, 2, 10),
    _k("t_u4_k1_seven_masked", 3, 12, 6, 5, 2, 1, 1, 0),
    _k("t_u4_k1_biased_cell", 4, 12, 6, 5, 2, 1, 1, 0),
    _k("t_u4_exact", 3, 12, 6, 5, 1, 4, 2, 0, ey=1, ex=1),
    _k("t_u4_table_full", 3, 12, 3, 4, 1, 11, 4, 0, ey=3, ex=2),
    _k("t_u4_table_full_pad_beyond_k", 2, 12, 5, 5, 1, 11, 4, 12),
    _k("t_u16_pad_beyond_k", 16, 12, 9, 8, 1, 2, 1, 3),
)

# ---- filters: ms at n = 32 | 33, mgroups at n = 64 | 65 (ms = 2), ragged n inside a dword and inside a 32-row tile (the byte stores, the
# `row0 >= n` skip), a y window at a channel offset off the dword grid
_add(
    _k("n_ms1", 5, 32, 4, 5, 2, 3, 1, 1),
    _k("n_ms2", 5, 33, 4, 5, 2, 3, 1, 1),
    _k("n_ms2_one_group", 20, 64, 4, 5, 2, 3, 2, 1),
    _k("n_ms2_two_groups", 20, 65, 4, 5, 2, 3, 2, 1),
    _k("n_ragged", 3, 1, 4, 5, 2, 3, 1, 0, act="linear"),
    _k("n_ragged", 12, 7, 4, 5, 2, 3, 1, 1),
    _k("n_ragged", 6, 37, 4, 5, 2, 3, 1, 1),
    _k("n_ragged_three_groups", 12, 131, 4, 5, 2, 2, 1, 0),
    _k("n_y_window_at_18_of_64", 12, 21, 4, 5, 2, 3, 1, 1, ywin=(64, 18)),
    _k("n_y_window_at_32_of_64", 5, 20, 4, 5, 2, 3, 2, 1, ywin=(64, 32)),
)

# ---- the preferred width at OW = 8 | 9 and 16 | 17; tiles along x at OW = 32 | 33, along y at OH = th | th + 1 for each width; partial tiles on
# both axes; the blockIdx decomposition with tiles_x, tiles_y, mgroups > 1 and B = 3 together, for each tile width and each unit
_add(
    _k("w_tw8_th32", 5, 8, 32, 8, 1, 2, 1, 0),
    _k("w_tw8_th32_two_rows_of_tiles", 5, 8, 33, 8, 1, 2, 1, 0),
    _k("w_tw16_th16", 12, 8, 16, 9, 1, 2, 1, 0),
    _k("w_tw16_th16_two_rows_of_tiles", 12, 8, 17, 16, 1, 2, 1, 0),
    _k("w_tw32_th8", 3, 8, 8, 17, 1, 2, 1, 0),
    _k("w_tw32_th8_two_rows_of_tiles", 3, 8, 9, 32, 1, 2, 1, 0),
    _k("w_tw32_two_columns_of_tiles", 12, 8, 8, 33, 1, 2, 1, 0),
    _k("w_u8_tw16", 7, 20, 7, 12, 2, 3, 2, 1, act="relu"),
    _k("w_u8_tw32_partial_tiles_both_axes", 6, 20, 9, 35, 2, 2, 1, 0),
    _k("w_u4_ms2_tw8", 3, 40, 6, 7, 2, 5, 2, 2, act="linear"),
    _k("w_u4_ms2_tw16", 1, 48, 7, 13, 2, 3, 1, 1),
    _k("w_blockidx_tw32", 5, 70, 19, 40, 3, 3, 1, 1),
    _k("w_blockidx_tw32_s2", 20, 70, 11, 70, 3, 5, 2, 2, ey=1, ex=1, act="relu6"),
    _k("w_blockidx_tw32_plain_cells", 3, 67, 10, 35, 3, 4, 3, 0),
)

# ---- LDS: for each unit the preferred width fits | the fall-back to 8 (first configuration, OW 9..16, stride above k) | the fall-back to 16
# (stride below k) | the second configuration (128 filters x 64 pixels, four waves along M) at each width | nothing fits; dynamic LDS on each
# side of 64 KiB for each instantiation <U, 1, 1>, <U, 2, 1>, <U, 1, 4>, the large launch first and a small one of the same instantiation
# behind it; the second configuration's filter groups at n = 128 | 129
_add(
    # U = 16
    _k("l_u16_111_over_64K", 16, 8, 9, 8, 1, 4, 4, 0),
    _k("l_u16_111_under_64K", 16, 8, 9, 8, 1, 4, 3, 0),
    _k("l_u16_121_over_64K", 9, 40, 5, 20, 1, 5, 4, 2),
    _k("l_u16_121_under_64K", 9, 40, 5, 20, 1, 5, 3, 2),
    _k("l_u16_fall16_from_8", 10, 12, 18, 7, 2, 11, 6, 5),
    _k("l_u16_fall16_from_32", 18, 36, 17, 18, 1, 11, 6, 0),
    _k("l_u16_114_tw8", 16, 8, 9, 8, 2, 3, 7, 1),
    _k("l_u16_114_tw8_over_64K", 16, 40, 10, 7, 1, 8, 8, 4),
    _k("l_u16_114_tw16_n128", 12, 128, 5, 12, 1, 3, 7, 1),
    _k("l_u16_114_tw16_n129_two_groups", 12, 129, 9, 14, 3, 3, 7, 1, ey=3, ex=5),
    _k("l_u16_114_tw32_blockidx", 24, 130, 5, 37, 3, 2, 7, 0, act="relu6"),
    _k("l_u16_114_fall16", 16, 8, 5, 6, 1, 4, 14, 2),
    _k("l_u16_refused_tw8", 16, 8, 1, 1, 1, 11, 13, 0),
    _k("l_u16_refused_tw16", 9, 40, 2, 9, 1, 11, 13, 5),
    # U = 8
    _k("l_u8_111_over_64K", 8, 8, 33, 5, 1, 2, 6, 0),
    _k("l_u8_111_under_64K", 8, 8, 33, 5, 1, 2, 5, 0),
    _k("l_u8_121_over_64K", 5, 33, 7, 20, 1, 7, 6, 3),
    _k("l_u8_121_tw16_under_64K", 5, 33, 7, 12, 1, 7, 2, 3),
    _k("l_u8_121_tw8", 7, 40, 9, 6, 2, 5, 1, 2),
    _k("l_u8_fall8_from_16", 8, 12, 20, 10, 1, 8, 9, 4),
    _k("l_u8_114_tw8", 6, 12, 9, 7, 2, 9, 9, 4),
    _k("l_u8_114_tw8_over_64K", 8, 130, 9, 5, 1, 7, 12, 3),
    _k("l_u8_114_tw16_n129_two_groups", 5, 129, 6, 13, 3, 9, 9, 0, ey=4),
    _k("l_u8_114_tw32_blockidx", 8, 132, 5, 35, 3, 9, 9, 8, act="linear"),
    _k("l_u8_114_fall16", 7, 12, 5, 6, 1, 10, 19, 5),
    _k("l_u8_refused", 8, 12, 1, 2, 1, 7, 20, 0),
    # U = 4
    _k("l_u4_111_over_64K", 3, 8, 12, 9, 1, 8, 8, 0),
    _k("l_u4_111_under_64K", 3, 8, 12, 9, 1, 8, 7, 0),
    _k("l_u4_121_over_64K", 4, 40, 5, 20, 1, 9, 9, 4),
    _k("l_u4_121_under_64K", 4, 40, 5, 20, 1, 9, 2, 4),
    _k("l_u4_fall8_from_16", 3, 12, 20, 10, 1, 8, 13, 4),
    _k("l_u4_114_tw8_plain_cells", 3, 12, 9, 8, 2, 9, 13, 4),
    _k("l_u4_114_tw8_over_64K", 3, 12, 9, 7, 1, 9, 17, 0),
    _k("l_u4_114_tw16_n129_two_groups", 3, 129, 6, 13, 3, 9, 13, 4, ex=7),
    _k("l_u4_114_tw32_blockidx_biased_cells", 2, 131, 5, 34, 3, 9, 13, 0, act="relu"),
    _k("l_u4_114_fall16", 3, 12, 5, 6, 1, 7, 28, 3),
    _k("l_u4_refused", 3, 12, 1, 1, 1, 11, 28, 0),
)


# ------------------------------------------------------------------------------------------------------------ operands
ZP_ACT, S_ACT = 23, np.float32(0.0625)


def oracle_dequant(u8):
    """the quant_stop float tail of u8 [B, n, OH, OW] -> float32 [B, n, OH * OW]"""
    import oracle
    return oracle.dequant(u8.reshape(u8.shape[0], u8.shape[1], -1), ZP_ACT, S_ACT)


class Operands:
    """one case's image batch and layer, and the exact reference under both store modes (computed once).  x is the tensor the call reads (the
    window's channels when x is a window of `wide`)."""

    def __init__(self, cs):
        import oracle
        rng = np.random.default_rng(sum(map(ord, cs.name)))
        self.cs = cs
        cx = cs.xwin[0] if cs.xwin else cs.c
        self.wide = rng.integers(0, 256, (cs.B, cx, cs.H, cs.W), dtype=np.uint8)
        off = cs.xwin[1] if cs.xwin else 0
        self.x = self.wide[:, off:off + cs.c]
        self.wq, self.zp_w = lg.rand_layer(rng, cs.n, cs.c, cs.k)[:2]
        self.zp_in = int(rng.integers(0, 256))
        self.want = None
        OH, OW = cs.out_hw()
        if OH < 1 or OW < 1 or (cs.k == 1 and (cs.stride != 1 or cs.pad)):  # refused for its shape: no reference exists
            self.bias, self.mv, self.sv = lg.rand_layer(rng, cs.n, cs.c, cs.k)[2:]
            return
        acc, OH, OW = conv_acc_ref(self.x, self.wq, self.zp_w, cs.k, cs.stride, cs.pad, self.zp_in)
        # "some-wrap" multipliers; where the two store modes then agree on every byte (maps of a few pixels), the stronger regime
        for gain in ("some-wrap", "much-wrap"):
            self.bias, self.mv, self.sv = lg.rand_layer(rng, cs.n, cs.c, cs.k, gain)[2:]
            self.want = {"int32": np.ascontiguousarray(acc.reshape(cs.n, cs.B, OH * OW).transpose(1, 0, 2))}
            for name, store in (("wrap", oracle.STORE_WRAP), ("sat", oracle.STORE_SATURATE)):
                u8 = oracle.requant(acc, self.bias, self.mv, self.sv, ZP_ACT, oracle.ACT[cs.act], store)
                self.want[name] = np.ascontiguousarray(u8.reshape(cs.n, cs.B, OH, OW).transpose(1, 0, 2, 3))
            if self.stores_differ():
                break

    def stores_differ(self):
        return bool((self.want["wrap"] != self.want["sat"]).any())

    def want_ref_f32(self, store):
        """the ref-f32 twin's accumulators and bytes: the oracle's fp32 accumulation, image by image"""
        import oracle
        cs = self.cs
        st = oracle.STORE_WRAP if store == "wrap" else oracle.STORE_SATURATE
        accs = [oracle.conv_acc(self.x[b], self.wq, self.zp_w, cs.k, cs.stride, cs.pad, self.zp_in, oracle.ACC_REF_F32) for b in range(cs.B)]
        u8s = [oracle.requant(a, self.bias, self.mv, self.sv, ZP_ACT, oracle.ACT[cs.act], st) for a in accs]
        OH, OW = cs.out_hw()
        return np.stack(accs).reshape(cs.B, cs.n, OH * OW), np.stack(u8s).reshape(cs.B, cs.n, OH, OW)
