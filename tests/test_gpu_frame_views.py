"""Frame views on the device: a batch slot looks at a rectangle of its frame under an EXIF orientation (mi355_frame_view), in every kind of
frames, through the C-ABI and through the host.

What a view call must give is the EXISTING u8 calls' contract on the view materialised as an RGB frame: frame_views.apply_view of the RGB frame
the kind's entry stands for (the util modules' converters), then frame_geometry.expected_rgb -- the oracle's letterbox, the quantiser line, the
min / max words.  Never the new kernels.  Outputs live between guards of sentinel bytes and are compared whole, as tests/test_gpu_frame_geometry.py
does it (its Guarded, source builders and variant list are used here); every comparison is exact."""
import ctypes as C
import functools
import io
import os

import numpy as np
import pytest

import frame_geometry as fg
import frame_views as fv
import frames_bayer_util as fb
import frames_packed_util as fp
import frames_util
import test_gpu_frame_geometry as tg
from frames_util import CFG, ROOT, _bits, _wts
from yolo_quantization_amd import binding

pytestmark = pytest.mark.gpu
EINVAL = -22
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module", autouse=True)
def _dev():
    binding.init(0)


def S():
    return binding.shim()


class ViewRun:
    """One batch through the two view calls of a kind.  lays: (planes, entry) of every DISTINCT frame; slots: which distinct frame each slot
    looks at (the table entries share the device frames); views: one per slot.  ptr_off: bytes between an aligned address and every plane."""

    def __init__(self, kind, struct, lays, slots, views, w, h, out_off=0, ptr_off=0):
        self.kind, self.B, self.w, self.h = kind, len(slots), w, h
        assert len(views) == self.B
        self.bufs, entries = [], []
        for planes, entry in lays:
            ptrs, pitches = [], []
            for p in planes:
                pitch = (p.shape[1] + 4) | 1  # odd, at least 4 bytes of 0xEE behind every row
                raw = np.concatenate([np.full(ptr_off, 0xEE, np.uint8), frames_util._padded(p, pitch).ravel()])
                self.bufs.append(binding.DevBuf.from_numpy(raw))
                ptrs.append(self.bufs[-1].ptr.value + ptr_off)
                pitches.append(pitch)
            entries.append(np.frombuffer(bytes(entry(ptrs, pitches)), np.uint8))
        raw = np.ascontiguousarray(np.stack(entries)[np.asarray(slots)])
        self.table = (struct * self.B)()
        C.memmove(self.table, raw.ctypes.data, raw.nbytes)
        self.table_dev = binding.DevBuf.from_numpy(raw)
        self.views = (binding.FrameView * self.B)(*[binding.frame_view(tuple(v)) for v in views])
        self.views_dev = binding.DevBuf.from_numpy(np.frombuffer(bytes(self.views), np.uint8))
        self.bufs += [self.table_dev, self.views_dev]
        self.mm = tg.Guarded(8 * self.B, init=np.full(2 * self.B, 7.0, np.float32).view(np.uint8))
        self.out = tg.Guarded(self.B * 3 * h * w, off=out_off)

    def minmax(self, views_host=None, plain=False):
        if plain:
            return getattr(S(), f"mi355_frames_{self.kind}_letterbox_minmax")(self.table_dev.ptr, self.table, self.B, self.w, self.h, self.mm.ptr, None)
        call = getattr(S(), f"mi355_frames_{self.kind}_view_letterbox_minmax")
        return call(self.table_dev.ptr, self.table, self.views_dev.ptr, views_host or self.views, self.B, self.w, self.h, self.mm.ptr, None)

    def quantize(self, scales, zps, views_host=None, plain=False):
        pairs = [binding.DevBuf.from_numpy(np.asarray(scales, np.float32)), binding.DevBuf.from_numpy(np.asarray(zps, np.uint8))]
        self.bufs += pairs
        if plain:
            return getattr(S(), f"mi355_frames_{self.kind}_letterbox_quantize")(self.table_dev.ptr, self.table, self.B, self.w, self.h, pairs[0].ptr,
                                                                                pairs[1].ptr, self.out.ptr, None)
        call = getattr(S(), f"mi355_frames_{self.kind}_view_letterbox_quantize")
        return call(self.table_dev.ptr, self.table, self.views_dev.ptr, views_host or self.views, self.B, self.w, self.h, pairs[0].ptr, pairs[1].ptr,
                    self.out.ptr, None)

    def free(self):
        for b in self.bufs + [self.mm, self.out]:
            b.free()


def _both_passes(run, wants, what, plain=False, free=True):
    """wants: fg.Want per SLOT.  The min / max words of every slot first, then every byte of every slot."""
    mm, q = np.stack([x.mm for x in wants]), np.stack([x.q for x in wants])
    binding.check(run.minmax(plain=plain), what + ": minmax")
    run.mm.check(mm, what + ": min / max words", unit=4)
    run.out.check(None, what + ": the min / max pass stores no byte")
    binding.check(run.quantize([x.scale for x in wants], [x.zp for x in wants], plain=plain), what + ": quantize")
    run.out.check(q, what + ": bytes")
    run.mm.check(mm, what + ": the quantiser stores no min / max word", unit=4)
    if free:
        run.free()


def _refused_and_untouched(run, views, message, what):
    """the view calls with another host view table: refused with `message`, nothing launched, no byte of either output written"""
    bad = (binding.FrameView * run.B)(*[binding.frame_view(tuple(v)) for v in views])
    want = (f"invalid argument: frames_{run.kind}: " + message).encode()
    assert run.minmax(views_host=bad) == EINVAL and S().mi355_last_error() == want, what
    assert run.quantize(np.ones(run.B, np.float32), np.zeros(run.B, np.uint8), views_host=bad) == EINVAL and S().mi355_last_error() == want, what
    run.mm.check(None, what + ": a refused call writes no min / max word")
    run.out.check(None, what + ": a refused call writes no byte")


@functools.lru_cache(maxsize=None)
def _want(frame_key, view, w, h):
    return fv.expected_view(_RGB[frame_key], view, w, h)


_RGB = {}


def _wants(key, rgb, views, w, h):
    _RGB[key] = rgb
    return [_want(key, tuple(v), w, h) for v in views]


# ----------------------------------------------------------------------------------------------------- u8: every rectangle, every orient
@pytest.mark.parametrize("case", fv.U8_CASES, ids=lambda c: f"{c[0][0]}x{c[0][1]}-{c[1]}-into_{c[3][0]}x{c[3][1]}")
def test_u8_one_frame_under_every_orient(case):
    """one frame, one slot per orient the letterbox accepts for the rectangle; the orients it refuses are refused, and write nothing.  The frame
    is stored as BGR for the 16 x 12 network"""
    (fw, fh), label, rect, (w, h) = case
    rgb = fv.rgb_frame(fw, fh, 100 * fw + fh)
    order = "bgr" if (w, h) == (16, 12) else "rgb"
    lay = frames_util._lay_u8(np.ascontiguousarray(rgb[:, :, ::-1]) if order == "bgr" else rgb, 0, order)
    views = [fv.View(*rect, o) for o in fv.ORIENTS]
    ok = [v for v in views if fv.accepted(v, w, h)]
    no = [v for v in views if not fv.accepted(v, w, h)]
    run = ViewRun("u8", binding.FrameU8, [lay], [0] * max(len(ok), 1), ok or views[:1], w, h, fv.OUT_OFF[(w, h)])
    for v in no:
        _refused_and_untouched(run, (ok or views[:1])[:-1] + [v], fg.DEGENERATE, f"{label} orient {v.orient}")
    if ok:
        _both_passes(run, _wants((fw, fh), rgb, ok, w, h), label, free=False)
    run.free()


def test_u8_two_frames_alternating_under_sixteen_views():
    a, b = fv.rgb_frame(13, 9, 1), fv.rgb_frame(8, 6, 2)
    slots = [i % 2 for i in range(16)]
    views = [fv.View(*((3, 1, 7, 5) if s == 0 else (1, 0, 6, 5)), 1 + i // 2) for i, s in enumerate(slots)]
    wants = [_wants("alt%d" % s, (a, b)[s], [v], 16, 12)[0] for s, v in zip(slots, views)]
    lays = [frames_util._lay_u8(a, 0), frames_util._lay_u8(b, 1)]
    assert set(slots) == {0, 1} and len(views) == 16
    _both_passes(ViewRun("u8", binding.FrameU8, lays, slots, views, 16, 12, out_off=1), wants, "two frames alternating")


# -------------------------------------------------------------------------------------------------------------------- the other sources
BAYER_BOTH_TONES = [("bayer", p, ("u8", 0, t)) for p in fb.BAYER for t in (False, True)]
VARIANTS = tg.VARIANTS + [v for v in BAYER_BOTH_TONES if v not in tg.VARIANTS]
KIND_RUNS = [(v, n) for v in VARIANTS for n in fv.KIND_NETS]


def _kind_views(variant):
    extra = [fv.View(*r, o) for r in (fv.BAYER_INSIDE, fv.BAYER_EDGE) for o in fv.ORIENTS] if variant[0] == "bayer" else []
    return fv.KIND_VIEWS + extra


@pytest.mark.parametrize("variant,net", KIND_RUNS, ids=[f"{tg._vid(v)}-into_{n[0]}x{n[1]}" for v, n in KIND_RUNS])
def test_every_kind_at_the_offsets_its_addressing_cares_about(variant, net):
    """two 13 x 9 frames alternating over the slots, one slot per (rectangle, orient): x0 in 0..3, y0 in {0, 1}, rectangles touching the far edges,
    the whole frame; Bayer also strictly inside at odd (x0, y0) -- the crop of D(frame), not D(crop) -- and on the frame's far edges"""
    w, h = net
    fw, fh = fv.KIND_FRAME
    made = [tg._source(variant, fw, fh, 1000 * k + 77) for k in range(2)]
    views = _kind_views(variant)
    slots = [i % 2 for i in range(len(views))]
    wants = [_wants((tg._vid(variant), s), np.ascontiguousarray(made[s][3]), [v], w, h)[0] for s, v in zip(slots, views)]
    _both_passes(ViewRun(made[0][0], made[0][1], [m[2] for m in made], slots, views, w, h, fv.OUT_OFF[net]), wants, tg._vid(variant))


PACKED = [v for v in tg.VARIANTS if v[0] == "packed"]


@pytest.mark.parametrize("variant", PACKED, ids=tg._vid)
def test_packed_frames_at_an_odd_address(variant):
    made = tg._source(variant, 13, 9, 31)
    views = fv.KIND_VIEWS[:32]
    wants = _wants((tg._vid(variant), "odd"), np.ascontiguousarray(made[3]), views, 12, 12)
    run = ViewRun(made[0], made[1], [made[2]], [0] * len(views), views, 12, 12, ptr_off=1)
    assert run.table[0].data % 2 == 1
    _both_passes(run, wants, tg._vid(variant) + " at an odd address")


@pytest.mark.parametrize("variant", VARIANTS, ids=tg._vid)
def test_the_identity_view_equals_the_call_without_views(variant):
    made = [tg._source(variant, fw, fh, 5 + fw) for fw, fh in ((13, 9), (8, 6))]
    views = [fv.View(0, 0, 13, 9, 1), fv.View(0, 0, 8, 6, 1)]
    wants = [fg.expected_rgb(np.ascontiguousarray(m[3]), 12, 12) for m in made]
    run = ViewRun(made[0][0], made[0][1], [m[2] for m in made], [0, 1], views, 12, 12)
    _both_passes(run, wants, tg._vid(variant) + ": without views", plain=True, free=False)
    plain = run.out.buf.to_numpy(np.uint8, run.out.buf.nbytes), run.mm.buf.to_numpy(np.uint8, run.mm.buf.nbytes)
    run.mm.free(); run.out.free()
    run.mm = tg.Guarded(16, init=np.full(4, 7.0, np.float32).view(np.uint8))
    run.out = tg.Guarded(2 * 3 * 12 * 12)
    _both_passes(run, wants, tg._vid(variant) + ": identity views", free=False)
    assert np.array_equal(run.out.buf.to_numpy(np.uint8, run.out.buf.nbytes), plain[0]) and np.array_equal(run.mm.buf.to_numpy(np.uint8, run.mm.buf.nbytes), plain[1])
    run.free()


def test_refused_views_launch_nothing():
    rgb = fv.rgb_frame(13, 9, 3)
    good = [fv.View(1, 1, 7, 5, 6), fv.View(0, 0, 13, 9, 1)]
    run = ViewRun("u8", binding.FrameU8, [frames_util._lay_u8(rgb, 0)], [0, 0], good, 12, 12)
    for name, view, message in fv.REFUSED_VIEWS:
        _refused_and_untouched(run, [good[0], view], message, name)
    _both_passes(run, _wants("refused", rgb, good, 12, 12), "the good views behind the refusals")


# ---------------------------------------------------------------------------------------------------------------------- through the host
HOST_VIEWS = [fv.View(1, 1, 7, 5, 6), fv.View(3, 1, 10, 8, 1), fv.View(0, 0, 13, 9, 7), fv.View(2, 0, 6, 6, 4)]  # slots 0..2 share a frame
TONE = (np.random.default_rng(8).permutation(768) % 256).astype(np.uint8).reshape(3, 256)


def _host_frame(kind, w, h, seed):
    """(what prepare_from_frames_<kind> takes for one frame, the RGB frame it stands for)"""
    rng = np.random.default_rng(seed)
    b = lambda *s: rng.integers(0, 256, s, dtype=np.uint8)  # noqa: E731
    rows, cols = (np.arange(h) >> 1)[:, None], (np.arange(w) >> 1)[None, :]
    if kind == "u8":
        f = b(h, w, 3)
        return f, f
    if kind == "nv12":
        y, uv = b(h, w), b((h + 1) // 2, (w + 1) // 2, 2)
        return (y, uv), frames_util.yuv_to_rgb(y, uv[rows, cols, 0], uv[rows, cols, 1], binding.YUV_MATRIX["bt601"])
    if kind == "planar":
        y, u, v = b(h, w), b((h + 1) // 2, (w + 1) // 2), b((h + 1) // 2, (w + 1) // 2)
        return (y, u, v), frames_util.yuv_to_rgb(y, u[rows, cols], v[rows, cols], binding.YUV_MATRIX["bt601"])
    if kind == "packed":
        f = fp.packed_frame("yuyv", w, h, seed)
        return (f, w), fp.packed_to_rgb(f, w, "yuyv", "bt601")
    if kind == "p010":
        y16, uv16 = fp.p010_frame(w, h, seed)
        return (y16, uv16), fp.p010_to_rgb(y16, uv16, "bt601")
    assert kind == "bayer"
    raw = b(h, w)
    return raw, fb.demosaic(raw, "grbg", "u8", 0, TONE)


def _prepare(net, kind, frames):
    if kind == "u8":
        return net.prepare_from_frames_u8(frames)
    if kind == "nv12":
        return net.prepare_from_frames_nv12(frames)
    if kind == "planar":
        return net.prepare_from_frames_planar(frames, "i420")
    if kind == "packed":
        return net.prepare_from_frames_packed(frames, "yuyv")
    if kind == "p010":
        return net.prepare_from_frames_p010(frames)
    return net.prepare_from_frames_bayer(frames, "grbg", "u8", 0, TONE)


def _host_batch(kind, seed):
    """(frames for the entry point, frame sizes, the materialised views)"""
    (fa, ra), (fb_, rb) = _host_frame(kind, 13, 9, seed), _host_frame(kind, 8, 6, seed + 1)
    frames, rgbs = [fa, fa, fa, fb_], [ra, ra, ra, rb]
    return frames, [(13, 9)] * 3 + [(8, 6)], [fv.apply_view(np.ascontiguousarray(r), v) for r, v in zip(rgbs, HOST_VIEWS)]


def _same_input(a, b, what):
    assert np.array_equal(a._pull_input(), b._pull_input()), f"{what}: input bytes"
    (sa, za), (sb, zb) = a.input_quantization(), b.input_quantization()
    assert np.array_equal(_bits(sa), _bits(sb)) and np.array_equal(za, zb), f"{what}: scales / zero points"


HOST_RUNS = ([(k, m) for k in ("u8", "nv12", "planar", "packed", "p010", "bayer") for m in ("shared_scale", "per_image")]
             + [(k, m) for k in ("nv12", "bayer") for m in ("on_device", "on_device_per_image", "graph")])


@pytest.mark.parametrize("kind,mode", HOST_RUNS, ids=[f"{k}-{m}" for k, m in HOST_RUNS])
def test_host_views_equal_the_u8_path_on_the_materialised_views(tmp_path, kind, mode):
    wts = _wts(tmp_path)
    a, b = binding.Net(CFG, wts, batch=4, use_graph=mode == "graph"), binding.Net(CFG, wts, batch=4)
    for n in (a, b):
        n.set_input_per_image(mode in ("per_image", "on_device_per_image", "graph"))
        if mode.startswith("on_device"):
            n.set_input_on_device(True)
    for seed in (10, 20):  # the second batch replays the graph and reuses arena and tables
        frames, sizes, mat = _host_batch(kind, seed)
        a.set_frame_views(HOST_VIEWS)
        _prepare(a, kind, frames)
        b.prepare_from_frames_u8(mat)
        _same_input(a, b, f"{kind} {mode} seed {seed}")
        x = a._pull_input().reshape(4, 3, 12, 12)
        if mode in ("per_image", "on_device_per_image", "graph"):  # every slot is quantised with its own pair
            for slot in range(4):
                assert np.array_equal(x[slot], fg.expected_rgb(mat[slot], 12, 12).q), f"slot {slot}: the u8 contract on the view"
        frames_util._assert_same_run(frames_util._layers_and_dets(a, mat), frames_util._layers_and_dets(b, mat), f"{kind} {mode}")
    # views cleared: what a network that never had any gives for the whole frames
    a.set_frame_views(None)
    _prepare(a, kind, frames)
    whole = [np.ascontiguousarray(r) for r in (_host_frame(kind, 13, 9, 20)[1],) * 3 + (_host_frame(kind, 8, 6, 21)[1],)]
    b.prepare_from_frames_u8(whole)
    _same_input(a, b, f"{kind} {mode}: views cleared")
    a.close(); b.close()


def test_host_none_views_rebatch_and_bad_views(tmp_path):
    wts = _wts(tmp_path)
    a, b = binding.Net(CFG, wts, batch=2), binding.Net(CFG, wts, batch=2)
    f = fv.rgb_frame(13, 9, 4)
    a.set_frame_views([None, (1, 1, 7, 5, 8)], sizes=[(13, 9)] * 2)
    a.prepare_from_frames_u8([f, f])
    b.prepare_from_frames_u8([f, fv.apply_view(f, (1, 1, 7, 5, 8))])
    _same_input(a, b, "None is the whole frame")
    with pytest.raises(ValueError):
        a.set_frame_views([None, None])
    with pytest.raises(ValueError):
        a.set_frame_views([(0, 0, 1, 1, 1)])
    a.close(); b.close()


def test_host_replica_owns_its_views(tmp_path):
    wts = _wts(tmp_path)
    parent, ref = binding.Net(CFG, wts, batch=4), binding.Net(CFG, wts, batch=4)
    for n in (parent, ref):
        n.set_input_per_image(True)
    frames, sizes, mat = _host_batch("nv12", 30)
    parent.set_frame_views(HOST_VIEWS)
    _prepare(parent, "nv12", frames)
    rep = parent.replica()
    _prepare(rep, "nv12", frames)  # no views of its own: the whole frames
    ref.prepare_from_frames_u8([np.ascontiguousarray(_host_frame("nv12", 13, 9, 30)[1])] * 3 + [np.ascontiguousarray(_host_frame("nv12", 8, 6, 31)[1])])
    _same_input(rep, ref, "a replica starts without views")
    other = [fv.View(0, 0, 13, 9, 3), fv.View(5, 2, 8, 7, 5), fv.View(1, 0, 12, 9, 2), fv.View(0, 0, 8, 6, 6)]
    rep.set_frame_views(other)
    _prepare(rep, "nv12", frames)
    rgbs = [_host_frame("nv12", 13, 9, 30)[1]] * 3 + [_host_frame("nv12", 8, 6, 31)[1]]
    ref.prepare_from_frames_u8([fv.apply_view(np.ascontiguousarray(r), v) for r, v in zip(rgbs, other)])
    _same_input(rep, ref, "the replica's own views")
    ref.prepare_from_frames_u8(mat)
    _prepare(parent, "nv12", frames)
    _same_input(parent, ref, "the parent keeps its views")
    rep.close(); ref.close(); parent.close()


def test_host_frames_on_device_under_views(tmp_path):
    wts = _wts(tmp_path)
    a, b = binding.Net(CFG, wts, batch=4), binding.Net(CFG, wts, batch=4)
    frames, sizes, mat = _host_batch("nv12", 40)
    bufs, dev = [], []
    for y, uv in (frames[0], frames[3]):
        h, w = y.shape
        by, buv = binding.DevBuf.from_numpy(frames_util._padded(y, w + 3)), binding.DevBuf.from_numpy(uv)
        bufs += [by, buv]
        dev.append((by.ptr.value, buv.ptr.value, w, h, w + 3, 2 * ((w + 1) // 2)))
    a.set_frame_views(HOST_VIEWS)
    a.prepare_from_frames_nv12([dev[0]] * 3 + [dev[1]], on_device=True)
    b.prepare_from_frames_u8(mat)
    _same_input(a, b, "frames on the device")
    a.close(); b.close()
    for x in bufs:
        x.free()


@pytest.mark.parametrize("kind,name,ext", [("jpeg", "422_51x37", ".jpg"), ("png", "grey16_trns_23x19", ".png")])
def test_host_coded_inputs_under_views(tmp_path, kind, name, ext):
    with np.load(os.path.join(GOLDEN, kind + "_expected.npz")) as z:
        rgb = np.ascontiguousarray(z[name])
    with open(os.path.join(GOLDEN, kind, name + ext), "rb") as f:
        data = f.read()
    fh, fw = rgb.shape[:2]
    views = [fv.View(0, 0, fw, fh, 6), fv.View(fw // 3, fh // 3, fw - fw // 3, fh - fh // 3, 2)]
    wts = _wts(tmp_path)
    a, b = binding.Net(CFG, wts, batch=2), binding.Net(CFG, wts, batch=2)
    for n in (a, b):
        n.set_input_per_image(True)
    a.set_frame_views(views)
    sizes = a.prepare_from_png([data, data]) if kind == "png" else a.prepare_from_jpeg([data, data])
    assert sizes == [(fw, fh)] * 2, "the sizes stay the frame's"
    b.prepare_from_frames_u8([fv.apply_view(rgb, v) for v in views])
    _same_input(a, b, kind)
    a.close(); b.close()


def test_detect_views_equals_the_slots_detections_mapped_and_merged(tmp_path):
    """four overlapping tiles of one frame: the boxes of detect_views are the slots' own boxes (detect on the tiles' sizes, no NMS) sent through
    view_box_to_frame, every one of them once, and one NMS over the frame then zeroes scores that no per-slot NMS would"""
    wts = _wts(tmp_path)
    net = binding.Net(CFG, wts, batch=4)
    f = fv.rgb_frame(40, 30, 6)
    views = binding.tile_views(40, 30, 2, 2, 8, orient=6)
    net.set_frame_views(views)
    net.prepare_from_frames_u8([f] * 4)
    net.forward()
    net.sync()
    vw, vh = [fv.view_size(v)[0] for v in views], [fv.view_size(v)[1] for v in views]
    per_slot = net.detect(vw, vh, thresh=0.005, nms=0)
    merged = net.detect_views(40, 30, thresh=0.005, nms=0)
    assert list(merged) == [0]
    want = np.concatenate([np.stack([binding.view_box_to_frame(v, 40, 30, bx) for bx in d["boxes"]]) if d["kept"] else np.zeros((0, 4), np.float32)
                           for v, d in zip(views, per_slot)])
    assert len(want) > 4 and np.array_equal(merged[0]["boxes"], want) and np.array_equal(merged[0]["probs"], np.concatenate([d["probs"] for d in per_slot]))
    once = net.detect_views(40, 30, thresh=0.005, nms=0.3)[0]
    key = lambda d: sorted(map(tuple, np.concatenate([d["boxes"], d["objectness"][:, None]], axis=1).tolist()))  # noqa: E731
    assert key(once) == key(merged[0]), "the NMS permutes and zeroes scores, it drops no row"
    assert (once["probs"] > 0).sum() < (merged[0]["probs"] > 0).sum()
    net.close()


# ----------------------------------------------------------------------------------------------------------------------------- the CLI
def test_cli_view_orient_and_tiles(tmp_path):
    import subprocess
    from PIL import Image
    exe = os.path.join(ROOT, "yolo_quantization_amd", "bin", "darknet")
    wts = _wts(tmp_path, seed=1)
    names, data = str(tmp_path / "x.names"), str(tmp_path / "x.data")
    open(names, "w").write("\n".join(["ant", "bee", "cat", "dog", "eel"]) + "\n")
    open(data, "w").write(f"classes= 5\nnames = {names}\n")
    a = np.random.default_rng(8).integers(0, 256, (37, 53, 3), dtype=np.uint8)
    views = {"frame": a, "turned": np.rot90(a, -1), "cut": a[5:29, 7:40], "cut_turned": np.rot90(a[5:29, 7:40], 1)}
    paths = {}
    for k, v in views.items():
        paths[k] = str(tmp_path / f"{k}.ppm")
        frames_util._write_ppm(paths[k], v)

    def run(extra):
        r = subprocess.run([exe, "detector", "test", data, CFG, wts] + extra + ["-thresh", "0.3", "-boxes"], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        return frames_util._blocks(r.stdout)

    def boxes(blocks):
        assert len(blocks) == 1, "one block per image"
        return blocks[0][1:]
    plain = run([paths["frame"], "-frames", "u8"])
    assert run([paths["frame"], "-frames", "u8", "-orient", "1"]) == plain and any(line.startswith("box:") for line in boxes(plain))
    # a full-frame view under orient 6 gives the boxes of the turned picture, mapped back: the scores are the turned picture's
    scores = lambda lines: sorted(line.split("box:")[0] for line in lines if not line.startswith("box:"))  # noqa: E731
    assert scores(boxes(run([paths["frame"], "-frames", "u8", "-orient", "6"]))) == scores(boxes(run([paths["turned"], "-frames", "u8"])))
    assert scores(boxes(run([paths["frame"], "-frames", "u8", "-view", "7,5,33,24"]))) == scores(boxes(run([paths["cut"], "-frames", "u8"])))
    assert scores(boxes(run([paths["frame"], "-frames", "u8", "-view", "7,5,33,24", "-orient", "8"]))) == scores(boxes(run([paths["cut_turned"], "-frames", "u8"])))
    tiled = run([paths["frame"], "-frames", "u8", "-tiles", "2x2,8"])
    assert len(tiled) == 1 and "batch 4" not in tiled[0][0] and any(line.startswith("box:") for line in boxes(tiled))
    # -orient exif: a Pillow-written JPEG with orientation 6 equals -orient 6 on the same file; a PPM gets 1
    im = Image.fromarray(np.ascontiguousarray(a[:32, :48]))
    exif = im.getexif()
    exif[0x0112] = 6
    jpg = str(tmp_path / "turned.jpg")
    im.save(jpg, format="JPEG", exif=exif, subsampling=0, progressive=False, optimize=False)
    assert binding.jpeg_exif_orientation(open(jpg, "rb").read()) == 6
    assert run([jpg, "-orient", "exif"]) == run([jpg, "-orient", "6"]) != run([jpg])
    assert run([paths["frame"], "-frames", "u8", "-orient", "exif"]) == plain
    r = subprocess.run([exe, "detector", "test", data, CFG, wts, paths["frame"], "-orient", "6"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "-frames" in r.stderr
