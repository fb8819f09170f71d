"""Frame views without a device: the numpy restatement of tests/frame_views.py against a per-pixel loop and against Pillow's exif_transpose,
the case tables, every refusal through the shim's host-side check (fake device pointers: a refused call never passes them on; no accepted
table is passed here), network_tile_views, network_view_box_to_frame, the merge of network_detections_views on built detections, and
jpeg_exif_orientation_host on built segments, Pillow-written files and, as a stand-alone program under ASan + UBSan, hostile bytes."""
import ctypes as C
import io
import os
import subprocess

import numpy as np
import pytest

import frame_geometry as fg
import frame_views as fv
import frames_bayer_util as fb
from yolo_quantization_amd import binding

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
EINVAL = -22


# ----------------------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("orient", fv.ORIENTS)
def test_apply_view_equals_the_index_maps_and_pillow(orient):
    from PIL import Image, ImageOps
    rgb = fv.rgb_frame(13, 9, 5)
    for rect in list(fv.rects(13, 9).values()) + fv.KIND_RECTS:
        view = fv.View(*rect, orient)
        got = fv.apply_view(rgb, view)
        assert got.shape[:2] == fv.view_size(view)[::-1] and got.flags.c_contiguous
        assert np.array_equal(got, fv.apply_view_by_loop(rgb, view)), view
        im = Image.fromarray(np.ascontiguousarray(rgb[view.y0:view.y0 + view.h, view.x0:view.x0 + view.w]))
        exif = im.getexif()
        exif[0x0112] = orient
        buf = io.BytesIO()
        im.save(buf, format="PNG", exif=exif)  # lossless, and Pillow reads the orientation back from it
        upright = ImageOps.exif_transpose(Image.open(io.BytesIO(buf.getvalue())))
        assert np.array_equal(np.asarray(upright.convert("RGB")), got), view


def test_the_eight_orients_are_distinct_and_the_maps_are_bijections():
    rgb = fv.rgb_frame(5, 3, 1)
    seen = {fv.apply_view(rgb, (0, 0, 5, 3, o)).tobytes() + bytes(fv.view_size((0, 0, 5, 3, o))) for o in fv.ORIENTS}
    assert len(seen) == 8
    for o in fv.ORIENTS:
        view = fv.View(2, 1, 4, 3, o)
        vw, vh = fv.view_size(view)
        hit = {fv.tap_to_frame(view, u, t) for t in range(vh) for u in range(vw)}
        assert hit == {(x, y) for x in range(2, 6) for y in range(1, 4)}
        # neighbouring view taps are neighbouring frame pixels: the 2 x 2 cell of the kernels' Viewed source
        for t in range(vh - 1):
            for u in range(vw - 1):
                cell = [fv.tap_to_frame(view, u + d, t + r) for r in (0, 1) for d in (0, 1)]
                xs, ys = {c[0] for c in cell}, {c[1] for c in cell}
                assert len(xs) == 2 and len(ys) == 2 and max(xs) - min(xs) == 1 and max(ys) - min(ys) == 1


def test_every_clause_of_the_tables_is_reached():
    hits = {name: 0 for name in fv.RECT_CLAUSES}
    for f, label, r, n in fv.U8_CASES:
        for name, clause in fv.RECT_CLAUSES.items():
            hits[name] += bool(clause(f, r))
    assert all(hits.values()), hits
    assert {n for _, _, _, n in fv.U8_CASES} == set(fv.NETS) and {f for f, _, _, _ in fv.U8_CASES} == set(fv.FRAMES)
    # every orient is accepted somewhere and refused somewhere; the one-pixel clauses of either axis are reached after a transpose
    acc = [(f, label, r, n, o, fv.accepted(r + (o,), *n)) for f, label, r, n in fv.U8_CASES for o in fv.ORIENTS]
    for o in fv.ORIENTS:
        assert any(a[5] for a in acc if a[4] == o) and any(not a[5] for a in acc if a[4] == o)
    one_wide = [a for a in acc if a[5] and fv.view_size(a[2] + (a[4],))[0] == 1 and fv.view_size(a[2] + (a[4],))[1] > 1]
    one_high = [a for a in acc if a[5] and fv.view_size(a[2] + (a[4],))[1] == 1 and fv.view_size(a[2] + (a[4],))[0] > 1]
    assert {a[4] >= 5 for a in one_wide} == {False, True} and {a[4] >= 5 for a in one_high} == {False, True}
    # the offsets the kinds' addressing cares about
    xs, ys = {r[0] for r in fv.KIND_RECTS}, {r[1] for r in fv.KIND_RECTS}
    assert {0, 1, 2, 3} <= xs and {0, 1} <= ys and {x % 4 for x in xs} == {0, 1, 2, 3}
    assert any(r[0] % 2 == 1 and (r[0] + r[2]) % 2 == 1 for r in fv.KIND_RECTS), "a view that starts and ends inside a 4:2:2 macropixel"
    assert all(fv.accepted(v, *n) for v in fv.KIND_VIEWS for n in fv.KIND_NETS)
    assert len(fv.KIND_VIEWS) == 8 * len(fv.KIND_RECTS)
    assert fv.OUT_OFF[(7, 5)] == 3 and fv.OUT_OFF[(16, 12)] == 1


@pytest.mark.parametrize("pattern", fb.BAYER)
def test_a_bayer_view_is_a_crop_of_the_demosaiced_frame_not_a_demosaic_of_the_crop(pattern):
    """the case the device test runs must tell the two definitions apart: on its border pixels, and by the colour phase of an odd offset"""
    raw = np.random.default_rng(11).integers(0, 256, (fv.FRAME_H, fv.FRAME_W), dtype=np.uint8)
    full = fb.demosaic(raw, pattern)
    x0, y0, w, h = fv.BAYER_INSIDE
    assert x0 % 2 == 1 and y0 % 2 == 1 and x0 + w < fv.FRAME_W and y0 + h < fv.FRAME_H, "strictly inside, odd offset"
    want = full[y0:y0 + h, x0:x0 + w]
    wrong = fb.demosaic(np.ascontiguousarray(raw[y0:y0 + h, x0:x0 + w]), pattern)
    border = np.ones((h, w), bool)
    border[1:-1, 1:-1] = False
    assert (want != wrong).any(axis=2)[border].sum() > border.sum() // 2, "most border pixels differ"
    # a crop with the phase kept (even offset) still differs on the border: reflection at the cut instead of the real neighbours
    even = fb.demosaic(np.ascontiguousarray(raw[2:2 + h, 2:2 + w]), pattern)
    assert np.array_equal(even[1:-1, 1:-1], full[3:1 + h, 3:1 + w]) and (even != full[2:2 + h, 2:2 + w]).any()
    x0, y0, w, h = fv.BAYER_EDGE
    assert x0 + w == fv.FRAME_W and y0 + h == fv.FRAME_H and x0 % 2 == 1 and y0 % 2 == 1, "touches the frame's far edges"


# ------------------------------------------------------------------------------------------------------------------------- the refusals
def _u8_table(sizes):
    table = (binding.FrameU8 * len(sizes))()
    for b, (w, h) in enumerate(sizes):
        table[b] = binding.FrameU8(0x1000, w, h, 3 * max(w, 1), binding.FRAME_ORDER["rgb"], (C.c_int * 2)(0, 0))
    return table


def _views(vs):
    table = (binding.FrameView * len(vs))()
    for b, v in enumerate(vs):
        table[b] = v if isinstance(v, binding.FrameView) else binding.frame_view(v)
    return table


def _refused(kind, table, views, B, w, h, message):
    S, fake = binding.shim(), C.c_void_p(0x1000)
    want = (f"invalid argument: frames_{kind}: " + message).encode()
    assert getattr(S, f"mi355_frames_{kind}_view_letterbox_minmax")(fake, table, fake, views, B, w, h, fake, None) == EINVAL
    assert S.mi355_last_error() == want
    assert getattr(S, f"mi355_frames_{kind}_view_letterbox_quantize")(fake, table, fake, views, B, w, h, fake, fake, fake, None) == EINVAL
    assert S.mi355_last_error() == want


@pytest.mark.parametrize("r", fv.REFUSED_VIEWS, ids=lambda r: r[0])
def test_view_refusals_through_the_shims_host_side_check(r):
    """the bad view is the second slot's: the first slot's frame and view are good ones"""
    name, view, message = r
    _refused("u8", _u8_table([(fv.FRAME_W, fv.FRAME_H)] * 2), _views([(1, 1, 7, 5, 6), view]), 2, 12, 12, message)


def test_reserved_words_and_the_order_of_the_refusals():
    good = (0, 0, 13, 9, 1)
    for k in range(3):
        v = binding.frame_view(good)
        v.reserved[k] = 1
        _refused("u8", _u8_table([(13, 9)]), _views([v]), 1, 12, 12, fv.M_RESERVED)
    v = binding.frame_view((0, 0, 0, 0, 1))
    v.reserved[2] = -1
    _refused("u8", _u8_table([(13, 9)]), _views([v]), 1, 12, 12, fv.M_RESERVED)  # reserved before the size
    v.orient = 9
    _refused("u8", _u8_table([(13, 9)]), _views([v]), 1, 12, 12, fv.M_ORIENT)    # orient before reserved
    # the frame's own refusals come first, in their words, whatever the view says
    bad_view = (0, 0, 0, 0, 0)
    _refused("u8", _u8_table([(0, 9)]), _views([bad_view]), 1, 12, 12, fg.BAD_FRAME)
    t = _u8_table([(13, 9)])
    t[0].pitch = 38
    _refused("u8", t, _views([bad_view]), 1, 12, 12, "pitch < 3 * w")
    t = _u8_table([(13, 9)])
    t[0].data = None
    _refused("u8", t, _views([bad_view]), 1, 12, 12, "null frame pointer")
    # the batch's and the network's before any frame; a slot's refusals before the next slot's
    _refused("u8", _u8_table([(13, 9)]), _views([bad_view]), 0, 12, 12, fg.BAD_BATCH)
    _refused("u8", _u8_table([(13, 9)]), _views([bad_view]), 1, 1, 12, fg.BAD_NET)
    _refused("u8", _u8_table([(13, 9), (0, 0)]), _views([(0, 0, 14, 9, 1), good]), 2, 12, 12, fv.M_RECT)
    # a frame the letterbox refuses whole is served through a view it accepts: the geometry is the view's
    _refused("u8", _u8_table([(13, 1)]), _views([(0, 0, 13, 1, 1)]), 1, 12, 12, fg.DEGENERATE)
    assert fv.accepted((0, 0, 2, 1, 1), 16, 12)


@pytest.mark.parametrize("kind", ["yuv", "planar", "packed", "p010", "bayer"])
def test_every_kind_refuses_a_view_behind_its_own_prefix_and_after_its_own_checks(kind):
    ci2, z = (C.c_int * 2)(0, 0), 0x1000
    good = {"yuv": lambda: binding.FrameYUV(z, z, 13, 9, 13, 14, 0, 0, ci2),
            "planar": lambda: binding.FramePlanar((C.c_void_p * 3)(z, z, z), 13, 9, (C.c_int * 3)(13, 7, 7), 0, 0, (C.c_int * 3)(0, 0, 0)),
            "packed": lambda: binding.FramePacked(z, 13, 9, 52, 0, 0, 0),
            "p010": lambda: binding.FrameP010(z, z, 13, 9, 26, 28, 0, 0, ci2),
            "bayer": lambda: binding.FrameBayer(z, None, 13, 9, 13, 0, 0, 0, ci2)}[kind]
    struct = type(good())
    table = (struct * 1)(good())
    _refused(kind, table, _views([(0, 0, 13, 9, 0)]), 1, 12, 12, fv.M_ORIENT)
    _refused(kind, table, _views([(12, 8, 2, 1, 1)]), 1, 12, 12, fv.M_RECT)
    _refused(kind, table, _views([(0, 8, 13, 1, 8)]), 1, 12, 12, fg.DEGENERATE)
    own = {"yuv": ("pitch_y", 12, "pitch_y < w"), "planar": ("format", 9, "unknown format (MI355_PLANAR_I420 .. _BGR)"),
           "packed": ("pitch", 51, "pitch < 4 * w"), "p010": ("pitch_y", 25, "pitch_y < 2 * w"), "bayer": ("shift", 9, "shift outside 0..8")}[kind]
    setattr(table[0], own[0], own[1])
    _refused(kind, table, _views([(0, 0, 13, 9, 0)]), 1, 12, 12, own[2])


def test_null_view_tables_are_refused_with_the_calls_own_message():
    S, fake = binding.shim(), C.c_void_p(0x1000)
    t, v = _u8_table([(13, 9)]), _views([(0, 0, 13, 9, 1)])
    assert S.mi355_frames_u8_view_letterbox_minmax(fake, t, None, v, 1, 12, 12, fake, None) == EINVAL
    assert S.mi355_last_error() == b"invalid argument: frames_u8: view_letterbox_minmax: null"
    assert S.mi355_frames_u8_view_letterbox_quantize(fake, t, fake, None, 1, 12, 12, fake, fake, fake, None) == EINVAL
    assert S.mi355_last_error() == b"invalid argument: frames_u8: view_letterbox_quantize: null"


def test_the_view_struct_matches_the_header(tmp_path):
    src = '#include <stddef.h>\n#include <stdio.h>\n#include "mi355_yolo_int8.h"\nint main(void) {\n'
    src += '    printf("%zu", sizeof(mi355_frame_view));\n'
    for f, _ in binding.FrameView._fields_:
        src += f'    printf(" %zu", offsetof(mi355_frame_view, {f}));\n'
    src += '    printf(" %d\\n", MI355_ABI_VERSION);\n    return 0;\n}\n'
    c, exe = tmp_path / "layout.c", tmp_path / "layout"
    c.write_text(src)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    vals = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert vals[0] == C.sizeof(binding.FrameView) == 32
    assert vals[1:-1] == [getattr(binding.FrameView, f).offset for f, _ in binding.FrameView._fields_]
    assert vals[-1] == 6, "new structs and new calls do not bump the ABI"


# ------------------------------------------------------------------------------------------------------------------------------- tiles
TILINGS = [(3840, 2160, 4, 3, 64), (13, 9, 2, 2, 1), (13, 9, 3, 2, 0), (100, 50, 3, 1, 7), (416, 416, 1, 1, 0), (5, 5, 5, 5, 0), (10, 7, 4, 3, 2),
           (1920, 1080, 2, 2, 8)]


@pytest.mark.parametrize("t", TILINGS, ids=lambda t: "x".join(map(str, t)))
def test_tile_views_cover_the_frame(t):
    fw, fh, cols, rows, overlap = t
    views = binding.tile_views(fw, fh, cols, rows, overlap, orient=6)
    assert len(views) == cols * rows
    (tw, xs), (th, ys) = fv.tiles(fw, cols, overlap), fv.tiles(fh, rows, overlap)
    assert tw == -((fw + (cols - 1) * overlap) // -cols) and th == -((fh + (rows - 1) * overlap) // -rows)
    assert views == [(x, y, tw, th, 6) for y in ys for x in xs], "row by row"
    covered = np.zeros((fh, fw), np.int32)
    for x0, y0, w, h, o in views:
        assert 0 <= x0 and 0 <= y0 and x0 + w <= fw and y0 + h <= fh
        covered[y0:y0 + h, x0:x0 + w] += 1
    assert covered.min() >= 1
    assert views[-1][0] + tw == fw and views[-1][1] + th == fh, "the last tile ends on the frame's edge"
    for i in range(cols - 1):
        assert xs[i] == min(i * (tw - overlap), fw - tw) and xs[i + 1] - xs[i] <= tw - overlap


def test_tile_views_shift_the_last_tile_and_refuse():
    assert binding.tile_views(10, 7, 4, 1, 2) == [(0, 0, 4, 7, 1), (2, 0, 4, 7, 1), (4, 0, 4, 7, 1), (6, 0, 4, 7, 1)]
    assert [v[0] for v in binding.tile_views(13, 9, 3, 1, 0)] == [0, 5, 8], "5-wide tiles: the last starts at 8, not 10"
    assert binding.tile_views(416, 416, 1, 1, 0) == [(0, 0, 416, 416, 1)]
    H = binding.host()
    out = (binding.FrameView * 16)()
    sentinel = bytes(out)
    for args in ((10, 10, 1, 1, 10, 1),    # overlap == the tile size
                 (10, 10, 2, 1, 10, 1),    # tiles larger than the frame
                 (10, 10, 2, 2, 9, 1),     # (10 + 9) / 2 rounds up to 10, overlap 9 < 10: accepted -- see below
                 (10, 10, 0, 1, 0, 1), (10, 10, 1, -1, 0, 1), (0, 10, 1, 1, 0, 1), (10, 10, 1, 1, -1, 1), (10, 10, 1, 1, 0, 0), (10, 10, 1, 1, 0, 9)):
        rc = H.network_tile_views(*args, out)
        if args == (10, 10, 2, 2, 9, 1):
            assert rc == 4 and [(v.x0, v.y0, v.w, v.h) for v in out[:4]] == [(0, 0, 10, 10)] * 4
            out = (binding.FrameView * 16)()
            continue
        assert rc == EINVAL and bytes(out) == sentinel, args
    assert fv.tiles(10, 1, 10) is None and fv.tiles(10, 2, 10) is None
    assert H.network_tile_views(10, 10, 1, 1, 0, 1, None) == EINVAL


# ------------------------------------------------------------------------------------------------------------------------------- boxes
def test_view_box_to_frame_equals_the_float64_restatement():
    fw, fh = 640, 360
    rng = np.random.default_rng(9)
    rect = (33, 17, 301, 207)
    edge = [(0, .5, 0, .5), (1, .5, 0, .5), (.5, 0, .5, 0), (.5, 1, .5, 0), (0, 0, 0, 0), (1, 1, 0, 0), (.5, .5, 1, 1), (.25, .5, .5, 1), (.5, .75, 1, .5)]
    boxes = edge + rng.random((40, 4)).astype(np.float32).tolist()
    for o in fv.ORIENTS:
        for b in boxes:
            view = rect + (o,)
            got = binding.view_box_to_frame(view, fw, fh, b)
            want = fv.box_to_frame(view, fw, fh, b)
            assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (o, b)
    # a box covering the view covers the rectangle; the view's corners go where the orient sends them
    for o in fv.ORIENTS:
        got = binding.view_box_to_frame(rect + (o,), fw, fh, (.5, .5, 1, 1)).astype(np.float64)
        assert np.allclose(got * [fw, fh, fw, fh], [33 + 150.5, 17 + 103.5, 301, 207], atol=1e-3)
    corner = {o: binding.view_box_to_frame(rect + (o,), fw, fh, (0, 0, 0, 0))[:2].astype(np.float64) * [fw, fh] for o in fv.ORIENTS}
    x1, y1 = 33 + 301, 17 + 207
    want = {1: (33, 17), 2: (x1, 17), 3: (x1, y1), 4: (33, y1), 5: (33, 17), 6: (33, y1), 7: (x1, y1), 8: (x1, 17)}
    assert all(np.allclose(corner[o], want[o], atol=1e-3) for o in fv.ORIENTS)
    # the pixel whose view coordinates are (u + .5, t + .5) is the pixel the index maps name
    for o in fv.ORIENTS:
        view = fv.View(2, 1, 4, 3, o)
        vw, vh = fv.view_size(view)
        for t in range(vh):
            for u in range(vw):
                c = binding.view_box_to_frame(view, 8, 6, ((u + .5) / vw, (t + .5) / vh, 0, 0))[:2].astype(np.float64) * [8, 6]
                x, y = fv.tap_to_frame(view, u, t)
                assert np.allclose(c, (x + .5, y + .5), atol=1e-5)
    assert np.array_equal(binding.view_box_to_frame(None, 8, 6, (.25, .5, .125, 1)), np.array([.25, .5, .125, 1], np.float32))


# ----------------------------------------------------------------------------------------------------------------------------- the merge
def _dets_of(records, classes):
    """detection arrays of slots from (box, objectness, probs) lists, through detections_from_records"""
    H = binding.host()
    B = len(records)
    rows, offsets = [], [0]
    for slot in records:
        for box, obj, probs in slot:
            rows.append([0, *box, obj, *probs])
        offsets.append(len(rows))
    recs = np.ascontiguousarray(np.array(rows, np.float32).reshape(-1, 6 + classes))
    dets, num = (C.c_void_p * B)(), (C.c_int * B)()
    H.detections_from_records(recs.ctypes.data, np.asarray(offsets, np.int32).ctypes.data, B, classes, C.c_float(0), dets, num)
    return dets, num


def _arrays(dets, num, f, classes):
    k = num[f]
    boxes, obj, probs = np.zeros((k, 4), np.float32), np.zeros(k, np.float32), np.zeros((k, classes), np.float32)
    binding.host().detections_to_arrays(dets[f], k, classes, boxes.ctypes.data, obj.ctypes.data, probs.ctypes.data)
    return boxes, obj, probs


def test_merge_maps_concatenates_and_suppresses_once_per_frame():
    H = binding.host()
    fw, fh, classes = 100, 60, 2
    views = binding.tile_views(fw, fh, 2, 1, 20)  # 60 wide, starts 0 and 40: columns 40..59 are seen twice
    assert views == [(0, 0, 60, 60, 1), (40, 0, 60, 60, 1)]
    own0, own1 = ((10 / 60, .5, 10 / 60, .2), .9, (.8, 0)), ((50 / 60, .5, 10 / 60, .2), .9, (0, .7))
    # one object at frame x = 50, seen by both tiles: at 50 in tile 0 and at 10 in tile 1
    both0, both1 = ((50 / 60, .25, 10 / 60, .2), .9, (.6, 0)), ((10 / 60, .25, 10 / 60, .2), .9, (.5, 0))
    records = [[own0, both0], [both1, own1], [own0], []]
    vs = _views(views + [(0, 0, 60, 60, 1), (0, 0, 100, 60, 1)])
    sizes = np.array([fw] * 4, np.int32), np.array([fh] * 4, np.int32)
    frame_of = np.array([0, 0, 2, 2], np.int32)
    for nms in (0.0, 0.45):
        sd, sn = _dets_of(records, classes)
        dets, num = (C.c_void_p * 4)(), (C.c_int * 4)()
        assert H.detections_views_merge(sd, sn, 4, vs, sizes[0].ctypes.data, sizes[1].ctypes.data, frame_of.ctypes.data, classes, C.c_float(nms),
                                        dets, num) == 0
        assert all(sd[b] is None and sn[b] == 0 for b in range(4)), "the slots' arrays are consumed"
        assert [num[f] for f in range(4)] == [4, 0, 1, 0] and dets[1] is None and dets[3] is None and dets[0] and dets[2]
        boxes, obj, probs = _arrays(dets, num, 0, classes)
        want = {(10., .8, 0.), (50., .6, 0.), (50., .5, 0.), (90., 0., .7)}
        if nms:
            want = {(10., .8, 0.), (50., .6, 0.), (50., 0., 0.), (90., 0., .7)}  # the weaker twin of the overlap's object is suppressed
        got = {(round(float(b[0]) * fw, 3), round(float(p[0]), 3), round(float(p[1]), 3)) for b, p in zip(boxes, probs)}
        assert got == want, (nms, got)
        for b in boxes:  # the same float32 values as the box call gives
            assert any(np.array_equal(b, binding.view_box_to_frame(v, fw, fh, r[0])) for v, slot in zip(views, records) for r in slot)
        assert np.allclose(boxes[:, 2] * fw, 10) and np.allclose(boxes[:, 3] * fh, 12)
        b2, _, p2 = _arrays(dets, num, 2, classes)
        assert np.allclose(b2[0] * [fw, fh, fw, fh], [10, 30, 10, 12]) and p2[0, 0] == np.float32(.8), "frame 2 is not merged with frame 0"
        H.free_detections_batch(dets, num, 4)
    # views == NULL: whole frames, boxes unchanged; a frame_of_slot outside the batch is refused and the slots are freed
    sd, sn = _dets_of(records, classes)
    dets, num = (C.c_void_p * 4)(), (C.c_int * 4)()
    ident = np.arange(4, dtype=np.int32)
    assert H.detections_views_merge(sd, sn, 4, None, sizes[0].ctypes.data, sizes[1].ctypes.data, ident.ctypes.data, classes, C.c_float(0), dets, num) == 0
    assert [num[f] for f in range(4)] == [2, 2, 1, 0] and dets[3]
    assert np.array_equal(_arrays(dets, num, 0, classes)[0], np.array([own0[0], both0[0]], np.float32))
    H.free_detections_batch(dets, num, 4)
    sd, sn = _dets_of(records, classes)
    bad = np.array([0, 4, 0, 0], np.int32)
    assert H.detections_views_merge(sd, sn, 4, vs, sizes[0].ctypes.data, sizes[1].ctypes.data, bad.ctypes.data, classes, C.c_float(0), dets, num) == EINVAL
    assert all(sd[b] is None for b in range(4)) and all(dets[f] is None for f in range(4))


def test_orient_6_turns_a_box_back():
    # view of the whole 100 x 60 frame under orient 6 is 60 x 100; an object at the view's top right is at the frame's top left
    got = binding.view_box_to_frame((0, 0, 100, 60, 6), 100, 60, (50 / 60, 10 / 100, 12 / 60, 8 / 100)).astype(np.float64) * [100, 60, 100, 60]
    assert np.allclose(got, [10, 10, 8, 12], atol=1e-4)


# -------------------------------------------------------------------------------------------------------------------------------- EXIF
def test_exif_orientation_of_built_segments():
    ex = binding.jpeg_exif_orientation
    for be in (False, True):
        for where in ("only", "first", "last"):
            for o in range(1, 9):
                assert ex(fv.jpeg_with([fv.exif_app1(o, be, where)])) == o, (be, where, o)
        assert ex(fv.jpeg_with([fv.exif_app1(6, be, "absent")])) == 1
        assert ex(fv.jpeg_with([fv.exif_app1(0, be)])) == 1 and ex(fv.jpeg_with([fv.exif_app1(9, be)])) == 1
        assert ex(fv.jpeg_with([fv.exif_app1(6, be, typ=4)])) == 1, "a LONG is not the tag's type"
        assert ex(fv.jpeg_with([fv.exif_app1(6, be, count=2)])) == 1
        assert ex(fv.jpeg_with([fv.exif_app1(6, be, ifd_offset=20)])) == 6, "an IFD that does not follow the header directly"
        seg = bytearray(fv.exif_app1(6, be))
        seg[14:18] = (5000).to_bytes(4, "big" if be else "little")  # the IFD offset, past the end of the segment
        assert ex(fv.jpeg_with([bytes(seg)])) == 1
        seg[14:18] = (0xFFFFFFFF).to_bytes(4, "little")
        assert ex(fv.jpeg_with([bytes(seg)])) == 1
        seg = bytearray(fv.exif_app1(6, be))
        seg[18:20] = (200).to_bytes(2, "big" if be else "little")  # more entries than the segment holds, the tag among the real ones
        assert ex(fv.jpeg_with([bytes(seg)])) == 6
        seg = bytearray(fv.exif_app1(6, be, "absent"))
        seg[18:20] = (200).to_bytes(2, "big" if be else "little")
        assert ex(fv.jpeg_with([bytes(seg)])) == 1
    good = fv.exif_app1(3)
    other_app1 = b"\xff\xe1\x00\x0ahttp://x"
    assert ex(fv.jpeg_with([other_app1, good])) == 3, "an APP1 that is no Exif block (XMP) is walked over"
    assert ex(fv.jpeg_with([b"\xff\xfe\x00\x04hi", b"\xff", good])) == 3, "a comment and a fill byte in front"
    assert ex(fv.jpeg_with([good], tail=b"")) == 3
    assert ex(fv.jpeg_with([])) == 1 and ex(b"") == 1 and ex(b"\xff\xd8") == 1 and ex(b"\x89PNG" + good) == 1
    assert ex(b"\xff\xd8\xff\xda\x00\x02" + good) == 1, "behind the scan nothing is looked for"
    assert ex(fv.jpeg_with([good.replace(b"II*\0", b"IM*\0")])) == 1 and ex(fv.jpeg_with([good.replace(b"II*\0", b"II+\0")])) == 1
    whole = fv.jpeg_with([good])
    cut = whole.index(b"Exif")
    assert {ex(whole[:n]) for n in range(cut + 30)} == {1}, "a segment whose length runs past the end is not read"
    assert [ex(whole[:n]) for n in (len(whole) - 7, len(whole) - 6, len(whole))] == [1, 3, 3], "complete exactly when the segment is"


def test_exif_orientation_of_pillow_written_files(tmp_path):
    from PIL import Image
    im = Image.fromarray(fv.rgb_frame(24, 16, 3))
    plain = io.BytesIO()
    im.save(plain, format="JPEG")
    assert binding.jpeg_exif_orientation(plain.getvalue()) == 1
    for o in range(1, 9):
        exif = im.getexif()
        exif[0x0112] = o
        buf = io.BytesIO()
        im.save(buf, format="JPEG", exif=exif)
        assert binding.jpeg_exif_orientation(buf.getvalue()) == o
        assert Image.open(io.BytesIO(buf.getvalue())).getexif()[0x0112] == o


def test_exif_reader_survives_hostile_input_under_sanitizers(tmp_path):
    """the stand-alone program (tests/jpeg_exif_fuzz_main.c + host/jpeg_exif.c) built with ASan + UBSan: built files in both byte orders as
    they are, every truncation of the first, 3000 seeded corruptions of each front; exit 0 and no report"""
    from PIL import Image
    exe = tmp_path / "jpeg_exif_fuzz"
    host = os.path.join(ROOT, "yolo_quantization_amd", "host")
    subprocess.run(["gcc", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all", "-I",
                    os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "jpeg_exif_fuzz_main.c"), os.path.join(host, "jpeg_exif.c"), "-o",
                    str(exe)], check=True)
    files = []
    blobs = [fv.jpeg_with([fv.exif_app1(6, False, "last")]), fv.jpeg_with([fv.exif_app1(8, True, "first")]),
             fv.jpeg_with([b"\xff\xe1\x00\x0ahttp://x", fv.exif_app1(3, True, ifd_offset=20)])]
    im = Image.fromarray(fv.rgb_frame(16, 8, 4))
    exif = im.getexif()
    exif[0x0112] = 5
    buf = io.BytesIO()
    im.save(buf, format="JPEG", exif=exif)
    blobs.append(buf.getvalue())
    for k, b in enumerate(blobs):
        p = tmp_path / f"exif_{k}.jpg"
        p.write_bytes(b)
        files.append(str(p))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe), "3000"] + files, capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-3000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.stdout.startswith("jpeg_exif_fuzz:")
