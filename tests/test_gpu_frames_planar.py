"""Frames of three separate planes (I420, YV12, I422, I444, planar RGB / BGR) through the batched device input path:
mi355_frames_planar_letterbox_minmax / _quantize (C-ABI), network_frames_planar_input_gpu (host), Net.prepare_from_frames_planar
(Python) and `detector test -frames i420 | yv12 | i422 | i444` (CLI).

Every comparison is exact: bytes and float bits, no tolerance.  The expected result of a frame never comes from the code under test:
it is what the NV12 calls give for the same Y plane and the interleaved chroma planes (I420), and what the u8 calls give for the
interleaved RGB frame that this file's numpy restatement of the sampling rule -- U[y >> sy][x >> sx] -- and the header's integer
formulas (yuv_to_rgb of frames_util) make of the planes.  Both of those paths are pinned to the oracle by their own tests."""
import functools
import os
import subprocess

import numpy as np
import pytest

import frames_util
from frames_util import (CFG, EINVAL, ROOT, SHIFTS, _assert_same_run, _bits, _blocks, _layers_and_dets, _padded, _write_ppm, _wts, plane_shapes,
                         yuv_to_rgb)
from yolo_quantization_amd import binding

pytestmark = pytest.mark.gpu

# fmt / matrix: one name for the batch or one per frame; pitch[b] = three pitches, rows padded with 0xEE bytes
_Launch = functools.partial(frames_util._Launch, "planar")
_LaunchNV12 = functools.partial(frames_util._Launch, "yuv")
_LaunchU8 = functools.partial(frames_util._Launch, "u8")
MATRICES = ["bt601", "bt601f", "bt709", "bt709f"]
FORMATS = ["i420", "yv12", "i422", "i444", "rgb", "bgr"]
# net size <- source sizes: odd widths and heights, so the last chroma column and row serve one luma column and row; up- and
# downscaling in one batch; letterbox bars on either axis; a width that is no multiple of 4; several workgroups per image
SHAPES = [(13, 11, [(9, 17)]), (52, 36, [(40, 30), (17, 50)]), (416, 416, [(640, 480)])]
SHAPE_IDS = ["w_not_multiple_of_4_odd_h", "letterbox_bars_up_and_down", "several_workgroups_per_image"]


@pytest.fixture(scope="module", autouse=True)
def _dev():
    binding.init(0)


def planar_to_rgb(planes, fmt, matrix="bt601", shifts=None):
    """interleaved RGB [h][w][3] of a frame: the planes in the order the format names them; pixel (x, y) of a YUV format takes
    Y[y][x], U[y >> sy][x >> sx], V[y >> sy][x >> sx] (nearest) and the integer formulas; RGB / BGR planes are stacked as they are.
    shifts: (sx, sy) other than the format's, for showing that a frame tells them apart"""
    if fmt in ("rgb", "bgr"):
        return np.ascontiguousarray(np.stack(planes if fmt == "rgb" else planes[::-1], axis=-1))
    y, u, v = planes if fmt != "yv12" else (planes[0], planes[2], planes[1])
    h, w = y.shape
    sx, sy = shifts or SHIFTS[fmt]
    rows, cols = (np.arange(h) >> sy)[:, None], (np.arange(w) >> sx)[None, :]
    return np.ascontiguousarray(yuv_to_rgb(y, u[rows, cols], v[rows, cols], MATRICES.index(matrix)))


def _frame(fmt, w, h, seed, lo=0, hi=256, clo=0, chi=256):
    """three random planes: plane 0 in lo..hi-1, planes 1 and 2 in clo..chi-1 (for rgb / bgr all three in lo..hi-1)"""
    rng = np.random.default_rng(seed)
    shp = plane_shapes(fmt, w, h)
    if fmt in ("rgb", "bgr"):
        clo, chi = lo, hi
    return tuple(rng.integers(a, b, s, dtype=np.uint8) for s, (a, b) in zip(shp, [(lo, hi), (clo, chi), (clo, chi)]))


def _run(cls, *a, **kw):
    L = cls(*a, **kw)
    got = L.run()
    L.free()
    return got


def _assert_same(got, want, what):
    """min / max words, scale bits, zero points and bytes of two launches"""
    for name, a, b in zip(("min / max", "scale", "zero point", "bytes"), got, want):
        a, b = (_bits(a), _bits(b)) if a.dtype == np.float32 else (a, b)
        assert a.shape == b.shape and np.array_equal(a, b), f"{what}: {name}"


def _interleave(u, v):
    return np.ascontiguousarray(np.stack([u, v], axis=-1))


# ------------------------------------------------------------------------------------------------------------ C-ABI level
@pytest.mark.parametrize("matrix", MATRICES)
@pytest.mark.parametrize("netw,neth,sources", SHAPES, ids=SHAPE_IDS)
def test_i420_equals_nv12_on_the_interleaved_chroma(netw, neth, sources, matrix):
    frames = [_frame("i420", w, h, 10 + k, 5 * k, 256 - 40 * k) for k, (w, h) in enumerate(sources)]
    got = _run(_Launch, frames, netw, neth, "i420", matrix)
    want = _run(_LaunchNV12, [(y, _interleave(u, v)) for y, u, v in frames], netw, neth, matrix=matrix)
    _assert_same(got, want, f"{netw}x{neth} <- {sources} {matrix}")
    assert len(np.unique(got[3])) > 16  # a real image, not a constant


def test_yv12_equals_i420_on_swapped_planes():
    frames = [_frame("i420", 40, 30, 31, 40, 200), _frame("i420", 17, 50, 32)]
    g420 = _run(_Launch, frames, 52, 36, "i420")
    g12 = _run(_Launch, [(y, v, u) for y, u, v in frames], 52, 36, "yv12")
    gx = _run(_Launch, frames, 52, 36, "yv12")  # the same planes read the other way round
    _assert_same(g12, g420, "yv12")
    _assert_same(gx, _run(_LaunchU8, [planar_to_rgb(f, "yv12") for f in frames], 52, 36), "yv12 on the unswapped planes")
    # the result really depends on the order: R and B change
    assert not np.array_equal(gx[3][0][0], g420[3][0][0]) and not np.array_equal(gx[3][0][2], g420[3][0][2])


@pytest.mark.parametrize("fmt", ["i422", "i444"])
@pytest.mark.parametrize("netw,neth,sources", SHAPES, ids=SHAPE_IDS)
def test_i422_and_i444_equal_u8_on_the_numpy_conversion(netw, neth, sources, fmt):
    """random chroma: every sample differs from its neighbours, so a sample taken at the wrong shift changes the frame"""
    frames = [_frame(fmt, w, h, 20 + k, 5 * k, 256 - 40 * k) for k, (w, h) in enumerate(sources)]
    matrix = MATRICES[(len(sources) + FORMATS.index(fmt)) % 4]
    rgb = [planar_to_rgb(f, fmt, matrix) for f in frames]
    for f, want in zip(frames, rgb):  # the expected frame tells this format's shifts from every larger one on either axis
        for wrong in [(1, 1)] + ([(1, 0), (0, 1)] if fmt == "i444" else []):
            assert not np.array_equal(planar_to_rgb(f, fmt, matrix, shifts=wrong), want)
    got = _run(_Launch, frames, netw, neth, fmt, matrix)
    _assert_same(got, _run(_LaunchU8, rgb, netw, neth), f"{fmt} {netw}x{neth} <- {sources}")


@pytest.mark.parametrize("matrix", MATRICES)
def test_conversion_sweep_every_chroma_pair_i444(matrix):
    """256 x 256 I444 frames into a 256 x 256 input, an identity letterbox: the chroma planes enumerate all 65 536 (U, V) pairs, each
    pixel having its own, at luma 0, 128 and 255 and, in a fourth frame, at random luma"""
    u, v = (np.ascontiguousarray(a) for a in np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij"))
    lumas = [np.full((256, 256), k, np.uint8) for k in (0, 128, 255)] + [np.random.default_rng(11).integers(0, 256, (256, 256), dtype=np.uint8)]
    frames = [(y, u, v) for y in lumas]
    rgb = [planar_to_rgb(f, "i444", matrix) for f in frames]
    allpx = np.concatenate([f.reshape(-1, 3) for f in rgb])
    for k in range(3):  # both clamp ends of every channel are reached
        assert allpx[:, k].min() == 0 and allpx[:, k].max() == 255
    got = _run(_Launch, frames, 256, 256, "i444", matrix)
    _assert_same(got, _run(_LaunchU8, rgb, 256, 256), matrix)
    # frame 3 spans 0..255 in every channel: scale 1 / 255, zero point 0, the quantised bytes are the converted bytes themselves
    assert got[2][3] == 0 and np.array_equal(got[3][3], rgb[3].transpose(2, 0, 1))


@pytest.mark.parametrize("fmt", ["rgb", "bgr"])
@pytest.mark.parametrize("netw,neth,sources", SHAPES, ids=SHAPE_IDS)
def test_planar_rgb_and_bgr_equal_u8_on_the_interleaved_frame(netw, neth, sources, fmt):
    frames = [_frame(fmt, w, h, 40 + k, 5 * k, 256 - 40 * k) for k, (w, h) in enumerate(sources)]
    inter = [np.ascontiguousarray(np.stack(f, axis=-1)) for f in frames]  # the planes in the order given
    got = _run(_Launch, frames, netw, neth, fmt)
    _assert_same(got, _run(_LaunchU8, inter, netw, neth, order=fmt), f"{fmt} {netw}x{neth}")
    assert not np.array_equal(got[3][0][0], got[3][0][2])  # the planes really differ
    if fmt == "bgr":  # and BGR is RGB on the reversed planes
        _assert_same(got, _run(_Launch, [f[::-1] for f in frames], netw, neth, "rgb"), "bgr against rgb")


@pytest.mark.parametrize("fmt", FORMATS)
def test_three_different_row_pitches(fmt):
    """all three planes carry their own padding (0xEE bytes), the chroma pitches odd: the tight frame's result"""
    sizes = [(53, 37), (9, 17)]
    frames = [_frame(fmt, w, h, 50 + k) for k, (w, h) in enumerate(sizes)]
    pitch = []
    for f in frames:
        p = [f[0].shape[1] + 5, f[1].shape[1] + 2, f[2].shape[1] + 9]
        p[1] += 1 - p[1] % 2  # odd
        p[2] += 1 - p[2] % 2
        assert len(set(a - b.shape[1] for a, b in zip(p, f))) == 3
        pitch.append(p)
    gp, gt = _run(_Launch, frames, 13, 11, fmt, pitch=pitch), _run(_Launch, frames, 13, 11, fmt)
    _assert_same(gp, gt, f"{fmt}: padded against tight")
    _assert_same(gp, _run(_LaunchU8, [planar_to_rgb(f, fmt) for f in frames], 13, 11), f"{fmt}: padded against u8")


def test_mixed_batch_of_all_six_formats_equals_single_frame_launches():
    sizes = [(53, 37), (12, 20), (5, 7), (12, 12), (31, 9), (9, 17)]
    ranges = [(0, 256, 0, 256), (16, 120, 100, 156), (60, 180, 90, 170), (0, 80, 120, 136), (100, 236, 0, 256), (30, 200, 0, 256)]
    matrix = ["bt601", "bt709", "bt601f", "bt709f", "bt601", "bt601"]
    frames = [_frame(f, w, h, 60 + k, *r) for k, (f, (w, h), r) in enumerate(zip(FORMATS, sizes, ranges))]
    mm, s, z, q = _run(_Launch, frames, 12, 12, FORMATS, matrix)
    assert len(set(zip(s.tolist(), z.tolist()))) >= 3
    rgb = [planar_to_rgb(f, fmt, m) for f, fmt, m in zip(frames, FORMATS, matrix)]
    want = _run(_LaunchU8, rgb, 12, 12)
    for b, f in enumerate(frames):
        one = _run(_Launch, [f], 12, 12, FORMATS[b], matrix[b])
        _assert_same((mm[b:b + 1], s[b:b + 1], z[b:b + 1], q[b:b + 1]), one, f"slot {b} ({FORMATS[b]}) against its own launch")
        _assert_same(one, tuple(x[b:b + 1] for x in want), f"slot {b} ({FORMATS[b]}) against u8")


REFUSED = ["null_plane_0", "null_plane_2", "pitch_0_below_w", "chroma_pitch_below_its_width_i420", "chroma_pitch_below_its_width_i444",
           "unknown_format", "unknown_matrix", "matrix_on_rgb", "resized_side_below_2"]


@pytest.mark.parametrize("what", REFUSED)
def test_refusals_launch_nothing(what):
    fmt = "i444" if what.endswith("i444") else ("rgb" if what == "matrix_on_rgb" else "i420")
    good = _frame(fmt, 12, 20, 71)
    bad = _frame(fmt, 1, 40, 72) if what == "resized_side_below_2" else _frame(fmt, 9, 17, 72)
    L = _Launch([good, bad], 12, 12, fmt)
    t = L.table[1]
    if what.startswith("null_plane"):
        t.plane[int(what[-1])] = None
    if what == "pitch_0_below_w":
        t.pitch[0] = 8
    if what == "chroma_pitch_below_its_width_i420":
        t.pitch[2] = 4  # (9 + 1) / 2 - 1
    if what == "chroma_pitch_below_its_width_i444":
        t.pitch[1] = 8  # a 4:2:0 pitch would pass here
    if what == "unknown_format":
        t.format = 6
    if what == "unknown_matrix":
        t.matrix = 4
    if what == "matrix_on_rgb":
        t.matrix = 1
    L.upload_table()
    mm_before = L.mm.to_numpy(np.float32, 4)
    assert L.minmax_rc() == EINVAL
    assert binding.shim().mi355_last_error().startswith(b"invalid argument: frames_planar:")  # the prefix every MI355_EINVAL carries
    assert L.quantize_rc([1 / 255.0, 1 / 255.0], [0, 0]) == EINVAL
    assert binding.shim().mi355_last_error().startswith(b"invalid argument: frames_planar:")
    binding.check(binding.shim().mi355_stream_sync(None), "sync")
    assert np.all(L.out_bytes() == 0xA5)  # the pattern the output buffer was filled with
    assert np.array_equal(_bits(L.mm.to_numpy(np.float32, 4)), _bits(mm_before))
    L.free()


# ------------------------------------------------------------------------------------------------------------ host level
def _host_frames(fmt, seed):
    """three frames of different sizes, luma and chroma ranges (w x h: wide, tall, network size)"""
    specs = [((53, 37), 0, 256, 0, 256), ((12, 20), 40, 140, 100, 156), ((12, 12), 100, 200, 120, 136)]
    return [_frame(fmt, w, h, seed + k, lo, hi, clo, chi) for k, ((w, h), lo, hi, clo, chi) in enumerate(specs)]


def _prepare_other_path(net, frames, fmt, matrix):
    """the same frames through the entry point that is the reference for this format: NV12 for i420, u8 for everything"""
    if fmt == "i420":
        return net.prepare_from_frames_nv12([(y, _interleave(u, v)) for y, u, v in frames], matrix=matrix)
    return net.prepare_from_frames_u8([planar_to_rgb(f, fmt, matrix) for f in frames])


def _same_prepared(got, want, what):
    got, want = (got, want) if isinstance(got, tuple) else ((got,), (want,))
    assert len(got) == len(want)
    for a, b in zip(got, want):
        a, b = (_bits(a), _bits(b)) if a.dtype == np.float32 else (a, b)
        assert np.array_equal(a, b), what


@pytest.mark.parametrize("fmt,matrix", [("i420", "bt601"), ("i444", "bt709"), ("rgb", "bt601")])
def test_host_shared_scale_equals_the_other_paths_and_rederives_layer0(tmp_path, fmt, matrix):
    wts = _wts(tmp_path)
    a, b = binding.Net(CFG, wts, batch=3, dump_int32=True), binding.Net(CFG, wts, batch=3, dump_int32=True)
    pairs = []
    for seed, rot in ((100, 0), (200, 1)):  # the second batch starts with another image: another pair, layer 0 is re-derived
        frames = _host_frames(fmt, seed)
        frames = frames[rot:] + frames[:rot]
        rgb = [planar_to_rgb(f, fmt, matrix) for f in frames]
        xa = a.prepare_from_frames_planar(frames, format=fmt, matrix=matrix)
        xb = _prepare_other_path(b, frames, fmt, matrix)
        _same_prepared(xa, xb, f"batch {seed}: uint8 input")
        sa, za = a.input_quantization()
        sb, zb = b.input_quantization()
        assert np.array_equal(_bits(sa), _bits(sb)) and np.array_equal(za, zb)
        pairs.append((float(sa[0]), int(za[0])))
        _assert_same_run(_layers_and_dets(a, rgb), _layers_and_dets(b, rgb), f"batch {seed}")
    assert pairs[0] != pairs[1]
    a.close(); b.close()


@pytest.mark.parametrize("fmt,matrix", [("i420", "bt709"), ("i444", "bt601f"), ("rgb", "bt601")])
def test_host_per_image_equals_the_other_paths(tmp_path, fmt, matrix):
    wts = _wts(tmp_path, seed=4)
    a, b = binding.Net(CFG, wts, batch=3, dump_int32=True), binding.Net(CFG, wts, batch=3, dump_int32=True)
    a.set_input_per_image(True)
    b.set_input_per_image(True)
    frames = _host_frames(fmt, 300)
    rgb = [planar_to_rgb(f, fmt, matrix) for f in frames]
    got = a.prepare_from_frames_planar(frames, format=fmt, matrix=matrix)
    _same_prepared(got, _prepare_other_path(b, frames, fmt, matrix), fmt)
    assert len(set(got[1].tolist())) == 3  # the scales really differ
    _assert_same_run(_layers_and_dets(a, rgb), _layers_and_dets(b, rgb), "per image")
    a.close(); b.close()


def test_host_graph_replay_per_image(tmp_path):
    wts = _wts(tmp_path, seed=2)
    net = binding.Net(CFG, wts, batch=3, use_graph=True)
    net.set_input_per_image(True)
    n1 = binding.Net(CFG, wts, batch=1)
    handle = None
    for seed, fmt in ((500, "i420"), (600, "i422")):
        frames = _host_frames(fmt, seed)
        xq, s, z = net.prepare_from_frames_planar(frames, format=fmt)
        net.forward()
        net.sync()
        outs = [net.pull(i) for i in range(net.n)]
        if handle is None:
            handle = net.graph_handle()
            assert handle
        assert net.graph_handle() == handle  # the same captured graph replays the second batch
        for b, f in enumerate(frames):
            x1 = n1.prepare_from_frames_u8([planar_to_rgb(f, fmt)])
            assert np.array_equal(xq[b * net.inputs:(b + 1) * net.inputs], x1)
            n1.forward()
            n1.sync()
            for i, inf in enumerate(net.info):
                per = inf["outputs"]
                w1 = n1.pull(i)
                for k in w1:
                    if k in outs[i]:
                        assert np.array_equal(outs[i][k][b * per:(b + 1) * per], w1[k]), f"seed {seed} slot {b} layer {i} {k}"
    n1.close()
    net.close()


def test_host_replica_beside_its_parent(tmp_path):
    wts = _wts(tmp_path, seed=6)
    parent = binding.Net(CFG, wts, batch=3)
    parent.set_input_per_image(True)
    ref = binding.Net(CFG, wts, batch=3)
    ref.set_input_per_image(True)
    fp, fr = _host_frames("i420", 700), _host_frames("yv12", 800)
    parent.prepare_from_frames_planar(fp)
    rep = parent.replica()
    xr, sr, zr = rep.prepare_from_frames_planar(fr, format="yv12")  # its own arena, table and bank
    xp, sp, zp = parent.prepare_from_frames_planar(fp)
    for _ in range(3):  # both executors queued side by side
        parent.forward()
        rep.forward()
    for net, fmt, frames, x, s, z in ((parent, "i420", fp, xp, sp, zp), (rep, "yv12", fr, xr, sr, zr)):
        net.sync()
        xw, sw, zw = ref.prepare_from_frames_u8([planar_to_rgb(f, fmt) for f in frames])
        assert np.array_equal(x, xw) and np.array_equal(_bits(s), _bits(sw)) and np.array_equal(z, zw)
        ref.forward()
        ref.sync()
        for i in range(net.n):
            got, want = net.pull(i), ref.pull(i)
            for k in want:
                if k in got:
                    assert np.array_equal(got[k], want[k]), f"layer {i} {k}"
    rep.close()
    ref.close()
    parent.close()


@pytest.mark.parametrize("fmt", ["i420", "i422", "bgr"])
def test_host_frames_on_device_equal_the_upload_path(tmp_path, fmt):
    """planes a decoder left in device memory are used in place"""
    wts = _wts(tmp_path, seed=7)
    net = binding.Net(CFG, wts, batch=3)
    net.set_input_per_image(True)
    frames = _host_frames(fmt, 900)
    want = net.prepare_from_frames_planar(frames, format=fmt)
    bufs, dev = [], []
    for f in frames:
        h, w = f[0].shape
        pitch = [f[0].shape[1] + 3, f[1].shape[1], f[2].shape[1] + 1]
        b3 = [binding.DevBuf.from_numpy(_padded(p, q)) for p, q in zip(f, pitch)]
        bufs += b3
        dev.append(tuple(x.ptr.value for x in b3) + (w, h) + tuple(pitch))
    got = net.prepare_from_frames_planar(dev, format=fmt, on_device=True)
    _same_prepared(got, want, fmt)
    ref = binding.Net(CFG, wts, batch=3)
    ref.set_input_per_image(True)
    _same_prepared(got, ref.prepare_from_frames_u8([planar_to_rgb(f, fmt) for f in frames]), f"{fmt} against u8")
    ref.close()
    net.close()
    for b in bufs:
        b.free()


def test_host_strided_planes_through_python(tmp_path):
    """rows of wider buffers are passed through as pitches (no copy); columns taken with a step are copied by the binding"""
    wts = _wts(tmp_path, seed=5)
    frames = _host_frames("i420", 400)
    views, stepped = [], []
    for f in frames:
        v3, s3 = [], []
        for k, p in enumerate(f):
            wide = np.full((p.shape[0], p.shape[1] + 3 + 2 * k), 0xEE, np.uint8)
            wide[:, :p.shape[1]] = p
            v = wide[:, :p.shape[1]]
            assert not v.flags["C_CONTIGUOUS"] and v.strides == (p.shape[1] + 3 + 2 * k, 1)
            v3.append(v)
            two = np.full((p.shape[0], 2 * p.shape[1]), 0xEE, np.uint8)
            two[:, ::2] = p
            s3.append(two[:, ::2])
        views.append(tuple(v3)); stepped.append(tuple(s3))
    net = binding.Net(CFG, wts, batch=3)
    net.set_input_per_image(True)
    want = net.prepare_from_frames_planar(frames)
    _same_prepared(net.prepare_from_frames_planar(views), want, "row strides")
    _same_prepared(net.prepare_from_frames_planar(stepped), want, "column steps")
    ref = binding.Net(CFG, wts, batch=3)
    ref.set_input_per_image(True)
    _same_prepared(want, ref.prepare_from_frames_nv12([(y, _interleave(u, v)) for y, u, v in frames]), "against nv12")
    with pytest.raises(ValueError):
        net.prepare_from_frames_planar([(y, u[:, :-1], v) for y, u, v in frames])  # a chroma plane of another size
    ref.close()
    net.close()


@pytest.mark.parametrize("fmt", ["rgb", "bgr"])
def test_host_chw_array_for_planar_rgb(tmp_path, fmt):
    """a uint8 [3][h][w] array, as a decoded tensor is laid out, is split along axis 0"""
    wts = _wts(tmp_path, seed=8)
    net, ref = binding.Net(CFG, wts, batch=3), binding.Net(CFG, wts, batch=3)
    frames = _host_frames(fmt, 1000)
    chw = [np.ascontiguousarray(np.stack(f)) for f in frames]
    assert all(c.shape == (3,) + f[0].shape for c, f in zip(chw, frames))
    got = net.prepare_from_frames_planar(chw, format=fmt)
    _same_prepared(got, net.prepare_from_frames_planar(frames, format=fmt), "tuple of planes")
    rgb = [planar_to_rgb(f, fmt) for f in frames]
    _same_prepared(got, ref.prepare_from_frames_u8(rgb), "u8")
    sa, sb = net.input_quantization(), ref.input_quantization()
    assert np.array_equal(_bits(sa[0]), _bits(sb[0])) and np.array_equal(sa[1], sb[1])
    with pytest.raises(ValueError):
        net.prepare_from_frames_planar(chw, format="i444")  # one array is not three YUV planes
    net.close(); ref.close()


class _DeviceTensor:
    """what Net.prepare_from_frames_planar asks of a device tensor (torch's names), over a buffer this library allocated: a uint8
    [3][h][w] view of rows `pitch` bytes apart"""

    def __init__(self, chw, pitch):
        c, h, w = chw.shape
        rows = np.full((c, h, pitch), 0xEE, np.uint8)
        rows[:, :, :w] = chw
        self.buf = binding.DevBuf.from_numpy(rows)
        self.shape, self._stride = (c, h, w), (h * pitch, pitch, 1)

    def data_ptr(self):
        return self.buf.ptr.value

    def stride(self, k):
        return self._stride[k]

    def element_size(self):
        return 1


def test_host_device_tensor_for_planar_rgb(tmp_path):
    """a uint8 [3][h][w] tensor in device memory (the layout of a decoded image) is used in place, a row-strided one too"""
    wts = _wts(tmp_path, seed=9)
    net = binding.Net(CFG, wts, batch=3)
    net.set_input_per_image(True)
    frames = _host_frames("bgr", 1100)
    want = net.prepare_from_frames_planar(frames, format="bgr")
    for extra in (0, 5):
        tensors = [_DeviceTensor(np.stack(f), f[0].shape[1] + extra) for f in frames]
        _same_prepared(net.prepare_from_frames_planar(tensors, format="bgr", on_device=True), want, f"row padding {extra}")
        with pytest.raises(ValueError):
            net.prepare_from_frames_planar(tensors, format="i444", on_device=True)  # one tensor is not three YUV planes
        for t in tensors:
            t.buf.free()
    net.close()


# ------------------------------------------------------------------------------------------------------------------- CLI
SPECS = [((37, 53), 0, 256, 0, 256), ((24, 24), 40, 140, 100, 156), ((30, 17), 100, 230, 60, 200), ((13, 15), 0, 90, 120, 136)]  # (h, w), ranges


@pytest.fixture
def cli(tmp_path):
    """run(args) -> the output blocks of `detector test`; run(args, ok=False) -> the finished process"""
    exe = os.path.join(ROOT, "yolo_quantization_amd", "bin", "darknet")
    wts = _wts(tmp_path, seed=1)
    names = str(tmp_path / "x.names")
    open(names, "w").write("\n".join(["ant", "bee", "cat", "dog", "eel"]) + "\n")
    data = str(tmp_path / "x.data")
    open(data, "w").write(f"classes= 5\nnames = {names}\n")

    def run(extra, ok=True):
        r = subprocess.run([exe, "detector", "test", data, CFG, wts] + extra + ["-thresh", "0.3", "-boxes"], capture_output=True, text=True,
                           timeout=300)
        if not ok:
            return r
        assert r.returncode == 0, r.stderr
        return _blocks(r.stdout)
    return run


def _write_list(path, entries):
    open(path, "w").write("\n".join(entries) + "\n")
    return str(path)


def test_cli_frames_i420_blocks_equal_nv12_on_the_reinterleaved_files(tmp_path, cli):
    i420s, nv12s, frames = [], [], []
    for k, ((h, w), lo, hi, clo, chi) in enumerate(SPECS):
        y, u, v = _frame("i420", w, h, 80 + k, lo, hi, clo, chi)
        p420, p12 = str(tmp_path / f"im{k}_{w}x{h}.i420"), str(tmp_path / f"im{k}_{w}x{h}.nv12")
        open(p420, "wb").write(y.tobytes() + u.tobytes() + v.tobytes())
        open(p12, "wb").write(y.tobytes() + _interleave(u, v).tobytes())  # the same frame, re-interleaved
        i420s.append(p420); nv12s.append(p12); frames.append((y, u, v))
    want = cli(["-list", _write_list(tmp_path / "nv12.txt", nv12s), "-batch", "3", "-frames", "nv12"])
    got = cli(["-list", _write_list(tmp_path / "i420.txt", i420s), "-batch", "3", "-frames", "i420"])
    assert [g[0] for g in got] == i420s and [w[0] for w in want] == nv12s
    assert [g[1:] for g in got] == [w[1:] for w in want]  # apart from the file names
    assert any(line.startswith("box:") for blk in want for line in blk)
    single = cli([i420s[0], "-frames", "i420"])[0][1:]
    assert single == cli([nv12s[0], "-frames", "nv12"])[0][1:]  # the single image too
    # YV12: the same bytes with the chroma planes in the other order
    y, u, v = frames[0]
    pyv = str(tmp_path / "im0_53x37.yv12")
    open(pyv, "wb").write(y.tobytes() + v.tobytes() + u.tobytes())
    assert cli([pyv, "-frames", "yv12"])[0][1:] == single
    # a file of the wrong length (alone and in a list), a name without a size, another format's extension, an unknown format:
    # refused, the first four with the reader's message
    short = str(tmp_path / "short_53x37.i420")
    open(short, "wb").write(open(i420s[0], "rb").read()[:-1])
    n = 53 * 37 + 2 * 19 * 27
    for args in ([short], ["-list", _write_list(tmp_path / "short.txt", [i420s[1], short]), "-batch", "3"]):
        r = cli(args + ["-frames", "i420"], ok=False)
        assert r.returncode != 0 and f"holds {n} bytes, the file holds {n - 1}" in r.stderr
    nosize = str(tmp_path / "nosize.i420")
    open(nosize, "wb").write(open(i420s[0], "rb").read())
    r = cli([nosize, "-frames", "i420"], ok=False)
    assert r.returncode != 0 and "_<W>x<H>.i420" in r.stderr
    r = cli([i420s[0], "-frames", "i444"], ok=False)
    assert r.returncode != 0 and "_<W>x<H>.i444" in r.stderr
    r = cli([i420s[0], "-frames", "rgb"], ok=False)
    assert r.returncode != 0 and "-frames:" in r.stderr and "i420" in r.stderr


@pytest.mark.parametrize("fmt", ["i444", "i422"])
def test_cli_frames_i444_and_i422_with_a_matrix_equal_u8_on_the_converted_ppm(tmp_path, cli, fmt):
    raws, ppms = [], []
    for k, ((h, w), lo, hi, clo, chi) in enumerate(SPECS):
        f = _frame(fmt, w, h, 90 + k, lo, hi, clo, chi)
        raw, ppm = str(tmp_path / f"im{k}_{w}x{h}.{fmt}"), str(tmp_path / f"im{k}.ppm")
        open(raw, "wb").write(b"".join(p.tobytes() for p in f))
        _write_ppm(ppm, planar_to_rgb(f, fmt, "bt709f"))
        raws.append(raw); ppms.append(ppm)
    got = cli(["-list", _write_list(tmp_path / "raw.txt", raws), "-batch", "3", "-frames", fmt, "-matrix", "bt709f"])
    want = cli(["-list", _write_list(tmp_path / "ppm.txt", ppms), "-batch", "3", "-frames", "u8"])
    assert [g[0] for g in got] == raws and [g[1:] for g in got] == [w[1:] for w in want]
    assert any(line.startswith("box:") for blk in want for line in blk)
    assert cli([raws[0], "-frames", fmt, "-matrix", "bt709f"])[0][1:] == cli([ppms[0], "-frames", "u8"])[0][1:]  # the single image too
