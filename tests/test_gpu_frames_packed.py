"""Packed frames (RGBA, BGRA, ARGB, ABGR; YUYV, UYVY, YVYU) and P010 frames through the batched device input path:
mi355_frames_packed_* / mi355_frames_p010_* (C-ABI), network_frames_packed_input_gpu / network_frames_p010_input_gpu (host),
Net.prepare_from_frames_packed / _p010 (Python) and `detector test -frames rgba | ... | yvyu | p010` (CLI).

Every comparison is exact: bytes and float bits, no tolerance.  The expected result of a frame never comes from the code under test:
the numpy converters of frames_packed_util (the specification, checked against a per-pixel loop by test_frames_packed_cpu.py) turn
it into a frame of a kind the project served before, and the sibling call gives the result -- the u8 calls on rgbx_to_rgb, the
planar calls with MI355_PLANAR_I422 on yuv422_to_planes, the NV12 calls on p010_to_nv12.  Those paths are pinned to the oracle by
their own tests.  The network input is tiny_unit.cfg's 12 x 12; the sources are the smallest at which these sources can go wrong."""
import functools
import os
import subprocess

import numpy as np
import pytest

import frames_util
from frames_packed_util import (MATRICES, RGBX, UNUSED, YUV422, Launch, assert_same, geometry_accepts, p010_frame, p010_to_nv12, p010_to_rgb,
                                packed_frame, packed_to_rgb, rgbx_to_rgb, run, yuv422_to_planes)
from frames_util import CFG, EINVAL, ROOT, _assert_same_run, _bits, _blocks, _layers_and_dets, _write_ppm, _wts
from yolo_quantization_amd import binding

pytestmark = pytest.mark.gpu

NET = 12  # the network input is NET x NET
# w x h: wide, odd both ways, downscaled (last macropixel half used, last chroma row and column of P010 shared) | tall | no resize |
# upscaled (two taps inside one macropixel and across two) | the smallest frames the geometry accepts
BATCHES = [[(53, 37), (12, 20), (12, 12)], [(5, 3), (2, 2), (3, 2)]]
REFUSED_SIZES = [(1, 7), (7, 1)]
PACKED = list(RGBX) + list(YUV422)
_LaunchU8 = functools.partial(frames_util._Launch, "u8")
_LaunchPlanar = functools.partial(frames_util._Launch, "planar")
_LaunchNV12 = functools.partial(frames_util._Launch, "yuv")


@pytest.fixture(scope="module", autouse=True)
def _dev():
    binding.init(0)


def test_the_sizes_are_what_the_geometry_accepts_and_refuses():
    assert all(geometry_accepts(w, h, NET, NET) for batch in BATCHES for w, h in batch)
    assert not any(geometry_accepts(w, h, NET, NET) for w, h in REFUSED_SIZES)
    assert geometry_accepts(1, 1, NET, NET) and not geometry_accepts(2, 13, NET, NET)  # served: both resized sides reach 2; refused: one is 1


def _sibling_packed(frames, fmt, matrix):
    """the result of the batch from the calls that served these pixels before"""
    if fmt in RGBX:
        return run(_LaunchU8, [rgbx_to_rgb(f.reshape(f.shape[0], w, 4), fmt) for f, w in frames], NET, NET)
    return run(_LaunchPlanar, [yuv422_to_planes(f, w, fmt) for f, w in frames], NET, NET, "i422", matrix)


# ------------------------------------------------------------------------------------------------------------ C-ABI level
@pytest.mark.parametrize("fmt", PACKED)
def test_packed_equals_the_sibling_call_on_the_converted_frames(fmt):
    """a group is one 4-byte load at any alignment: tight pitch (a multiple of 4), pitch + 8 and pitch + 5, each at an aligned and at an
    odd address"""
    for n, sizes in enumerate(BATCHES):
        frames = [(packed_frame(fmt, w, h, 100 * n + k), w) for k, (w, h) in enumerate(sizes)]
        for matrix in ["bt601"] if fmt in RGBX else MATRICES:
            want = _sibling_packed(frames, fmt, matrix)
            assert len(np.unique(want[3])) > 16  # a real image, not a constant
            got = {(extra, offset): run(Launch, "packed", frames, NET, NET, fmt, matrix, extra=extra, offset=offset)
                   for extra in (0, 5, 8) for offset in (0, 1)}
            for how, g in got.items():
                assert_same(g, want, f"{fmt} {matrix} {sizes} pitch + {how[0]}, address + {how[1]}")
            assert_same(got[0, 0], got[0, 1], f"{fmt} {matrix} {sizes}: aligned against unaligned groups")


def test_packed_formats_differ_where_they_must():
    """the same bytes read as another format give another image: the expected frames tell the formats apart"""
    f = packed_frame("rgba", 12, 12, 7)
    rgb = {fmt: packed_to_rgb(f, 12 if fmt in RGBX else 24, fmt) for fmt in PACKED}
    for a in RGBX:
        for b in RGBX:
            assert a == b or not np.array_equal(rgb[a], rgb[b])
    for a in YUV422:
        for b in YUV422:
            assert a == b or not np.array_equal(rgb[a], rgb[b])


@pytest.mark.parametrize("matrix", MATRICES)
def test_p010_equals_nv12_on_the_high_bytes(matrix):
    for n, sizes in enumerate(BATCHES):
        bits = (10, 12, 16)  # P010, P012, P016: the significant bits at the top
        frames = [p010_frame(w, h, 200 * n + k, bits[k]) for k, (w, h) in enumerate(sizes)]
        want = run(_LaunchNV12, [p010_to_nv12(*f) for f in frames], NET, NET, matrix=matrix)
        assert len(np.unique(want[3])) > 16
        for extra in (0, 6):
            for offset in (0, 1):  # single bytes are loaded: an odd address is as good as any
                got = run(Launch, "p010", frames, NET, NET, matrix=matrix, extra=extra, offset=offset)
                assert_same(got, want, f"{matrix} {sizes} pitch + {extra}, address + {offset}")


def _zeroed_packed(f, w, fmt):
    """the frame with every byte that must not matter set to zero"""
    z = f.copy()
    if fmt in RGBX:
        z.reshape(f.shape[0], w, 4)[:, :, UNUSED[fmt]] = 0
    elif w % 2:
        z[:, 4 * ((w + 1) // 2 - 1) + YUV422[fmt][1]] = 0  # Y1 of the last macropixel
    return z


@pytest.mark.parametrize("fmt", PACKED + ["p010"])
def test_bytes_that_must_not_matter_do_not(fmt):
    """the fourth byte of a pixel, the unused luma byte of an odd-width row's last macropixel, the low bytes of P010 samples and the row
    padding: random, then zero -- the same outputs"""
    sizes = BATCHES[0][:1] + BATCHES[1][:1] + BATCHES[1][2:]  # 53 x 37, 5 x 3, 3 x 2: odd widths
    rng = np.random.default_rng(5)
    if fmt == "p010":
        noisy = [tuple(rng.integers(0, 65536, p.shape, dtype=np.uint16) for p in p010_frame(w, h, 0)) for w, h in sizes]
        clean = [tuple(p & 0xFF00 for p in f) for f in noisy]
        assert all(not np.array_equal(a, b) for f, g in zip(noisy, clean) for a, b in zip(f, g))
        kind, how, extra = "p010", dict(matrix="bt709"), 6
    else:
        noisy = [(packed_frame(fmt, w, h, 300 + k), w) for k, (w, h) in enumerate(sizes)]
        clean = [(_zeroed_packed(f, w, fmt), w) for f, w in noisy]
        assert all(not np.array_equal(f[0], g[0]) for f, g in zip(noisy, clean))
        kind, how, extra = "packed", dict(format=fmt, matrix="bt601f"), 5
    want = run(Launch, kind, clean, NET, NET, extra=extra, pad=0, **how)
    for offset in (0, 1):
        assert_same(run(Launch, kind, noisy, NET, NET, extra=extra, offset=offset, pad=rng, **how), want, f"{fmt} address + {offset}: random")
        assert_same(run(Launch, kind, clean, NET, NET, extra=extra, offset=offset, pad=0, **how), want, f"{fmt} address + {offset}: zero")
    assert_same(run(Launch, kind, noisy, NET, NET, **how), want, f"{fmt} tight rows")


# what, the kind, the format, the size of the frame in slot 1, the change to its table entry, what the message says
REFUSED = [("packed_null_data", "packed", "bgra", (9, 17), lambda t: setattr(t, "data", None), "null frame pointer"),
           ("packed_w_zero", "packed", "bgra", (9, 17), lambda t: setattr(t, "w", 0), "need 1 <= w, h <= 32768"),
           ("packed_h_beyond_32768", "packed", "yuyv", (9, 17), lambda t: setattr(t, "h", 32769), "need 1 <= w, h <= 32768"),
           ("packed_rgbx_pitch_one_below_minimum", "packed", "argb", (9, 17), lambda t: setattr(t, "pitch", 35), "pitch < 4 * w"),
           ("packed_422_pitch_one_below_minimum", "packed", "uyvy", (9, 17), lambda t: setattr(t, "pitch", 19), "pitch < 4 * ((w + 1) / 2)"),
           ("packed_unknown_format", "packed", "yvyu", (9, 17), lambda t: setattr(t, "format", 7), "unknown format"),
           ("packed_negative_format", "packed", "rgba", (9, 17), lambda t: setattr(t, "format", -1), "unknown format"),
           ("packed_unknown_matrix", "packed", "yuyv", (9, 17), lambda t: setattr(t, "matrix", 4), "unknown matrix"),
           ("packed_matrix_on_bgra", "packed", "bgra", (9, 17), lambda t: setattr(t, "matrix", 1), "matrix must be 0"),
           ("packed_rgbx_1x7", "packed", "abgr", (1, 7), None, "degenerate aspect (resized side < 2)"),
           ("packed_422_7x1", "packed", "yuyv", (7, 1), None, "degenerate aspect (resized side < 2)"),
           ("packed_422_1x7", "packed", "uyvy", (1, 7), None, "degenerate aspect (resized side < 2)"),
           ("p010_null_y", "p010", None, (9, 17), lambda t: setattr(t, "y", None), "null plane pointer"),
           ("p010_null_uv", "p010", None, (9, 17), lambda t: setattr(t, "uv", None), "null plane pointer"),
           ("p010_w_beyond_32768", "p010", None, (9, 17), lambda t: setattr(t, "w", 32769), "need 1 <= w, h <= 32768"),
           ("p010_luma_pitch_one_below_minimum", "p010", None, (9, 17), lambda t: setattr(t, "pitch_y", 17), "pitch_y < 2 * w"),
           ("p010_chroma_pitch_one_below_minimum", "p010", None, (9, 17), lambda t: setattr(t, "pitch_uv", 19), "pitch_uv < 4 * ((w + 1) / 2)"),
           ("p010_unknown_matrix", "p010", None, (9, 17), lambda t: setattr(t, "matrix", 4), "unknown matrix"),
           ("p010_layout_set", "p010", None, (9, 17), lambda t: setattr(t, "layout", 1), "layout and reserved must be 0"),
           ("p010_reserved_set", "p010", None, (9, 17), lambda t: t.reserved.__setitem__(1, 1), "layout and reserved must be 0"),
           ("p010_1x7", "p010", None, (1, 7), None, "degenerate aspect (resized side < 2)"),
           ("p010_7x1", "p010", None, (7, 1), None, "degenerate aspect (resized side < 2)")]


@pytest.mark.parametrize("what,kind,fmt,size,change,message", REFUSED, ids=[r[0] for r in REFUSED])
def test_refusals_launch_nothing(what, kind, fmt, size, change, message):
    """MI355_EINVAL with the sibling's wording behind this kind's prefix, from both calls, and nothing was written"""
    frame = (lambda w, h, s: (packed_frame(fmt, w, h, s), w)) if kind == "packed" else p010_frame
    L = Launch(kind, [frame(12, 20, 71), frame(*size, 72)], NET, NET, fmt)
    if change:
        change(L.table[1])
    L.upload_table()
    mm_before = L.mm.to_numpy(np.float32, 4)
    prefix = f"invalid argument: frames_{kind}: ".encode()
    assert L.minmax_rc() == EINVAL
    assert binding.shim().mi355_last_error().startswith(prefix + message.encode())
    assert L.quantize_rc([1 / 255.0, 1 / 255.0], [0, 0]) == EINVAL
    assert binding.shim().mi355_last_error().startswith(prefix + message.encode())
    binding.check(binding.shim().mi355_stream_sync(None), "sync")
    assert np.all(L.out_bytes() == 0xA5)  # the pattern the output buffer was filled with
    assert np.array_equal(_bits(L.mm.to_numpy(np.float32, 4)), _bits(mm_before))
    L.free()


# ------------------------------------------------------------------------------------------------------------ host level
SIZES = BATCHES[0]
HOST_KINDS = [("bgra", "bt601"), ("argb", "bt601"), ("yuyv", "bt709"), ("uyvy", "bt601f"), ("p010", "bt709f")]


def _host_frames(kind, seed, sizes=SIZES):
    """a batch as the Python methods take it: uint8 [h][w][4] | (uint8 [h][row_bytes], w) | (y16, uv16) with noisy low bytes"""
    if kind == "p010":
        rng = np.random.default_rng(seed)
        return [tuple(rng.integers(0, 65536, p.shape, dtype=np.uint16) for p in p010_frame(w, h, 0)) for w, h in sizes]
    frames = [packed_frame(kind, w, h, seed + k) for k, (w, h) in enumerate(sizes)]
    return [f.reshape(h, w, 4) for f, (w, h) in zip(frames, sizes)] if kind in RGBX else [(f, w) for f, (w, _) in zip(frames, sizes)]


def _rgb(kind, frames, matrix):
    """the interleaved RGB frames the batch stands for"""
    if kind == "p010":
        return [p010_to_rgb(y, uv, matrix) for y, uv in frames]
    if kind in RGBX:
        return [rgbx_to_rgb(f, kind) for f in frames]
    return [packed_to_rgb(f, w, kind, matrix) for f, w in frames]


def _prepare(net, kind, frames, matrix):
    if kind == "p010":
        return net.prepare_from_frames_p010(frames, matrix=matrix)
    return net.prepare_from_frames_packed(frames, format=kind, **({} if kind in RGBX else {"matrix": matrix}))


def _same_prepared(got, want, what):
    got, want = (got, want) if isinstance(got, tuple) else ((got,), (want,))
    assert len(got) == len(want)
    for a, b in zip(got, want):
        a, b = (_bits(a), _bits(b)) if a.dtype == np.float32 else (a, b)
        assert np.array_equal(a, b), what


def _same_quantization(a, b, what):
    (sa, za), (sb, zb) = a.input_quantization(), b.input_quantization()
    assert np.array_equal(_bits(sa), _bits(sb)) and np.array_equal(za, zb), what
    return sa, za


@pytest.mark.parametrize("per_image", [False, True], ids=["shared_scale", "per_image"])
@pytest.mark.parametrize("kind,matrix", HOST_KINDS, ids=[k for k, _ in HOST_KINDS])
def test_host_equals_the_u8_path_on_the_converted_frames(tmp_path, kind, matrix, per_image):
    wts = _wts(tmp_path, seed=4 if per_image else 3)
    a, b = binding.Net(CFG, wts, batch=3, dump_int32=True), binding.Net(CFG, wts, batch=3, dump_int32=True)
    a.set_input_per_image(per_image)
    b.set_input_per_image(per_image)
    pairs = []
    for seed, rot in ((100, 0), (200, 1)):  # the second batch starts with another image: in shared-scale mode layer 0 is re-derived
        frames = _host_frames(kind, seed)
        frames = frames[rot:] + frames[:rot]
        rgb = _rgb(kind, frames, matrix)
        _same_prepared(_prepare(a, kind, frames, matrix), b.prepare_from_frames_u8(rgb), f"batch {seed}: uint8 input")
        s, z = _same_quantization(a, b, f"batch {seed}")
        pairs.append((s.tolist(), z.tolist()))
        _assert_same_run(_layers_and_dets(a, rgb), _layers_and_dets(b, rgb), f"batch {seed}")
    assert per_image or len(set(pairs[0][0])) == 1  # one pair for the batch | one per image
    a.close(); b.close()


def test_host_one_frame_in_several_slots(tmp_path):
    """the same array in two slots goes up once and is read by both"""
    wts = _wts(tmp_path, seed=4)
    for kind, matrix in (("bgra", "bt601"), ("yvyu", "bt709"), ("p010", "bt601")):
        a, b = binding.Net(CFG, wts, batch=3), binding.Net(CFG, wts, batch=3)
        a.set_input_per_image(True)
        b.set_input_per_image(True)
        two = _host_frames(kind, 400, SIZES[:2])
        frames = [two[0], two[1], two[0]]
        rgb = _rgb(kind, frames, matrix)
        got = _prepare(a, kind, frames, matrix)
        _same_prepared(got, b.prepare_from_frames_u8(rgb), kind)
        n = a.inputs
        assert np.array_equal(got[0][:n], got[0][2 * n:]) and not np.array_equal(got[0][:n], got[0][n:2 * n])
        _assert_same_run(_layers_and_dets(a, rgb), _layers_and_dets(b, rgb), kind)
        a.close(); b.close()


def test_host_graph_replay_per_image(tmp_path):
    wts = _wts(tmp_path, seed=2)
    net = binding.Net(CFG, wts, batch=3, use_graph=True)
    net.set_input_per_image(True)
    ref = binding.Net(CFG, wts, batch=3)
    ref.set_input_per_image(True)
    handle = None
    for seed, (kind, matrix) in ((500, ("yuyv", "bt601")), (600, ("p010", "bt709")), (700, ("abgr", "bt601"))):
        frames = _host_frames(kind, seed)
        got = _prepare(net, kind, frames, matrix)
        net.forward()
        net.sync()
        outs = [net.pull(i) for i in range(net.n)]
        if handle is None:
            handle = net.graph_handle()
            assert handle
        assert net.graph_handle() == handle  # the same captured graph replays the later batches
        _same_prepared(got, ref.prepare_from_frames_u8(_rgb(kind, frames, matrix)), kind)
        ref.forward()
        ref.sync()
        for i in range(net.n):
            want = ref.pull(i)
            for k in want:
                if k in outs[i]:
                    assert np.array_equal(outs[i][k], want[k]), f"seed {seed} layer {i} {k}"
    ref.close()
    net.close()


def test_host_replica_beside_its_parent(tmp_path):
    wts = _wts(tmp_path, seed=6)
    parent = binding.Net(CFG, wts, batch=3)
    parent.set_input_per_image(True)
    ref = binding.Net(CFG, wts, batch=3)
    ref.set_input_per_image(True)
    fp, fr = _host_frames("uyvy", 700), _host_frames("p010", 800)
    _prepare(parent, "uyvy", fp, "bt709")
    rep = parent.replica()
    xr, sr, zr = _prepare(rep, "p010", fr, "bt601f")  # its own arena, table and bank
    xp, sp, zp = _prepare(parent, "uyvy", fp, "bt709")
    for _ in range(3):  # both executors queued side by side
        parent.forward()
        rep.forward()
    for net, kind, matrix, frames, x, s, z in ((parent, "uyvy", "bt709", fp, xp, sp, zp), (rep, "p010", "bt601f", fr, xr, sr, zr)):
        net.sync()
        xw, sw, zw = ref.prepare_from_frames_u8(_rgb(kind, frames, matrix))
        assert np.array_equal(x, xw) and np.array_equal(_bits(s), _bits(sw)) and np.array_equal(z, zw)
        ref.forward()
        ref.sync()
        for i in range(net.n):
            got, want = net.pull(i), ref.pull(i)
            for k in want:
                if k in got:
                    assert np.array_equal(got[k], want[k]), f"{kind} layer {i} {k}"
    rep.close()
    ref.close()
    parent.close()


class _DeviceTensor:
    """what the Python methods ask of a device tensor (torch's names: data_ptr(), shape, stride() in elements, element_size()), over a
    buffer this library allocated -- its memory belongs to the HIP runtime the library is linked to, which a tensor of a torch build
    that carries a runtime of its own does not.  A view of `a` whose rows lie `extra` bytes further apart than they need to."""

    def __init__(self, a, extra):
        a = np.ascontiguousarray(a)
        item, row = a.dtype.itemsize, a[0].size * a.dtype.itemsize
        assert extra % item == 0
        rows = np.full((a.shape[0], row + extra), 0xEE, np.uint8)
        rows[:, :row] = a.view(np.uint8).reshape(a.shape[0], row)
        self.buf = binding.DevBuf.from_numpy(rows)
        self.shape, self._item = a.shape, item
        self._stride = ((row + extra) // item,) + tuple(s // item for s in a.strides[1:])

    def data_ptr(self):
        return self.buf.ptr.value

    def stride(self, k):
        return self._stride[k]

    def element_size(self):
        return self._item


@pytest.mark.parametrize("kind,matrix", [("rgba", "bt601"), ("yuyv", "bt709f"), ("p010", "bt709")])
def test_host_frames_on_device_equal_the_upload_path(tmp_path, kind, matrix):
    """frames a decoder or a capture left in device memory are used in place, padded rows too"""
    wts = _wts(tmp_path, seed=7)
    net, ref = binding.Net(CFG, wts, batch=3), binding.Net(CFG, wts, batch=3)
    net.set_input_per_image(True)
    ref.set_input_per_image(True)
    frames = _host_frames(kind, 900)
    want = _prepare(net, kind, frames, matrix)
    _same_prepared(want, ref.prepare_from_frames_u8(_rgb(kind, frames, matrix)), f"{kind} against u8")
    for extra in (0, 6):
        tensors = []
        if kind == "p010":
            dev = [tuple(_DeviceTensor(p, extra) for p in f) for f in frames]
            tensors = [t for f in dev for t in f]
        elif kind in RGBX:
            dev = tensors = [_DeviceTensor(f, extra) for f in frames]
        else:
            tensors = [_DeviceTensor(f, extra) for f, _ in frames]
            dev = [(t, w) for t, (_, w) in zip(tensors, frames)]
        _same_prepared(_prepare(net, kind, dev, matrix), want, f"{kind} on the device, rows + {extra}")
        for t in tensors:
            t.buf.free()
    with pytest.raises(ValueError):
        _prepare(net, kind, frames[:2] + dev[2:], matrix)  # host and device frames in one batch
    net.close(); ref.close()


def test_host_strided_rows_through_python(tmp_path):
    """rows of wider arrays are passed through as pitches (no copy)"""
    wts = _wts(tmp_path, seed=5)
    net = binding.Net(CFG, wts, batch=3)
    net.set_input_per_image(True)
    for kind, matrix in (("bgra", "bt601"), ("yuyv", "bt601"), ("p010", "bt601")):
        frames = _host_frames(kind, 1000)
        want = _prepare(net, kind, frames, matrix)

        def wide(a):
            big = np.full((a.shape[0], a.shape[1] + 3) + a.shape[2:], 0xEE, a.dtype)
            big[:, :a.shape[1]] = a
            v = big[:, :a.shape[1]]
            assert not v.flags["C_CONTIGUOUS"]
            return v
        if kind == "p010":
            views = [tuple(wide(p) for p in f) for f in frames]
        elif kind in RGBX:
            views = [wide(f) for f in frames]
        else:
            views = [(wide(f), w) for f, w in frames]
        _same_prepared(_prepare(net, kind, views, matrix), want, f"{kind}: row strides")
    even = packed_frame("yuyv", 12, 20, 1)
    got = net.prepare_from_frames_packed([even] * 3, format="yuyv")  # no tuple: w = row_bytes / 2
    _same_prepared(got, net.prepare_from_frames_packed([(even, 12)] * 3, format="yuyv"), "w from the row")
    net.close()


def test_one_net_fed_every_kind_in_turn_equals_the_u8_path(tmp_path):
    """one frame table serves entries of 32, 48 and 64 bytes in turn, the arena grows with the frames; after every feed the result is
    that of a Net which is only ever fed through prepare_from_frames_u8"""
    wts = _wts(tmp_path, seed=4)
    net, ref = binding.Net(CFG, wts, batch=3, dump_int32=True), binding.Net(CFG, wts, batch=3, dump_int32=True)
    net.set_input_per_image(True)
    ref.set_input_per_image(True)
    rng = np.random.default_rng(1234)
    feeds = [("u8", "bt601"), ("bgra", "bt601"), ("p010", "bt709"), ("i420", "bt601f"), ("yuyv", "bt709f"), ("nv12", "bt601"), ("argb", "bt601"),
             ("p010", "bt601"), ("u8", "bt601")]
    for n, (kind, matrix) in enumerate(feeds):
        sizes = [(w + 7 * n, h + 5 * n) for w, h in SIZES]  # larger every time: the arena is re-allocated
        m = MATRICES.index(matrix)
        if kind == "u8":
            rgb = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for w, h in sizes]
            got = net.prepare_from_frames_u8(rgb)
        elif kind in ("i420", "nv12"):
            planes = [tuple(rng.integers(0, 256, s, dtype=np.uint8) for s in frames_util.plane_shapes("i420", w, h)) for w, h in sizes]
            rows, cols = [(np.arange(h) >> 1)[:, None] for _, h in sizes], [(np.arange(w) >> 1)[None, :] for w, _ in sizes]
            rgb = [np.ascontiguousarray(frames_util.yuv_to_rgb(y, u[r, c], v[r, c], m)) for (y, u, v), r, c in zip(planes, rows, cols)]
            got = (net.prepare_from_frames_planar(planes, format="i420", matrix=matrix) if kind == "i420" else
                   net.prepare_from_frames_nv12([(y, np.ascontiguousarray(np.stack([u, v], axis=-1))) for y, u, v in planes], matrix=matrix))
        else:
            frames = _host_frames(kind, 2000 + n, sizes)
            rgb = _rgb(kind, frames, matrix)
            got = _prepare(net, kind, frames, matrix)
        what = f"feed {n} ({kind})"
        _same_prepared(got, ref.prepare_from_frames_u8(rgb), what)
        _same_quantization(net, ref, what)
        _assert_same_run(_layers_and_dets(net, rgb), _layers_and_dets(ref, rgb), what)
    net.close(); ref.close()


# ------------------------------------------------------------------------------------------------------------------- CLI
CLI_SIZES = [(53, 37), (24, 24), (17, 30), (15, 13)]  # w x h


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


@pytest.mark.parametrize("fmt,matrix", [("bgra", None), ("yuyv", "bt709f"), ("p010", "bt709")])
def test_cli_frames_equal_u8_on_the_converted_ppm(tmp_path, cli, fmt, matrix):
    raws, ppms = [], []
    for k, (w, h) in enumerate(CLI_SIZES):
        raw, ppm = str(tmp_path / f"im{k}_{w}x{h}.{fmt}"), str(tmp_path / f"im{k}.ppm")
        if fmt == "p010":
            y, uv = p010_frame(w, h, 90 + k)
            open(raw, "wb").write(y.astype("<u2").tobytes() + uv.astype("<u2").tobytes())
            _write_ppm(ppm, p010_to_rgb(y, uv, matrix))
        else:
            f = packed_frame(fmt, w, h, 90 + k)
            open(raw, "wb").write(f.tobytes())
            _write_ppm(ppm, packed_to_rgb(f, w, fmt, matrix or "bt601"))
        assert os.path.getsize(raw) == {"bgra": 4 * w * h, "yuyv": 4 * ((w + 1) // 2) * h,
                                        "p010": 2 * w * h + 4 * ((w + 1) // 2) * ((h + 1) // 2)}[fmt]
        raws.append(raw); ppms.append(ppm)
    how = ["-frames", fmt] + (["-matrix", matrix] if matrix else [])
    got = cli(["-list", _write_list(tmp_path / "raw.txt", raws), "-batch", "3"] + how)
    want = cli(["-list", _write_list(tmp_path / "ppm.txt", ppms), "-batch", "3", "-frames", "u8"])
    assert [g[0] for g in got] == raws and [g[1:] for g in got] == [w[1:] for w in want]  # apart from the file names
    assert any(line.startswith("box:") for blk in want for line in blk)
    assert cli([raws[0]] + how)[0][1:] == cli([ppms[0], "-frames", "u8"])[0][1:]  # the single image too
    # a short file (alone and in a list), a name without a size and another format's extension: the reader's messages
    n = os.path.getsize(raws[0])
    short = str(tmp_path / f"short_53x37.{fmt}")
    open(short, "wb").write(open(raws[0], "rb").read()[:-1])
    for args in ([short], ["-list", _write_list(tmp_path / "short.txt", [raws[1], short]), "-batch", "3"]):
        r = cli(args + how, ok=False)
        assert r.returncode != 0 and f"holds {n} bytes, the file holds {n - 1}" in r.stderr
    nosize = str(tmp_path / f"nosize.{fmt}")
    open(nosize, "wb").write(open(raws[0], "rb").read())
    r = cli([nosize] + how, ok=False)
    assert r.returncode != 0 and f"_<W>x<H>.{fmt}" in r.stderr
    other = {"bgra": "rgba", "yuyv": "uyvy", "p010": "yuyv"}[fmt]
    r = cli([raws[0], "-frames", other], ok=False)
    assert r.returncode != 0 and f"_<W>x<H>.{other}" in r.stderr


def test_cli_refuses_a_matrix_with_an_rgb_format_and_unknown_formats(tmp_path, cli):
    f = packed_frame("bgra", 53, 37, 1)
    raw = str(tmp_path / "im_53x37.bgra")
    open(raw, "wb").write(f.tobytes())
    r = cli([raw, "-frames", "bgra", "-matrix", "bt709"], ok=False)
    assert r.returncode != 0 and "-matrix does not go with -frames rgba | bgra | argb | abgr" in r.stderr
    r = cli([raw, "-frames", "rgbx"], ok=False)
    msg = r.stderr
    assert r.returncode != 0 and "-frames:" in msg
    old, new = [msg.index(k) for k in ("`u8`", "`nv12`", "`i420`", "`i444`")], [msg.index(k) for k in ("`rgba`", "`yvyu`", "`p010`")]
    assert old == sorted(old) and new == sorted(new) and old[-1] < new[0]  # the old kinds first
