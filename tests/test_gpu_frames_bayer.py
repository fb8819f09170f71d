"""Raw sensor frames (Bayer RGGB / BGGR / GRBG / GBRG and mono; 8-bit, 16-bit, CSI-2 RAW10 and RAW12 samples; optional tone tables)
through the batched device input path: mi355_frames_bayer_* (C-ABI), network_frames_bayer_input_gpu (host),
Net.prepare_from_frames_bayer (Python) and `detector test -frames rggb | bggr | grbg | gbrg | mono` (CLI).

Every comparison is exact: bytes and float bits, no tolerance.  The expected result of a frame never comes from the code under test:
frames_bayer_util.demosaic (the definition of mi355_yolo_int8.h in numpy, checked against a per-pixel loop by
test_frames_bayer_cpu.py) turns it into the interleaved RGB frame D(frame), and the u8 calls, pinned to the oracle by their own
tests, give the result."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import frames_util
import input_on_device_cases as cases
from frames_bayer_util import BAYER, PATTERNS, SAMPLES, demosaic, pack, row_bytes
from frames_packed_util import assert_same, geometry_accepts, run
from frames_util import CFG, EINVAL, ROOT, _assert_same_run, _bits, _blocks, _layers_and_dets, _write_ppm, _wts
from yolo_quantization_amd import binding, synth

pytestmark = pytest.mark.gpu

NETS = [(12, 12), (16, 10)]  # network inputs, w x h
# w x h, one batch: the smallest Bayer frames, upscaled so that every tap sits on reflected borders | downscaled ones that skip samples
SIZES = [(2, 2), (3, 2), (2, 3), (5, 7), (13, 9), (33, 17), (40, 28)]
_LaunchU8 = functools.partial(frames_util._Launch, "u8")


@pytest.fixture(scope="module", autouse=True)
def _dev():
    binding.init(0)


def _samples(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


class Frame:
    """one raw frame as the C-ABI test lays it out: `data` uint8 [h][row_bytes], the bytes in memory"""

    def __init__(self, frame, pattern, sample, shift=0, tone=None, w=None):
        frame = np.asarray(frame)
        self.data = np.ascontiguousarray(frame).astype("<u2").view(np.uint8).reshape(frame.shape[0], -1) if sample == "u16" else frame
        self.h = frame.shape[0]
        self.w = frame.shape[1] if w is None else w
        self.pattern, self.sample, self.shift, self.tone = pattern, sample, shift, tone
        assert self.data.shape[1] == row_bytes(sample, self.w)
        self.rgb = demosaic(frame, pattern, sample, shift, tone, w)  # D(frame)


def _frame(w, h, pattern, sample, seed, shift=None, tone=None):
    """a random frame of the layout whose raw8 is random too; the bits below the kept ones are not zero"""
    shift = (2, 4, 6, 8, 0)[seed % 5] if shift is None else shift
    shift = shift if sample == "u16" else 0
    return Frame(pack(_samples(w, h, seed), sample, shift), pattern, sample, shift, tone, w if sample.startswith("mipi") else None)


class Launch(frames_util._Launch):
    """One batch of Frames through the two Bayer calls.  extra: bytes added to every frame's tight pitch; offset: bytes between the
    (aligned) device allocation and the frame's first byte.  A tone table goes up once per distinct array (`is`), so frames that
    share an array share a device pointer."""

    def __init__(self, frames, netw, neth, extra=0, offset=0):
        B = len(frames)
        self.kind, self.B, self.netw, self.neth = "bayer", B, netw, neth
        self.bufs, tones = [], {}
        self.table = (binding.FrameBayer * B)()
        for b, f in enumerate(frames):
            q = f.data.shape[1] + extra
            raw = np.full(offset + f.h * q, 0xEE, np.uint8)
            raw[offset:].reshape(f.h, q)[:, :f.data.shape[1]] = f.data
            self.bufs.append(binding.DevBuf.from_numpy(raw))
            data = self.bufs[-1].ptr.value
            assert data % 4 == 0
            tone = None
            if f.tone is not None:
                if id(f.tone) not in tones:
                    tones[id(f.tone)] = binding.DevBuf.from_numpy(np.ascontiguousarray(f.tone, np.uint8))
                    self.bufs.append(tones[id(f.tone)])
                tone = tones[id(f.tone)].ptr.value
            self.table[b] = binding.FrameBayer(data + offset, tone, f.w, f.h, q, binding.BAYER_PATTERN[f.pattern],
                                               binding.RAW_SAMPLE[f.sample], f.shift, (C.c_int * 2)(0, 0))
        self.out = binding.DevBuf.from_numpy(np.full(B * 3 * neth * netw, 0xA5, np.uint8))
        self.mm = binding.DevBuf.from_numpy(np.full(2 * B, 7.0, np.float32))
        self.pairs = None


def _want(frames, netw, neth):
    return run(_LaunchU8, [f.rgb for f in frames], netw, neth)


def test_the_sizes_are_what_the_geometry_accepts():
    assert all(geometry_accepts(w, h, nw, nh) for w, h in SIZES + [(8, 5), (11, 5), (6, 5), (7, 5)] for nw, nh in NETS)
    # a frame of one column is served where both resized sides reach 2 (legal for MONO), refused where one does not
    assert geometry_accepts(1, 1, 12, 12) and geometry_accepts(1, 5, 12, 12) and not geometry_accepts(1, 7, 12, 12)


# ------------------------------------------------------------------------------------------------------------ C-ABI level
@pytest.mark.parametrize("sample", SAMPLES)
@pytest.mark.parametrize("pattern", PATTERNS)
def test_bayer_equals_the_u8_calls_on_the_demosaiced_frames(pattern, sample):
    """16-bit samples and MIPI groups are read at any address: data at +0, +1 and +3 from an aligned base, tight and odd padded
    pitches, both network inputs"""
    frames = [_frame(w, h, pattern, sample, 10 * k + PATTERNS.index(pattern)) for k, (w, h) in enumerate(SIZES)]
    if sample == "mipi10":
        frames += [_frame(w, 5, pattern, sample, 90 + w) for w in (8, 9, 10, 11)]  # every position of the last group
    if sample == "mipi12":
        frames += [_frame(w, 5, pattern, sample, 90 + w) for w in (6, 7)]
    ramp = (np.arange(256, dtype=np.uint8).reshape(16, 16) * 37).astype(np.uint8)  # one frame whose samples run through all 256 values
    assert len(np.unique(ramp)) == 256
    frames.append(Frame(pack(ramp, sample, 4 if sample == "u16" else 0), pattern, sample, 4 if sample == "u16" else 0, None,
                        16 if sample.startswith("mipi") else None))
    if sample == "u16":  # samples beyond their nominal range saturate
        for shift in (0, 2, 8):
            v = np.random.default_rng(shift).integers(0, 65536, (9, 13), dtype=np.uint16)
            v[0, :4] = [255 << shift, min((255 << shift) + 1, 65535), 65535, (256 << shift) & 65535]
            frames.append(Frame(v, pattern, sample, shift))
            assert shift == 8 or (frames[-1].rgb == 255).any()
    for netw, neth in NETS:
        want = _want(frames, netw, neth)
        assert len(np.unique(want[3])) > 16  # real images, not constants
        for extra, offset in ((0, 0), (0, 1), (0, 3), (3, 0), (5, 1), (7, 3)):
            got = run(Launch, frames, netw, neth, extra=extra, offset=offset)
            assert_same(got, want, f"{pattern} {sample} into {netw} x {neth}: pitch + {extra}, address + {offset}")


def test_patterns_differ_where_they_must():
    """the same samples behind another filter give another image: the expected frames tell the patterns apart"""
    s = _samples(13, 9, 3)
    rgb = {p: demosaic(s, p) for p in PATTERNS}
    assert all(a == b or not np.array_equal(rgb[a], rgb[b]) for a in PATTERNS for b in PATTERNS)


@pytest.mark.parametrize("size", [(1, 1), (1, 5)])
def test_mono_frames_of_one_column_get_the_u8_calls_verdict(size):
    """MONO needs w, h >= 1 only, so the Bayer kind's own clauses pass a frame of one column; the letterbox geometry, which every kind
    shares, serves it where both resized sides reach 2: both kinds give the same bytes, scales and zero points.  Where a resized side
    falls below 2 (1 x 7 into 12 x 12) both refuse it with the same words, and nothing is launched."""
    w, h = size
    f = Frame(_samples(w, h, 1), "mono", "u8")
    assert f.rgb.shape == (h, w, 3) and np.array_equal(f.rgb[:, :, 0], f.rgb[:, :, 2])
    good = _frame(5, 7, "mono", "u8", 2)
    assert geometry_accepts(w, h, 12, 12)
    assert_same(run(Launch, [good, f], 12, 12), run(_LaunchU8, [good.rgb, f.rgb], 12, 12), f"mono {w} x {h}")
    f = Frame(_samples(1, 7, 1), "mono", "u8")
    for L, prefix in ((Launch([good, f], 12, 12), b"frames_bayer"), (_LaunchU8([good.rgb, f.rgb], 12, 12), b"frames_u8")):
        L.upload_table()
        assert L.minmax_rc() == EINVAL
        assert binding.shim().mi355_last_error().startswith(b"invalid argument: " + prefix + b": degenerate aspect (resized side < 2)")
        assert L.quantize_rc([1 / 255.0] * 2, [0, 0]) == EINVAL
        binding.check(binding.shim().mi355_stream_sync(None), "sync")
        assert np.all(L.out_bytes() == 0xA5)
        L.free()


def test_refusals_launch_nothing():
    """one refusal of the kind's own on the device (the CPU file has every clause): MI355_EINVAL from both calls, nothing written"""
    L = Launch([_frame(5, 7, "rggb", "u8", 1), _frame(13, 9, "rggb", "u8", 2)], 12, 12)
    L.table[1].pitch = 12
    L.upload_table()
    mm_before = L.mm.to_numpy(np.float32, 4)
    assert L.minmax_rc() == EINVAL
    assert binding.shim().mi355_last_error().startswith(b"invalid argument: frames_bayer: pitch < w")
    assert L.quantize_rc([1 / 255.0] * 2, [0, 0]) == EINVAL
    binding.check(binding.shim().mi355_stream_sync(None), "sync")
    assert np.all(L.out_bytes() == 0xA5)
    assert np.array_equal(_bits(L.mm.to_numpy(np.float32, 4)), _bits(mm_before))
    L.free()


def _tone(seed):
    return np.random.default_rng(seed).integers(0, 256, (3, 256), dtype=np.uint8)


IDENTITY = np.tile(np.arange(256, dtype=np.uint8), (3, 1))


@pytest.mark.parametrize("sample", ["u8", "u16", "mipi12"])
def test_tone_tables(sample):
    sizes = [(5, 7), (13, 9), (33, 17), (2, 2)]
    pats = ["grbg", "bggr", "mono", "rggb"]
    mk = lambda tones: [_frame(w, h, p, sample, 40 + k, tone=t) for k, ((w, h), p, t) in enumerate(zip(sizes, pats, tones))]
    plain = run(Launch, mk([None] * 4), 12, 12)
    assert_same(run(Launch, mk([IDENTITY] * 4), 12, 12), plain, "an identity table equals NULL")
    one, each = _tone(1), [_tone(2 + k) for k in range(4)]
    batches = {"one random table, one pointer for the batch": mk([one] * 4), "every frame its own table": mk(each),
               "NULL and tables mixed": mk([None, each[1], None, one])}
    for what, frames in batches.items():
        want = _want(frames, 12, 12)
        for offset in (0, 1):
            got = run(Launch, frames, 12, 12, extra=offset, offset=offset)
            assert_same(got, want, what)
            assert not np.array_equal(got[3], plain[3])
    L = Launch(batches["one random table, one pointer for the batch"], 12, 12)
    assert len({L.table[b].tone for b in range(4)}) == 1
    L.free()
    L = Launch(batches["every frame its own table"], 12, 12)
    assert len({L.table[b].tone for b in range(4)}) == 4
    L.free()


# ------------------------------------------------------------------------------------------------------------ host level
HOST_SIZES = [(33, 17), (5, 7), (12, 12)]
HOST_KINDS = [("rggb", "u8"), ("bggr", "u16"), ("grbg", "mipi10"), ("gbrg", "mipi12"), ("mono", "u16")]


def _host_frames(pattern, sample, seed, sizes=HOST_SIZES, shift=2):
    """(what prepare_from_frames_bayer takes, D(frame)) per frame"""
    shift = shift if sample == "u16" else 0
    out = []
    for k, (w, h) in enumerate(sizes):
        f = pack(_samples(w, h, seed + k), sample, shift)
        out.append(((f, w) if sample.startswith("mipi") else f, f, w))
    return [a for a, _, _ in out], lambda tone=None: [demosaic(f, pattern, sample, shift, _per(tone, b), w) for b, (_, f, w) in enumerate(out)]


def _per(tone, b):
    return tone[b] if isinstance(tone, list) else tone


def _same_prepared(got, want, what):
    got, want = (got, want) if isinstance(got, tuple) else ((got,), (want,))
    assert len(got) == len(want)
    for a, b in zip(got, want):
        a, b = (_bits(a), _bits(b)) if a.dtype == np.float32 else (a, b)
        assert np.array_equal(a, b), what


def _same_quantization(a, b, what):
    (sa, za), (sb, zb) = a.input_quantization(), b.input_quantization()
    assert np.array_equal(_bits(sa), _bits(sb)) and np.array_equal(za, zb), what


@pytest.mark.parametrize("per_image", [False, True], ids=["shared_scale", "per_image"])
@pytest.mark.parametrize("pattern,sample", HOST_KINDS, ids=[f"{p}_{s}" for p, s in HOST_KINDS])
def test_host_equals_the_u8_path_on_the_demosaiced_frames(tmp_path, pattern, sample, per_image):
    wts = _wts(tmp_path, seed=4 if per_image else 3)
    a, b = binding.Net(CFG, wts, batch=3, dump_int32=True), binding.Net(CFG, wts, batch=3, dump_int32=True)
    a.set_input_per_image(per_image)
    b.set_input_per_image(per_image)
    for seed, tone in ((100, None), (200, _tone(9)), (300, [_tone(10), None, _tone(11)])):
        frames, rgb_of = _host_frames(pattern, sample, seed)  # frames of different sizes in one batch
        rgb = rgb_of(tone)
        got = a.prepare_from_frames_bayer(frames, pattern, sample, 2 if sample == "u16" else 0, tone)
        _same_prepared(got, b.prepare_from_frames_u8(rgb), f"batch {seed}: uint8 input")
        _same_quantization(a, b, f"batch {seed}")
        _assert_same_run(_layers_and_dets(a, rgb), _layers_and_dets(b, rgb), f"batch {seed}")
    a.close(); b.close()


def test_host_one_frame_in_several_slots_and_strided_rows(tmp_path):
    wts = _wts(tmp_path, seed=4)
    a, b = binding.Net(CFG, wts, batch=3), binding.Net(CFG, wts, batch=3)
    a.set_input_per_image(True)
    b.set_input_per_image(True)
    for pattern, sample in (("rggb", "u8"), ("gbrg", "u16"), ("bggr", "mipi10")):
        two, rgb_of = _host_frames(pattern, sample, 400, HOST_SIZES[:2])
        tone = _tone(12)
        rgb2 = rgb_of(tone)
        frames, rgb = [two[0], two[1], two[0]], [rgb2[0], rgb2[1], rgb2[0]]
        shift = 2 if sample == "u16" else 0
        got = a.prepare_from_frames_bayer(frames, pattern, sample, shift, tone)
        _same_prepared(got, b.prepare_from_frames_u8(rgb), f"{pattern} {sample}")
        n = a.inputs
        assert np.array_equal(got[0][:n], got[0][2 * n:]) and not np.array_equal(got[0][:n], got[0][n:2 * n])

        def wide(f):  # rows of a wider array are passed through as the pitch (no copy)
            arr, w = f if isinstance(f, tuple) else (f, None)
            big = np.full((arr.shape[0], arr.shape[1] + 3), 0xEE, arr.dtype)
            big[:, :arr.shape[1]] = arr
            v = big[:, :arr.shape[1]]
            assert not v.flags["C_CONTIGUOUS"]
            return v if w is None else (v, w)
        _same_prepared(a.prepare_from_frames_bayer([wide(f) for f in frames], pattern, sample, shift, tone), got, f"{pattern} {sample}: row strides")
    a.close(); b.close()


class _DeviceTensor:
    """what the Python method asks of a device tensor (torch's names: data_ptr(), shape, stride() in elements, element_size()), over a
    buffer this library allocated -- its memory belongs to the HIP runtime the library is linked to.  A view of `a` whose rows lie
    `extra` bytes further apart than they need to."""

    def __init__(self, a, extra=0):
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


def _on_device(frames, extra):
    tensors = [_DeviceTensor(f[0] if isinstance(f, tuple) else f, extra) for f in frames]
    return [(t, f[1]) if isinstance(f, tuple) else t for t, f in zip(tensors, frames)], tensors


@pytest.mark.parametrize("pattern,sample", [("rggb", "u8"), ("grbg", "u16"), ("mono", "mipi12")])
def test_host_frames_and_tone_on_device_equal_the_upload_path(tmp_path, pattern, sample):
    wts = _wts(tmp_path, seed=7)
    net = binding.Net(CFG, wts, batch=3)
    net.set_input_per_image(True)
    frames, _ = _host_frames(pattern, sample, 900)
    shift = 2 if sample == "u16" else 0
    tones = [_tone(13), None, _tone(14)]
    want = net.prepare_from_frames_bayer(frames, pattern, sample, shift, tones)
    dev_tones = [None if t is None else _DeviceTensor(t) for t in tones]
    for extra in (0, 6):
        dev, tensors = _on_device(frames, extra)
        _same_prepared(net.prepare_from_frames_bayer(dev, pattern, sample, shift, dev_tones, on_device=True), want, f"rows + {extra}")
        for t in tensors:
            t.buf.free()
    with pytest.raises(ValueError):
        net.prepare_from_frames_bayer(frames[:2] + dev[2:], pattern, sample, shift, on_device=True)  # host and device frames in one batch
    for t in dev_tones:
        if t is not None:
            t.buf.free()
    net.close()


def test_host_input_on_device_adds_no_host_wait(tmp_path):
    """set_input_on_device: device frames are only enqueued -- host_waits() stands still over three steps -- and the result is the
    synchronous path's"""
    cfg = cases.write_net_cfg(tmp_path / "net.cfg", 12)
    wts = str(tmp_path / "net.weights")
    synth.synth_weights(cfg, wts, seed=3)
    net, ref = binding.Net(cfg, wts, batch=3), binding.Net(cfg, wts, batch=3)
    for n in (net, ref):
        n.set_input_per_image(True)
    net.set_input_on_device(True)
    tone_h = _tone(15)
    tone = _DeviceTensor(tone_h)
    batches = [_host_frames("gbrg", "u16", 1000 + 10 * k) for k in range(4)]
    devs = [_on_device(f, 2) for f, _ in batches]
    net.prepare_from_frames_bayer(devs[0][0], "gbrg", "u16", 2, tone, on_device=True)  # warm-up: preparation, allocations
    net.forward()
    net.sync()
    before = net.host_waits()
    for k in (1, 2, 3):
        assert net.prepare_from_frames_bayer(devs[k][0], "gbrg", "u16", 2, tone, on_device=True) is None
        net.forward()
    assert net.host_waits() == before
    net.sync()
    assert not net.input_status().any()
    rgb = batches[3][1](tone_h)
    xw, sw, zw = ref.prepare_from_frames_u8(rgb)
    assert np.array_equal(net._pull_input(), xw)
    s, z = net.input_quantization()
    assert np.array_equal(_bits(s), _bits(sw)) and np.array_equal(z, zw)
    ref.forward()
    ref.sync()
    for i in range(net.n):
        got, want = net.pull(i), ref.pull(i)
        for key in want:
            if key in got:
                assert np.array_equal(got[key], want[key]), f"layer {i} {key}"
    for _, tensors in devs:
        for t in tensors:
            t.buf.free()
    tone.buf.free()
    net.close(); ref.close()


def test_host_graph_replay_and_a_replica(tmp_path):
    wts = _wts(tmp_path, seed=2)
    net = binding.Net(CFG, wts, batch=3, use_graph=True)
    ref = binding.Net(CFG, wts, batch=3)
    for n in (net, ref):
        n.set_input_per_image(True)
    handle = None
    for seed, (pattern, sample) in ((500, ("rggb", "mipi10")), (600, ("mono", "u8")), (700, ("bggr", "u16"))):
        frames, rgb_of = _host_frames(pattern, sample, seed)
        tone = _tone(seed)
        got = net.prepare_from_frames_bayer(frames, pattern, sample, 2 if sample == "u16" else 0, tone)
        net.forward()
        net.sync()
        outs = [net.pull(i) for i in range(net.n)]
        if handle is None:
            handle = net.graph_handle()
            assert handle
        assert net.graph_handle() == handle  # the same captured graph replays the later batches
        _same_prepared(got, ref.prepare_from_frames_u8(rgb_of(tone)), f"{pattern} {sample}")
        ref.forward()
        ref.sync()
        for i in range(net.n):
            want = ref.pull(i)
            for k in want:
                if k in outs[i]:
                    assert np.array_equal(outs[i][k], want[k]), f"seed {seed} layer {i} {k}"
    rep = net.replica()  # its own arena, table and bank
    fr, rgb_r = _host_frames("grbg", "mipi12", 800)
    fp, rgb_p = _host_frames("gbrg", "u8", 810)
    xr = rep.prepare_from_frames_bayer(fr, "grbg", "mipi12")
    xp = net.prepare_from_frames_bayer(fp, "gbrg", "u8", tone=IDENTITY)
    for _ in range(2):  # both executors queued side by side
        net.forward()
        rep.forward()
    for n, x, rgb in ((net, xp, rgb_p()), (rep, xr, rgb_r())):
        n.sync()
        _same_prepared(x, ref.prepare_from_frames_u8(rgb), "replica")
        ref.forward()
        ref.sync()
        for i in range(n.n):
            got, want = n.pull(i), ref.pull(i)
            for k in want:
                if k in got:
                    assert np.array_equal(got[k], want[k]), f"replica layer {i} {k}"
    rep.close(); ref.close(); net.close()


def test_one_net_fed_kinds_in_turn_equals_the_u8_path(tmp_path):
    """Bayer, then u8, then planar, then Bayer with another layout on one network: one frame table serves entries of 48, 32, 64 and
    48 bytes in turn, the arena grows with the frames"""
    wts = _wts(tmp_path, seed=4)
    net, ref = binding.Net(CFG, wts, batch=3, dump_int32=True), binding.Net(CFG, wts, batch=3, dump_int32=True)
    net.set_input_per_image(True)
    ref.set_input_per_image(True)
    rng = np.random.default_rng(1234)
    for n, kind in enumerate(["bayer_u8", "u8", "planar", "bayer_mipi10", "bayer_u16"]):
        sizes = [(w + 7 * n, h + 5 * n) for w, h in HOST_SIZES]  # larger every time: the arena is re-allocated
        if kind == "u8":
            rgb = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for w, h in sizes]
            got = net.prepare_from_frames_u8(rgb)
        elif kind == "planar":
            rgb = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for w, h in sizes]
            got = net.prepare_from_frames_planar([np.ascontiguousarray(f.transpose(2, 0, 1)) for f in rgb], format="rgb")
        else:
            sample, pattern = kind.split("_")[1], BAYER[n % 4]
            frames, rgb_of = _host_frames(pattern, sample, 2000 + n, sizes)
            tone = _tone(n) if n else None
            rgb = rgb_of(tone)
            got = net.prepare_from_frames_bayer(frames, pattern, sample, 2 if sample == "u16" else 0, tone)
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


@pytest.mark.parametrize("pattern,sample,shift,toned", [("rggb", "u8", 0, False), ("grbg", "u16", 2, False), ("mono", "mipi12", 0, True)])
def test_cli_frames_equal_u8_on_the_demosaiced_ppm(tmp_path, cli, pattern, sample, shift, toned):
    tone = _tone(21) if toned else None
    tone_file = str(tmp_path / "tone.bin")
    open(tone_file, "wb").write(_tone(21).tobytes())
    raws, ppms = [], []
    for k, (w, h) in enumerate(CLI_SIZES):
        raw, ppm = str(tmp_path / f"im{k}_{w}x{h}.{pattern}"), str(tmp_path / f"im{k}.ppm")
        f = pack(_samples(w, h, 90 + k), sample, shift)
        open(raw, "wb").write(f.astype("<u2").tobytes() if sample == "u16" else f.tobytes())
        assert os.path.getsize(raw) == row_bytes(sample, w) * h
        _write_ppm(ppm, demosaic(f, pattern, sample, shift, tone, w))
        raws.append(raw); ppms.append(ppm)
    how = ["-frames", pattern] + (["-raw", sample] if sample != "u8" else []) + (["-raw_shift", str(shift)] if shift else []) + \
          (["-tone", tone_file] if toned else [])
    got = cli(["-list", _write_list(tmp_path / "raw.txt", raws), "-batch", "3"] + how)
    want = cli(["-list", _write_list(tmp_path / "ppm.txt", ppms), "-batch", "3", "-frames", "u8"])
    assert [g[0] for g in got] == raws and [g[1:] for g in got] == [w[1:] for w in want]  # apart from the file names
    assert any(line.startswith("box:") for blk in want for line in blk)
    assert cli([raws[0]] + how)[0][1:] == cli([ppms[0], "-frames", "u8"])[0][1:]  # the single image too
    n = os.path.getsize(raws[0])
    short = str(tmp_path / f"short_53x37.{pattern}")
    open(short, "wb").write(open(raws[0], "rb").read()[:-1])
    r = cli([short] + how, ok=False)
    assert r.returncode != 0 and f"holds {n} bytes, the file holds {n - 1}" in r.stderr


def test_cli_refusals(tmp_path, cli):
    raw = str(tmp_path / "im_53x37.rggb")
    open(raw, "wb").write(_samples(53, 37, 1).tobytes())
    jpg = os.path.join(ROOT, "tests", "golden", "jpeg", "420_48x32.jpg")
    tone768, tone767 = str(tmp_path / "t768.bin"), str(tmp_path / "t767.bin")
    open(tone768, "wb").write(bytes(768))
    open(tone767, "wb").write(bytes(767))
    open(str(tmp_path / "t769.bin"), "wb").write(bytes(769))
    for args, message in (([raw, "-frames", "rggb", "-matrix", "bt709"], "-matrix goes with -frames nv12"),
                          ([raw, "-frames", "u8", "-raw", "u16"], "-raw, -raw_shift and -tone go with -frames rggb"),
                          ([raw, "-raw", "u16"], "-raw, -raw_shift and -tone go with -frames rggb"),
                          ([raw, "-frames", "nv12", "-tone", tone768], "-raw, -raw_shift and -tone go with -frames rggb"),
                          ([raw, "-frames", "rggb", "-raw", "u12"], "-raw: u8 (the default), u16, mipi10 and mipi12 are known"),
                          ([raw, "-frames", "rggb", "-raw", "u16", "-raw_shift", "9"], "-raw_shift: 0 .. 8"),
                          ([raw, "-frames", "rggb", "-raw_shift", "2"], "-raw_shift goes with -raw u16"),
                          ([raw, "-frames", "rggb", "-tone", tone767], "-tone: the file must hold exactly 768 bytes"),
                          ([raw, "-frames", "rggb", "-tone", str(tmp_path / "t769.bin")], "-tone: the file must hold exactly 768 bytes"),
                          ([jpg, "-frames", "rggb"], "a JPEG image does not go with raw -frames formats"),
                          (["-list", _write_list(tmp_path / "l.txt", [raw, jpg]), "-batch", "2", "-frames", "rggb"],
                           "-list: a JPEG file does not go with raw -frames formats"),
                          ([raw, "-frames", "bggr"], "_<W>x<H>.bggr")):
        r = cli(args, ok=False)
        assert r.returncode != 0 and message in r.stderr, (args, r.stderr[-300:])
    r = cli([raw, "-frames", "rgbg"], ok=False)
    msg = r.stderr
    assert r.returncode != 0 and "-frames:" in msg
    old, new = [msg.index(k) for k in ("`u8`", "`nv12`", "`i420`", "`rgba`", "`p010`")], [msg.index(k) for k in ("`rggb`", "`gbrg`", "`mono`")]
    assert old == sorted(old) and new == sorted(new) and old[-1] < new[0]  # the old kinds first
