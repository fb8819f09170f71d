"""8-bit interleaved frames through the batched device input path: mi355_frames_u8_letterbox_minmax / _quantize (C-ABI),
network_frames_u8_input_gpu (host), Net.prepare_from_frames_u8 (Python) and `detector test -frames u8` (CLI).

Every comparison is exact: bytes and float bits, no tolerance.  The expected result of a frame is the oracle's letterbox + layer-0
quantiser on the planes load_image_color makes of it (byte / 255), and the float path of this library on the same planes."""
import functools
import os
import subprocess

import numpy as np
import pytest

import frames_util
from frames_util import (CFG, EINVAL, ROOT, _assert_frame, _assert_same_run, _bits, _blocks, _expected, _layers_and_dets, _planes, _write_ppm,
                         _wts)
from yolo_quantization_amd import binding

pytestmark = pytest.mark.gpu

_Launch = functools.partial(frames_util._Launch, "u8")  # order="rgb" | "bgr"; pitch[b] > 3 w pads every row with 0xEE bytes


@pytest.fixture(scope="module", autouse=True)
def _dev():
    binding.init(0)


def _frame(w, h, seed, lo=0, hi=256):
    return np.random.default_rng(seed).integers(lo, hi, (h, w, 3), dtype=np.uint8)


def _all_bytes_frame():
    f = _frame(12, 12, 5)
    f.reshape(-1)[:256] = np.random.default_rng(6).permutation(256).astype(np.uint8)  # every byte value 0..255 at least once
    return f


SMALL = [("wide", lambda: _frame(53, 37, 1, 0, 180)), ("tall", lambda: _frame(12, 20, 2, 30, 256)), ("identity", _all_bytes_frame),
         ("upscale", lambda: _frame(5, 7, 3, 10, 100)), ("2x2", lambda: _frame(2, 2, 4))]


@pytest.mark.parametrize("name", [n for n, _ in SMALL])
def test_small_net_single_frame_equals_oracle(name):
    frame = dict(SMALL)[name]()
    if name == "identity":
        assert len(np.unique(frame)) == 256
    L = _Launch([frame], 12, 12)
    got = L.run()
    _assert_frame(got, 0, frame, 12, 12, name)
    if name == "identity":  # exact byte -> float -> byte round trip
        assert got[2][0] == 0 and np.array_equal(got[3][0], frame.transpose(2, 0, 1))
    L.free()


@pytest.mark.parametrize("netw,neth,sources", [(13, 11, [(9, 17)]), (52, 36, [(40, 30), (17, 50)]), (416, 416, [(640, 480)])],
                         ids=["w_not_multiple_of_4_odd_h", "letterbox_bars", "several_workgroups_per_image"])
def test_net_shapes_equal_oracle(netw, neth, sources):
    frames = [_frame(w, h, 10 + k, 5 * k, 256 - 40 * k) for k, (w, h) in enumerate(sources)]
    L = _Launch(frames, netw, neth)
    got = L.run()
    for b, f in enumerate(frames):
        _assert_frame(got, b, f, netw, neth, f"{netw}x{neth} <- {sources[b]}")
    L.free()


def test_mixed_batch_equals_single_frame_launches():
    frames = [mk() for _, mk in SMALL]
    L = _Launch(frames, 12, 12)
    mm, s, z, q = L.run()
    assert len(set(zip(s.tolist(), z.tolist()))) > 1
    for b, f in enumerate(frames):
        L1 = _Launch([f], 12, 12)
        mm1, s1, z1, q1 = L1.run()
        assert np.array_equal(_bits(mm[b]), _bits(mm1[0])) and _bits(s[b]) == _bits(s1[0]) and z[b] == z1[0], f"slot {b}"
        assert np.array_equal(q[b], q1[0]), f"slot {b}"
        _assert_frame((mm, s, z, q), b, f, 12, 12, f"slot {b}")
        L1.free()
    L.free()


def test_row_pitch():
    frames = [_frame(53, 37, 21), _frame(9, 17, 22)]
    L = _Launch(frames, 13, 11, pitch=[3 * 53 + 5, 3 * 9 + 5])
    got = L.run()
    for b, f in enumerate(frames):
        _assert_frame(got, b, f, 13, 11, f"pitch slot {b}")
    L.free()


def test_bgr_equals_rgb_on_reversed_channels():
    frame = _frame(40, 30, 31)
    Lb = _Launch([frame], 52, 36, order="bgr")
    Lr = _Launch([np.ascontiguousarray(frame[..., ::-1])], 52, 36, order="rgb")
    gb, gr = Lb.run(), Lr.run()
    for a, b in zip(gb, gr):
        assert np.array_equal(a, b)
    _assert_frame(gb, 0, frame[..., ::-1], 52, 36, "bgr")
    assert not np.array_equal(gb[3][0][0], gb[3][0][2])  # the planes really differ
    Lb.free(); Lr.free()


@pytest.mark.parametrize("what", ["resized_side_below_2", "pitch_below_3w", "null_pointer"])
def test_refusals_launch_nothing(what):
    good = _frame(12, 20, 41)
    bad = _frame(1, 40, 42) if what == "resized_side_below_2" else _frame(9, 17, 42)
    L = _Launch([good, bad], 12, 12)
    if what == "pitch_below_3w":
        L.table[1].pitch = 3 * 9 - 1
    if what == "null_pointer":
        L.table[1].data = None
    L.upload_table()
    mm_before = L.mm.to_numpy(np.float32, 4)
    assert L.minmax_rc() == EINVAL
    assert b"frames_u8" in binding.shim().mi355_last_error()
    assert L.quantize_rc([1 / 255.0, 1 / 255.0], [0, 0]) == EINVAL
    binding.check(binding.shim().mi355_stream_sync(None), "sync")
    assert np.all(L.out_bytes() == 0xA5)  # the pattern the output buffer was filled with
    assert np.array_equal(_bits(L.mm.to_numpy(np.float32, 4)), _bits(mm_before))
    L.free()


# ------------------------------------------------------------------------------------------------------------ host level
def _host_frames(seed):
    """three frames of different sizes and byte ranges (w x h: wide, tall, network size)"""
    specs = [((53, 37), 0, 256), ((12, 20), 40, 140), ((12, 12), 100, 230)]
    return [_frame(w, h, seed + k, lo, hi) for k, ((w, h), lo, hi) in enumerate(specs)]


def test_host_shared_scale_equals_float_path_and_rederives_layer0(tmp_path):
    wts = _wts(tmp_path)
    a, b = binding.Net(CFG, wts, batch=3, dump_int32=True), binding.Net(CFG, wts, batch=3, dump_int32=True)
    pairs = []
    for seed, rot in ((100, 0), (200, 1)):  # the second batch starts with another image: another pair, layer 0 is re-derived
        frames = _host_frames(seed)
        frames = frames[rot:] + frames[:rot]
        xa = a.prepare_from_frames_u8(frames)
        xb = b.prepare_from_images_gpu([_planes(f) for f in frames])
        assert np.array_equal(xa, xb), f"batch {seed}: uint8 input"
        sa, za = a.input_quantization()
        sb, zb = b.input_quantization()
        assert np.array_equal(_bits(sa), _bits(sb)) and np.array_equal(za, zb)
        want0 = _expected(frames[0], 12, 12)
        assert np.array_equal(xa[:a.inputs], want0[1].ravel()) and _bits(sa[0]) == _bits(want0[2]) and za[0] == want0[3]
        pairs.append((float(sa[0]), int(za[0])))
        _assert_same_run(_layers_and_dets(a, frames), _layers_and_dets(b, frames), f"batch {seed}")
    assert pairs[0] != pairs[1]
    a.close(); b.close()


def test_host_per_image_equals_float_path(tmp_path):
    wts = _wts(tmp_path, seed=4)
    a, b = binding.Net(CFG, wts, batch=3, dump_int32=True), binding.Net(CFG, wts, batch=3, dump_int32=True)
    a.set_input_per_image(True)
    b.set_input_per_image(True)
    frames = _host_frames(300)
    xa, sa, za = a.prepare_from_frames_u8(frames)
    xb, sb, zb = b.prepare_from_images_gpu([_planes(f) for f in frames])
    assert np.array_equal(xa, xb)
    assert np.array_equal(_bits(sa), _bits(sb)) and np.array_equal(za, zb)
    assert len(set(sa.tolist())) == 3  # the scales really differ
    for k, f in enumerate(frames):
        _, q, s, z = _expected(f, 12, 12)
        assert np.array_equal(xa[k * a.inputs:(k + 1) * a.inputs], q.ravel()) and _bits(sa[k]) == _bits(s) and za[k] == z, f"slot {k}"
    _assert_same_run(_layers_and_dets(a, frames), _layers_and_dets(b, frames), "per image")
    a.close(); b.close()


def test_host_strided_and_bgr_frames_through_python(tmp_path):
    """rows of a wider buffer are passed through as a pitch (no copy), BGR frames by name"""
    wts = _wts(tmp_path, seed=5)
    frames = _host_frames(400)
    wide = [np.full((f.shape[0], f.shape[1] + 3, 3), 0xEE, np.uint8) for f in frames]
    views = []
    for f, wbuf in zip(frames, wide):
        wbuf[:, :f.shape[1]] = f
        v = wbuf[:, :f.shape[1]]
        assert not v.flags["C_CONTIGUOUS"] and v.strides == (3 * f.shape[1] + 9, 3, 1)
        views.append(v)
    net = binding.Net(CFG, wts, batch=3)
    net.set_input_per_image(True)
    want = net.prepare_from_frames_u8(frames)
    got = net.prepare_from_frames_u8(views)
    got_bgr = net.prepare_from_frames_u8([f[..., ::-1] for f in views], order="bgr")  # negative channel stride: copied by the binding
    for g in (got, got_bgr):
        for x, y in zip(g, want):
            assert np.array_equal(x, y)
    net.close()


def test_host_graph_replay_per_image(tmp_path):
    wts = _wts(tmp_path, seed=2)
    net = binding.Net(CFG, wts, batch=3, use_graph=True)
    net.set_input_per_image(True)
    n1 = binding.Net(CFG, wts, batch=1)
    handle = None
    for seed in (500, 600):
        frames = _host_frames(seed)
        xq, s, z = net.prepare_from_frames_u8(frames)
        net.forward()
        net.sync()
        outs = [net.pull(i) for i in range(net.n)]
        if handle is None:
            handle = net.graph_handle()
            assert handle
        assert net.graph_handle() == handle  # the same captured graph replays the second batch
        for b, f in enumerate(frames):
            x1 = n1.prepare_from_images_gpu([_planes(f)])
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
    fp, fr = _host_frames(700), _host_frames(800)
    parent.prepare_from_frames_u8(fp)
    rep = parent.replica()
    xr, sr, zr = rep.prepare_from_frames_u8(fr)  # its own arena, table and bank
    xp, sp, zp = parent.prepare_from_frames_u8(fp)
    for _ in range(3):  # both executors queued side by side
        parent.forward()
        rep.forward()
    for net, frames, x, s, z in ((parent, fp, xp, sp, zp), (rep, fr, xr, sr, zr)):
        net.sync()
        xw, sw, zw = ref.prepare_from_images_gpu([_planes(f) for f in frames])
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


# ------------------------------------------------------------------------------------------------------------------- CLI
def test_cli_frames_u8_blocks_equal_the_float_path(tmp_path):
    exe = os.path.join(ROOT, "yolo_quantization_amd", "bin", "darknet")
    wts = _wts(tmp_path, seed=1)
    names = str(tmp_path / "x.names")
    open(names, "w").write("\n".join(["ant", "bee", "cat", "dog", "eel"]) + "\n")
    data = str(tmp_path / "x.data")
    open(data, "w").write(f"classes= 5\nnames = {names}\n")
    rng = np.random.default_rng(8)
    specs = [((37, 53), 0, 256), ((24, 24), 40, 140), ((30, 17), 100, 230), ((12, 12), 0, 90)]  # the PPMs of the -list test
    paths = []
    for k, ((h, w), lo, hi) in enumerate(specs):
        p = str(tmp_path / f"im{k}.ppm")
        _write_ppm(p, rng.integers(lo, hi, (h, w, 3), dtype=np.uint8))
        paths.append(p)
    lst = str(tmp_path / "list.txt")
    open(lst, "w").write("\n".join(paths) + "\n")
    args = ["-thresh", "0.3", "-boxes"]

    def run(extra):
        r = subprocess.run([exe, "detector", "test", data, CFG, wts] + extra + args, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        return _blocks(r.stdout)

    want = run(["-list", lst, "-batch", "3"])
    got = run(["-list", lst, "-batch", "3", "-frames", "u8"])
    assert [g[0] for g in got] == paths and got == want
    assert any(line.startswith("box:") for blk in want for line in blk)
    assert run([paths[0], "-frames", "u8"]) == run([paths[0]])  # the single image too
