"""NV12 / NV21 frames through the batched device input path: mi355_frames_yuv_letterbox_minmax / _quantize (C-ABI),
network_frames_nv12_input_gpu (host), Net.prepare_from_frames_nv12 (Python) and `detector test -frames nv12` (CLI).

Every comparison is exact: bytes and float bits, no tolerance.  The expected result of a frame never comes from the code under test:
this file's numpy conversion (nv12_to_rgb, the specified integer formulas with the coefficient table of frames_util written
out as numbers) makes the interleaved RGB frame, and that goes where the u8 tests' frames go: the oracle's letterbox + layer-0
quantiser on its planes (byte / 255), and at host level Net.prepare_from_frames_u8 of a second Net."""
import functools
import os
import subprocess

import numpy as np
import pytest

import frames_util
from frames_util import (CFG, EINVAL, ROOT, _assert_frame, _assert_same_run, _bits, _blocks, _expected, _layers_and_dets, _padded, _write_ppm,
                         _wts, yuv_to_rgb)
from yolo_quantization_amd import binding

pytestmark = pytest.mark.gpu

# pitch[b] = (pitch_y, pitch_uv) pads every row with 0xEE bytes; layout / matrix: one name for the batch or one per frame
_Launch = functools.partial(frames_util._Launch, "yuv")
MATRICES = ["bt601", "bt601f", "bt709", "bt709f"]


@pytest.fixture(scope="module", autouse=True)
def _dev():
    binding.init(0)


def nv12_to_rgb(y, uv, matrix="bt601", layout="nv12"):
    """interleaved RGB [h][w][3] of a frame: pixel (x, y) takes Y[y][x] and the chroma pair at [y // 2][x // 2] (nearest)"""
    h, w = y.shape
    c = uv[(np.arange(h) // 2)[:, None], (np.arange(w) // 2)[None, :]]
    u, v = (c[..., 0], c[..., 1]) if layout == "nv12" else (c[..., 1], c[..., 0])
    return yuv_to_rgb(y, u, v, MATRICES.index(matrix))


def _yuv(w, h, seed, lo=0, hi=256, clo=0, chi=256):
    """(y [h][w], uv [(h + 1) // 2][(w + 1) // 2][2]) with luma in lo..hi-1 and chroma in clo..chi-1"""
    rng = np.random.default_rng(seed)
    return (rng.integers(lo, hi, (h, w), dtype=np.uint8), rng.integers(clo, chi, ((h + 1) // 2, (w + 1) // 2, 2), dtype=np.uint8))


def _same(ga, gb):
    return all(np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)
               for a, b in zip(ga, gb))


# the u8 file's small sources: odd widths and heights (a ragged last chroma column and row), upscaling, the 2 x 2 edge handling
SMALL = [("53x37", lambda: _yuv(53, 37, 1, 0, 200)), ("12x20", lambda: _yuv(12, 20, 2, 30, 256)), ("5x7", lambda: _yuv(5, 7, 3, 10, 100, 60, 200)),
         ("3x3", lambda: _yuv(3, 3, 4)), ("2x2", lambda: _yuv(2, 2, 5))]


@pytest.mark.parametrize("name", [n for n, _ in SMALL])
def test_small_net_single_frame_equals_oracle(name):
    y, uv = dict(SMALL)[name]()
    L = _Launch([(y, uv)], 12, 12)
    got = L.run()
    _assert_frame(got, 0, nv12_to_rgb(y, uv), 12, 12, name)
    L.free()


@pytest.mark.parametrize("matrix", MATRICES)
def test_conversion_sweep_every_chroma_pair(matrix):
    """512 x 512 into a 512 x 512 input, an identity letterbox: the chroma plane enumerates all 65 536 (U, V) pairs, the four luma
    samples of a pair are 0, 255 and two random bytes"""
    u, v = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    uv = np.ascontiguousarray(np.stack([u, v], axis=-1))
    assert len(np.unique(uv.reshape(-1, 2).astype(np.int32) @ [256, 1])) == 65536
    y = np.random.default_rng(11).integers(0, 256, (512, 512), dtype=np.uint8)
    y[0::2, 0::2] = 0
    y[1::2, 1::2] = 255
    rgb = nv12_to_rgb(y, uv, matrix)
    for k in range(3):  # both clamp ends of every channel are reached
        assert rgb[..., k].min() == 0 and rgb[..., k].max() == 255
    L = _Launch([(y, uv)], 512, 512, matrix=matrix)
    got = L.run()
    _assert_frame(got, 0, rgb, 512, 512, matrix)
    assert got[2][0] == 0 and np.array_equal(got[3][0], rgb.transpose(2, 0, 1))  # scale 1 / 255, zero point 0: the converted bytes
    L.free()


@pytest.mark.parametrize("netw,neth,sources", [(13, 11, [(9, 17)]), (52, 36, [(40, 30), (17, 50)]), (416, 416, [(640, 480)])],
                         ids=["w_not_multiple_of_4_odd_h", "letterbox_bars", "several_workgroups_per_image"])
def test_net_shapes_equal_oracle(netw, neth, sources):
    frames = [_yuv(w, h, 10 + k, 5 * k, 256 - 40 * k) for k, (w, h) in enumerate(sources)]
    L = _Launch(frames, netw, neth)
    got = L.run()
    for b, (y, uv) in enumerate(frames):
        _assert_frame(got, b, nv12_to_rgb(y, uv), netw, neth, f"{netw}x{neth} <- {sources[b]}")
    L.free()


def test_nv21_equals_nv12_on_swapped_pairs():
    y, uv = _yuv(40, 30, 31, 40, 200)
    vu = np.ascontiguousarray(uv[..., ::-1])
    L12, L21, Lx = _Launch([(y, uv)], 52, 36), _Launch([(y, vu)], 52, 36, layout="nv21"), _Launch([(y, uv)], 52, 36, layout="nv21")
    g12, g21, gx = L12.run(), L21.run(), Lx.run()
    assert _same(g12, g21)
    _assert_frame(g21, 0, nv12_to_rgb(y, vu, layout="nv21"), 52, 36, "nv21")
    _assert_frame(gx, 0, nv12_to_rgb(y, uv, layout="nv21"), 52, 36, "nv21 on the unswapped plane")
    # the result really depends on the chroma: read the other way round, the R and the B plane change
    assert not np.array_equal(gx[3][0][0], g12[3][0][0]) and not np.array_equal(gx[3][0][2], g12[3][0][2])
    for L in (L12, L21, Lx):
        L.free()


@pytest.mark.parametrize("extra_uv", [6, 7], ids=["even_chroma_pitch", "odd_chroma_pitch"])
def test_row_pitches(extra_uv):
    """padded rows (0xEE) give the tight frame's result; an odd chroma pitch puts every other row's pairs at odd addresses"""
    frames = [_yuv(53, 37, 21), _yuv(9, 17, 22)]
    pitch = [(w + 5, 2 * ((w + 1) // 2) + extra_uv) for w in (53, 9)]
    Lp, Lt = _Launch(frames, 13, 11, pitch=pitch), _Launch(frames, 13, 11)
    gp, gt = Lp.run(), Lt.run()
    assert _same(gp, gt)
    for b, (y, uv) in enumerate(frames):
        _assert_frame(gp, b, nv12_to_rgb(y, uv), 13, 11, f"pitch slot {b}")
    Lp.free(); Lt.free()


def test_mixed_batch_equals_single_frame_launches():
    frames = [_yuv(53, 37, 41, 0, 256), _yuv(12, 20, 42, 16, 120, 100, 156), _yuv(5, 7, 43, 60, 180, 90, 170), _yuv(12, 12, 44, 0, 80, 120, 136),
              _yuv(31, 9, 45, 100, 236)]
    matrix = ["bt601", "bt709", "bt601f", "bt709f", "bt709"]
    layout = ["nv12", "nv21", "nv12", "nv21", "nv12"]
    L = _Launch(frames, 12, 12, layout=layout, matrix=matrix)
    mm, s, z, q = L.run()
    assert len(set(zip(s.tolist(), z.tolist()))) >= 2
    for b, (y, uv) in enumerate(frames):
        L1 = _Launch([(y, uv)], 12, 12, layout=layout[b], matrix=matrix[b])
        mm1, s1, z1, q1 = L1.run()
        assert np.array_equal(_bits(mm[b]), _bits(mm1[0])) and _bits(s[b]) == _bits(s1[0]) and z[b] == z1[0], f"slot {b}"
        assert np.array_equal(q[b], q1[0]), f"slot {b}"
        _assert_frame((mm, s, z, q), b, nv12_to_rgb(y, uv, matrix[b], layout[b]), 12, 12, f"slot {b}")
        L1.free()
    L.free()


@pytest.mark.parametrize("what", ["null_uv", "pitch_uv_below_minimum", "unknown_matrix", "resized_side_below_2"])
def test_refusals_launch_nothing(what):
    good = _yuv(12, 20, 51)
    bad = _yuv(1, 40, 52) if what == "resized_side_below_2" else _yuv(9, 17, 52)
    L = _Launch([good, bad], 12, 12)
    if what == "null_uv":
        L.table[1].uv = None
    if what == "pitch_uv_below_minimum":
        L.table[1].pitch_uv = 2 * ((9 + 1) // 2) - 1
    if what == "unknown_matrix":
        L.table[1].matrix = 4
    L.upload_table()
    mm_before = L.mm.to_numpy(np.float32, 4)
    assert L.minmax_rc() == EINVAL
    assert binding.shim().mi355_last_error().startswith(b"invalid argument: frames_yuv:")  # the prefix every MI355_EINVAL carries
    assert L.quantize_rc([1 / 255.0, 1 / 255.0], [0, 0]) == EINVAL
    assert binding.shim().mi355_last_error().startswith(b"invalid argument: frames_yuv:")  # the prefix every MI355_EINVAL carries
    binding.check(binding.shim().mi355_stream_sync(None), "sync")
    assert np.all(L.out_bytes() == 0xA5)  # the pattern the output buffer was filled with
    assert np.array_equal(_bits(L.mm.to_numpy(np.float32, 4)), _bits(mm_before))
    L.free()


# ------------------------------------------------------------------------------------------------------------ host level
def _host_frames(seed):
    """three frames of different sizes, luma and chroma ranges (w x h: wide, tall, network size)"""
    specs = [((53, 37), 0, 256, 0, 256), ((12, 20), 40, 140, 100, 156), ((12, 12), 100, 200, 120, 136)]
    return [_yuv(w, h, seed + k, lo, hi, clo, chi) for k, ((w, h), lo, hi, clo, chi) in enumerate(specs)]


def _rgb(frames, matrix="bt601", layout="nv12"):
    return [nv12_to_rgb(y, uv, matrix, layout) for y, uv in frames]


def test_host_shared_scale_equals_u8_path_and_rederives_layer0(tmp_path):
    wts = _wts(tmp_path)
    a, b = binding.Net(CFG, wts, batch=3, dump_int32=True), binding.Net(CFG, wts, batch=3, dump_int32=True)
    pairs = []
    for seed, rot in ((100, 0), (200, 1)):  # the second batch starts with another image: another pair, layer 0 is re-derived
        frames = _host_frames(seed)
        frames = frames[rot:] + frames[:rot]
        rgb = _rgb(frames)
        xa = a.prepare_from_frames_nv12(frames)
        xb = b.prepare_from_frames_u8(rgb)
        assert np.array_equal(xa, xb), f"batch {seed}: uint8 input"
        sa, za = a.input_quantization()
        sb, zb = b.input_quantization()
        assert np.array_equal(_bits(sa), _bits(sb)) and np.array_equal(za, zb)
        want0 = _expected(rgb[0], 12, 12)
        assert np.array_equal(xa[:a.inputs], want0[1].ravel()) and _bits(sa[0]) == _bits(want0[2]) and za[0] == want0[3]
        pairs.append((float(sa[0]), int(za[0])))
        _assert_same_run(_layers_and_dets(a, rgb), _layers_and_dets(b, rgb), f"batch {seed}")
    assert pairs[0] != pairs[1]
    a.close(); b.close()


def test_host_per_image_equals_u8_path(tmp_path):
    wts = _wts(tmp_path, seed=4)
    a, b = binding.Net(CFG, wts, batch=3, dump_int32=True), binding.Net(CFG, wts, batch=3, dump_int32=True)
    a.set_input_per_image(True)
    b.set_input_per_image(True)
    frames = _host_frames(300)
    rgb = _rgb(frames, "bt709")
    xa, sa, za = a.prepare_from_frames_nv12(frames, matrix="bt709")
    xb, sb, zb = b.prepare_from_frames_u8(rgb)
    assert np.array_equal(xa, xb)
    assert np.array_equal(_bits(sa), _bits(sb)) and np.array_equal(za, zb)
    assert len(set(sa.tolist())) == 3  # the scales really differ
    for k, f in enumerate(rgb):
        _, q, s, z = _expected(f, 12, 12)
        assert np.array_equal(xa[k * a.inputs:(k + 1) * a.inputs], q.ravel()) and _bits(sa[k]) == _bits(s) and za[k] == z, f"slot {k}"
    _assert_same_run(_layers_and_dets(a, rgb), _layers_and_dets(b, rgb), "per image")
    a.close(); b.close()


def test_host_graph_replay_per_image(tmp_path):
    wts = _wts(tmp_path, seed=2)
    net = binding.Net(CFG, wts, batch=3, use_graph=True)
    net.set_input_per_image(True)
    n1 = binding.Net(CFG, wts, batch=1)
    handle = None
    for seed in (500, 600):
        frames = _host_frames(seed)
        xq, s, z = net.prepare_from_frames_nv12(frames)
        net.forward()
        net.sync()
        outs = [net.pull(i) for i in range(net.n)]
        if handle is None:
            handle = net.graph_handle()
            assert handle
        assert net.graph_handle() == handle  # the same captured graph replays the second batch
        for b, f in enumerate(_rgb(frames)):
            x1 = n1.prepare_from_frames_u8([f])
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
    parent.prepare_from_frames_nv12(fp)
    rep = parent.replica()
    xr, sr, zr = rep.prepare_from_frames_nv12(fr, layout="nv21")  # its own arena, table and bank
    xp, sp, zp = parent.prepare_from_frames_nv12(fp)
    for _ in range(3):  # both executors queued side by side
        parent.forward()
        rep.forward()
    for net, rgb, x, s, z in ((parent, _rgb(fp), xp, sp, zp), (rep, _rgb(fr, layout="nv21"), xr, sr, zr)):
        net.sync()
        xw, sw, zw = ref.prepare_from_frames_u8(rgb)
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


def test_host_frames_on_device_equal_the_upload_path(tmp_path):
    """planes a decoder left in device memory are used in place"""
    wts = _wts(tmp_path, seed=7)
    net = binding.Net(CFG, wts, batch=3)
    net.set_input_per_image(True)
    frames = _host_frames(900)
    want = net.prepare_from_frames_nv12(frames)
    bufs, dev = [], []
    for y, uv in frames:
        h, w = y.shape
        by, buv = binding.DevBuf.from_numpy(_padded(y, w + 3)), binding.DevBuf.from_numpy(uv)
        bufs += [by, buv]
        dev.append((by.ptr.value, buv.ptr.value, w, h, w + 3, 2 * ((w + 1) // 2)))
    got = net.prepare_from_frames_nv12(dev, on_device=True)
    for g, x in zip(got, want):
        assert np.array_equal(g, x)
    assert np.array_equal(got[0][:net.inputs], _expected(_rgb(frames)[0], 12, 12)[1].ravel())
    net.close()
    for b in bufs:
        b.free()


def test_host_strided_planes_through_python(tmp_path):
    """rows of a wider buffer are passed through as pitches (no copy)"""
    wts = _wts(tmp_path, seed=5)
    frames = _host_frames(400)
    views = []
    for y, uv in frames:
        wy = np.full((y.shape[0], y.shape[1] + 7), 0xEE, np.uint8)
        wuv = np.full((uv.shape[0], uv.shape[1] + 2, 2), 0xEE, np.uint8)
        wy[:, :y.shape[1]] = y
        wuv[:, :uv.shape[1]] = uv
        vy, vuv = wy[:, :y.shape[1]], wuv[:, :uv.shape[1]]
        assert not vy.flags["C_CONTIGUOUS"] and vy.strides == (y.shape[1] + 7, 1)
        assert not vuv.flags["C_CONTIGUOUS"] and vuv.strides == (2 * uv.shape[1] + 4, 2, 1)
        views.append((vy, vuv))
    net = binding.Net(CFG, wts, batch=3)
    net.set_input_per_image(True)
    want = net.prepare_from_frames_nv12(frames)
    got = net.prepare_from_frames_nv12(views)
    got_vu = net.prepare_from_frames_nv12([(y, uv[..., ::-1]) for y, uv in views], layout="nv21")  # negative stride: copied by the binding
    for g in (got, got_vu):
        for x, w in zip(g, want):
            assert np.array_equal(x, w)
    assert np.array_equal(want[0][net.inputs:2 * net.inputs], _expected(_rgb(frames)[1], 12, 12)[1].ravel())
    net.close()


# ------------------------------------------------------------------------------------------------------------------- CLI
def test_cli_frames_nv12_blocks_equal_the_u8_path(tmp_path):
    exe = os.path.join(ROOT, "yolo_quantization_amd", "bin", "darknet")
    wts = _wts(tmp_path, seed=1)
    names = str(tmp_path / "x.names")
    open(names, "w").write("\n".join(["ant", "bee", "cat", "dog", "eel"]) + "\n")
    data = str(tmp_path / "x.data")
    open(data, "w").write(f"classes= 5\nnames = {names}\n")
    specs = [((37, 53), 0, 256, 0, 256), ((24, 24), 40, 140, 100, 156), ((30, 17), 100, 230, 60, 200), ((13, 15), 0, 90, 120, 136)]
    raws, ppms, frames = [], [], []
    for k, ((h, w), lo, hi, clo, chi) in enumerate(specs):
        y, uv = _yuv(w, h, 80 + k, lo, hi, clo, chi)
        raw = str(tmp_path / f"im{k}_{w}x{h}.nv12")
        with open(raw, "wb") as f:
            f.write(y.tobytes() + uv.tobytes())
        ppm = str(tmp_path / f"im{k}.ppm")
        _write_ppm(ppm, nv12_to_rgb(y, uv))
        raws.append(raw); ppms.append(ppm); frames.append((y, uv))
    lst_raw, lst_ppm = str(tmp_path / "raw.txt"), str(tmp_path / "ppm.txt")
    open(lst_raw, "w").write("\n".join(raws) + "\n")
    open(lst_ppm, "w").write("\n".join(ppms) + "\n")
    args = ["-thresh", "0.3", "-boxes"]

    def run(extra, ok=True):
        r = subprocess.run([exe, "detector", "test", data, CFG, wts] + extra + args, capture_output=True, text=True, timeout=300)
        if not ok:
            return r
        assert r.returncode == 0, r.stderr
        return _blocks(r.stdout)

    want = run(["-list", lst_ppm, "-batch", "3", "-frames", "u8"])
    got = run(["-list", lst_raw, "-batch", "3", "-frames", "nv12"])
    assert [g[0] for g in got] == raws and [w[0] for w in want] == ppms
    assert [g[1:] for g in got] == [w[1:] for w in want]  # apart from the file names
    assert any(line.startswith("box:") for blk in want for line in blk)
    assert run([raws[0], "-frames", "nv12"])[0][1:] == run([ppms[0], "-frames", "u8"])[0][1:]  # the single image too
    # another matrix, against its own conversion; NV21 reads the pairs the other way round
    ppm709 = str(tmp_path / "im0_709f.ppm")
    _write_ppm(ppm709, nv12_to_rgb(*frames[0], matrix="bt709f"))
    assert run([raws[0], "-frames", "nv12", "-matrix", "bt709f"])[0][1:] == run([ppm709, "-frames", "u8"])[0][1:]
    ppm21 = str(tmp_path / "im0_21.ppm")
    _write_ppm(ppm21, nv12_to_rgb(*frames[0], layout="nv21"))
    assert run([raws[0], "-frames", "nv21"])[0][1:] == run([ppm21, "-frames", "u8"])[0][1:]
    # a file of the wrong length, a name without a size: refused, and the message says which
    short = str(tmp_path / "short_53x37.nv12")
    open(short, "wb").write(open(raws[0], "rb").read()[:-1])
    r = run([short, "-frames", "nv12"], ok=False)
    n = 53 * 37 + 19 * 2 * 27
    assert r.returncode != 0 and f"holds {n} bytes, the file holds {n - 1}" in r.stderr
    nosize = str(tmp_path / "nosize.nv12")
    open(nosize, "wb").write(open(raws[0], "rb").read())
    r = run([nosize, "-frames", "nv12"], ok=False)
    assert r.returncode != 0 and "_<W>x<H>.nv12" in r.stderr
