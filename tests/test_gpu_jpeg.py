"""The JPEG input path on the device: mi355_jpeg_idct and mi355_jpeg_to_rgb through the C-ABI against the numpy restatement of
stb_image's integer arithmetic (jpeg_ref) on built inputs, every fixture through binding.jpeg_decode against the bytes the compiled
reference loaded (tests/golden/jpeg_expected.npz), Net.prepare_from_jpeg against prepare_from_frames_u8 on those bytes, and the CLI on
.jpg files against the CLI on the PPM of the same pixels.  Every comparison is exact."""
import ctypes as C
import glob
import os
import subprocess

import numpy as np
import pytest

import jpeg_ref
from frames_util import CFG, ROOT, _bits, _blocks, _write_ppm, _wts
from yolo_quantization_amd import binding

pytestmark = pytest.mark.gpu

JPEG_DIR = os.path.join(ROOT, "tests", "golden", "jpeg")
NAMES = sorted(n for n in (os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(JPEG_DIR, "*.jpg")))
               if n not in ("progressive", "cmyk"))
# fixtures the 12 x 12 test network's letterbox can serve (both resized sides >= 2), of every sampling, both other colour modes,
# restart intervals and several scans
NET_NAMES = ["420_51x37", "422_restart2_51x37", "444_48x32", "440_23x61", "411_61x23", "410_61x27", "grey_51x37", "rgb_adobe0_48x32",
             "420_noninterleaved_37x27", "420_3x4", "h1v4_11x43", "444_q100_51x37"]


@pytest.fixture(scope="module", autouse=True)
def _dev():
    binding.init(0)


@pytest.fixture(scope="module")
def expected():
    with np.load(os.path.join(ROOT, "tests", "golden", "jpeg_expected.npz")) as z:
        return {k: z[k] for k in z.files}


def data_of(name):
    with open(os.path.join(JPEG_DIR, name + ".jpg"), "rb") as f:
        return f.read()


# ------------------------------------------------------------------------------------------------------------------ inverse DCT
def _check_idct(planes, what):
    want = [jpeg_ref.idct_plane(c, q) for c, q in planes]  # OverflowError: the input would leave stb's 32-bit arithmetic
    got = binding.jpeg_idct(planes)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and np.array_equal(g, w), f"{what}: plane {k}"
    return want


def _mixed_coefficients(rng, bh, bw):
    """a DC level that reaches both clamps and the range between them, a third of the AC positions filled"""
    c = (rng.integers(-24, 25, (bh, bw, 64)) * (rng.random((bh, bw, 64)) < 0.3)).astype(np.int16)
    c[:, :, 0] = rng.integers(-90, 91, (bh, bw))
    return c


@pytest.mark.parametrize("blocks", [1, 7, 8, 9, 31, 32, 33, 65])
def test_idct_block_counts_around_the_wave_and_workgroup_size(blocks):
    rng = np.random.default_rng(blocks)
    q = rng.integers(1, 25, 64).astype(np.uint16)
    want = _check_idct([(_mixed_coefficients(rng, 1, blocks), q)], f"{blocks} blocks in a row")
    if blocks >= 31:
        assert (want[0] == 0).mean() > .02 and (want[0] == 255).mean() > .02 and ((want[0] > 0) & (want[0] < 255)).mean() > .3
    if blocks == 65:
        _check_idct([(_mixed_coefficients(rng, 5, 13), q)], "13 x 5 blocks")


def test_idct_several_planes_of_different_sizes_in_one_launch():
    rng = np.random.default_rng(100)
    shapes = [(1, 1), (3, 5), (6, 7), (1, 33), (2, 2), (9, 4), (1, 1)]  # 1 + 15 + 42 + 33 + 4 + 36 + 1 blocks: planes start mid-workgroup
    planes = [(_mixed_coefficients(rng, bh, bw), rng.integers(1, 30, 64).astype(np.uint16)) for bh, bw in shapes]
    want = _check_idct(planes, "seven planes")
    assert len({w.tobytes() for w in want}) == len(want)


def test_idct_dc_only():
    dc = np.arange(-1024, 1024, 4).astype(np.int16)
    c = np.zeros((8, 64, 64), np.int16)
    c[:, :, 0] = dc.reshape(8, 64)
    for qdc in (1, 8, 16):
        q = np.full(64, 7, np.uint16)
        q[0] = qdc
        want = _check_idct([(c, q)], f"DC only x {qdc}")
        assert all((w.reshape(-1, 8, w.shape[1] // 8, 8).std(axis=(1, 3)) == 0).all() for w in want)  # flat blocks


@pytest.mark.parametrize("big", [28000, 300])
def test_idct_each_ac_position_alone(big):
    c = np.zeros((2, 63, 64), np.int16)
    for k in range(1, 64):
        c[0, k - 1, k] = big
        c[1, k - 1, k] = -big
    c[:, :, 0] = 40  # +/- around a mid grey: both clamps with 28000, none with 300
    want = _check_idct([(c, np.ones(64, np.uint16))], f"one AC coefficient of +/- {big}")
    assert ((want[0] == 0).any() and (want[0] == 255).any()) == (big == 28000)


def test_idct_products_that_wrap_16_bits_and_16_bit_tables():
    rng = np.random.default_rng(7)
    c = np.zeros((4, 16, 64), np.int16)
    q = np.ones(64, np.uint16)
    q[0], q[1], q[8], q[9] = 300, 4000, 65535, 21846  # 16-bit quantisers
    c[:, :, 0] = rng.integers(215, 223, (4, 16))  # 215 .. 222 x 300 = 64500 .. 66600 -> wraps to -1036 .. 1064
    c[:, :, 1] = rng.integers(16, 18, (4, 16))    # 16 x 4000 -> -1536, 17 x 4000 -> 2464
    c[:, :, 8] = rng.integers(-400, 401, (4, 16))  # x 65535 == x -1 in 16 bits
    c[:, :, 9] = 3 * rng.integers(-1, 2, (4, 16))  # 3 x 21846 = 65538 -> 2
    d = jpeg_ref.dequantise(c, q)
    prod = c.astype(np.int64) * q
    assert all((np.abs(prod[:, :, k]) > 32767).any() for k in (0, 1, 8, 9)) and np.abs(d).max() <= 2464
    assert np.array_equal(d[:, :, 8], -c[:, :, 8]) and set(np.unique(d[:, :, 9])) == {-2, 0, 2}
    _check_idct([(c, q)], "wrapping products")


def test_idct_random_coefficients_random_tables():
    rng = np.random.default_rng(8)
    planes = []
    for k in range(6):
        c = (rng.integers(-60, 61, (4, 8, 64)) * (rng.random((4, 8, 64)) < 0.15)).astype(np.int16)
        c[:, :, 0] = rng.integers(-200, 200, (4, 8))
        planes.append((c, rng.integers(1, 3 + 10 * k, 64).astype(np.uint16)))
    want = _check_idct(planes, "random")
    allv = np.concatenate([w.ravel() for w in want])
    assert (allv == 0).mean() > .05 and (allv == 255).mean() > .05 and ((allv > 0) & (allv < 255)).mean() > .2


def test_idct_refusals_launch_nothing():
    L = binding.shim()
    c = binding.DevBuf.from_numpy(np.zeros(64, np.int16))
    q = binding.DevBuf.from_numpy(np.ones(64, np.uint16))
    o = binding.DevBuf.from_numpy(np.full(64, 0xA5, np.uint8))
    t = (binding.JpegPlane * 1)()
    t[0].coef, t[0].quant, t[0].out, t[0].blocks_w, t[0].blocks_h, t[0].first_block = c.ptr, q.ptr, o.ptr, 1, 1, 0
    tdev = binding.DevBuf.from_numpy(np.frombuffer(bytes(t), np.uint8))
    for field, value in (("blocks_w", 0), ("first_block", 3), ("out", None), ("coef", C.c_void_p(c.ptr.value + 2))):
        keep = getattr(t[0], field)
        setattr(t[0], field, value)
        assert L.mi355_jpeg_idct(tdev.ptr, t, 1, None) == -22 and b"jpeg_idct:" in L.mi355_last_error(), field
        setattr(t[0], field, keep)
    assert L.mi355_jpeg_idct(tdev.ptr, t, 0, None) == -22
    binding.check(L.mi355_stream_sync(None), "sync")
    assert (o.to_numpy(np.uint8, 64) == 0xA5).all()
    for b in (c, q, o, tdev):
        b.free()


# ----------------------------------------------------------------------------------------------------------- upsampling + colour
WIDTHS = [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 33]
HEIGHTS = [1, 2, 3, 4, 5, 17]


def _component(rng, w, h, hs, vs, pad):
    """a random plane of the component's real size, `pad` more rows and columns of other bytes around it that no pixel may depend on"""
    rows, cols = -(-h // vs), -(-w // hs)
    return {"plane": rng.integers(0, 256, (rows + pad, cols + pad), dtype=np.uint8), "rows": rows, "hs": hs, "vs": vs}


def _check_to_rgb(images, what, pitch_pad=0):
    got = binding.jpeg_to_rgb(images, pitch_pad=pitch_pad)
    for k, (g, im) in enumerate(zip(got, images)):
        want = jpeg_ref.to_rgb(im["w"], im["h"], im["mode"], im["components"])
        assert np.array_equal(g, want), f"{what}: image {k} ({im['w']} x {im['h']})"


@pytest.mark.parametrize("hs,vs", [(hs, vs) for hs in (1, 2, 3, 4) for vs in (1, 2, 3, 4)])
def test_to_rgb_every_sampling_every_size_in_one_launch(hs, vs):
    """72 images of different sizes in one launch: Y at (1, 1), both chroma planes at (hs, vs), YCbCr -> RGB"""
    rng = np.random.default_rng(10 * hs + vs)
    images = [{"w": w, "h": h, "mode": "ycbcr",
               "components": [_component(rng, w, h, 1, 1, 0), _component(rng, w, h, hs, vs, 1), _component(rng, w, h, hs, vs, 2)]}
              for w in WIDTHS for h in HEIGHTS]
    _check_to_rgb(images, f"({hs}, {vs})")


@pytest.mark.parametrize("mode", ["rgb", "grey", "ycbcr"])
def test_to_rgb_colour_modes_mixed_samplings_and_padded_pitch(mode):
    rng = np.random.default_rng(len(mode))
    factors = [(2, 2), (2, 1), (1, 2), (4, 2), (1, 1), (3, 1)]  # the first component is upsampled too
    images = []
    for k, (w, h) in enumerate([(33, 17), (16, 4), (5, 5), (1, 1), (2, 17), (9, 3)]):
        comps = [_component(rng, w, h, *factors[(k + j) % len(factors)], j) for j in range(1 if mode == "grey" else 3)]
        images.append({"w": w, "h": h, "mode": mode, "components": comps})
    for pad in (0, 1, 7):  # 3 w + pad: rows at every alignment, the bytes behind a row untouched (binding.jpeg_to_rgb checks them)
        _check_to_rgb(images, f"{mode} pitch + {pad}", pitch_pad=pad)


def test_to_rgb_ycbcr_reaches_both_clamps_and_the_masked_green_term():
    # every (Cb, Cr) pair at four luma levels: 256 x 256 x 4 pixels
    cb, cr = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8))
    images = [{"w": 256, "h": 256, "mode": "ycbcr",
               "components": [{"plane": np.full((256, 256), yy, np.uint8), "hs": 1, "vs": 1}, {"plane": cb, "hs": 1, "vs": 1}, {"plane": cr, "hs": 1, "vs": 1}]}
              for yy in (0, 77, 200, 255)]
    _check_to_rgb(images, "all chroma pairs")
    want = jpeg_ref.to_rgb(256, 256, "ycbcr", images[1]["components"])
    assert (want == 0).any() and (want == 255).any()


def test_to_rgb_refusals_launch_nothing():
    L = binding.shim()
    plane = binding.DevBuf.from_numpy(np.zeros(64, np.uint8))
    out = binding.DevBuf.from_numpy(np.full(192, 0xA5, np.uint8))
    t = (binding.JpegImage * 1)()
    t[0].rgb, t[0].w, t[0].h, t[0].pitch, t[0].mode = out.ptr, 8, 8, 24, 2
    t[0].comp[0].plane, t[0].comp[0].pitch, t[0].comp[0].rows, t[0].comp[0].hs, t[0].comp[0].vs = plane.ptr, 8, 8, 1, 1
    tdev = binding.DevBuf.from_numpy(np.frombuffer(bytes(t), np.uint8))
    for obj, field, value in ((t[0], "pitch", 23), (t[0], "mode", 3), (t[0], "w", 0), (t[0].comp[0], "rows", 7), (t[0].comp[0], "pitch", 7),
                              (t[0].comp[0], "hs", 5), (t[0].comp[0], "plane", None), (t[0], "mode", 0)):  # mode 0 reads comp[1], which is null
        keep = getattr(obj, field)
        setattr(obj, field, value)
        assert L.mi355_jpeg_to_rgb(tdev.ptr, t, 1, None) == -22 and b"jpeg_to_rgb:" in L.mi355_last_error(), field
        setattr(obj, field, keep)
    binding.check(L.mi355_stream_sync(None), "sync")
    assert (out.to_numpy(np.uint8, 192) == 0xA5).all()
    for b in (plane, out, tdev):
        b.free()


# ------------------------------------------------------------------------------------------------------------- whole files
def test_every_fixture_decodes_to_the_bytes_the_reference_loaded(expected):
    assert len(NAMES) >= 40
    for n in NAMES:
        got = binding.jpeg_decode(data_of(n))
        assert got.shape == expected[n].shape and np.array_equal(got, expected[n]), n


def test_all_fixtures_as_one_batch(expected, tmp_path):
    got = binding.jpeg_decode([data_of(n) for n in NAMES])  # the C-ABI calls: 2 launches for all of them
    for n, g in zip(NAMES, got):
        assert np.array_equal(g, expected[n]), n
    net = binding.Net(CFG, _wts(tmp_path), batch=1)
    files = {n: data_of(n) for n in NAMES}
    for names in (NAMES[::-3], NAMES, NAMES[:1] * 3):  # network_jpeg_decode_gpu: buffers grow, are reused, one image's bytes in every slot
        got = binding.jpeg_decode([files[n] for n in names], net=net)
        for n, g in zip(names, got):
            assert np.array_equal(g, expected[n]), n
    net.close()


def test_a_bad_slot_is_named_and_nothing_is_launched(expected, tmp_path):
    net = binding.Net(CFG, _wts(tmp_path), batch=3)
    good = [data_of(n) for n in NET_NAMES[:3]]
    sizes = net.prepare_from_jpeg(good)
    before = net._pull_input()
    waits = net.host_waits()
    for bad, message in ((data_of("progressive"), "jpeg slot 1: progressive"), (data_of("cmyk"), "jpeg slot 1: 4 components"),
                         (good[1][:200], "jpeg slot 1: "), (b"P6\n1 1\n255\n", "jpeg slot 1: no SOI")):
        with pytest.raises(binding.JpegError, match=message):
            net.prepare_from_jpeg([good[0], bad, good[2]])
        with pytest.raises(binding.JpegError, match=message):
            binding.jpeg_decode([good[0], bad, good[2]], net=net)
        with pytest.raises(binding.JpegError, match=message):
            binding.jpeg_decode([good[0], bad, good[2]])
    assert net.host_waits() == waits  # the refused calls never reached the device
    assert np.array_equal(net._pull_input(), before)
    assert sizes == [expected[n].shape[1::-1] for n in NET_NAMES[:3]]
    net.close()


# ------------------------------------------------------------------------------------------------------------- host level
def _run(net, sizes):
    net.forward()
    net.sync()
    deep = max(i for i, inf in enumerate(net.info) if inf["type"] == binding.T_CONV)
    return net.pull(deep), net.detect([s[0] for s in sizes], [s[1] for s in sizes], thresh=0.005)


def _assert_same_input_and_run(a, b, sizes, what):
    xa, xb = a._pull_input(), b._pull_input()
    assert np.array_equal(xa, xb), f"{what}: input bytes"
    (sa, za), (sb, zb) = a.input_quantization(), b.input_quantization()
    assert np.array_equal(_bits(sa), _bits(sb)) and np.array_equal(za, zb), f"{what}: scales / zero points"
    (la, da), (lb, db) = _run(a, sizes), _run(b, sizes)
    for k in lb:
        assert np.array_equal(la[k], lb[k]), f"{what}: deep layer {k}"
    assert len(da) == len(db) == a.batch
    for slot, (x, y) in enumerate(zip(da, db)):
        assert x.keys() == y.keys()
        for k in x:
            assert np.array_equal(x[k], y[k]), f"{what}: detections of slot {slot}: {k}"
    return xa


@pytest.mark.parametrize("mode", ["shared", "per_image", "on_device", "on_device_per_image"])
def test_prepare_from_jpeg_equals_frames_u8_on_the_expected_pixels(expected, tmp_path, mode):
    wts = _wts(tmp_path)
    a, b = binding.Net(CFG, wts, batch=3), binding.Net(CFG, wts, batch=3)
    for net in (a, b):
        if "per_image" in mode:
            net.set_input_per_image(True)
        if "on_device" in mode:
            net.set_input_on_device(True)
    seen = set()
    for first in (0, 3, 6, 9):  # four consecutive batches of different images: the staging block and the device buffers are reused
        names = NET_NAMES[first:first + 3]
        sizes = a.prepare_from_jpeg([data_of(n) for n in names])
        assert sizes == [expected[n].shape[1::-1] for n in names]
        b.prepare_from_frames_u8([expected[n] for n in names])
        seen.add(_assert_same_input_and_run(a, b, sizes, f"{mode} {names}").tobytes())
    assert len(seen) == 4  # four different inputs
    a.close(); b.close()


def test_prepare_from_jpeg_graph_replay_and_replica(expected, tmp_path):
    wts = _wts(tmp_path, seed=5)
    parent = binding.Net(CFG, wts, batch=3, use_graph=True)
    parent.set_input_per_image(True)
    ref = binding.Net(CFG, wts, batch=3)
    ref.set_input_per_image(True)
    handle = None
    for first in (0, 3):  # the captured graph replays the second batch
        names = NET_NAMES[first:first + 3]
        sizes = parent.prepare_from_jpeg([os.path.join(JPEG_DIR, n + ".jpg") for n in names])  # paths
        ref.prepare_from_frames_u8([expected[n] for n in names])
        _assert_same_input_and_run(parent, ref, sizes, f"graph {names}")
        handle = handle or parent.graph_handle()
        assert handle and parent.graph_handle() == handle
    rep = parent.replica()  # its own staging block, buffers and stream
    na, nb = NET_NAMES[6:9], NET_NAMES[9:12]
    sa = rep.prepare_from_jpeg([data_of(n) for n in na])
    sb = parent.prepare_from_jpeg([data_of(n) for n in nb])
    for _ in range(2):
        parent.forward()
        rep.forward()
    for net, names, sizes in ((rep, na, sa), (parent, nb, sb)):
        ref.prepare_from_frames_u8([expected[n] for n in names])
        _assert_same_input_and_run(net, ref, sizes, f"replica {names}")
    rep.close()
    ref.close()
    parent.close()


# ------------------------------------------------------------------------------------------------------------------- CLI
def test_cli_on_jpeg_files_prints_what_it_prints_for_the_ppm_of_the_same_pixels(expected, tmp_path):
    exe = os.path.join(ROOT, "yolo_quantization_amd", "bin", "darknet")
    wts = _wts(tmp_path, seed=1)
    names = str(tmp_path / "x.names")
    open(names, "w").write("\n".join(["ant", "bee", "cat", "dog", "eel"]) + "\n")
    data = str(tmp_path / "x.data")
    open(data, "w").write(f"classes= 5\nnames = {names}\n")
    picks = ["420_51x37", "440_23x61", "grey_51x37", "410_61x27", "rgb_ids_48x32"]
    jpg = [os.path.join(JPEG_DIR, n + ".jpg") for n in picks]
    ppm = []
    for n in picks:
        ppm.append(str(tmp_path / (n + ".ppm")))
        _write_ppm(ppm[-1], expected[n])
    renamed = str(tmp_path / "no_extension")  # a JPEG is recognised by its first two bytes
    open(renamed, "wb").write(data_of(picks[2]))
    args = ["-thresh", "0.3", "-boxes"]

    def run(extra, ok=True):
        r = subprocess.run([exe, "detector", "test", data, CFG, wts] + extra + args, capture_output=True, text=True, timeout=300)
        assert (r.returncode == 0) == ok, r.stderr
        return _blocks(r.stdout) if ok else r.stderr

    def lines(blocks):  # everything but the file name
        return [b[1:] for b in blocks]

    def listed(paths, name):
        p = str(tmp_path / name)
        open(p, "w").write("\n".join(paths) + "\n")
        return p

    one_jpg, one_ppm = run([jpg[0]]), run([ppm[0]])
    assert lines(one_jpg) == lines(one_ppm) and one_jpg[0][0] == jpg[0]
    assert lines(run([jpg[0], "-batch", "2", "-input_device"])) == lines(one_ppm)
    want = run(["-list", listed(ppm, "ppm.txt"), "-batch", "3"])
    assert any(line.startswith("box:") for blk in want for line in blk)
    got = run(["-list", listed(jpg, "jpg.txt"), "-batch", "3"])
    assert [g[0] for g in got] == jpg and lines(got) == lines(want)
    mixed = [jpg[0], ppm[1], renamed, ppm[3], jpg[4]]  # .jpg, .ppm and a nameless JPEG in one list, of different sizes
    got = run(["-list", listed(mixed, "mixed.txt"), "-batch", "3"])
    assert [g[0] for g in got] == mixed and lines(got) == lines(want)
    assert lines(run(["-list", listed(mixed, "mixed2.txt"), "-batch", "2", "-frames", "u8", "-input_device"])) == lines(want)
    bad = os.path.join(JPEG_DIR, "progressive.jpg")
    err = run(["-list", listed([jpg[0], ppm[1], bad], "bad.txt"), "-batch", "3"], ok=False)
    assert "slot 2" in err and bad in err and "progressive" in err
    err = run([os.path.join(JPEG_DIR, "cmyk.jpg")], ok=False)
    assert "slot 0" in err and "CMYK" in err
    png = str(tmp_path / "x.png")
    open(png, "wb").write(b"\x89PNG\r\n\x1a\n" + bytes(64))
    assert "PNG, BMP, GIF" in run([png], ok=False)
