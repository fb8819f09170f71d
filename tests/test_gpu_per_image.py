"""Per-image input quantisation (set_input_quantization_per_image): every image of a batch gets its own layer-0 scale / zero point.

Slot b of every layer (and its detections) must equal the batch-1 run of the same network on image b alone, and the oracle prepared
with that image's own (scale, zero point).  The batches here really differ in min / max -- negative values (zero point > 0), a
near-constant image, contrast-scaled / flipped / shifted copies of the real test image -- so the shared-scale path is wrong in every
slot past 0, and two images share one (scale, zero point) to exercise bank-entry sharing."""
import os

import numpy as np
import pytest

from yolo_quantization_amd import binding, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module", autouse=True)
def _dev():
    binding.init(0)


def _synth_images(c, h, w, B, seed):
    """B float images [c][h][w] with distinct ranges; images 0 and 1 share one (scale, zero point)."""
    rng = np.random.default_rng(seed)
    out = []
    for b in range(B):
        u = rng.random((c, h, w), dtype=np.float32)
        kind = b % 5
        if b == 1:
            x = out[0][::-1].copy()  # same min / max as image 0: same bank entry
        elif kind == 0:
            x = u * np.float32(0.8 + 0.05 * b)
        elif kind == 1:
            x = (u - np.float32(0.35)) * np.float32(2.0 + 0.1 * b)  # negatives: zero point > 0
        elif kind == 2:
            x = np.float32(0.5) + u * np.float32(1e-3)  # near-constant
        elif kind == 3:
            x = -u * np.float32(0.2 + 0.01 * b)  # all negative
        else:
            x = u * np.float32(3.0) - np.float32(0.1 * (b % 7))
        out.append(np.ascontiguousarray(x, np.float32))
    return out


def _real_images(B):
    r = np.load(os.path.join(GOLDEN, "realimg_416.npz"))
    base = synth.dequantized_float_image(r["input_u8"], r["scale"], r["zero_point"], r["fmin"], r["imin"], r["fmax"], r["imax"])
    out = []
    for b in range(B):
        x = base
        if b % 4 == 1:
            x = x[:, ::-1, :]
        if b % 4 == 2:
            x = x[:, :, ::-1]
        if b % 3 == 1:
            x = np.roll(x, 13 * b, axis=2)  # shifted window
        if b == 1:
            x = out[0][:, :, ::-1]  # same min / max as image 0: same bank entry
        else:
            x = x * np.float32(0.6 + 0.02 * b) - np.float32(0.004 * b)  # contrast / offset: own scale and zero point
        out.append(np.ascontiguousarray(x, np.float32))
    return out


def _wts(tmp_path, cfg, seed=3):
    p = str(tmp_path / (os.path.basename(cfg) + ".weights"))
    synth.synth_weights(cfg, p, seed=seed)
    return p


def _layers(net):
    net.sync()
    return [net.pull(i) for i in range(net.n)]


def _slot(arr, b, per):
    return arr[b * per:(b + 1) * per]


def _batch1(cfg, wts, img, **kw):
    n1 = binding.Net(cfg, wts, batch=1, **kw)
    xq = n1.prepare_from_float_gpu(img)
    n1.forward()
    outs = _layers(n1)
    info = n1.info
    n1.close()
    return xq, outs, info


def _assert_slot_equals(outs, b, want, info, what):
    for i, inf in enumerate(info):
        per = inf["outputs"]
        for k in want[i]:
            if k in outs[i]:
                assert np.array_equal(_slot(outs[i][k], b, per), want[i][k]), f"{what}: slot {b} layer {i} {k}"


@pytest.mark.parametrize("accum", [binding.ACC_EXACT, binding.ACC_REF_F32])
def test_tiny_unit_per_image_equals_batch1_and_oracle(tmp_path, accum):
    import oracle
    cfg = os.path.join(ROOT, "cfg", "tiny_unit.cfg")
    wts = _wts(tmp_path, cfg)
    B = 5
    imgs = _synth_images(3, 12, 12, B, seed=11)
    net = binding.Net(cfg, wts, batch=B, accum=accum, dump_int32=True)
    net.set_input_per_image(True)
    xq, s, z = net.prepare_from_float_gpu(np.stack(imgs))
    assert len(set(zip(s.tolist(), z.tolist()))) == B - 1  # images 0 and 1 share an entry, the others differ
    assert (z > 0).any()
    net.forward()
    outs = _layers(net)
    onet = oracle.OracleNet(cfg, wts)
    for b in range(B):
        q, sb, zb = oracle.quantize_image(imgs[b])
        assert np.array_equal(_slot(xq, b, net.inputs), q.ravel()), f"input slot {b}"
        assert np.float32(s[b]) == sb and int(z[b]) == zb
        x1, want1, info = _batch1(cfg, wts, imgs[b], accum=accum, dump_int32=True)
        assert np.array_equal(x1, q.ravel())
        _assert_slot_equals(outs, b, want1, info, "batch-1")
        onet.prepare(sb, zb)
        ref = onet.forward(q.reshape(3, 12, 12), accum=accum)
        for i, inf in enumerate(net.info):
            if inf["type"] == binding.T_YOLO:
                continue
            per = inf["outputs"]
            assert np.array_equal(_slot(outs[i]["u8"], b, per), ref[i]["u8"].ravel()), f"oracle: slot {b} layer {i} u8"
            if inf["type"] == binding.T_CONV:
                assert np.array_equal(_slot(outs[i]["int32"], b, per), ref[i]["int32"].ravel()), f"oracle: slot {b} layer {i} int32"
    # the host quantiser gives the same bytes and scales
    net2 = binding.Net(cfg, wts, batch=B, accum=accum, dump_int32=True)
    net2.set_input_per_image(True)
    xh, sh, zh = net2.prepare_from_float(np.stack(imgs))
    assert np.array_equal(xh, xq) and np.array_equal(sh, s) and np.array_equal(zh, z)
    net2.forward()
    outs2 = _layers(net2)
    for i in range(net.n):
        for k in outs[i]:
            assert np.array_equal(outs2[i][k], outs[i][k]), f"host quantiser: layer {i} {k}"
    net2.close()
    net.close()


@pytest.mark.parametrize("cfgname", ["yolov3-tiny_quant.cfg", "yolov3-tiny_quant_relu6.cfg"])
def test_yolov3_tiny_batch_per_image(tmp_path, cfgname):
    cfg = os.path.join(ROOT, "cfg", cfgname)
    wts = _wts(tmp_path, cfg, seed=5)
    B = 64
    imgs = _real_images(B)
    net = binding.Net(cfg, wts, batch=B, keep_head_float=True)
    net.set_input_per_image(True)
    xq, s, z = net.prepare_from_float_gpu(np.stack(imgs))
    assert len(set(zip(s.tolist(), z.tolist()))) == B - 1
    net.forward()
    assert net.conv_kernel(0) == 1  # layer 0 on the first-layer MFMA kernel, per image
    kmap = {i: net.conv_kernel(i) for i in range(net.n) if net.info[i]["type"] == binding.T_CONV}
    assert kmap[0] == 1 and kmap[2] == 7 and kmap[4] == 2
    heads = [i for i, inf in enumerate(net.info) if inf["type"] == binding.T_YOLO]
    net.sync()
    got = {i: net.pull(i)["f32"] for i in heads}
    dets = {i: net.detections(i, net.info[i - 1]["n"] // 3 - 5, 416, 416, 0.005, 1, 2048) for i in heads}  # room for every cell
    # the shared-scale kernel map is unchanged
    ref_net = binding.Net(cfg, wts, batch=B)
    ref_net.prepare_from_float_gpu(np.stack(imgs))
    ref_net.forward()
    ref_net.sync()
    assert {i: ref_net.conv_kernel(i) for i in kmap} == kmap
    ref_net.close()
    n1 = binding.Net(cfg, wts, batch=1, keep_head_float=True)
    for b in list(range(0, B, 7)) + [1, B - 1]:
        x1 = n1.prepare_from_float_gpu(imgs[b])
        assert np.array_equal(_slot(xq, b, net.inputs), x1), f"input slot {b}"
        n1.forward()
        n1.sync()
        for i in heads:
            per = net.info[i]["outputs"]
            assert np.array_equal(_slot(got[i], b, per), n1.pull(i)["f32"]), f"slot {b} head {i}"
            c1, r1 = n1.detections(i, net.info[i - 1]["n"] // 3 - 5, 416, 416, 0.005, 1, 2048)
            cb, rb = dets[i]
            assert cb[b] == c1[0] and np.array_equal(rb[b][:cb[b]], r1[0][:c1[0]]), f"slot {b} detections {i}"
    n1.close()
    net.close()


def test_graph_replay_follows_new_images_without_recapture(tmp_path):
    cfg = os.path.join(ROOT, "cfg", "yolov3-tiny_quant.cfg")
    wts = _wts(tmp_path, cfg, seed=7)
    B = 8
    a = _real_images(B)
    b_imgs = _synth_images(3, 416, 416, B, seed=3)
    eager = binding.Net(cfg, wts, batch=B)
    graph = binding.Net(cfg, wts, batch=B, use_graph=True)
    for n in (eager, graph):
        n.set_input_per_image(True)
    heads = [i for i, inf in enumerate(eager.info) if inf["type"] == binding.T_YOLO]
    for imgs in (a, b_imgs, a):
        res = []
        for n in (eager, graph):
            n.prepare_from_float_gpu(np.stack(imgs))
            n.forward()
            n.sync()
            res.append([n.pull(i)["f32"] for i in heads])
        for x, y in zip(*res):
            assert np.array_equal(x, y)
    eager.close()
    graph.close()


_SMALL_CFG = """[net]
batch=1
subdivisions=1
width={w}
height={h}
channels=3

[convolutional]
batch_normalize=1
filters={n}
size=3
stride=1
pad=1
activation=leaky
quantized=1
quant_stop=0

[maxpool]
size=2
stride=2
quantized=1
quant_stop=0

[convolutional]
batch_normalize=1
filters=16
size=3
stride=1
pad=1
activation=leaky
quantized=1
quant_stop=0
"""


@pytest.mark.parametrize("planar", [True, False])
def test_other_first_layer_kernels(tmp_path, planar):
    """YOLOv3's 3 -> 32 without a pool (conv_first_mfma_kernel) at 608, batch 4; the VALU first-layer kernels at batch 3: an odd map
    (conv_first_u8_kernel, maxpool apart) and 24 filters on an even map (conv_first_pool_u8_kernel)"""
    cases = [(os.path.join(ROOT, "cfg", "yolov3_chain_quant.cfg"), 4)]
    for tag, (w, h, n) in {"odd": (13, 11, 16), "f24": (12, 10, 24)}.items():
        p = str(tmp_path / f"{tag}.cfg")
        open(p, "w").write(_SMALL_CFG.format(w=w, h=h, n=n))
        cases.append((p, 3))
    for cfgp, B in cases:
        wp = _wts(tmp_path, cfgp, seed=4)
        d = synth.read_cfg(cfgp)[0]
        H, W = int(d["height"]), int(d["width"])
        imgs = _synth_images(3, H, W, B, seed=B)
        net = binding.Net(cfgp, wp, batch=B)
        if not planar:
            net.set("input_direct", 0)
        net.set_input_per_image(True)
        net.prepare_from_float_gpu(np.stack(imgs))
        net.forward()
        outs = _layers(net)
        assert net.conv_kernel(0) == 1
        for b in range(B):
            n1 = binding.Net(cfgp, wp, batch=1)
            if not planar:
                n1.set("input_direct", 0)
            n1.prepare_from_float_gpu(imgs[b])
            n1.forward()
            want = _layers(n1)
            _assert_slot_equals(outs, b, want, n1.info, os.path.basename(cfgp))
            n1.close()
        net.close()


def test_replicas_in_flight_carry_their_own_images(tmp_path):
    cfg = os.path.join(ROOT, "cfg", "yolov3-tiny_quant.cfg")
    wts = _wts(tmp_path, cfg, seed=8)
    B = 4
    parent = binding.Net(cfg, wts, batch=B)
    parent.set_input_per_image(True)
    parent.prepare_from_float_gpu(np.stack(_real_images(B)))
    ex = [parent] + [parent.replica() for _ in range(3)]
    batches = [_synth_images(3, 416, 416, B, seed=20 + k) for k in range(4)]
    for n, imgs in zip(ex, batches):
        n.prepare_from_float_gpu(np.stack(imgs))
    for n in ex:
        n.forward()  # four batches in flight
    heads = [i for i, inf in enumerate(parent.info) if inf["type"] == binding.T_YOLO]
    got = []
    for n in ex:
        n.sync()
        got.append({i: n.pull(i)["f32"] for i in heads})
    n1 = binding.Net(cfg, wts, batch=1)
    for k, imgs in enumerate(batches):
        for b in range(B):
            n1.prepare_from_float_gpu(imgs[b])
            n1.forward()
            n1.sync()
            for i in heads:
                per = parent.info[i]["outputs"]
                assert np.array_equal(_slot(got[k][i], b, per), n1.pull(i)["f32"]), f"executor {k} slot {b} head {i}"
    n1.close()
    for r in ex[1:]:
        r.close()
    parent.close()


def test_detections_with_per_image_sizes_equal_oracle(tmp_path):
    import oracle
    cfg = os.path.join(ROOT, "cfg", "yolov3-tiny_quant.cfg")
    wts = _wts(tmp_path, cfg, seed=5)
    B = 3
    imgs = _real_images(B)
    net = binding.Net(cfg, wts, batch=B)
    net.set_input_per_image(True)
    net.prepare_from_float_gpu(np.stack(imgs))
    net.forward()
    net.sync()
    sizes = [(555, 1480), (640, 480), (416, 300)]
    sec = [s for s in synth.read_cfg(cfg) if s["type"] == "[yolo]"]
    heads = [i for i, inf in enumerate(net.info) if inf["type"] == binding.T_YOLO]
    for i, ys in zip(heads, sec):
        classes = int(ys["classes"])
        mask = np.array([int(v) for v in ys["mask"].split(",")], np.int32)
        anchors = np.array([float(v) for v in ys["anchors"].split(",")], np.float32)
        counts, recs = net.detections_sizes(i, classes, [w for w, _ in sizes], [h for _, h in sizes], 0.005, 0, 2048)
        out = net.pull(i)["f32"]
        per = net.info[i]["outputs"]
        hh, ww = net.info[i]["out_h"], net.info[i]["out_w"]
        for b, (imw, imh) in enumerate(sizes):
            cnt, want = oracle.yolo_detections(_slot(out, b, per), len(mask), classes, hh, ww, anchors, mask, 416, 416, imw, imh,
                                               0.005, 0, 2048)
            assert counts[b] == cnt
            k = min(cnt, 2048)
            g = recs[b][:k]
            # centre, objectness and scores bit-exact; width / height to a few ulp (the reference's exp, see mi355_yolo_detections)
            assert np.array_equal(g[:, [0, 1, 2, 5]], want[:, [0, 1, 2, 5]]) and np.array_equal(g[:, 6:], want[:, 6:])
            np.testing.assert_allclose(g[:, 3:5], want[:, 3:5], rtol=1e-5)
    net.close()


def test_general_kernel_first_layer_is_refused_and_mode_off_keeps_image0_scale(tmp_path):
    cfg = os.path.join(ROOT, "cfg", "kxk_unit.cfg")
    wts = _wts(tmp_path, cfg, seed=1)
    net = binding.Net(cfg, wts, batch=2)
    assert net.H.set_input_quantization_per_image(net.h, 1) == -22  # MI355_EINVAL
    with pytest.raises(binding.MI355Error):
        net.set_input_per_image(True)
    net.close()
    cfg = os.path.join(ROOT, "cfg", "tiny_unit.cfg")
    wts = _wts(tmp_path, cfg)
    imgs = _synth_images(3, 12, 12, 3, seed=5)
    net = binding.Net(cfg, wts, batch=3)
    xq = net.prepare_from_float_gpu(np.stack(imgs))  # mode off: image 0 defines the scale of every slot
    import oracle
    _, s0, z0 = oracle.quantize_image(imgs[0])
    for b in range(3):
        want = np.clip(np.round((imgs[b].astype(np.float32) / s0).astype(np.float64)) + z0, 0, 255).astype(np.uint8)
        assert np.array_equal(_slot(xq, b, net.inputs), want.ravel())
    net.close()


def test_bank_cache_evicts_and_reuses_entries(tmp_path):
    """B = 4, a bank of 8 slots: three batches of four new keys each (the third evicts the first's), then the second batch again
    (all cached).  Every slot equals its batch-1 run each time."""
    cfg = os.path.join(ROOT, "cfg", "tiny_unit.cfg")
    wts = _wts(tmp_path, cfg, seed=6)
    B = 4
    rng = np.random.default_rng(12)
    batches = [[(rng.random((3, 12, 12), dtype=np.float32) - np.float32(0.1 * k)) * np.float32(1.0 + 0.3 * (4 * j + k))
                for k in range(B)] for j in range(3)]
    net = binding.Net(cfg, wts, batch=B)
    net.set_input_per_image(True)
    n1 = binding.Net(cfg, wts, batch=1)
    for j, want_packed in ((0, 4), (1, 4), (2, 4), (1, 0), (0, 4)):
        _, s, z = net.prepare_from_float_gpu(np.stack(batches[j]))
        assert len(set(zip(s.tolist(), z.tolist()))) == B
        assert net.bank_packed() == want_packed, f"batch {j}"
        net.forward()
        outs = _layers(net)
        for b in range(B):
            n1.prepare_from_float_gpu(batches[j][b])
            n1.forward()
            _assert_slot_equals(outs, b, _layers(n1), n1.info, f"batch {j}")
    eb = net.bank_entry_bytes()
    assert eb % 256 == 0 and eb >= binding.shim().mi355_conv_pack_size(net.info[0]["n"], 3, 3)
    n1.close()
    net.close()


def test_graph_is_not_recaptured_when_images_change(tmp_path):
    cfg = os.path.join(ROOT, "cfg", "tiny_unit.cfg")
    wts = _wts(tmp_path, cfg, seed=2)
    B = 3
    net = binding.Net(cfg, wts, batch=B, use_graph=True)
    net.set_input_per_image(True)
    n1 = binding.Net(cfg, wts, batch=1)
    handle = None
    for seed in (1, 2, 3):
        imgs = _synth_images(3, 12, 12, B, seed=seed)
        net.prepare_from_float_gpu(np.stack(imgs))
        net.forward()
        outs = _layers(net)
        if handle is None:
            handle = net.graph_handle()
            assert handle
        assert net.graph_handle() == handle  # the same captured graph replays every batch
        for b in range(B):
            n1.prepare_from_float_gpu(imgs[b])
            n1.forward()
            _assert_slot_equals(outs, b, _layers(n1), n1.info, f"graph seed {seed}")
    n1.close()
    net.close()


def test_letterboxed_images_per_image(tmp_path):
    """prepare_from_images_gpu: images of different sizes and ranges letterboxed on the device, then quantised per image"""
    cfg = os.path.join(ROOT, "cfg", "tiny_unit.cfg")
    wts = _wts(tmp_path, cfg, seed=9)
    rng = np.random.default_rng(3)
    ims = [rng.random((3, 37, 53), dtype=np.float32) * np.float32(0.4),
           rng.random((3, 20, 12), dtype=np.float32) * np.float32(0.9) + np.float32(0.05),
           rng.random((3, 12, 12), dtype=np.float32) * np.float32(0.2) + np.float32(0.3)]
    net = binding.Net(cfg, wts, batch=3)
    net.set_input_per_image(True)
    xq, s, z = net.prepare_from_images_gpu(ims)
    assert len(set(s.tolist())) == 3
    net.forward()
    outs = _layers(net)
    n1 = binding.Net(cfg, wts, batch=1)
    for b, im in enumerate(ims):
        x1 = n1.prepare_from_images_gpu([im])
        assert np.array_equal(_slot(xq, b, net.inputs), x1), f"input slot {b}"
        n1.forward()
        _assert_slot_equals(outs, b, _layers(n1), n1.info, "letterbox")
    n1.close()
    net.close()


def _write_ppm(path, rgb_hwc):
    with open(path, "wb") as f:
        f.write(f"P6\n{rgb_hwc.shape[1]} {rgb_hwc.shape[0]}\n255\n".encode())
        f.write(np.ascontiguousarray(rgb_hwc, np.uint8).tobytes())


def _blocks(stdout):
    """per-image blocks of `detector test` output, the timing line reduced to the file name"""
    out, cur = [], None
    for line in stdout.splitlines():
        if ": Predicted in " in line:
            cur = [line.split(": Predicted in ")[0]]
            out.append(cur)
        elif cur is not None:
            cur.append(line)
    return out


def test_cli_list_blocks_equal_single_image_runs(tmp_path):
    import subprocess
    exe = os.path.join(ROOT, "yolo_quantization_amd", "bin", "darknet")
    cfg = os.path.join(ROOT, "cfg", "tiny_unit.cfg")
    wts = _wts(tmp_path, cfg, seed=1)
    names = str(tmp_path / "x.names")
    open(names, "w").write("\n".join(["ant", "bee", "cat", "dog", "eel"]) + "\n")
    data = str(tmp_path / "x.data")
    open(data, "w").write(f"classes= 5\nnames = {names}\n")
    rng = np.random.default_rng(8)
    specs = [((37, 53), 0, 256), ((24, 24), 40, 140), ((30, 17), 100, 230), ((12, 12), 0, 90)]  # sizes and byte ranges differ
    paths = []
    for k, ((h, w), lo, hi) in enumerate(specs):
        p = str(tmp_path / f"im{k}.ppm")
        _write_ppm(p, rng.integers(lo, hi, (h, w, 3), dtype=np.uint8))
        paths.append(p)
    lst = str(tmp_path / "list.txt")
    open(lst, "w").write("\n".join(paths) + "\n")
    args = ["-thresh", "0.3", "-boxes"]
    r = subprocess.run([exe, "detector", "test", data, cfg, wts, "-list", lst, "-batch", "3"] + args, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr
    got = _blocks(r.stdout)
    assert [g[0] for g in got] == paths  # one block per image, in list order (two batches: 3 + 1)
    for p, g in zip(paths, got):
        r1 = subprocess.run([exe, "detector", "test", data, cfg, wts, p] + args, capture_output=True, text=True, timeout=300)
        assert r1.returncode == 0, r1.stderr
        (want,) = _blocks(r1.stdout)
        assert g == want, p
        assert any(line.startswith("box:") for line in want) or want[1] == "0"
