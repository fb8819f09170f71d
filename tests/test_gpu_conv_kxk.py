"""GPU suite (`-m gpu`) for the general-shape convolution (conv_kxk.hip, kernel id 9) and its ref-f32 twin: layer grid against
the oracle, tensor windows, the kxk_unit net against the oracle net, kernel ids and run modes.  Nothing here reads the
reference's sources."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle
from yolo_quantization_amd import binding, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def device():
    binding.init(0)


def _rand_layer(rng, n, c, k, m_lo=2.0 ** -13, m_hi=2.0 ** -8):
    wq = rng.integers(0, 256, (n, c * k * k), dtype=np.uint8)
    zp_w = rng.integers(90, 166, n, dtype=np.uint8)
    bias = rng.integers(-20000, 20000, n).astype(np.int32)
    M = rng.uniform(m_lo, m_hi, n)
    shift = np.floor(-np.log2(M)).astype(int)
    M0 = np.round(M * 2.0 ** shift * 2 ** 31)
    return wq, zp_w, bias, M0 * 2.0 ** -31, 2.0 ** -shift.astype(np.float64)


def _oracle(x, wq, zp_w, k, s, pad, zp_in, bias, mv, sv, zp_act, act, store, accum):
    accs, u8s = [], []
    for b in range(x.shape[0]):
        a = oracle.conv_acc(x[b], wq, zp_w, k, s, pad, zp_in, accum)
        accs.append(a)
        u8s.append(oracle.requant(a, bias, mv, sv, zp_act, act, store))
    return np.stack(accs), np.stack(u8s)


# (B, c, n, H, W, k, stride, pad, act)
GRID = [
    (1, 3, 64, 38, 38, 7, 2, 3, "leaky"),      # 7x7 stride-2 stem on the RGB image (cs = 4)
    (2, 3, 96, 35, 35, 11, 4, 0, "relu"),      # AlexNet's 11x11 stride 4
    (1, 1, 17, 13, 11, 5, 1, 2, "linear"),     # one channel, odd map
    (2, 8, 16, 12, 12, 2, 1, 0, "leaky"),      # even size, padding 0
    (1, 24, 32, 13, 13, 3, 1, 1, "leaky"),     # 3x3 on c % 16 != 0
    (1, 40, 255, 9, 7, 4, 2, 3, "relu6"),      # pad = k - 1
    (1, 64, 64, 26, 26, 5, 1, 2, "leaky"),
    (1, 256, 64, 10, 10, 5, 2, 2, "leaky"),
    (3, 24, 17, 11, 9, 5, 3, 4, "linear"),     # stride 3, pad = k - 1
    (1, 8, 16, 5, 5, 2, 1, 3, "leaky"),        # whole windows in the padding
    (2, 3, 64, 20, 20, 5, 2, 2, "leaky"),
    (1, 4, 8, 9, 9, 3, 2, 1, "relu6"),         # 4 channels in a 16-byte cell (dense 4-byte units)
    (1, 9, 33, 9, 9, 3, 1, 1, "leaky"),
    (2, 17, 40, 15, 31, 1, 1, 0, "linear"),    # 1x1 on c = 17
    (1, 1, 1, 1, 1, 11, 1, 5, "leaky"),        # 1x1 map, 11x11 kernel
    (1, 32, 40, 60, 60, 11, 6, 5, "leaky"),    # large stride: still the 256-pixel tile, at width 16 (101 x 101 cells: 112 bytes under the LDS limit)
    (1, 40, 17, 19, 23, 7, 4, 3, "relu"),
    (1, 512, 64, 7, 7, 7, 1, 3, "leaky"),      # K = 25088
    (2, 3, 16, 32, 30, 3, 2, 1, "leaky"),      # 3x3 stride-2 stem on the image (yolov4-tiny): the 3x3 blob's general section
    (1, 64, 64, 13, 13, 3, 1, 0, "leaky"),     # 3x3 at padding 0 on c % 16 == 0
    (1, 64, 32, 20, 20, 3, 3, 1, "relu6"),     # 3x3 stride 3 on c % 16 == 0
    (1, 32, 48, 12, 12, 3, 2, 2, "linear"),    # 3x3 stride 2 at padding 2
]
MODES = [("exact", binding.ACC_EXACT, binding.STORE_WRAP), ("exact", binding.ACC_EXACT, binding.STORE_SATURATE),
         ("ref_f32", binding.ACC_REF_F32, binding.STORE_WRAP)]


@pytest.mark.parametrize("case", GRID, ids=lambda c: "B%d_c%d_n%d_%dx%d_k%d_s%d_p%d_%s" % c)
@pytest.mark.parametrize("mode", MODES, ids=["exact-wrap", "exact-sat", "ref_f32"])
def test_layer_grid_vs_oracle(case, mode):
    B, c, n, H, W, k, s, pad, act = case
    _, accum, store = mode
    rng = np.random.default_rng(sum(case[:8]) + 7 * accum + store)
    x = rng.integers(0, 256, (B, c, H, W), dtype=np.uint8)
    wq, zp_w, bias, mv, sv = _rand_layer(rng, n, c, k)
    zp_in, zp_act = int(rng.integers(0, 256)), int(rng.integers(0, 200))
    xt = binding.DevTensor.from_nchw(x, zp_in)
    got = binding.conv_forward(xt, wq, zp_w, k, bias, mv, sv, zp_in, zp_act, 0.05, binding.ACT[act], store, accum,
                               want_acc=True, want_f32=True, stride=s, pad=pad)
    assert binding.shim().mi355_last_conv_kernel() == (9 if accum == binding.ACC_EXACT else 6)
    acc, u8 = _oracle(x, wq, zp_w, k, s, pad, zp_in, bias, mv, sv, zp_act, oracle.ACT[act], store,
                      oracle.ACC_EXACT if accum == binding.ACC_EXACT else oracle.ACC_REF_F32)
    OH, OW = (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1
    assert np.array_equal(got["int32"], acc), "int32 accumulators"
    assert np.array_equal(got["u8"].reshape(B, n, OH * OW), u8), "uint8 activations"
    assert np.array_equal(got["f32"], oracle.dequant(u8, zp_act, np.float32(0.05))), "quant_stop float tail"
    if accum == binding.ACC_EXACT:  # without acc_out / y_f32 the same bytes
        fast = binding.conv_forward(xt, wq, zp_w, k, bias, mv, sv, zp_in, zp_act, 0.05, binding.ACT[act], store, accum,
                                    want_acc=False, want_f32=False, stride=s, pad=pad)
        assert np.array_equal(fast["u8"], got["u8"])


@pytest.mark.parametrize("case", [(1, 24, 40, 13, 11, 5, 2, 2, "leaky"), (1, 3, 16, 20, 20, 3, 2, 1, "relu6"), (2, 8, 17, 9, 9, 4, 1, 3, "linear")])
@pytest.mark.parametrize("store", [binding.STORE_WRAP, binding.STORE_SATURATE], ids=["wrap", "saturate"])
def test_shift_value_not_a_power_of_two(case, store):
    """shift_value that is not an exact power of two (the reference's prep never makes one, a user may): the kernel's two-step
    requant_u8 branch instead of the folded multiplier."""
    B, c, n, H, W, k, s, pad, act = case
    rng = np.random.default_rng(sum(case[:8]))
    x = rng.integers(0, 256, (B, c, H, W), dtype=np.uint8)
    wq, zp_w, bias, mv, sv = _rand_layer(rng, n, c, k)
    sv = sv * rng.uniform(0.55, 0.95, n)  # 0 < shift_value <= 1, no longer 2^-s
    xt = binding.DevTensor.from_nchw(x, 11)
    got = binding.conv_forward(xt, wq, zp_w, k, bias, mv, sv, 11, 23, 0.05, binding.ACT[act], store, binding.ACC_EXACT,
                               want_acc=True, want_f32=True, stride=s, pad=pad)
    assert binding.shim().mi355_last_conv_kernel() == 9
    acc, u8 = _oracle(x, wq, zp_w, k, s, pad, 11, bias, mv, sv, 23, oracle.ACT[act], store, oracle.ACC_EXACT)
    assert np.array_equal(got["int32"], acc)
    assert np.array_equal(got["u8"].reshape(B, n, -1), u8)
    assert np.array_equal(got["f32"], oracle.dequant(u8, 23, np.float32(0.05)))


def test_input_from_a_channel_window():
    """x as a channel window of a wider tensor (a route's buffer read by the next layer): channels [16, 16 + c) of 64; a window
    that does not start on the kernel's unit is refused with its own message, nothing launched."""
    B, c, n, H, W, k, s, pad = 2, 24, 20, 15, 13, 5, 2, 2
    rng = np.random.default_rng(12)
    xw = rng.integers(0, 256, (B, 64, H, W), dtype=np.uint8)
    wq, zp_w, bias, mv, sv = _rand_layer(rng, n, c, k)
    OH, OW = (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1
    S = binding.shim()
    wide = binding.DevTensor.from_nchw(xw, 9)
    blob = binding.DevBuf.from_numpy(binding.conv_pack(wq, zp_w, c, k, bias, mv, sv))
    d = binding.ConvDesc(n, c, k, s, pad, binding.ACT["leaky"], binding.STORE_WRAP, binding.ACC_EXACT, 9, 23, 0.05)
    y = binding.DevTensor(B, OH, OW, n, 23)
    win = binding.Tensor.from_buffer_copy(wide.t)
    win.C = c
    win.data = C.c_void_p(wide.t.data + 16)
    binding.check(S.mi355_conv_forward(C.byref(d), C.byref(win), blob.ptr, None, None, y.ref(), None, None, None), "window")
    binding.check(S.mi355_stream_sync(None), "sync")
    _, u8 = _oracle(xw[:, 16:16 + c], wq, zp_w, k, s, pad, 9, bias, mv, sv, 23, oracle.ACT["leaky"], oracle.STORE_WRAP, oracle.ACC_EXACT)
    assert np.array_equal(y.to_nchw().reshape(B, n, -1), u8)
    win.data = C.c_void_p(wide.t.data + 4)
    assert S.mi355_conv_forward(C.byref(d), C.byref(win), blob.ptr, None, None, y.ref(), None, None, None) == -22
    assert "aligned" in S.mi355_last_error().decode()


def test_grid_exercises_wrap_and_int32_overflow():
    """Wrap-on-store cases exist in the grid's data, and a saturated K = 7 x 7 x 1024 layer whose exact accumulators leave int32
    wraps exactly like the oracle's."""
    B, c, n, H, W, k = 1, 1024, 16, 7, 7, 7
    x = np.full((B, c, H, W), 255, np.uint8)
    rng = np.random.default_rng(5)
    wq, zp_w, bias, mv, sv = _rand_layer(rng, n, c, k)
    wq[:] = 255
    zp_w[:] = 0
    xt = binding.DevTensor.from_nchw(x, 255)
    got = binding.conv_forward(xt, wq, zp_w, k, bias, mv, sv, 255, 23, 0.05, binding.ACT["leaky"], binding.STORE_WRAP,
                               binding.ACC_EXACT, want_acc=True, stride=1, pad=3)
    acc, u8 = _oracle(x, wq, zp_w, k, 1, 3, 255, bias, mv, sv, 23, oracle.ACT["leaky"], oracle.STORE_WRAP, oracle.ACC_EXACT)
    assert (acc < 0).any(), "the true sum exceeds 2^31: the int32 accumulator must have wrapped"
    assert np.array_equal(got["int32"], acc)
    assert np.array_equal(got["u8"].reshape(B, n, H * W), u8)


def test_output_into_a_channel_window():
    """y as a channel window of a wider tensor (a route's buffer): the layer's channels land at the offset, the other channels
    of every cell keep their bytes."""
    B, c, n, H, W, k, s, pad = 2, 24, 20, 14, 14, 5, 2, 2
    rng = np.random.default_rng(11)
    x = rng.integers(0, 256, (B, c, H, W), dtype=np.uint8)
    wq, zp_w, bias, mv, sv = _rand_layer(rng, n, c, k)
    OH, OW = (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1
    S = binding.shim()
    xt = binding.DevTensor.from_nchw(x, 7)
    for coff in (0, 16, 36):
        wide = binding.DevTensor(B, OH, OW, 64, 23)
        before = wide.to_nchw()
        win = binding.Tensor.from_buffer_copy(wide.t)
        win.C = n
        win.data = C.c_void_p(wide.t.data + coff)
        blob = binding.DevBuf.from_numpy(binding.conv_pack(wq, zp_w, c, k, bias, mv, sv))
        d = binding.ConvDesc(n, c, k, s, pad, binding.ACT["leaky"], binding.STORE_WRAP, binding.ACC_EXACT, 7, 23, 0.05)
        binding.check(S.mi355_conv_forward(C.byref(d), xt.ref(), blob.ptr, None, None, C.byref(win), None, None, None), "window")
        binding.check(S.mi355_stream_sync(None), "sync")
        got = wide.to_nchw()
        _, u8 = _oracle(x, wq, zp_w, k, s, pad, 7, bias, mv, sv, 23, oracle.ACT["leaky"], oracle.STORE_WRAP, oracle.ACC_EXACT)
        assert np.array_equal(got[:, coff:coff + n].reshape(B, n, -1), u8), coff
        keep = np.ones(64, bool)
        keep[coff:coff + n] = False
        assert np.array_equal(got[:, keep], before[:, keep]), coff


# ------------------------------------------------------------------------------------------------ whole networks
def _run(cfg, wts, x, accum, graph=False):
    net = binding.Net(cfg, wts, batch=x.shape[0], accum=accum, dump_int32=True, use_graph=graph)
    xq = net.prepare_from_float(synth.image_u8_to_float(x))
    assert np.array_equal(xq, x.ravel())
    net.forward()
    if graph:
        net.forward()
    net.sync()
    outs = [net.pull(i) for i in range(net.n)]
    kern = [net.conv_kernel(i) for i in range(net.n)]
    return net, outs, kern


@pytest.mark.parametrize("accum", [binding.ACC_EXACT, binding.ACC_REF_F32], ids=["exact", "ref_f32"])
@pytest.mark.parametrize("seed,act_gain", [(1, 1.0), (2, 4.0)])
def test_kxk_unit_net_vs_oracle(cfg_dir, tmp_path, accum, seed, act_gain):
    """kxk_unit through the plain-C host equals the oracle net on every tensor (int32, u8, float tails; yolo floats to 1 ulp).
    Seed 2 scales the activations up so that wrapping stores occur."""
    cfg = os.path.join(cfg_dir, "kxk_unit.cfg")
    wts = str(tmp_path / "k.weights")
    synth.synth_weights(cfg, wts, seed=seed, act_gain=act_gain)
    x = synth.synth_image_u8(3, 48, 48, seed=100 + seed, batch=2)
    net, outs, kern = _run(cfg, wts, x, accum)
    info = net.info
    net.close()
    convs = [i for i, inf in enumerate(info) if inf["type"] == binding.T_CONV]
    assert [kern[i] for i in convs] == [9 if accum == binding.ACC_EXACT else 6] * len(convs)
    onet = oracle.OracleNet(cfg, wts)
    onet.prepare(np.float32(1.0 / 255.0), 0)
    oacc = oracle.ACC_EXACT if accum == binding.ACC_EXACT else oracle.ACC_REF_F32
    for b in range(2):
        want = onet.forward(x[b], accum=oacc)
        for i, inf in enumerate(info):
            per = inf["outputs"]
            sl = slice(b * per, (b + 1) * per)
            if inf["type"] == binding.T_CONV:
                assert np.array_equal(outs[i]["int32"][sl], want[i]["int32"].ravel()), f"image {b} layer {i} int32"
            if inf["type"] != binding.T_YOLO:
                assert np.array_equal(outs[i]["u8"][sl], want[i]["u8"].ravel()), f"image {b} layer {i} u8"
            if inf["quant_stop"] and inf["type"] != binding.T_YOLO:
                assert np.array_equal(outs[i]["f32"][sl], want[i]["f32"].ravel()), f"image {b} layer {i} f32"
            if inf["type"] == binding.T_YOLO:
                np.testing.assert_allclose(outs[i]["f32"][sl], want[i]["f32"].ravel(), rtol=0, atol=2e-7)


def test_kxk_unit_run_modes_equal_plain_run(cfg_dir, tmp_path):
    """Graph capture, a replica in flight beside its parent, and an NKD5 export / import give the plain run's bytes."""
    cfg = os.path.join(cfg_dir, "kxk_unit.cfg")
    wts = str(tmp_path / "k.weights")
    synth.synth_weights(cfg, wts, seed=3)
    x = synth.synth_image_u8(3, 48, 48, seed=9, batch=2)
    x2 = synth.synth_image_u8(3, 48, 48, seed=10, batch=2)
    net, want, _ = _run(cfg, wts, x, binding.ACC_EXACT)
    net.close()
    gnet, got, _ = _run(cfg, wts, x, binding.ACC_EXACT, graph=True)
    gnet.close()
    for i in range(len(want)):
        for key in want[i]:
            assert np.array_equal(got[i][key], want[i][key]), ("graph", i, key)
    # replica: parent and replica run different inputs back to back on their own streams
    parent = binding.Net(cfg, wts, batch=2)
    parent.prepare_fixed(1.0 / 255.0, 0)
    parent.push_input(x2); parent.forward(); parent.sync()
    want2 = [parent.pull(i) for i in range(parent.n)]
    parent.push_input(x); parent.forward(); parent.sync()
    want1 = [parent.pull(i) for i in range(parent.n)]
    rep = parent.replica()
    rep.push_input(x2); parent.push_input(x)
    rep.sync(); parent.sync()
    for _ in range(4):
        rep.forward(); parent.forward()
    rep.sync(); parent.sync()
    for i in range(parent.n):
        a, r = parent.pull(i), rep.pull(i)
        for key in a:
            if key != "int32":
                assert np.array_equal(a[key], want1[i][key]), ("parent", i, key)
                assert np.array_equal(r[key], want2[i][key]), ("replica", i, key)
    rep.close()  # a parent is freed after its replicas
    packed = parent.export_packed()
    imp = binding.Net(cfg, None, batch=2)
    imp.import_packed(packed)
    imp.push_input(x); imp.forward(); imp.sync()
    for i in range(imp.n):
        g = imp.pull(i)
        for key in g:
            if key != "int32":
                assert np.array_equal(g[key], want1[i][key]), ("import", i, key)
    imp.close()
    parent.close()


@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("accum", [binding.ACC_EXACT, binding.ACC_REF_F32], ids=["exact", "ref_f32"])
def test_kxk_unit_net_vs_reference_golden(golden_dir, cfg_dir, tmp_path, seed, accum):
    """kxk_unit through the plain-C host equals the tensors the reference itself produced (tests/golden/kxk_unit_seed*.npz):
    every tensor in ref-f32 mode; in exact mode too, since the generator marks every accumulator of this net fp32-exact."""
    g = np.load(os.path.join(golden_dir, f"kxk_unit_seed{seed}.npz"))
    cfg = os.path.join(cfg_dir, "kxk_unit.cfg")
    wts = str(tmp_path / "w.weights")
    assert synth.synth_weights(cfg, wts, seed=seed, act_gain=float(g["act_gain"]))["sha256"] == str(g["weights_sha256"])
    net, outs, _ = _run(cfg, wts, g["input_u8"][None], accum)
    info = net.info
    net.close()
    for i, inf in enumerate(info):
        if inf["type"] == binding.T_CONV:
            assert accum == binding.ACC_REF_F32 or g[f"L{i}_fp32_exact"].all()
            assert np.array_equal(outs[i]["int32"], g[f"L{i}_int32"]), f"layer {i} int32"
        if inf["type"] != binding.T_YOLO:
            assert np.array_equal(outs[i]["u8"], g[f"L{i}_u8"]), f"layer {i} u8"
        if inf["type"] == binding.T_YOLO:
            np.testing.assert_allclose(outs[i]["f32"], g[f"L{i}_f32"], rtol=0, atol=2e-7)
        elif inf["quant_stop"]:
            assert np.array_equal(outs[i]["f32"], g[f"L{i}_f32"]), f"layer {i} f32"


# per conv layer, the kernel family (mi355_last_conv_kernel) that served it before the general kernel existed (read on the GPU from the
# parent commit's build: batch 1, synthetic weights / image of seed 1, default plan)
IDS_BEFORE = {
    "yolov3-tiny_quant.cfg": [1, 7, 2, 2, 5, 5, 5, 3, 5, 3, 3, 5, 3],
    "yolov3_quant.cfg": [1, 2, 3, 2, 2, 3, 2, 3, 2, 5, 3, 5, 3, 5, 3, 5, 3, 5, 3, 5, 3, 5, 3, 5, 3, 5, 5, 3, 5, 3, 5, 3, 5, 3, 5, 3, 5, 3,
                         5, 3, 5, 3, 5, 5, 3, 5, 3, 5, 3, 5, 3, 5, 3, 5, 3, 5, 3, 5, 3, 3, 5, 5, 3, 5, 3, 5, 3, 3, 5, 5, 3, 5, 3, 5, 3],
}


@pytest.mark.parametrize("cfg_name,size", [("yolov3-tiny_quant.cfg", 416), ("yolov3_quant.cfg", 608)])
def test_existing_nets_keep_their_kernels(cfg_dir, tmp_path, cfg_name, size):
    """The dispatcher reaches the general kernel only where the others refuse: every layer of yolov3-tiny@416 / YOLOv3@608 reports the
    kernel it reported before."""
    cfg = os.path.join(cfg_dir, cfg_name)
    wts = str(tmp_path / "w.weights")
    synth.synth_weights(cfg, wts, seed=1)
    net = binding.Net(cfg, wts, batch=1)
    net.prepare_fixed(1.0 / 255.0, 0)
    net.push_input(synth.synth_image_u8(3, size, size, seed=1)[None]); net.forward(); net.sync()
    kern = [net.conv_kernel(i) for i in range(net.n) if net.info[i]["type"] == binding.T_CONV]
    net.close()
    assert kern == IDS_BEFORE[cfg_name]
