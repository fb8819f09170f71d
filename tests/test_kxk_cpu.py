"""CPU suite for the general-shape convolution (conv_kxk.hip): packing of the shapes outside the specialised kernels, the
refused cases, and the plain-C host on a cfg made of such layers.  No GPU: the packing runs on the host, and the refusals
are decided before anything is launched."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
from yolo_quantization_amd import binding, synth

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
EINVAL = -22
HDR = np.dtype([("magic", "<u4"), ("n", "<i4"), ("c", "<i4"), ("ksize", "<i4"), ("mpad", "<i4"), ("cb", "<i4"),
                ("nchunks", "<i4"), ("upc", "<i4"), ("spc", "<i4"), ("ksteps", "<i4"), ("ktrue", "<i4"), ("first", "<i4"),
                ("off_wp", "<u8"), ("off_cw", "<u8"), ("off_dzp", "<u8"), ("off_bias", "<u8"), ("off_mval", "<u8"),
                ("off_sval", "<u8"), ("total", "<u8"), ("off_shift", "<u8"), ("pow2", "<i4"), ("generic", "<i4"),
                ("off_mprime", "<u8"), ("off_cwb", "<u8"), ("off_ws", "<u8"), ("off_ept", "<u8"), ("off_gen", "<u8")])


def _hdr(blob):
    return {k: int(v) for k, v in zip(HDR.names, np.frombuffer(blob[:HDR.itemsize].tobytes(), HDR)[0])}


def _layer(rng, n, c, k):
    wq = rng.integers(0, 256, (n, c * k * k), dtype=np.uint8)
    zp_w = rng.integers(90, 166, n, dtype=np.uint8)
    bias = rng.integers(-20000, 20000, n).astype(np.int32)
    shift = rng.integers(7, 12, n)
    M = np.round(rng.uniform(0.5, 1.0, n) * 2 ** 31) * 2.0 ** -31
    return wq, zp_w, bias, M, 2.0 ** -shift.astype(np.float64)


def _unit(c):
    return 4 if c <= 4 else (8 if c <= 8 else 16)


@pytest.mark.parametrize("n,c,k", [(64, 3, 7), (96, 3, 11), (256, 256, 5), (32, 24, 3), (16, 8, 2), (17, 1, 1), (40, 66, 4)])
def test_general_shapes_pack(n, c, k):
    """mi355_conv_pack_size / mi355_conv_pack accept the shape, and the A fragments hold w - 128 at (tap slot, channel) of the
    documented dense-K order with zero weights on padding taps, padding channels and padding filters."""
    S = binding.shim()
    rng = np.random.default_rng(n * 1000 + c * 10 + k)
    wq, zp_w, bias, M, sv = _layer(rng, n, c, k)
    sz = S.mi355_conv_pack_size(n, c, k)
    assert sz > 0
    blob = binding.conv_pack(wq, zp_w, c, k, bias, M, sv, activation=binding.ACT["leaky"], zp_act=23)
    assert blob.nbytes == sz
    h = _hdr(blob)
    assert h["generic"] == 1 and h["off_gen"] == h["off_wp"] and h["total"] == sz and h["n"] == n and h["c"] == c and h["ksize"] == k
    U = _unit(c)
    tpl = 16 // U
    assert h["cb"] == U and h["mpad"] % 128 == 0 and h["mpad"] >= n
    assert h["spc"] == -(-k * k // (2 * tpl)) and h["nchunks"] == (-(-c // 16) if U == 16 else 1)
    assert h["ksteps"] == h["nchunks"] * h["spc"]
    frag = blob[h["off_wp"]:h["off_wp"] + h["mpad"] // 32 * h["ksteps"] * 1024].view(np.int8)
    frag = frag.reshape(h["mpad"] // 32, h["ksteps"], 64, 16)
    want = np.zeros_like(frag)
    w = (wq.astype(np.int16) - 128).astype(np.int8).reshape(n, c, k * k)
    for g in range(h["ksteps"]):
        ch, st = divmod(g, h["spc"])
        for kh in range(2):
            for e in range(16):
                t, ci = (2 * st + kh) * tpl + e // U, ch * U + e % U
                if t < k * k and ci < c:
                    for mt in range(-(-n // 32)):
                        rows = np.arange(32 * mt, min(32 * mt + 32, n))
                        want[mt, g, 32 * kh + rows - 32 * mt, e] = w[rows, ci, t]
    assert np.array_equal(frag, want)
    # the zero-point algebra's per-channel constant over the TRUE K only: cw = 128 sum(w') + 128 K (128 - zp_w)
    cw = blob[h["off_cw"]:h["off_cw"] + 4 * n].view(np.int32)
    K = c * k * k
    ref = 128 * (wq.astype(np.int64) - 128).sum(1) + 128 * K * (128 - zp_w.astype(np.int64))
    assert np.array_equal(cw, ((ref + 2 ** 31) % 2 ** 32 - 2 ** 31).astype(np.int32))


def test_specialised_shapes_keep_their_packing():
    """The yolov3 shapes keep the specialised packing; 3x3 blobs carry the general kernel's fragments as a last section (for the
    strides / paddings the 3x3 kernels refuse), 1x1 blobs none (1x1 layers only exist at stride 1, pad 0)."""
    S = binding.shim()
    for (n, c, k) in ((16, 3, 3), (64, 32, 3), (256, 128, 1), (1024, 512, 3), (255, 256, 1)):
        rng = np.random.default_rng(n + c + k)
        wq, zp_w, bias, M, sv = _layer(rng, n, c, k)
        blob = binding.conv_pack(wq, zp_w, c, k, bias, M, sv)
        h = _hdr(blob)
        assert h["generic"] == 0 and blob.nbytes == S.mi355_conv_pack_size(n, c, k)
        if k == 1:
            assert h["off_gen"] == 0
            continue
        U = _unit(c)
        ksteps = (-(-c // 16) if U == 16 else 1) * -(-9 // (32 // U))
        gen = blob[h["off_gen"]:].view(np.int8)
        assert h["off_gen"] > max(h["off_wp"], h["off_ws"], h["off_ept"]) and gen.size == -(-n // 128) * 4 * ksteps * 1024
        # the first K-step of filter 0: taps 0 / 1 (unit 16) or taps 0..3 / 4..7 (unit 4) of the first channels
        w = (wq.astype(np.int16) - 128).astype(np.int8).reshape(n, c, 9)
        f = gen.reshape(-1, ksteps, 64, 16)[0, 0]
        if U == 16:
            assert np.array_equal(f[0], w[0, :16, 0]) and np.array_equal(f[32], w[0, :16, 1])
        else:
            assert np.array_equal(f[0].reshape(4, 4)[:, :3], w[0, :, :4].T)


def _desc(n, c, k, stride, pad):
    return binding.ConvDesc(n, c, k, stride, pad, binding.ACT["leaky"], 0, 0, 0, 23, 0.05)


def _fake_tensor(B, H, W, Cc):
    t = binding.Tensor()
    assert binding.shim().mi355_tensor_describe(C.byref(t), B, H, W, Cc)
    t.data = C.c_void_p(0x1000)  # never dereferenced: every case below is refused before a launch
    return t


def test_refused_cases_return_einval():
    S = binding.shim()
    rng = np.random.default_rng(0)
    # size 12: no packing, no forward
    assert S.mi355_conv_pack_size(16, 8, 12) == 0
    wq, zp_w, bias, M, sv = _layer(rng, 16, 8, 12)
    blob = np.zeros(1 << 16, np.uint8)
    assert S.mi355_conv_pack(16, 8, 12, wq.ctypes.data, zp_w.ctypes.data, bias.ctypes.data, M.ctypes.data, sv.ctypes.data,
                             blob.ctypes.data) == EINVAL
    assert "11" in S.mi355_last_error().decode()
    x = _fake_tensor(1, 20, 20, 8)
    d = _desc(16, 8, 12, 1, 6)
    assert S.mi355_conv_forward(C.byref(d), C.byref(x), blob.ctypes.data, None, None, None, None, None, None) == EINVAL
    assert "11" in S.mi355_last_error().decode()
    # 1x1 with stride 2 or padding: the reference's 1x1 branch is not a convolution there
    for (c, stride, pad) in ((8, 2, 0), (8, 1, 1), (24, 2, 0)):
        x = _fake_tensor(1, 20, 20, c)
        for accum in (binding.ACC_EXACT, binding.ACC_REF_F32):
            d = binding.ConvDesc(16, c, 1, stride, pad, binding.ACT["leaky"], 0, accum, 0, 23, 0.05)
            assert S.mi355_conv_forward(C.byref(d), C.byref(x), blob.ctypes.data, blob.ctypes.data, blob.ctypes.data, None, None, None,
                                        None) == EINVAL
            assert "1x1" in S.mi355_last_error().decode()


def test_grouped_convolution_is_refused_by_the_parser(tmp_path):
    cfg = tmp_path / "groups.cfg"
    txt = open(os.path.join(ROOT, "cfg", "kxk_unit.cfg")).read().replace("filters=48\n", "filters=48\ngroups=2\n", 1)
    cfg.write_text(txt)
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from yolo_quantization_amd import binding\n"
            "binding.host().parse_network_cfg(%r.encode(), 0)\n" % (ROOT, str(cfg)))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "grouped" in (r.stderr + r.stdout)


def test_host_parses_and_preps_kxk_unit(cfg_dir, tmp_path):
    """The plain-C host reads kxk_unit.cfg (7x7 / 5x5 / 4x4 sizes, strides 1-3, padding 0, channel counts off 16) and packs
    every conv layer: quantization_prep_host no longer stops on "unsupported convolution shape"."""
    cfg = os.path.join(cfg_dir, "kxk_unit.cfg")
    wts = str(tmp_path / "k.weights")
    synth.synth_weights(cfg, wts, seed=1)
    net = binding.Net(cfg, wts, batch=2)
    convs = [(inf["size"], inf["stride"], inf["pad"], inf["c"], inf["n"], inf["out_h"]) for inf in net.info if inf["type"] == binding.T_CONV]
    assert convs == [(7, 2, 3, 3, 24, 24), (3, 1, 1, 24, 48, 24), (3, 1, 0, 48, 40, 22), (5, 1, 2, 40, 20, 22),
                     (4, 1, 0, 20, 17, 19), (5, 2, 2, 17, 33, 10), (3, 3, 1, 66, 40, 4), (5, 1, 2, 40, 21, 4)]
    net.prepare_host_only()
    assert net.packed_size() > 0
    net.close()


def test_three_filter_conv_feeding_a_glue_layer_is_refused(tmp_path):
    """A 3-filter convolution stores the image's 4-byte plain cells; the glue kernels read 16-byte biased groups, so the host
    refuses such a layer in front of a maxpool / route / upsample / shortcut at prep time instead of computing wrong bytes."""
    cfg = tmp_path / "n3.cfg"
    cfg.write_text(open(os.path.join(ROOT, "cfg", "kxk_unit.cfg")).read().replace("filters=33\n", "filters=3\n", 1))  # the conv before the maxpool
    wts = str(tmp_path / "n3.weights")
    synth.synth_weights(str(cfg), wts, seed=1)
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from yolo_quantization_amd import binding\n"
            "net = binding.Net(%r, %r, batch=1)\n"
            "net.prepare_host_only()\n" % (ROOT, str(cfg), wts))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "3-filter" in (r.stderr + r.stdout)


@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("accum", [oracle.ACC_REF_F32, oracle.ACC_EXACT], ids=["ref_f32", "exact"])
def test_oracle_kxk_unit_vs_reference_golden(golden_dir, cfg_dir, tmp_path, seed, accum):
    """The oracle's restatement of im2col + GEMM for the general shapes (7x7 / 5x5 / 4x4 / 3x3 sizes, strides 1-3, padding 0,
    channel counts off 16, a route of unaligned channel counts, a yolo head) against the tensors the reference itself produced
    (tests/golden/kxk_unit_seed*.npz, tests/golden/make_golden_kxk.py).  ref-f32: every tensor.  Exact: every accumulator the
    generator marks as inside the fp32-exact regime (all of them on this net), then every tensor."""
    g = np.load(os.path.join(golden_dir, f"kxk_unit_seed{seed}.npz"))
    cfg = os.path.join(cfg_dir, "kxk_unit.cfg")
    wts = str(tmp_path / "w.weights")
    assert synth.synth_weights(cfg, wts, seed=seed, act_gain=float(g["act_gain"]))["sha256"] == str(g["weights_sha256"])
    net = oracle.OracleNet(cfg, wts)
    L0 = net.layers[0]
    x = synth.synth_image_u8(L0.c, L0.h, L0.w, seed=int(g["img_seed"]))
    assert np.array_equal(x, g["input_u8"])
    net.prepare(np.float32(1.0 / 255.0), 0)
    outs = net.forward(x, accum=accum, store=oracle.STORE_WRAP)
    nwrap = 0
    for i, L in enumerate(net.layers):
        if L.type == "conv":
            for k in ("biases_int32", "M_value", "shift_value", "M0", "shift"):
                assert np.array_equal(net.p[i][k], g[f"L{i}_{k}"]), (i, k)
            m = g[f"L{i}_fp32_exact"].ravel() if accum == oracle.ACC_EXACT else np.ones(g[f"L{i}_int32"].size, bool)
            assert m.all() or accum == oracle.ACC_EXACT
            assert np.array_equal(outs[i]["int32"].ravel()[m], g[f"L{i}_int32"][m]), f"layer {i} accumulators"
            sat = oracle.requant(outs[i]["int32"], net.p[i]["biases_int32"], net.p[i]["M_value"], net.p[i]["shift_value"],
                                 net.w[i]["zp_act"], oracle.ACT[L.activation], oracle.STORE_SATURATE)
            nwrap += int((sat.ravel() != g[f"L{i}_u8"]).sum())
        if L.type != "yolo":
            assert np.array_equal(outs[i]["u8"].ravel(), g[f"L{i}_u8"]), f"layer {i} uint8"
        if L.type == "yolo":
            np.testing.assert_allclose(outs[i]["f32"].ravel(), g[f"L{i}_f32"], rtol=0, atol=2e-7)
        elif L.quant_stop:
            assert np.array_equal(outs[i]["f32"].ravel(), g[f"L{i}_f32"]), f"layer {i} f32"
    assert (nwrap > 0) == (seed == 2), "seed 2 (act_gain 8) must exercise wrap-on-store, seed 1 need not"
