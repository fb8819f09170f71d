"""Transposed convolution without a device: the host prep of tr_unit against the oracle's prep on the flipped weights, the parsed sizes,
the blob size, the packer's, the parser's and the prep's refusals (no kernel is launched by any of them)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
from yolo_quantization_amd import binding, synth

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
DECONVS = {1: (16, 16, 12, 4, 2, 1, 24), 3: (16, 32, 12, 2, 2, 0, 24)}  # layer: n, c, H = W, k, s, p, OH = OW


def test_host_prep_equals_the_oracle_on_the_flipped_weights(cfg_dir, tmp_path):
    cfg, wts = os.path.join(cfg_dir, "tr_unit.cfg"), str(tmp_path / "tr.weights")
    recs = {r["i"]: r for r in synth.synth_weights(cfg, wts, seed=6)["layers"]}
    net = binding.Net(cfg, wts, batch=2)
    net.prepare_host_only(1.0 / 255.0, 0)
    assert [i for i, inf in enumerate(net.info) if inf["type"] == binding.T_DECONV] == list(DECONVS)
    for i, (n, c, hw, k, s, p, ohw) in DECONVS.items():
        inf = net.info[i]
        assert (inf["n"], inf["c"], inf["h"], inf["w"], inf["size"], inf["stride"], inf["pad"]) == (n, c, hw, hw, k, s, p)
        assert (inf["out_c"], inf["out_h"], inf["out_w"]) == (n, ohw, ohw) and ohw == (hw - 1) * s + k - 2 * p
        got, r = net.prep(i), recs[i]
        want = oracle.prep_conv(n, c, k, r["w_hat"], r["zp_w"], r["s_w"], got["s_in"], got["zp_in"], got["s_act"], r["biases"], *r["bn"])
        for key in want:
            assert np.array_equal(got[key], want[key]), (i, key)
    net.close()


def test_pack_size_is_a_function_of_n_c_k_s():
    size = binding.shim().mi355_conv_tr_pack_size
    assert size(1, 16, 4, 2) == size(128, 16, 4, 2) < size(129, 16, 4, 2)       # rows padded to the largest M tile
    assert size(16, 1, 4, 2) == size(16, 16, 4, 2) < size(16, 17, 4, 2) == size(16, 32, 4, 2) < size(16, 33, 4, 2)
    assert size(16, 32, 2, 2) < size(16, 32, 3, 2) < size(16, 32, 4, 2) < size(16, 32, 11, 2)
    # fragments are dense per phase: k4 is 16 K-steps on 32 channels at stride 1, 2 and 4 alike; only the two int32 per (phase, row) grow
    assert len({size(16, 32, 4, st) - 2 * 4 * st * st * 128 for st in (1, 2, 4)}) == 1
    for bad in ((0, 16, 3, 2), (16, 0, 3, 2), (16, 16, 0, 2), (16, 16, 12, 2), (16, 16, 3, 0), (16, 16, 3, 9)):
        assert size(*bad) == 0, bad


@pytest.mark.parametrize("k,s,mv,msg", [(12, 2, 0.5, "1 <= ksize <= 11"), (3, 9, 0.5, "1 <= stride <= 8"), (3, 2, 1.5, "0 < M_value < 1")])
def test_pack_refusals(k, s, mv, msg):
    w = np.zeros((16, 8, k, k), np.uint8)
    S = binding.shim()
    blob = np.full(1 << 16, 7, np.uint8)
    args = [np.zeros(8, np.uint8), np.zeros(8, np.int32), np.full(8, mv), np.full(8, 0.5)]
    rc = S.mi355_conv_tr_pack(8, 16, k, s, w.ctypes.data, *[a.ctypes.data for a in args], blob.ctypes.data)
    assert rc == -22 and msg in S.mi355_last_error().decode()
    assert (blob == 7).all()


K4 = "size=4\nstride=2\npadding=1\nactivation=leaky"


@pytest.mark.parametrize("old,new,accum,msg", [
    ("[convolutional]", "[deconvolutional]", 0, "first layer"),                                     # layer 0, on the image
    (K4, K4.replace("leaky", "logistic"), 0, "activation=logistic"),
    (K4, K4.replace("padding=1", "padding=4"), 0, "0..size-1"),
    (K4, K4.replace("stride=2", "stride=9"), 0, "stride must be 1..8"),
    (K4, K4.replace("size=4", "size=12"), 0, "size must be 1..11"),
    ("filters=16\nsize=2", "filters=3\nsize=2", 0, "3-filter [deconvolutional]"),                   # prep: in front of the route
    (K4, K4, 1, "MI355_ACC_EXACT only"),                                                            # prep: a ref-f32 net
    ("[deconvolutional]", "[deconv]", 0, None),                                                     # the short name parses and preps
])
def test_parser_and_prep_refusals(cfg_dir, tmp_path, old, new, accum, msg):
    txt = open(os.path.join(cfg_dir, "tr_unit.cfg")).read()
    assert old in txt
    cfg = tmp_path / "t.cfg"
    cfg.write_text(txt.replace(old, new, 1))
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from yolo_quantization_amd import binding, synth\n"
            "binding.host().parse_network_cfg(%r.encode(), 0)\n"
            "synth.synth_weights(%r, %r, seed=6)\n"
            "binding.Net(%r, %r, batch=1, accum=%d).prepare_host_only()\nprint('prepared')\n"
            % (ROOT, str(cfg), str(cfg), str(tmp_path / "t.weights"), str(cfg), str(tmp_path / "t.weights"), accum))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    if msg is None:
        assert r.returncode == 0 and "prepared" in r.stdout, r.stderr
    else:
        assert r.returncode != 0 and "prepared" not in r.stdout and msg in (r.stderr + r.stdout)
