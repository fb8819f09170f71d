"""Depthwise convolution without a device: the host prep of dw_unit against its dense twin, the blob size, the parser's refusals."""
import os
import subprocess
import sys

import numpy as np
import pytest

from yolo_quantization_amd import binding, synth

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def test_host_prep_equals_the_dense_twin(cfg_dir, tmp_path):
    """biases_int32, M_value, shift_value, M0 and shift of every layer of dw_unit equal those of the net with `groups` removed and the
    weights expanded with the zero-point fill (identity 2)."""
    cfg = os.path.join(cfg_dir, "dw_unit.cfg")
    twin_cfg = str(tmp_path / "twin.cfg")
    with open(twin_cfg, "w") as f:
        f.write("".join(line for line in open(cfg) if not line.startswith("groups=")))
    wts, twin_wts = str(tmp_path / "dw.weights"), str(tmp_path / "twin.weights")
    synth.synth_weights(cfg, wts, seed=4)
    synth.synth_weights(cfg, twin_wts, seed=4, dense_twin=True)
    net, twin = binding.Net(cfg, wts, batch=2), binding.Net(twin_cfg, twin_wts, batch=2)
    net.prepare_host_only(1.0 / 255.0, 0)
    twin.prepare_host_only(1.0 / 255.0, 0)
    convs = [i for i, inf in enumerate(net.info) if inf["type"] == binding.T_CONV]
    assert convs == [0, 1, 2, 3, 5, 6]
    for i in convs:
        a, b = net.prep(i), twin.prep(i)
        for key in a:
            assert np.array_equal(a[key], b[key]), (i, key)
    assert net.packed_size() < twin.packed_size()
    net.close()
    twin.close()


def test_pack_size_is_a_function_of_c_and_k():
    S = binding.shim()
    assert S.mi355_conv_dw_pack_size(16, 3) == S.mi355_conv_dw_pack_size(64, 3) < S.mi355_conv_dw_pack_size(65, 3)
    assert S.mi355_conv_dw_pack_size(64, 3) < S.mi355_conv_dw_pack_size(64, 5) < S.mi355_conv_dw_pack_size(64, 11)
    assert S.mi355_conv_dw_pack_size(0, 3) == S.mi355_conv_dw_pack_size(16, 0) == S.mi355_conv_dw_pack_size(16, 12) == 0


@pytest.mark.parametrize("old,new,msg", [
    ("groups=32\nfilters=32\nsize=3", "groups=2\nfilters=32\nsize=3", "groups < channels"),
    ("groups=16\nfilters=16", "groups=16\nfilters=32", "channel multipliers"),
    ("filters=16\nsize=3", "groups=3\nfilters=3\nsize=3", "first layer"),  # layer 0, on the 3-channel image
    ("groups=16\n", "groups=1\n", None),                                   # groups=1 parses as before
])
def test_parser_refusals(cfg_dir, tmp_path, old, new, msg):
    txt = open(os.path.join(cfg_dir, "dw_unit.cfg")).read()
    assert old in txt
    txt = txt.replace(old, new, 1)
    cfg = tmp_path / "t.cfg"
    cfg.write_text(txt)
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from yolo_quantization_amd import binding\n"
            "binding.host().parse_network_cfg(%r.encode(), 0)\nprint('parsed')\n" % (ROOT, str(cfg)))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    if msg is None:
        assert r.returncode == 0 and "parsed" in r.stdout
    else:
        assert r.returncode != 0 and msg in (r.stderr + r.stdout)
