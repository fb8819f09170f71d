"""Dilated convolution without a device: the numpy definition against the oracle at dilation 1 and against the stuffed
dense twin, the parser's sizes and refusals, and the plan of cfg/dil_unit.cfg (no kernel is launched by any of them)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
from yolo_quantization_amd import binding

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
BRANCHES = {1: 2, 3: 3, 5: 5}  # dil_unit.cfg: layer -> dilation


def dil_acc(x, wq, zp_w, k, d, p, zp_in):
    """The layer's definition in int64, wrapped to int32.  x: [c, H, W] uint8, wq: [n, c k k] uint8 -> [n, OH * OW]"""
    c, H, W = x.shape
    OH, OW = H + 2 * p - d * (k - 1), W + 2 * p - d * (k - 1)
    xp = np.pad(x.astype(np.int64), ((0, 0), (p, p), (p, p)), constant_values=zp_in)
    w = wq.reshape(-1, c, k, k).astype(np.int64) - np.asarray(zp_w, np.int64)[:, None, None, None]
    acc = sum(np.einsum("jc,chw->jhw", w[:, :, ky, kx], xp[:, ky * d:ky * d + OH, kx * d:kx * d + OW]) for ky in range(k) for kx in range(k))
    return acc.reshape(len(wq), OH * OW).astype(np.int32)


def stuffed_twin(wq, zp_w, c, k, d):
    """weights of the dense D x D layer that defines the same layer: zp_w[j] off the tap lattice"""
    D = d * (k - 1) + 1
    w = np.broadcast_to(np.asarray(zp_w, np.uint8)[:, None, None, None], (len(wq), c, D, D)).copy()
    w[:, :, ::d, ::d] = wq.reshape(-1, c, k, k)
    return w.reshape(len(wq), -1), D


@pytest.mark.parametrize("k,d,p", [(3, 1, 1), (2, 1, 0), (5, 1, 2), (3, 2, 2), (3, 5, 1), (2, 3, 1), (5, 2, 4), (6, 2, 0), (3, 4, 9)])
def test_definition_against_the_oracle_and_the_stuffed_twin(k, d, p):
    rng = np.random.default_rng(100 * k + d)
    c, n, H, W = 5, 4, 12, 13
    x = rng.integers(0, 256, (c, H, W), dtype=np.uint8)
    wq = rng.integers(0, 256, (n, c * k * k), dtype=np.uint8)
    zp_w = rng.integers(0, 256, n, dtype=np.uint8)
    wt, D = stuffed_twin(wq, zp_w, c, k, d)
    assert D <= 11
    assert np.array_equal(dil_acc(x, wq, zp_w, k, d, p, 9), oracle.conv_acc(x, wt, zp_w, D, 1, p, 9))


CONV = "[convolutional]\nfilters=%d\nsize=%d\nstride=%d\n%s\ndilation=%d\nactivation=leaky\nquantized=1\n"
HEAD = "[net]\nbatch=1\nheight=16\nwidth=20\nchannels=3\n" + CONV % (16, 3, 1, "pad=1", 1)


@pytest.mark.parametrize("k,pad,d,oh,ow", [(3, "pad=1", 2, 16, 20), (3, "pad=1", 6, 16, 20), (5, "pad=1", 3, 16, 20), (3, "padding=1", 2, 14, 18),
                                           (2, "pad=1", 3, 19, 23), (3, "padding=0", 7, 2, 6), (3, "pad=1", 1, 16, 20)])
def test_parsed_sizes(tmp_path, k, pad, d, oh, ow):
    cfg = tmp_path / "t.cfg"
    cfg.write_text(HEAD + CONV % (8, k, 1, pad, d))
    net = binding.Net(str(cfg), None, batch=1)
    inf = net.info[1]
    assert (inf["dilation"], inf["out_h"], inf["out_w"], inf["out_c"]) == (d, oh, ow, 8)
    assert inf["pad"] == (d * (k // 2) if pad == "pad=1" else int(pad.split("=")[1]))
    assert net.conv_kernel(1) == (13 if d > 1 else 0)
    net.close()


@pytest.mark.parametrize("txt,msg", [
    (HEAD + CONV % (8, 3, 1, "pad=1", 0), "dilation must be >= 1"),
    (HEAD + CONV % (8, 3, 2, "pad=1", 2), "needs stride=1"),
    (HEAD + CONV % (8, 1, 1, "pad=1", 2), "needs size >= 2"),
    (HEAD + (CONV % (16, 3, 1, "pad=1", 2)).replace("]\n", "]\ngroups=16\n"), "needs groups=1"),
    (HEAD.split("[convolutional]")[0] + CONV % (8, 3, 1, "pad=1", 2), "dilated first layer"),
    (HEAD + CONV % (3, 3, 1, "pad=1", 2), "4-byte cells"),
    (HEAD + CONV % (8, 3, 1, "padding=0", 8), "output map is empty"),
], ids=lambda v: v.replace(" ", "_") if len(v) < 30 else "")
def test_parser_refusals(tmp_path, txt, msg):
    """(the host dies through error(), as the reference does: a child process parses)"""
    cfg = tmp_path / "t.cfg"
    cfg.write_text(txt)
    code = ("import sys; sys.path.insert(0, %r)\nfrom yolo_quantization_amd import binding\n"
            "binding.host().parse_network_cfg(%r.encode(), 0)\nprint('parsed')\n" % (ROOT, str(cfg)))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "parsed" not in r.stdout and msg in r.stderr


def test_dil_unit_plans_kernel_13_on_its_branches(cfg_dir):
    net = binding.Net(os.path.join(cfg_dir, "dil_unit.cfg"), None, batch=3)
    for i, inf in enumerate(net.info):
        d = BRANCHES.get(i, 1 if inf["type"] == binding.T_CONV else 0)
        assert inf["dilation"] == d and net.conv_kernel(i) == (13 if d > 1 else 0)
        assert (inf["out_h"], inf["out_w"]) == (20, 20)
        if d > 1:  # no fusion with or of a dilated layer, and its tensor is its own: the route over the branches copies
            assert not any(net.plan(j)[key] for j in (i - 1, i) for key in binding.PLAN_KEYS[:2] + binding.PLAN_KEYS[3:8])
    net.close()
