"""No device: the depthwise-separable block's call is exported and mirrored, and the chained reference the GPU suite checks the fused
kernel against equals the dense-twin construction of DESIGN.md 7b (the depthwise layer as a dense layer whose off-diagonal weights are
the filter's zero point), so that reference is the reference's own arithmetic."""
import os

import numpy as np

import oracle
from yolo_quantization_amd import binding, synth


def test_shim_exports_conv_sep_forward():
    S = binding.shim()
    assert hasattr(S, "mi355_conv_sep_forward")
    assert len(S.mi355_conv_sep_forward.argtypes) == 9
    assert callable(binding.conv_sep_forward)


def test_chained_reference_equals_dense_twin():
    rng = np.random.default_rng(7)
    c, n, H, W, k, s, pad, zi, zm = 17, 5, 6, 7, 3, 2, 1, 9, 21
    x = rng.integers(0, 256, (c, H, W), dtype=np.uint8)
    wd = rng.integers(0, 256, (c, k * k), dtype=np.uint8)
    zwd = rng.integers(0, 256, c, dtype=np.uint8)
    wp = rng.integers(0, 256, (n, c), dtype=np.uint8)
    zwp = rng.integers(0, 256, n, dtype=np.uint8)
    bias = rng.integers(-3000, 3000, c).astype(np.int32)
    M, S = np.full(c, 0.75), np.full(c, 2.0 ** -7)
    per_channel = np.concatenate([oracle.conv_acc(x[j:j + 1], wd[j:j + 1], zwd[j:j + 1], k, s, pad, zi) for j in range(c)])
    twin = np.repeat(zwd[:, None, None], c, axis=1).repeat(k * k, axis=2)  # [c][c][k k]: zp_w off the diagonal
    twin[np.arange(c), np.arange(c)] = wd
    dense = oracle.conv_acc(x, twin.reshape(c, -1), zwd, k, s, pad, zi)
    assert np.array_equal(per_channel, dense)
    OH, OW = (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1
    m = oracle.requant(dense, bias, M, S, zm, oracle.ACT["leaky"]).reshape(c, OH, OW)
    acc = oracle.conv_acc(m, wp, zwp, 1, 1, 0, zm)
    want = (wp.astype(np.int64) - zwp[:, None]) @ m.reshape(c, -1).astype(np.int64)
    assert np.array_equal(acc, want.astype(np.int32))


def test_host_exports_set_fuse_separable():
    assert hasattr(binding.host(), "set_fuse_separable")


def test_set_fuse_separable_plans_pairs_and_keeps_plan_records(cfg_dir, tmp_path):
    """The planner without a device: the flag returns 0, pairs exactly the cfg's three blocks, leaves the eight-int dnq_layer_plan
    records as they were, and off again plans what the parent plans."""
    cfg = os.path.join(cfg_dir, "sep_unit.cfg")
    wts = str(tmp_path / "sep.weights")
    synth.synth_weights(cfg, wts, seed=4)
    net = binding.Net(cfg, wts, batch=1)
    net.prepare_host_only(1.0 / 255.0, 0)
    before = [net.plan(i) for i in range(net.n)]
    assert not any(net.is_fused(i) for i in (1, 3, 5, 7, 10))
    assert net.H.set_fuse_separable(net.h, 1) == 0
    assert [i for i in range(net.n) if net.is_fused(i)] == [1, 3, 5], "7 is routed, 10 feeds the head that fuses with yolo"
    assert [net.plan(i) for i in range(net.n)] == before
    assert net.H.set_fuse_separable(net.h, 0) == 0
    assert not any(net.is_fused(i) for i in range(net.n)) and [net.plan(i) for i in range(net.n)] == before
    net.close()
