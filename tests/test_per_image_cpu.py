"""Per-image input quantisation, host half: the bank entry the per-image path derives for an image's (scale, zero point)
(network_layer0_entry -- the same code the per-image quantisers run) against the oracle's constants for that image packed by the
shim, and the network's own layer-0 record left as it was.  Runs wherever the host library loads; no GPU needed."""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host():
    from yolo_quantization_amd import binding
    try:
        return binding, binding.host()
    except (OSError, binding.MI355Error) as e:  # the libraries are not built here
        pytest.skip(f"host library unavailable: {e}")


def _images():
    rng = np.random.default_rng(4)
    u = [rng.random((3, 12, 12), dtype=np.float32) for _ in range(4)]
    return [u[0], (u[1] - np.float32(0.4)) * np.float32(3.0), np.float32(0.5) + u[2] * np.float32(1e-3), -u[3] * np.float32(0.25)]


def _record(H, h, n):
    b = np.zeros(n, np.int32); mv = np.zeros(n, np.float64); sv = np.zeros(n, np.float64)
    m0 = np.zeros(n, np.int32); sh = np.zeros(n, np.int32); q = np.zeros(4, np.float32)
    H.dnq_layer_prep(h, 0, b.ctypes.data, mv.ctypes.data, sv.ctypes.data, m0.ctypes.data, sh.ctypes.data, q.ctypes.data)
    return [b, mv, sv, m0, sh, q]


def test_layer0_bank_entries_equal_oracle_constants_packed(tmp_path):
    import oracle
    from yolo_quantization_amd import synth
    binding, H = _host()
    cfg = os.path.join(ROOT, "cfg", "tiny_unit.cfg")
    wts = str(tmp_path / "w.weights")
    synth.synth_weights(cfg, wts, seed=1)
    onet = oracle.OracleNet(cfg, wts)
    d, L = onet.w[0], onet.layers[0]
    h = H.load_network(cfg.encode(), wts.encode(), 0)
    try:
        H.quantization_prep_host(h, np.float32(1.0 / 255.0), 0)
        before = _record(H, h, L.n)
        zps = set()
        for x in _images():
            q, s, z = oracle.quantize_image(x)
            zps.add(z)
            size = binding.shim().mi355_conv_pack_size(L.n, L.c, L.size)
            got = np.zeros(size, np.uint8)
            H.network_layer0_entry(h, C.c_float(s), z, got.ctypes.data)
            p = oracle.prep_conv(L.n, L.c, L.size, d["wq"], d["zp_w"], d["s_w"], s, z, d["s_act"], d["biases"], d.get("scales"),
                                 d.get("mean"), d.get("var"))
            want = binding.conv_pack(d["wq"], d["zp_w"], L.c, L.size, p["biases_int32"], p["M_value"], p["shift_value"],
                                     activation=9, zp_act=d["zp_act"])  # tiny_unit's layer 0: leaky (MI355_ACT_LEAKY)
            assert np.array_equal(got, want), f"bank entry for scale {s} zero point {z}"
            after = _record(H, h, L.n)
            assert all(np.array_equal(a, b) for a, b in zip(before, after)), "network_layer0_entry changed the layer-0 record"
        assert len(zps) > 1  # the images really have different zero points
    finally:
        H.free_network(h)


def test_per_image_refuses_a_three_filter_first_layer():
    """A 3-filter layer stores 4-byte plain cells, which only the general kernel writes, and the general kernel is not served per image:
    mi355_conv_forward_per_image answers MI355_EINVAL before anything is launched (arguments checked on the host: no device needed)."""
    from yolo_quantization_amd import binding
    S = binding.shim()
    x, y = binding.Tensor(), binding.Tensor()
    S.mi355_tensor_describe(C.byref(x), 2, 8, 8, 3)
    S.mi355_tensor_describe(C.byref(y), 2, 8, 8, 3)
    assert y.cs == 4
    buf = np.zeros(1 << 16, np.uint8)  # never read: the call is refused on its arguments
    x.data = y.data = buf.ctypes.data
    d = binding.ConvDesc(n=3, c=3, ksize=3, stride=1, pad=1, activation=9)
    eb = (int(S.mi355_conv_pack_size(3, 3, 3)) + 255) & ~255
    rc = S.mi355_conv_forward_per_image(C.byref(d), C.byref(x), buf.ctypes.data, eb, buf.ctypes.data, buf.ctypes.data, None, None,
                                        C.byref(y), None, None, None)
    assert rc < 0 and b"not served per image" in S.mi355_last_error()
