"""Grouped convolution without a device: the blob size, the packer's determinism and the two identities of DESIGN.md 7e against each
other through the oracle (no kernel is launched)."""
import numpy as np
import pytest

import oracle
from yolo_quantization_amd import binding
from test_gpu_conv_group import group_acc


def test_the_three_calls_are_exported():
    for name in ("mi355_conv_group_pack_size", "mi355_conv_group_pack", "mi355_conv_group_forward"):
        assert hasattr(binding.shim(), name)


def test_pack_size_is_a_function_of_n_c_g_k():
    size = binding.shim().mi355_conv_group_pack_size
    for bad in ((0, 16, 1, 3), (16, 0, 1, 3), (16, 16, 0, 3), (16, 16, -1, 3), (16, 18, 4, 3), (18, 16, 4, 3), (16, 16, 4, 0), (16, 16, 4, 12)):
        assert size(*bad) == 0, bad
    assert size(32, 32, 2, 1) < size(32, 32, 2, 3) < size(32, 32, 2, 5) < size(32, 32, 2, 11)   # grows with k
    assert size(16, 32, 2, 3) < size(32, 32, 2, 3) < size(48, 48, 3, 3) < size(272, 144, 2, 3)  # and with the M tiles
    # the block structure is exploited: cardinality 32 on 512 channels packs a piece per tile, the dense layer 32
    assert size(512, 512, 1, 3) > 16 * size(512, 512, 32, 3)


def _layer(rng, c, n, g, k):
    wq = rng.integers(0, 256, (n, c // g * k * k), dtype=np.uint8)
    return wq, rng.integers(0, 256, n, dtype=np.uint8), rng.integers(-99, 99, n).astype(np.int32), np.full(n, 0.5), np.full(n, 2.0 ** -9)


def test_packing_is_deterministic_and_sized_by_pack_size():
    wq, zp_w, bias, mv, sv = _layer(np.random.default_rng(5), 24, 48, 2, 3)
    a = binding.conv_group_pack(wq, zp_w, 2, 24, 3, bias, mv, sv)
    b = binding.conv_group_pack(wq.copy(), zp_w, 2, 24, 3, bias, mv, sv)
    assert a.size == binding.shim().mi355_conv_group_pack_size(48, 24, 2, 3) and np.array_equal(a, b)
    rc = binding.shim().mi355_conv_group_pack(48, 24, 5, 3, wq.ctypes.data, zp_w.ctypes.data, bias.ctypes.data, mv.ctypes.data,
                                              sv.ctypes.data, a.ctypes.data)
    assert rc == -22 and binding.shim().mi355_last_error().decode().startswith("invalid argument: conv_group_pack:") and np.array_equal(a, b)


@pytest.mark.parametrize("c,n,g", [(24, 48, 2), (16, 32, 16), (9, 15, 3)])
def test_dense_twin_equals_one_convolution_per_group(c, n, g):
    """identity 2 against identity 1: the dense c -> n layer whose weights outside a filter's group are its zero point"""
    rng = np.random.default_rng(c)
    k, s, p, zp_in, cg, ng = 3, 2, 1, 201, c // g, n // g
    wq, zp_w = _layer(rng, c, n, g, k)[:2]
    x = rng.integers(0, 256, (c, 6, 5), dtype=np.uint8)
    twin = np.repeat(zp_w[:, None], c * k * k, axis=1).reshape(n, c, k * k)
    for j in range(n):
        twin[j, j // ng * cg:(j // ng + 1) * cg] = wq[j].reshape(cg, k * k)
    assert np.array_equal(oracle.conv_acc(x, twin.reshape(n, -1), zp_w, k, s, p, zp_in), group_acc(x, wq, zp_w, g, k, s, p, zp_in))
