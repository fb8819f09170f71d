"""Input quantisation on the device, without a device: the arithmetic of the two kernels (input_dev.hip), restated in plain Python /
numpy in input_on_device_cases.py, against the host prep -- Net.layer0_entry(scale, zero point), the bank entry the synchronous path
uploads -- byte for byte, over every first layer and pair of the table; and which states of the entry that table reaches.

Models.  "synthetic": synth.synth_weights as it is.  "crafted": the same file with layer 0's biases and rolling means zeroed (the folded
bias is 0, so the integer bias stays inside int32 at ANY input scale -- with the synthetic biases of ~0.1 a multiplier below 2^-32 always
comes with a float bias sum beyond 2^31) and filter 0's weight zero point set to 0 (a filter whose real weights are all >= 0).

States of an entry: the header's pow2 and the four EPT_* flags.
  pow2 = 1, EPT_POW2 set      every pair of a sane scale
  pow2 = 0, EPT_POW2 clear    crafted model, the two tiny scales (some multiplier below 2^-32: its shift exceeds 31)
  EPT_NOINT set / clear       set with pow2 = 0 and by channels whose range fails intrq_make; clear for LEAKY / RELU6 entries of sane scales
  EPT_D2 set / clear          set by the crafted model (filter 0's correction is 128 - 0), clear in every synthetic one
  EPT_NEVER clear             always.  EPT_NEVER set is NOT reachable: for 0 < M' < 1 the accumulator 0 requantises to q = 0, stored as the
                              zero point itself, so a wrap-safe range exists, and small_safe_range's analytic guesses (256 - zp) / M' and
                              -(10 zp + 5) / M' (or -(zp + 1) / M') lie at most a few accumulators outside it: the first, one-by-one steps
                              of its search reach it.  The sweep asserts that no entry sets it."""
import numpy as np
import pytest

import input_on_device_cases as cases
from yolo_quantization_amd import binding, synth

TINY = cases.TINY


def _net(tmp_path, filters, act, crafted):
    net = binding.Net(*cases.make_model(tmp_path, filters, act, crafted))
    net.prepare_host_only(1.0 / 255.0, 0)
    return net


def _sweep(tmp_path, filters, act, crafted):
    """every pair's restated entry against the host's -> the (pow2, flags) states seen"""
    net = _net(tmp_path, filters, act, crafted)
    hdr, ch = cases.consts_of(net)
    assert hdr["n"] == filters and hdr["K"] == 27 and hdr["activation"] == cases.ACT_ID[act]
    start = net.layer0_entry(1.0 / 255.0, 0)
    table = dict(cases.pairs_table(), **(TINY if crafted else {}))
    seen = set()
    for name, (s, z) in table.items():
        want = net.layer0_entry(s, z)
        status, got, flags, pow2 = cases.derive_entry(start, hdr, ch, act, s, z)
        assert status == 0, name
        assert np.array_equal(got, want), f"{name}: bytes differ at {np.flatnonzero(got != want)[:8]}"
        h = cases.blob_header(want)
        assert h["pow2"] == int(pow2) and bool(flags & cases.EPT_POW2) == pow2
        seen.add((pow2, flags))
    # where the host dies the restatement names the reason and leaves the slot alone
    status, got, _, _ = cases.derive_entry(start, hdr, ch, act, *cases.M_TOO_LARGE)
    assert status == cases.M_RANGE and np.array_equal(got, start)
    if not crafted:  # the synthetic biases cannot follow a multiplier below 2^-32
        status, got, _, _ = cases.derive_entry(start, hdr, ch, act, *TINY["tiny 2^-40"])
        assert status == cases.BIAS_RANGE and np.array_equal(got, start)
    net.close()
    return seen


@pytest.mark.parametrize("act", cases.ACTS)
@pytest.mark.parametrize("filters", cases.FILTERS)
def test_restated_entries_equal_the_host_prep(tmp_path, filters, act):
    seen = _sweep(tmp_path, filters, act, crafted=False)
    assert all(pow2 and not flags & (cases.EPT_NEVER | cases.EPT_D2) for pow2, flags in seen)


def test_states_the_table_reaches(tmp_path):
    seen = set()
    for filters, act in cases.STATE_MODELS:
        for crafted in (False, True):
            d = tmp_path / f"{filters}{act}{int(crafted)}"
            d.mkdir()
            seen |= _sweep(d, filters, act, crafted)
    assert {p for p, _ in seen} == {True, False}  # pow2 in both states
    for bit, name in ((cases.EPT_POW2, "EPT_POW2"), (cases.EPT_NOINT, "EPT_NOINT"), (cases.EPT_D2, "EPT_D2")):
        assert {bool(f & bit) for _, f in seen} == {True, False}, name
    assert not any(f & cases.EPT_NEVER for _, f in seen)  # unreachable: see the module docstring


def test_pairs_equal_the_host_quantiser():
    """pair_of (the pair kernel's expressions) against quant_image_with_min_max on a two-element image"""
    import ctypes as C
    for mx, mn in [(1.0, 0.0), (1.0, -0.5), (0.7, -0.0), (0.0, -1.0), (1e-3, -3.0), (0.0, -1e-30), (254.0 / 255.0, 0.0), (3.0, -0.1), (0.5, -0.5)]:
        x = np.array([mx, mn], np.float32)
        out = np.zeros(2, np.uint8)
        s, z = C.c_float(), C.c_uint8()
        binding.host().quant_image_with_min_max(2, x.ctypes.data, out.ctypes.data, C.byref(s), C.byref(z))
        ps, pz = cases.pair_of(mx, mn)
        assert np.float32(s.value).tobytes() == ps.tobytes() and z.value == pz, (mx, mn)
