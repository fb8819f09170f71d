"""One network fed by the three coded-image input paths in turn -- JPEG with the host entropy decode, PNG, JPEG with the entropy decode
on the device -- so that they share, regrow and reuse their buffers: after every call the network's input bytes, scales and zero points
are those of a twin fed the expected pixels (tests/golden/jpeg_expected.npz, png_expected.npz) through prepare_from_frames_u8, a
refused batch costs no wait and spoils nothing, and a repeated batch costs each path exactly one wait.  Every comparison is exact."""
import os

import numpy as np
import pytest

from frames_util import CFG, ROOT, _bits, _wts
from yolo_quantization_amd import binding

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden")
# every batch is one the 12 x 12 test network's letterbox can serve (both resized sides >= 2)
JPEG_SMALL = ["420_3x4", "h1v4_11x43", "420_noninterleaved_37x27"]
JPEG_MIDDLE = ["444_48x32", "grey_51x37", "rgb_adobe0_48x32"]
JPEG_LARGEST = ["444_q100_51x37", "440_24x64", "411_64x24"]
PNG_MIDDLE = ["pal8_trns_23x19", "rgb16_trns_23x19", "rgb8_adam7_64x61"]
PNG_SMALLEST = ["pal4_adam7_2x5", "grey16_plain_3x4", "rgb8_adam7_4x3"]
# the 1 x 1 fixtures go through the same buffers of the network by binding.png_decode(net=...), which stops at the RGB frames
# (tests/test_gpu_frame_geometry.py sends them through prepare_from_png and prepare_from_jpeg, letterbox included)
PNG_ONE_PIXEL = ["rgb8_adam7_1x1", "pal4_adam7_1x1", "grey16_plain_1x1"]
B = 3


@pytest.fixture(scope="module", autouse=True)
def _dev():
    binding.init(0)


@pytest.fixture(scope="module")
def expected():
    out = {}
    for kind in ("jpeg", "png"):
        with np.load(os.path.join(GOLDEN, kind + "_expected.npz")) as z:
            out[kind] = {k: z[k] for k in z.files}
    return out


def _file(kind, name):
    with open(os.path.join(GOLDEN, kind, name + (".jpg" if kind == "jpeg" else ".png")), "rb") as f:
        return f.read()


def _nets(tmp_path):
    wts = _wts(tmp_path)
    net, twin = binding.Net(CFG, wts, batch=B), binding.Net(CFG, wts, batch=B)
    for n in (net, twin):
        n.set_input_on_device(True)  # the frame step waits for nothing: every wait counted below is a coded-image path's
    return net, twin


def _feed(net, path, files):
    """one call of `path`: "jpeg" (host entropy decode), "png", or "jpeg_device" """
    if path == "png":
        return net.prepare_from_png(files)
    net.set_jpeg_entropy_on_device(path == "jpeg_device")
    return net.prepare_from_jpeg(files)


def _kind(path):
    return "png" if path == "png" else "jpeg"


def _good(net, twin, expected, path, names, what):
    want = [expected[_kind(path)][n] for n in names]
    sizes = _feed(net, path, [_file(_kind(path), n) for n in names])
    assert sizes == [w.shape[1::-1] for w in want], what
    twin.prepare_from_frames_u8(want)
    assert np.array_equal(net._pull_input(), twin._pull_input()), f"{what}: input bytes"
    (sa, za), (sb, zb) = net.input_quantization(), twin.input_quantization()
    assert sa.shape == (B,) and np.array_equal(_bits(sa), _bits(sb)) and np.array_equal(za, zb), f"{what}: scales / zero points"


def test_three_paths_in_turn_share_and_regrow_their_buffers(expected, tmp_path):
    net, twin = _nets(tmp_path)
    _good(net, twin, expected, "jpeg", JPEG_SMALL, "1. jpeg")
    _good(net, twin, expected, "png", PNG_MIDDLE, "2. png")
    _good(net, twin, expected, "jpeg_device", JPEG_MIDDLE, "3. jpeg, entropy decode on the device")
    _good(net, twin, expected, "jpeg", JPEG_LARGEST, "4. jpeg, the buffers grow after the entropy layout used them")
    for got, n in zip(binding.png_decode([_file("png", n) for n in PNG_ONE_PIXEL], net=net), PNG_ONE_PIXEL):
        assert got.shape == (1, 1, 3) and np.array_equal(got, expected["png"][n]), f"5. png, {n}"
    _good(net, twin, expected, "png", PNG_SMALLEST, "5. png, the buffers are larger than needed")
    _good(net, twin, expected, "jpeg_device", ["420_51x37"] * B, "6. jpeg on the device, one file in every slot")
    # 7. a refused slot 1: named, no wait, and the next good call is exact
    for path, bad, message, names in (("jpeg", "progressive", "jpeg slot 1: progressive", JPEG_MIDDLE),
                                      ("png", "refuse_invalid_filter", "png slot 1: invalid filter", PNG_MIDDLE),
                                      ("jpeg_device", "progressive", "jpeg slot 1: progressive", JPEG_SMALL)):
        kind = _kind(path)
        files = [_file(kind, names[0]), _file(kind, bad), _file(kind, names[2])]
        waits = net.host_waits()
        with pytest.raises(binding.PngError if kind == "png" else binding.JpegError, match=message):
            _feed(net, path, files)
        assert net.host_waits() == waits, f"7. {path}: the refused call waited"
        _good(net, twin, expected, path, names, f"7. {path} after its refusal")
    net.close(); twin.close()


def test_a_repeated_batch_costs_each_path_one_wait(expected, tmp_path):
    """No buffer grows on the third call with one batch.  The host modes wait once, for the upload of the call before, which may still
    read the staging block they rewrite; the device entropy decode leaves no upload pending and waits once, for its status words."""
    net, twin = _nets(tmp_path)
    for path, names in (("jpeg", JPEG_MIDDLE), ("png", PNG_MIDDLE), ("jpeg_device", JPEG_MIDDLE)):
        files = [_file(_kind(path), n) for n in names]
        _feed(net, path, files)
        _feed(net, path, files)
        waits = net.host_waits()
        _feed(net, path, files)
        got = net.host_waits() - waits
        print(f"{path}: {got} wait(s) in the third call")
        assert got == 1, path
        _good(net, twin, expected, path, names, f"{path} a fourth time")
    net.close(); twin.close()
