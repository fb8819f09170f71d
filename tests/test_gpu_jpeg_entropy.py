"""mi355_jpeg_entropy on the device: the coefficient planes it fills equal jpeg_decode_host's, bit for bit, on every fixture and on
built streams that sit on the edges of the kernel -- subsequence counts around the round of 256 lanes, 31-bit symbols across every
bit offset of a subsequence and of a round, 300 restart intervals in a launch, unit grids narrower than their planes and of 6 and 18
blocks a unit, a stream that settles one lane a step --; damaged streams set their status word and leave their neighbours alone;
refusals launch nothing; and with Net.set_jpeg_entropy_on_device the JPEG input path and the CLI give what they give without it,
byte for byte.  None of the built streams is a photograph: each is the smallest at which its edge exists."""
import ctypes as C
import glob
import os
import re
import subprocess

import numpy as np
import pytest

import jpeg_streams
from frames_util import CFG, ROOT, _bits, _wts
from yolo_quantization_amd import binding

pytestmark = pytest.mark.gpu

JPEG_DIR = os.path.join(ROOT, "tests", "golden", "jpeg")
NAMES = sorted(n for n in (os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(JPEG_DIR, "*.jpg")))
               if n not in ("progressive", "cmyk"))
# fixtures the 12 x 12 test network's letterbox can serve (tests/test_gpu_jpeg.py)
NET_NAMES = ["420_51x37", "422_restart2_51x37", "444_48x32", "440_23x61", "411_61x23", "410_61x27", "grey_51x37", "rgb_adobe0_48x32",
             "420_noninterleaved_37x27", "420_3x4", "h1v4_11x43", "444_q100_51x37"]


@pytest.fixture(scope="module", autouse=True)
def _dev():
    binding.init(0)


def data_of(name):
    with open(os.path.join(JPEG_DIR, name + ".jpg"), "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def fixtures():
    """every decodable fixture with what jpeg_decode_host makes of it, once"""
    return {n: (data_of(n), binding.jpeg_coefficients(data_of(n))) for n in NAMES}


def _check(files, subseq_bits, what):
    """files: {name: (data, jpeg_coefficients(data))}; ONE launch for every segment of every file"""
    names = sorted(files)
    planes, status = binding.jpeg_entropy([files[n][0] for n in names], subseq_bits=subseq_bits)
    for n, per, st in zip(names, planes, status):
        assert st == [0] * len(st), f"{what} at {subseq_bits}: status of {n}"
        for k, (a, c) in enumerate(zip(per, files[n][1]["components"])):
            assert np.array_equal(a, c["coef"]), f"{what} at {subseq_bits}: {n}, component {k}"
    return status


def _decoded(streams):
    return {n: (d, binding.jpeg_coefficients(d)) for n, d in streams.items()}


@pytest.mark.parametrize("subseq_bits", [32, 64, 1024])
def test_every_fixture_in_one_launch(fixtures, subseq_bits):
    assert len(fixtures) >= 40
    status = _check(fixtures, subseq_bits, "fixtures")
    assert sum(len(s) for s in status) > len(fixtures)  # several scans and restart intervals among them


def test_subsequence_counts_around_the_round_of_256_lanes():
    files = _decoded(jpeg_streams.round_edge_streams())
    assert len(files) == 8
    _check(files, 32, "round edges")
    _check(files, 64, "round edges")


def test_31_bit_symbols_across_every_subsequence_and_round_edge():
    files = _decoded(jpeg_streams.symbol_edge_streams())
    assert len(files) == 32
    for bits in (32, 64):  # bit 8192 is the edge of the first round at 32, bit 16384 at 64: the streams are 8500 bits and more
        _check(files, bits, "symbol edges")
    assert all(len(binding.jpeg_scan(d)["segments"][0]["data"]) * 8 > 8192 + 64 for d, _ in files.values())


def test_300_restart_intervals_in_one_launch():
    data = jpeg_streams.restart_stream()
    want = binding.jpeg_coefficients(data)
    assert want["restart_interval"] == 1 and (np.abs(want["components"][0]["coef"][0, :, 0].astype(int)) > 100).sum() > 200
    (status,) = _check({"restart": (data, want)}, 32, "restart")
    assert len(status) == 300


def test_unit_grids():
    files = _decoded(jpeg_streams.unit_grid_streams())
    for bits in (32, 256):
        _check(files, bits, "unit grids")


def test_slow_settle_on_the_device():
    data, coef = jpeg_streams.slow_settle()
    want = binding.jpeg_coefficients(data)
    assert all(np.array_equal(c["coef"], mine) for c, mine in zip(want["components"], coef))
    _check({"slow": (data, want)}, 32, "slow settle")


def test_damaged_streams_set_their_status_and_leave_their_neighbours_alone(fixtures, tmp_path):
    damaged = jpeg_streams.damaged_streams()
    good = [fixtures[n] for n in ("420_51x37", "422_restart2_51x37", "grey_51x37", "444_noninterleaved_29x19")]
    items, kinds = [good[0][0]], [None]
    for (name, (data, code)), g in zip(damaged.items(), good[1:]):
        items += [data, g[0]]
        kinds += [code, None]
    for bits in (32, 1024):
        planes, status = binding.jpeg_entropy(items, subseq_bits=bits)
        gi = 0
        for per, st, code in zip(planes, status, kinds):
            if code is None:
                assert st == [0] * len(st)
                for a, c in zip(per, good[gi][1]["components"]):
                    assert np.array_equal(a, c["coef"]), f"neighbour {gi} at {bits}"
                gi += 1
            else:
                assert st == [code]
                assert per[0][0, :2, 0].tolist() == [1, 0] and per[0][0, :2, 1].tolist() == [1, 1]  # the blocks in front of the damage
    # the host library names the slot, and nothing follows the decode
    net = binding.Net(CFG, _wts(tmp_path), batch=3)
    net.set_jpeg_entropy_on_device(True)
    net.prepare_from_jpeg([data_of(n) for n in NET_NAMES[:3]])
    before = net._pull_input()
    reasons = {1: "bad huffman code", 2: "bad DC category", 3: "coefficient index past the end of the block"}
    for name, (data, code) in damaged.items():
        with pytest.raises(binding.JpegError, match=rf"jpeg slot 1: {reasons[code]} \(device\)"):
            net.prepare_from_jpeg([data_of(NET_NAMES[0]), data, data_of(NET_NAMES[2])])
        with pytest.raises(binding.JpegError, match=rf"jpeg slot 2: {reasons[code]} \(device\)"):
            binding.jpeg_decode([data_of(NET_NAMES[0]), data_of(NET_NAMES[1]), data], net=net)
    assert np.array_equal(net._pull_input(), before)  # no letterbox, no quantise
    net.close()


def test_refusals_launch_nothing(tmp_path):
    L = binding.shim()
    scan = binding.jpeg_scan(data_of("grey_8x8"))
    (seg,) = scan["segments"]
    bits = binding.DevBuf.from_numpy(np.frombuffer(seg["data"] + bytes(12), np.uint8))
    huff = binding.DevBuf.from_numpy(np.frombuffer(b"".join(bytes(h) for h in scan["huff"]), np.uint8))
    coef = binding.DevBuf.from_numpy(np.full(64, 0x5A5A, np.int16))
    status = binding.DevBuf.from_numpy(np.full(1, 77, np.int32))
    t = (binding.JpegSegment * 1)()
    t[0].bits, t[0].huff, t[0].nbytes, t[0].ncomp, t[0].nhuff = bits.ptr, huff.ptr, len(seg["data"]), 1, 2
    t[0].coef[0] = coef.ptr.value
    t[0].bh[0] = t[0].bv[0] = t[0].blocks_w[0] = t[0].blocks_h[0] = 1
    t[0].dc[0], t[0].ac[0] = 0, 1
    t[0].units_x = t[0].units_y = t[0].nunits = 1
    tdev = binding.DevBuf.from_numpy(np.frombuffer(bytes(t), np.uint8))
    for field, value in (("bits", None), ("bits", bits.ptr.value + 2), ("huff", None), ("ncomp", 0), ("ncomp", 4), ("nhuff", 1), ("units_x", 2),
                         ("nunits", 2), ("first_unit", 1), ("nunits", 0), ("nbytes", (1 << 28) + 1), ("reserved", 1)):
        keep = getattr(t[0], field)
        setattr(t[0], field, value)
        assert L.mi355_jpeg_entropy(tdev.ptr, t, 1, 32, status.ptr, None) == -22 and b"jpeg_entropy:" in L.mi355_last_error(), field
        setattr(t[0], field, keep)
    for arr, value in ((t[0].bh, 5), (t[0].bv, 0), (t[0].dc, 2), (t[0].ac, -1), (t[0].coef, None), (t[0].blocks_w, 0)):
        keep = arr[0]
        arr[0] = value
        assert L.mi355_jpeg_entropy(tdev.ptr, t, 1, 32, status.ptr, None) == -22 and b"jpeg_entropy:" in L.mi355_last_error()
        arr[0] = keep
    for subseq_bits in (0, 31, 48, 8224):
        assert L.mi355_jpeg_entropy(tdev.ptr, t, 1, subseq_bits, status.ptr, None) == -22 and b"jpeg_entropy:" in L.mi355_last_error()
    assert L.mi355_jpeg_entropy(tdev.ptr, t, 0, 32, status.ptr, None) == -22
    assert L.mi355_jpeg_entropy(None, t, 1, 32, status.ptr, None) == -22 and L.mi355_jpeg_entropy(tdev.ptr, t, 1, 32, None, None) == -22
    binding.check(L.mi355_stream_sync(None), "sync")
    assert (coef.to_numpy(np.int16, 64) == 0x5A5A).all() and status.to_numpy(np.int32, 1)[0] == 77
    # the record as it is launches, and stores the non-zero coefficients only
    assert L.mi355_jpeg_entropy(tdev.ptr, t, 1, 32, status.ptr, None) == 0
    binding.check(L.mi355_stream_sync(None), "sync")
    want = binding.jpeg_coefficients(data_of("grey_8x8"))["components"][0]["coef"].ravel()
    got = coef.to_numpy(np.int16, 64)
    assert status.to_numpy(np.int32, 1)[0] == 0 and np.array_equal(got[want != 0], want[want != 0]) and (got[want == 0] == 0x5A5A).all()
    for b in (bits, huff, coef, status, tdev):
        b.free()
    # header refusals through the host library: nothing reaches the device
    net = binding.Net(CFG, _wts(tmp_path), batch=3)
    net.set_jpeg_entropy_on_device(True)
    good = [data_of(n) for n in NET_NAMES[:3]]
    net.prepare_from_jpeg(good)
    waits = net.host_waits()
    for bad, message in ((data_of("progressive"), "jpeg slot 1: progressive"), (data_of("cmyk"), "jpeg slot 1: 4 components"),
                         (good[1][:200], "jpeg slot 1: "), (b"P6\n1 1\n255\n", "jpeg slot 1: no SOI")):
        with pytest.raises(binding.JpegError, match=message):
            net.prepare_from_jpeg([good[0], bad, good[2]])
    assert net.host_waits() == waits
    net.close()


# ------------------------------------------------------------------------------------------------------------- whole path
def _run(net, sizes):
    net.forward()
    net.sync()
    deep = max(i for i, inf in enumerate(net.info) if inf["type"] == binding.T_CONV)
    return net.pull(deep), net.detect([s[0] for s in sizes], [s[1] for s in sizes], thresh=0.005)


def _assert_same_input_and_run(a, b, sizes, what):
    assert np.array_equal(a._pull_input(), b._pull_input()), f"{what}: input bytes"
    (sa, za), (sb, zb) = a.input_quantization(), b.input_quantization()
    assert np.array_equal(_bits(sa), _bits(sb)) and np.array_equal(za, zb), f"{what}: scales / zero points"
    (la, da), (lb, db) = _run(a, sizes), _run(b, sizes)
    for k in lb:
        assert np.array_equal(la[k], lb[k]), f"{what}: deep layer {k}"
    for slot, (x, y) in enumerate(zip(da, db)):
        assert x.keys() == y.keys()
        for k in x:
            assert np.array_equal(x[k], y[k]), f"{what}: detections of slot {slot}: {k}"


def test_all_fixtures_decode_to_the_frames_of_the_host_path(tmp_path):
    """network_jpeg_decode_gpu on every fixture as one batch, mode on against mode off (the letterbox of the 12 x 12 test network
    cannot serve the smallest fixtures, so the frames are compared here and the input step below on those it can serve)"""
    wts = _wts(tmp_path)
    on, off = binding.Net(CFG, wts, batch=1), binding.Net(CFG, wts, batch=1)
    on.set_jpeg_entropy_on_device(True)
    files = [data_of(n) for n in NAMES]
    for bits in (None, 32):
        if bits:
            on.set_jpeg_entropy_on_device(True, subseq_bits=bits)
        for items in (files, files[::-3], files[:1] * 3):  # buffers grow, are reused, one image's bytes in every slot
            waits = on.host_waits()
            got, want = binding.jpeg_decode(items, net=on), binding.jpeg_decode(items, net=off)
            assert on.host_waits() > waits
            for k, (g, w) in enumerate(zip(got, want)):
                assert g.shape == w.shape and np.array_equal(g, w), k
    on.close(); off.close()


@pytest.mark.parametrize("mode", ["shared", "per_image", "on_device", "on_device_per_image"])
def test_prepare_from_jpeg_with_the_mode_on_equals_the_mode_off(tmp_path, mode):
    wts = _wts(tmp_path)
    B = len(NET_NAMES)
    a, b = binding.Net(CFG, wts, batch=B), binding.Net(CFG, wts, batch=B)
    a.set_jpeg_entropy_on_device(True)
    for net in (a, b):
        if "per_image" in mode:
            net.set_input_per_image(True)
        if "on_device" in mode:
            net.set_input_on_device(True)
    for again, names in enumerate((NET_NAMES, NET_NAMES[::-1])):  # the staging block and the device buffers are reused
        files = [data_of(n) for n in names]
        waits = a.host_waits()
        sizes = a.prepare_from_jpeg(files)
        if "on_device" in mode and again:  # (the first call also waits before it grows its buffers)
            assert a.host_waits() == waits + 1  # the status read is the one wait of the input step
        assert sizes == b.prepare_from_jpeg(files)
        _assert_same_input_and_run(a, b, sizes, f"{mode}")
    a.close(); b.close()


def test_prepare_from_jpeg_with_the_mode_on_graph_replay_and_replica(tmp_path):
    wts = _wts(tmp_path, seed=5)
    parent = binding.Net(CFG, wts, batch=3, use_graph=True)
    parent.set_input_per_image(True)
    parent.set_jpeg_entropy_on_device(True)
    ref = binding.Net(CFG, wts, batch=3)
    ref.set_input_per_image(True)
    handle = None
    for first in (0, 3):  # the captured graph replays the second batch
        files = [data_of(n) for n in NET_NAMES[first:first + 3]]
        sizes = parent.prepare_from_jpeg(files)
        ref.prepare_from_jpeg(files)
        _assert_same_input_and_run(parent, ref, sizes, "graph")
        handle = handle or parent.graph_handle()
        assert handle and parent.graph_handle() == handle
    rep = parent.replica()  # inherits the mode; its own staging block, buffers and stream
    fa, fb = [data_of(n) for n in NET_NAMES[6:9]], [data_of(n) for n in NET_NAMES[9:12]]
    sa, sb = rep.prepare_from_jpeg(fa), parent.prepare_from_jpeg(fb)
    for _ in range(2):
        parent.forward()
        rep.forward()
    for net, files, sizes in ((rep, fa, sa), (parent, fb, sb)):
        ref.prepare_from_jpeg(files)
        _assert_same_input_and_run(net, ref, sizes, "replica")
    damaged = jpeg_streams.damaged_streams()["no_code"][0]
    with pytest.raises(binding.JpegError, match=r"jpeg slot 0: bad huffman code \(device\)"):  # the replica decodes on the device too
        rep.prepare_from_jpeg([damaged, fa[1], fa[2]])
    rep.close()
    ref.close()
    parent.close()


def test_cli_with_jpeg_device_prints_what_it_prints_without(tmp_path):
    exe = os.path.join(ROOT, "yolo_quantization_amd", "bin", "darknet")
    wts = _wts(tmp_path, seed=1)
    names = str(tmp_path / "x.names")
    open(names, "w").write("\n".join(["ant", "bee", "cat", "dog", "eel"]) + "\n")
    data = str(tmp_path / "x.data")
    open(data, "w").write(f"classes= 5\nnames = {names}\n")
    jpg = [os.path.join(JPEG_DIR, n + ".jpg") for n in ["420_51x37", "440_23x61", "grey_51x37", "410_61x27", "422_restart2_51x37"]]
    listfile = str(tmp_path / "jpg.txt")
    open(listfile, "w").write("\n".join(jpg) + "\n")

    def run(extra, ok=True):
        r = subprocess.run([exe, "detector", "test", data, CFG, wts] + extra + ["-thresh", "0.3", "-boxes"], capture_output=True, text=True, timeout=300)
        assert (r.returncode == 0) == ok, r.stderr
        return re.sub(r": Predicted in .*", ": Predicted", r.stdout) if ok else r.stderr  # the one line that holds a wall-clock time

    for args in ([jpg[0]], ["-list", listfile, "-batch", "3"], [jpg[0], "-batch", "2", "-input_device"]):
        want, got = run(args), run(args + ["-jpeg_device"])
        assert got == want and any(line.startswith("box:") for line in want.splitlines())
    bad = str(tmp_path / "damaged.jpg")
    open(bad, "wb").write(jpeg_streams.damaged_streams()["index_past_63"][0])
    err = run([bad, "-jpeg_device"], ok=False)
    assert "slot 0" in err and "coefficient index past the end of the block (device)" in err
