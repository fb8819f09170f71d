"""The inflate of PNG streams on the device: mi355_png_inflate through the C-ABI on every fixture's stream and on the built streams of
png_inflate_streams against the host decoder (png_decode_host / png_inflate_host), and the whole input step with
set_png_inflate_on_device against the step without it.  Every comparison is exact.  Every launch of built inputs goes through
binding.png_inflate_device, which puts guard bytes before, between and behind the outputs and guard words around the status words and
raises if one changed."""
import glob
import os
import subprocess

import numpy as np
import pytest

import png_inflate_streams as pis
import png_streams
from frames_util import CFG, ROOT, _bits, _blocks, _write_ppm, _wts
from yolo_quantization_amd import binding

pytestmark = pytest.mark.gpu

PNG_DIR = os.path.join(ROOT, "tests", "golden", "png")
JPEG_DIR = os.path.join(ROOT, "tests", "golden", "jpeg")
NAMES = sorted(n for n in (os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(PNG_DIR, "*.png")))
               if not n.startswith("refuse_"))
NET_NAMES = ["rgb8_plain_51x37", "pal4_adam7_51x37", "grey16_plain_51x37", "rgba16_adam7_51x37", "ga8_plain_51x37", "grey1_adam7_64x61",
             "rgb8_adam7_64x61", "pal8_trns_23x19", "rgb16_trns_23x19", "rgba16_adam7_paeth_19x23", "grey4_plain_average_33x17",
             "rgb8_idat_uneven_51x37"]


@pytest.fixture(scope="module", autouse=True)
def _dev():
    binding.init(0)


@pytest.fixture(scope="module")
def expected():
    with np.load(os.path.join(ROOT, "tests", "golden", "png_expected.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def fixture_streams():
    """per fixture: (stream, cap, passes) and the host decoder's filtered bytes; computed once"""
    out = {}
    for n in NAMES:
        data = data_of(n)
        out[n] = (binding.png_stream_of(binding.png_scan(data)), binding.png_scanlines(data)["filtered"].tobytes())
    return out


def data_of(name):
    with open(os.path.join(PNG_DIR, name + ".png"), "rb") as f:
        return f.read()


def _launch(cases):
    outs, status = binding.png_inflate_device([c.z for c in cases], [c.cap for c in cases], [c.passes for c in cases])
    pis.check(cases, outs, status)
    return outs, status


# ------------------------------------------------------------------------------------------------------------------ the fixtures
@pytest.mark.parametrize("count", [87, 1, 2, 257])
def test_fixture_streams_in_one_launch(fixture_streams, count):
    assert len(NAMES) >= 87
    names = (NAMES * 3)[:count] if count != 87 else NAMES
    args = [fixture_streams[n][0] for n in names]
    outs, status = binding.png_inflate_device([a[0] for a in args], [a[1] for a in args], [a[2] for a in args])
    assert status == [0] * len(names)
    for n, out in zip(names, outs):
        assert out == fixture_streams[n][1], n


def test_refusal_files_that_reach_the_inflate_give_the_host_decoders_reason(fixture_streams):
    good = fixture_streams["rgb8_plain_51x37"]
    for name, (data, message) in png_streams.refusal_files().items():
        try:
            sc = binding.png_scan(data)
        except binding.PngError:
            continue
        z, cap, passes = binding.png_stream_of(sc)
        outs, status = binding.png_inflate_device([good[0][0], z, good[0][0]], [good[0][1], cap, good[0][1]], [good[0][2], passes, good[0][2]])
        assert status[0] == status[2] == 0 and outs[0] == outs[2] == good[1], name
        assert status[1] and message in binding.PNG_INFLATE_ERRORS[status[1]], (name, status)


# ------------------------------------------------------------------------------------------------------------------ built streams
@pytest.mark.parametrize("group", ["token_round_cases", "match_cases", "ring_cases", "cap_cases", "block_cases", "repeat_code_cases", "zlib_cases"])
def test_built_streams(group):
    _launch(getattr(pis, group)())


def test_every_status_between_two_good_streams():
    errors = pis.error_cases()
    assert {c.reason for c in errors} >= set(binding.PNG_INFLATE_ERRORS.values())
    cases = [pis.good_case(0)]
    for k, c in enumerate(errors):
        cases += [c, pis.good_case(k + 1)]
    _launch(cases)  # the good streams' outputs stay exact, the guards between them untouched


def test_filter_byte_5_in_pass_7_of_an_adam7_file(fixture_streams):
    import zlib
    (z, cap, passes), filtered = fixture_streams["rgb8_adam7_64x61"]
    assert len(passes) == 7
    raw = bytearray(filtered)
    raw[cap - (passes[6][1] + 1)] = 5  # the last row of the last pass
    bad = pis.Case("adam7_pass_7", zlib.compress(bytes(raw), 6)[2:-4], cap, "invalid filter", passes)
    raw[cap - (passes[6][1] + 1)] = 4
    raw[cap - 1] = 5  # not a filter byte
    good = pis.Case("adam7_pass_7_good", zlib.compress(bytes(raw), 6)[2:-4], cap, None, passes)
    _launch([good, bad, good])


def test_c_abi_refusals_launch_nothing():
    g = pis.good_case()
    for kw, words in ((dict(caps=[0]), "cap"), (dict(passes=[[(1, g.cap)]]), "add up"),
                      (dict(passes=[[(1, 1)] * 8]), "npasses"), (dict(passes=[[]]), "npasses"), (dict(passes=[[(0, 5), (1, g.cap - 1)]]), "pass")):
        a = dict(streams=[g.z], caps=[g.cap], passes=[None])
        a.update(kw)
        with pytest.raises(binding.MI355Error, match="png_inflate: .*" + words):
            binding.png_inflate_device(a["streams"], a["caps"], a["passes"])  # the guards and the status words are checked by the call
    L = binding.shim()
    table = (binding.PngStream * 1)()
    buf = binding.DevBuf.from_numpy(np.full(1024, 0xA5, np.uint8))
    t = table[0]
    t.nbytes, t.cap, t.npasses, t.rows[0], t.row_bytes[0] = 16, 64, 1, 1, 63

    def refused(words, nstreams=1, status=buf.ptr.value + 512):
        assert L.mi355_png_inflate(buf.ptr, table, nstreams, status, None) == -22  # MI355_EINVAL
        msg = L.mi355_last_error().decode()
        assert msg.split(": ", 1)[1].startswith("png_inflate:") and words in msg, msg  # "invalid argument: png_inflate: ..."

    t.z, t.out = None, buf.ptr.value + 256
    refused("null")
    t.z, t.out = buf.ptr.value, None
    refused("null")
    t.z, t.out = buf.ptr.value + 2, buf.ptr.value + 256
    refused("aligned")
    t.z, t.out = buf.ptr.value, buf.ptr.value + 257
    refused("aligned")
    t.z, t.out = buf.ptr.value, buf.ptr.value + 256
    t.nbytes = (1 << 28) + 1
    refused("2^28")
    t.nbytes, t.reserved = 16, 1
    refused("reserved")
    t.reserved, t.cap, t.row_bytes[0] = 0, 1 << 31, (1 << 31) - 1
    refused("cap")
    t.cap, t.row_bytes[0] = 64, 63
    refused("nstreams", nstreams=0)
    refused("nstreams", nstreams=65536)
    refused("null", status=None)
    assert L.mi355_png_inflate(None, table, 1, buf.ptr.value + 512, None) == -22
    assert (buf.to_numpy(np.uint8, 1024) == 0xA5).all()
    buf.free()


# ------------------------------------------------------------------------------------------------------------- the whole step
def _run(net, sizes):
    net.forward()
    net.sync()
    deep = max(i for i, inf in enumerate(net.info) if inf["type"] == binding.T_CONV)
    return net.pull(deep), net.detect([s[0] for s in sizes], [s[1] for s in sizes], thresh=0.005)


def _assert_same_input_and_run(a, b, sizes, what):
    xa, xb = a._pull_input(), b._pull_input()
    assert np.array_equal(xa, xb), f"{what}: input bytes"
    (sa, za), (sb, zb) = a.input_quantization(), b.input_quantization()
    assert np.array_equal(_bits(sa), _bits(sb)) and np.array_equal(za, zb), f"{what}: scales / zero points"
    (la, da), (lb, db) = _run(a, sizes), _run(b, sizes)
    for k in lb:
        assert np.array_equal(la[k], lb[k]), f"{what}: deep layer {k}"
    assert len(da) == len(db) == a.batch
    for slot, (x, y) in enumerate(zip(da, db)):
        assert x.keys() == y.keys()
        for k in x:
            assert np.array_equal(x[k], y[k]), f"{what}: detections of slot {slot}: {k}"
    return xa


def test_all_fixtures_decode_to_the_same_frames_with_the_mode_on(expected, tmp_path):
    net = binding.Net(CFG, _wts(tmp_path), batch=1)
    net.set_png_inflate_on_device(True)
    files = {n: data_of(n) for n in NAMES}
    for names in (NAMES[::-3], NAMES, NAMES[:1] * 3):  # buffers grow, are reused, one image's bytes in every slot
        waits = net.host_waits()
        got = binding.png_decode([files[n] for n in names], net=net)
        assert net.host_waits() - waits <= 2  # the status words; at most one more where a buffer grew
        for n, g in zip(names, got):
            assert np.array_equal(g, expected[n]), n
    net.close()


@pytest.mark.parametrize("mode", ["shared", "per_image", "on_device", "on_device_per_image"])
def test_prepare_from_png_mode_on_against_mode_off(expected, tmp_path, mode):
    wts = _wts(tmp_path)
    a, b = binding.Net(CFG, wts, batch=3), binding.Net(CFG, wts, batch=3)
    for net in (a, b):
        if "per_image" in mode:
            net.set_input_per_image(True)
        if "on_device" in mode:
            net.set_input_on_device(True)
    a.set_png_inflate_on_device(True)
    seen = set()
    for first in (9, 6, 3, 0):  # consecutive batches of different images, the larger files last: the buffers grow and are reused
        names = NET_NAMES[first:first + 3]
        sizes = a.prepare_from_png([data_of(n) for n in names])
        assert sizes == b.prepare_from_png([data_of(n) for n in names]) == [expected[n].shape[1::-1] for n in names]
        seen.add(_assert_same_input_and_run(a, b, sizes, f"{mode} {names}").tobytes())
    assert len(seen) == 4
    one = data_of(NET_NAMES[6])  # one file in every slot: scanned and inflated once
    sizes = a.prepare_from_png([one, one, one])
    b.prepare_from_png([one, one, one])
    _assert_same_input_and_run(a, b, sizes, f"{mode}: one file in three slots")
    # nothing grows any more: the decode waits exactly once, for the status words (the upload has completed with that wait, so no
    # call waits for a pending upload as the host mode's next call does); the frame step behind it reads min / max back, one more
    # wait, unless the input is derived on the device
    waits = a.host_waits()
    a.prepare_from_png([one, one, one])
    assert a.host_waits() - waits == (1 if "on_device" in mode else 2)
    waits = a.host_waits()
    binding.png_decode([one, one, one], net=a)  # network_png_decode_gpu alone
    assert a.host_waits() - waits == 1
    a.set_png_inflate_on_device(False)
    a.prepare_from_png([one, one, one])
    _assert_same_input_and_run(a, b, sizes, f"{mode}: the mode off again")
    a.close(); b.close()


def test_png_jpeg_ppm_in_turn_graph_replay_and_replica(expected, tmp_path):
    wts = _wts(tmp_path, seed=5)
    parent = binding.Net(CFG, wts, batch=3, use_graph=True)
    parent.set_input_per_image(True)
    parent.set_png_inflate_on_device(True)
    ref = binding.Net(CFG, wts, batch=3)
    ref.set_input_per_image(True)
    handle = None
    for first in (0, 3):  # the captured graph replays the second batch
        names = NET_NAMES[first:first + 3]
        sizes = parent.prepare_from_png([os.path.join(PNG_DIR, n + ".png") for n in names])  # paths
        ref.prepare_from_frames_u8([expected[n] for n in names])
        _assert_same_input_and_run(parent, ref, sizes, f"graph {names}")
        handle = handle or parent.graph_handle()
        assert handle and parent.graph_handle() == handle
    jpgs = [os.path.join(JPEG_DIR, "420_51x37.jpg")] * 3  # another format on the same network, then PNG again, then plain frames
    sizes = parent.prepare_from_jpeg(jpgs)
    ref.prepare_from_jpeg(jpgs)
    _assert_same_input_and_run(parent, ref, sizes, "jpeg in between")
    names = NET_NAMES[6:9]
    sizes = parent.prepare_from_png([data_of(n) for n in names])
    ref.prepare_from_frames_u8([expected[n] for n in names])
    _assert_same_input_and_run(parent, ref, sizes, "png after jpeg")
    parent.prepare_from_frames_u8([expected[n] for n in NET_NAMES[:3]])
    ref.prepare_from_frames_u8([expected[n] for n in NET_NAMES[:3]])
    _assert_same_input_and_run(parent, ref, [expected[n].shape[1::-1] for n in NET_NAMES[:3]], "frames after png")
    rep = parent.replica()  # inherits the mode; its own staging block, buffers and stream
    na, nb = NET_NAMES[6:9], NET_NAMES[9:12]
    waits = rep.host_waits()
    sa = rep.prepare_from_png([data_of(n) for n in na])
    assert rep.host_waits() > waits  # the replica inflates on the device too
    sb = parent.prepare_from_png([data_of(n) for n in nb])
    for _ in range(2):
        parent.forward()
        rep.forward()
    for net, names, sizes in ((rep, na, sa), (parent, nb, sb)):
        ref.prepare_from_frames_u8([expected[n] for n in names])
        _assert_same_input_and_run(net, ref, sizes, f"replica {names}")
    rep.close()
    ref.close()
    parent.close()


def test_a_damaged_file_in_slot_2_is_named_by_the_device_and_the_input_stays(expected, tmp_path):
    net = binding.Net(CFG, _wts(tmp_path), batch=3)
    net.set_png_inflate_on_device(True)
    good = [data_of(n) for n in NET_NAMES[:3]]
    sizes = net.prepare_from_png(good)
    before = net._pull_input()
    refused = png_streams.refusal_files()
    for name, message in (("invalid_filter", "png slot 2: invalid filter (device)"), ("bad_dist", "png slot 2: bad dist (device)"),
                          ("not_enough_pixels", "png slot 2: not enough pixels (device)"), ("bad_block_type", "png slot 2: bad block type (device)")):
        waits = net.host_waits()
        with pytest.raises(binding.PngError) as e:
            net.prepare_from_png([good[0], good[1], refused[name][0]])
        assert str(e.value) == message
        assert net.host_waits() == waits + 1  # the inflate ran; nothing behind it did
        assert np.array_equal(net._pull_input(), before)
        with pytest.raises(binding.PngError) as e:
            binding.png_decode([good[0], good[1], refused[name][0]], net=net)
        assert str(e.value) == message
    waits = net.host_waits()
    for bad, message in ((refused["no_plte"][0], "png slot 2: no PLTE"), (refused["bad_zlib_header"][0], "png slot 2: bad zlib header"),
                         (b"P6\n1 1\n255\n", "png slot 2: bad png sig")):  # a header refusal still launches nothing
        with pytest.raises(binding.PngError) as e:
            net.prepare_from_png([good[0], good[1], bad])
        assert str(e.value) == message
    assert net.host_waits() == waits
    assert np.array_equal(net._pull_input(), before)
    assert sizes == [expected[n].shape[1::-1] for n in NET_NAMES[:3]]
    net.close()


# ------------------------------------------------------------------------------------------------------------------- CLI
def test_cli_prints_the_same_with_and_without_png_device(expected, tmp_path):
    exe = os.path.join(ROOT, "yolo_quantization_amd", "bin", "darknet")
    wts = _wts(tmp_path, seed=1)
    names = str(tmp_path / "x.names")
    open(names, "w").write("\n".join(["ant", "bee", "cat", "dog", "eel"]) + "\n")
    data = str(tmp_path / "x.data")
    open(data, "w").write(f"classes= 5\nnames = {names}\n")
    picks = ["rgb8_plain_51x37", "pal4_adam7_51x37", "grey16_plain_51x37", "rgba16_adam7_51x37", "rgb8_adam7_64x61"]
    png = [os.path.join(PNG_DIR, n + ".png") for n in picks]
    ppm = str(tmp_path / "a.ppm")
    _write_ppm(ppm, expected[picks[1]])
    mixed = [png[0], os.path.join(JPEG_DIR, "420_51x37.jpg"), ppm, png[3], png[4], png[2]]
    lst = str(tmp_path / "mixed.txt")
    open(lst, "w").write("\n".join(mixed) + "\n")

    def run(extra, ok=True):
        r = subprocess.run([exe, "detector", "test", data, CFG, wts] + extra + ["-thresh", "0.3", "-boxes"], capture_output=True, text=True, timeout=300)
        assert (r.returncode == 0) == ok, r.stderr
        return _blocks(r.stdout) if ok else r.stderr  # stdout, the seconds of the timing lines apart

    for args in ([png[0]], ["-list", lst, "-batch", "3"], ["-list", lst, "-batch", "2", "-input_device"]):
        want = run(args)
        assert run(args + ["-png_device"]) == want and any(line.startswith("box:") for blk in want for line in blk)
        assert [b[0] for b in want] == (mixed if "-list" in args else [png[0]])
    bad = os.path.join(PNG_DIR, "refuse_invalid_filter.png")
    bad_list = str(tmp_path / "bad.txt")
    open(bad_list, "w").write("\n".join([png[0], ppm, bad]) + "\n")
    err = run(["-list", bad_list, "-batch", "3", "-png_device"], ok=False)
    assert "slot 2" in err and bad in err and "invalid filter (device)" in err
