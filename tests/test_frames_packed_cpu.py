"""CPU checks behind the packed (RGBA, BGRA, ARGB, ABGR, YUYV, UYVY, YVYU) and P010 frame input paths
(mi355_frames_packed_* / mi355_frames_p010_*, network_frames_packed_input_gpu / network_frames_p010_input_gpu): the constants and
struct layouts of the C header against their ctypes mirrors, the exported symbols, the numpy converters that specify both sources
(frames_packed_util) against a per-pixel loop, the refusals of the C-ABI calls and of the host entry points, which come before they
touch a device, and the CLI's raw-file reader.  No kernel is launched here."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from frames_packed_util import RGBX, YUV422, p010_to_nv12, packed_row_bytes, rgbx_to_rgb, yuv422_to_planes
from frames_util import ROOT
from yolo_quantization_amd import binding

PACKED = ["rgba", "bgra", "argb", "abgr", "yuyv", "uyvy", "yvyu"]
RAW_KIND = {**{f: 32 + k for k, f in enumerate(PACKED)}, "p010": 48}  # raw_frame_file.h


def _c_values(tmp_path, body):
    src = '#include <stddef.h>\n#include <stdio.h>\n#include "mi355_yolo_int8.h"\nint main(void) {\n' + body + "    return 0;\n}\n"
    c = tmp_path / "layout.c"
    c.write_text(src)
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    return [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]


@pytest.mark.parametrize("struct,mirror,size,fields", [
    ("mi355_frame_packed", "FramePacked", 32, ["data", "w", "h", "pitch", "format", "matrix", "reserved"]),
    ("mi355_frame_p010", "FrameP010", 48, ["y", "uv", "w", "h", "pitch_y", "pitch_uv", "layout", "matrix", "reserved"])])
def test_struct_mirrors_match_the_c_header(tmp_path, struct, mirror, size, fields):
    py = getattr(binding, mirror)
    names = [f[0] for f in py._fields_]
    assert names == fields
    body = f'    printf("%zu", sizeof({struct}));\n' + "".join(f'    printf(" %zu", offsetof({struct}, {n}));\n' for n in names)
    body += '    printf(" %d %zu %zu %zu\\n", MI355_ABI_VERSION, sizeof(mi355_frame_u8), sizeof(mi355_frame_yuv), sizeof(mi355_frame_planar));\n'
    vals = _c_values(tmp_path, body)
    nf = len(names)
    assert vals[0] == C.sizeof(py) == size
    assert vals[1:1 + nf] == [getattr(py, n).offset for n in names]
    assert sum(C.sizeof(t) for _, t in py._fields_) == C.sizeof(py)  # no hidden padding
    assert vals[1 + nf] == binding.ABI_VERSION == 6  # new structs and new calls do not bump the ABI
    assert vals[2 + nf:] == [C.sizeof(binding.FrameU8), C.sizeof(binding.FrameYUV), C.sizeof(binding.FramePlanar)] == [32, 48, 64]


def test_p010_entry_has_the_nv12_entrys_field_layout():
    assert [(n, getattr(binding.FrameP010, n).offset, getattr(binding.FrameP010, n).size) for n, _ in binding.FrameP010._fields_] == \
           [(n, getattr(binding.FrameYUV, n).offset, getattr(binding.FrameYUV, n).size) for n, _ in binding.FrameYUV._fields_]


def test_constants_match_the_c_header(tmp_path):
    body = ('    printf("%d %d %d %d %d %d %d %d %d %d %d %d\\n", MI355_PACKED_RGBA, MI355_PACKED_BGRA, MI355_PACKED_ARGB, MI355_PACKED_ABGR,'
            " MI355_PACKED_YUYV, MI355_PACKED_UYVY, MI355_PACKED_YVYU, MI355_YUV_BT601, MI355_YUV_BT601_FULL, MI355_YUV_BT709,"
            " MI355_YUV_BT709_FULL, MI355_ABI_VERSION);\n")
    vals = _c_values(tmp_path, body)
    assert vals[:7] == [binding.PACKED_FORMAT[k] for k in PACKED] == [0, 1, 2, 3, 4, 5, 6]
    assert vals[7:11] == [binding.YUV_MATRIX[k] for k in ("bt601", "bt601f", "bt709", "bt709f")] == [0, 1, 2, 3]
    assert vals[11] == binding.ABI_VERSION == 6
    assert set(binding.PACKED_RGBX) == set(RGBX) and set(PACKED) - set(RGBX) == set(YUV422)


def test_new_entry_points_are_exported():
    for n in ("mi355_frames_packed_letterbox_minmax", "mi355_frames_packed_letterbox_quantize", "mi355_frames_p010_letterbox_minmax",
              "mi355_frames_p010_letterbox_quantize"):
        assert hasattr(binding.shim(), n), n
    for n in ("network_frames_packed_input_gpu", "network_frames_p010_input_gpu"):
        assert hasattr(binding.host(), n), n
    assert hasattr(binding.Net, "prepare_from_frames_packed") and hasattr(binding.Net, "prepare_from_frames_p010")


# ----------------------------------------------------------------------------------------- the converters against a loop
@pytest.mark.parametrize("fmt", sorted(RGBX))
@pytest.mark.parametrize("w,h", [(5, 3), (1, 1), (4, 2)])
def test_rgbx_to_rgb_against_a_per_pixel_loop(fmt, w, h):
    frame = np.random.default_rng(w + 10 * h).integers(0, 256, (h, w, 4), dtype=np.uint8)
    layout = {"rgba": "RGBx", "bgra": "BGRx", "argb": "xRGB", "abgr": "xBGR"}[fmt]  # the bytes of a pixel, written out
    want = np.zeros((h, w, 3), np.uint8)
    for y in range(h):
        for x in range(w):
            for k, ch in enumerate("RGB"):
                want[y, x, k] = frame[y, x, layout.index(ch)]
    got = rgbx_to_rgb(frame, fmt)
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    other = frame.copy()
    other[:, :, layout.index("x")] ^= 0xFF  # the fourth byte changes nothing
    assert np.array_equal(rgbx_to_rgb(other, fmt), want)


@pytest.mark.parametrize("fmt", sorted(YUV422))
@pytest.mark.parametrize("w,h", [(5, 3), (1, 1), (1, 4), (6, 2), (7, 1)], ids=["odd_w", "one_pixel", "w1", "even_w", "one_row"])
def test_yuv422_to_planes_against_a_per_pixel_loop(fmt, w, h):
    cw = (w + 1) // 2
    frame = np.random.default_rng(w + 10 * h).integers(0, 256, (h, 4 * cw), dtype=np.uint8)
    layout = {"yuyv": "aUbV", "uyvy": "UaVb", "yvyu": "aVbU"}[fmt]  # a = Y0, b = Y1
    Y, U, V = np.zeros((h, w), np.uint8), np.zeros((h, cw), np.uint8), np.zeros((h, cw), np.uint8)
    for y in range(h):
        for x in range(w):
            mp = frame[y, 4 * (x // 2):4 * (x // 2) + 4]
            Y[y, x] = mp[layout.index("ab"[x % 2])]
            U[y, x // 2], V[y, x // 2] = mp[layout.index("U")], mp[layout.index("V")]
    got = yuv422_to_planes(frame, w, fmt)
    assert [g.shape for g in got] == [(h, w), (h, cw), (h, cw)] and all(g.dtype == np.uint8 for g in got)
    for g, wnt in zip(got, (Y, U, V)):
        assert np.array_equal(g, wnt)
    if w % 2:  # the last macropixel holds one valid pixel: its second luma byte changes nothing
        other = frame.copy()
        other[:, 4 * (cw - 1) + layout.index("b")] ^= 0xFF
        for g, wnt in zip(yuv422_to_planes(other, w, fmt), (Y, U, V)):
            assert np.array_equal(g, wnt)
    wide = np.concatenate([frame, np.full((h, 5), 0xEE, np.uint8)], axis=1)  # row padding is not part of the frame
    for g, wnt in zip(yuv422_to_planes(wide, w, fmt), (Y, U, V)):
        assert np.array_equal(g, wnt)


def test_p010_to_nv12_truncates_to_the_high_byte():
    samples = np.array([0x0000, 0x00FF, 0x0100, 0xFFC0, 0xFFFF], np.uint16)
    y16 = np.resize(samples, (3, 5))
    uv16 = np.resize(samples[::-1], (2, 3, 2))
    y, uv = p010_to_nv12(y16, uv16)
    assert y.dtype == uv.dtype == np.uint8 and y.shape == (3, 5) and uv.shape == (2, 3, 2)
    assert y[0].tolist() == [0x00, 0x00, 0x01, 0xFF, 0xFF]  # 0x00FF -> 0 (not rounded up to 1), 0xFFC0 and 0xFFFF -> 255
    for got, src in ((y, y16), (uv, uv16)):
        raw = src.astype("<u2").tobytes()  # the little-endian bytes a decoder writes: the sample's high byte is the second one
        for i, g in enumerate(got.ravel()):
            assert g == raw[2 * i + 1] == int(src.ravel()[i]) // 256


# ------------------------------------------------------------------------------------------------ C-ABI refusals
def _packed(**kw):
    e = dict(data=0x1000, w=9, h=17, pitch=36, format=1, matrix=0, reserved=0)  # a good 9 x 17 BGRA entry; data is never dereferenced
    e.update(kw)
    return binding.FramePacked(**e)


def _p010(**kw):
    e = dict(y=0x1000, uv=0x2000, w=9, h=17, pitch_y=18, pitch_uv=20, layout=0, matrix=0)
    reserved = kw.pop("reserved", (0, 0))
    e.update(kw)
    return binding.FrameP010(reserved=(C.c_int * 2)(*reserved), **e)


# one case per clause of the contract in mi355_yolo_int8.h and per kind: the bad entry and what the message says after the prefix
ABI_REFUSALS = [("packed_null_data", _packed(data=None), "null frame pointer"),
                ("packed_w_zero", _packed(w=0), "need 1 <= w, h <= 32768"),
                ("packed_h_beyond_32768", _packed(h=32769), "need 1 <= w, h <= 32768"),
                ("packed_rgbx_pitch_one_below_minimum", _packed(pitch=35), "pitch < 4 * w"),
                ("packed_422_pitch_one_below_minimum", _packed(format=4, pitch=19), "pitch < 4 * ((w + 1) / 2)"),
                ("packed_unknown_format", _packed(format=7), "unknown format"),
                ("packed_negative_format", _packed(format=-1), "unknown format"),
                ("packed_unknown_matrix", _packed(format=5, matrix=4), "unknown matrix"),
                ("packed_matrix_with_bgra", _packed(matrix=1), "matrix must be 0 with MI355_PACKED_RGBA"),
                ("packed_geometry_1x7", _packed(w=1, h=7, pitch=4), "degenerate aspect (resized side < 2)"),
                ("packed_geometry_7x1", _packed(format=4, w=7, h=1, pitch=16), "degenerate aspect (resized side < 2)"),
                ("p010_null_y", _p010(y=None), "null plane pointer"),
                ("p010_null_uv", _p010(uv=None), "null plane pointer"),
                ("p010_w_beyond_32768", _p010(w=32769), "need 1 <= w, h <= 32768"),
                ("p010_h_zero", _p010(h=0), "need 1 <= w, h <= 32768"),
                ("p010_luma_pitch_one_below_minimum", _p010(pitch_y=17), "pitch_y < 2 * w"),
                ("p010_chroma_pitch_one_below_minimum", _p010(pitch_uv=19), "pitch_uv < 4 * ((w + 1) / 2)"),
                ("p010_unknown_matrix", _p010(matrix=4), "unknown matrix"),
                ("p010_layout_set", _p010(layout=1), "layout and reserved must be 0"),
                ("p010_reserved_set", _p010(reserved=(0, 1)), "layout and reserved must be 0"),
                ("p010_geometry_1x7", _p010(w=1, h=7, pitch_y=2, pitch_uv=4), "degenerate aspect (resized side < 2)"),
                ("p010_geometry_7x1", _p010(w=7, h=1, pitch_y=14, pitch_uv=16), "degenerate aspect (resized side < 2)")]


@pytest.mark.parametrize("what,bad,message", ABI_REFUSALS, ids=[r[0] for r in ABI_REFUSALS])
def test_c_abi_calls_refuse_from_the_host_table_alone(what, bad, message):
    """table_host is validated before anything is launched, so a refusal needs no device: MI355_EINVAL and the message from both
    calls, for a bad entry behind a good one.  (That nothing was written is checked on the device, tests/test_gpu_frames_packed.py.)"""
    kind, good = ("packed", _packed()) if isinstance(bad, binding.FramePacked) else ("p010", _p010())
    S = binding.shim()
    table = (type(bad) * 2)(good, bad)
    fake = C.c_void_p(0x1000)  # device arguments: checked for null only, a refused call never passes them on
    want = f"invalid argument: frames_{kind}: {message}".encode()
    assert getattr(S, f"mi355_frames_{kind}_letterbox_minmax")(fake, table, 2, 12, 12, fake, None) == -22
    assert S.mi355_last_error().startswith(want), S.mi355_last_error()
    assert getattr(S, f"mi355_frames_{kind}_letterbox_quantize")(fake, table, 2, 12, 12, fake, fake, fake, None) == -22
    assert S.mi355_last_error().startswith(want), S.mi355_last_error()
    # a null argument and a batch beyond 65535 are refused too, before the table is read
    assert getattr(S, f"mi355_frames_{kind}_letterbox_minmax")(None, table, 2, 12, 12, fake, None) == -22
    assert S.mi355_last_error().startswith(f"invalid argument: frames_{kind}: letterbox_minmax: null".encode())
    assert getattr(S, f"mi355_frames_{kind}_letterbox_minmax")(fake, table, 65536, 12, 12, fake, None) == -22
    assert S.mi355_last_error().startswith(f"invalid argument: frames_{kind}: null table / need 1 <= B <= 65535".encode())


# -------------------------------------------------------------------------------------------------- host refusals
REFUSAL = """
import ctypes as C, sys
sys.path.insert(0, {root!r})
import numpy as np
from yolo_quantization_amd import binding
net = binding.Net({cfg!r}, None, batch=1)
w, h = 9, 7
one = lambda v: (C.c_int * 1)(v)
frame = np.zeros((h, 4 * w), np.uint8)
y, uv = np.zeros((h, 2 * w), np.uint8), np.zeros((4, 20), np.uint8)
ptr = {{k: (C.c_void_p * 1)(a.ctypes.data) for k, a in (("frame", frame), ("y", y), ("uv", uv))}}
ws, hs, pitch, pitch_y, pitch_uv = one(w), one(h), one({pitch}), one(2 * w), one(20)
fmt, matrix = {fmt}, {matrix}
{change}
if {packed}:
    net.H.network_frames_packed_input_gpu(net.h, ptr["frame"], ws, hs, pitch, fmt, matrix, 0)
else:
    net.H.network_frames_p010_input_gpu(net.h, ptr["y"], ptr["uv"], ws, hs, pitch_y, pitch_uv, matrix, 0)
print("returned")
"""

# what, the entry point (packed?), format id, matrix id, the pitch of a 9 x 7 packed frame, the change to a good call, the message
REFUSALS = [("packed_null_frame", True, 1, 0, 36, "ptr['frame'][0] = None", "null frame"),
            ("packed_null_array", True, 1, 0, 36, "ws = None", "null frames / sizes"),
            ("packed_w_zero", True, 1, 0, 36, "ws = one(0)", "need 1 <= w, h <= 32768"),
            ("packed_h_beyond_32768", True, 4, 0, 36, "hs = one(32769)", "need 1 <= w, h <= 32768"),
            ("packed_rgbx_pitch_one_below_minimum", True, 0, 0, 35, "", "need pitch >= 4 * w"),
            ("packed_422_pitch_one_below_minimum", True, 4, 0, 19, "", "need pitch >= 4 * w"),
            ("packed_unknown_format", True, 7, 0, 36, "", "unknown format"),
            ("packed_negative_format", True, -1, 0, 36, "", "unknown format"),
            ("packed_unknown_matrix", True, 5, 4, 36, "", "unknown matrix"),
            ("packed_matrix_with_bgra", True, 1, 1, 36, "", "matrix must be 0 with MI355_PACKED_RGBA"),
            ("packed_matrix_with_abgr", True, 3, 3, 36, "", "matrix must be 0 with MI355_PACKED_RGBA"),
            ("p010_null_plane", False, 0, 0, 0, "ptr['uv'][0] = None", "null plane"),
            ("p010_null_array", False, 0, 0, 0, "hs = None", "null planes / sizes"),
            ("p010_w_beyond_32768", False, 0, 0, 0, "ws = one(32769)", "need 1 <= w, h <= 32768"),
            ("p010_h_zero", False, 0, 0, 0, "hs = one(0)", "need 1 <= w, h <= 32768"),
            ("p010_luma_pitch_one_below_minimum", False, 0, 0, 0, "pitch_y = one(17)", "need pitch_y >= 2 * w"),
            ("p010_chroma_pitch_one_below_minimum", False, 0, 0, 0, "pitch_uv = one(19)", "need pitch_y >= 2 * w and pitch_uv >= 4 * ((w + 1) / 2)"),
            ("p010_unknown_matrix", False, 0, 4, 0, "", "unknown matrix"),
            ("p010_negative_matrix", False, 0, -1, 0, "", "unknown matrix")]


@pytest.mark.parametrize("what,packed,fmt,matrix,pitch,change,message", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_host_entries_refuse_before_they_touch_a_device(what, packed, fmt, matrix, pitch, change, message):
    """error() of the host library: its message and exit(-1), with or without a device in the box"""
    code = REFUSAL.format(root=ROOT, cfg=os.path.join(ROOT, "cfg", "tiny_unit.cfg"), packed=packed, fmt=fmt, matrix=matrix, pitch=pitch,
                          change=change)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 255 and "returned" not in r.stdout, (r.returncode, r.stderr[-500:])
    name = "network_frames_packed_input_gpu: " if packed else "network_frames_p010_input_gpu: "
    assert name + message in r.stderr, r.stderr[-500:]


def test_python_methods_refuse_malformed_frames():
    """raised by the binding before the host library is called: no device is needed"""
    net = binding.Net(os.path.join(ROOT, "cfg", "tiny_unit.cfg"), None, batch=1)
    z = np.zeros
    bad_packed = [(dict(format="bgra"), z((7, 9, 3), np.uint8)),                    # three bytes a pixel
                  (dict(format="bgra"), z((7, 9, 4), np.uint16)),                   # not bytes
                  (dict(format="bgra", matrix="bt709"), z((7, 9, 4), np.uint8)),    # a matrix with an RGB format
                  (dict(format="rgba"), (z((7, 9, 4), np.uint8), 9)),               # a width beside an RGB frame
                  (dict(format="yuyv"), z((7, 18), np.uint8)),                      # half a macropixel at the end of the row
                  (dict(format="uyvy"), (z((7, 16), np.uint8), 9)),                 # rows too short for nine pixels
                  (dict(format="yvyu"), z((7, 5, 4), np.uint8))]                    # not [h][row_bytes]
    for kw, f in bad_packed:
        with pytest.raises(ValueError):
            net.prepare_from_frames_packed([f], **kw)
    bad_p010 = [(z((7, 9), np.uint8), z((4, 5, 2), np.uint8)),     # 8-bit planes
                (z((7, 9), np.uint16), z((4, 4, 2), np.uint16)),   # a chroma plane of another size
                (z((7, 9), np.uint16), z((4, 10), np.uint16)),     # pairs not on an axis of their own
                z((7, 9), np.uint16)]                              # no pair
    for f in bad_p010:
        with pytest.raises(ValueError):
            net.prepare_from_frames_p010([f])
    class Tensor:  # what the binding asks of a device tensor, with torch's dtype names; refused before its address is used
        def __init__(self, shape, dtype, item):
            self.shape, self.dtype, self._item = shape, dtype, item

        def data_ptr(self):
            return 0x1000

        def element_size(self):
            return self._item

        def stride(self, k):
            return int(np.prod(self.shape[k + 1:]))
    for dtype in ("torch.int8", "torch.float8_e4m3fn", "torch.bool"):  # one byte an element, but no uint8
        with pytest.raises(ValueError):
            net.prepare_from_frames_packed([Tensor((7, 9, 4), dtype, 1)], format="bgra")
    for dtype in ("torch.int16", "torch.float16", "torch.bfloat16"):  # two bytes an element, but no uint16
        with pytest.raises(ValueError):
            net.prepare_from_frames_p010([(Tensor((7, 9), dtype, 2), Tensor((4, 5, 2), dtype, 2))])
    with pytest.raises(ValueError):
        net.prepare_from_frames_p010([(Tensor((7, 9), "torch.uint16", 2), Tensor((4, 5, 2), "torch.int16", 2))])
    with pytest.raises(ValueError):
        net.prepare_from_frames_packed([z((7, 9, 4), np.uint8)], format="rgb")  # three bytes a pixel go through prepare_from_frames_u8


# ---------------------------------------------------------------------------------------------- the CLI's raw-file reader
def raw_sizes(fmt, w, h):
    """(bytes of plane 0, bytes of the plane after it) of a raw file"""
    if fmt == "p010":
        return 2 * w * h, 4 * ((w + 1) // 2) * ((h + 1) // 2)
    return packed_row_bytes(fmt, w) * h, 0


READER_MAIN = r"""
#include <stdio.h>
#include <stdlib.h>
#include "raw_frame_file.h"
int main(int argc, char **argv)
{
    int w = -1, h = -1;
    size_t bytes[2] = {0, 0};
    char why[1024] = "";
    if (argc != 3) return 2;
    uint8_t *raw = load_raw_frame_file(argv[1], atoi(argv[2]), &w, &h, bytes, why, sizeof(why));
    if (!raw) { fprintf(stderr, "%s", why); return 1; }
    printf("%d %d %zu %zu\n", w, h, bytes[0], bytes[1]);
    fwrite(raw, 1, bytes[0] + bytes[1], stdout); /* one plane, or P010's two */
    free(raw);
    return 0;
}
"""


@pytest.fixture(scope="module")
def reader(tmp_path_factory):
    """the CLI's raw-file reader (host/raw_frame_file.c, linked into ./darknet only) behind a main of the test's: no device, no library"""
    d = tmp_path_factory.mktemp("packed_reader")
    host = os.path.join(ROOT, "yolo_quantization_amd", "host")
    (d / "main.c").write_text(READER_MAIN)
    exe = d / "reader"
    subprocess.run(["gcc", "-O1", "-Wall", "-Wextra", "-Werror", "-I", host, str(d / "main.c"), os.path.join(host, "raw_frame_file.c"), "-o",
                    str(exe)], check=True)

    def load(path, fmt):
        """(bytes, w, h, plane 0 bytes, next plane's bytes, message)"""
        r = subprocess.run([str(exe), str(path), str(RAW_KIND[fmt])], capture_output=True)
        if r.returncode:
            assert r.returncode == 1 and not r.stdout
            return None, -1, -1, -1, -1, r.stderr.decode()
        head, _, body = r.stdout.partition(b"\n")
        w, h, n0, n1 = (int(v) for v in head.split())
        return body, w, h, n0, n1, r.stderr.decode()
    return load


SIZES_WRITTEN_OUT = {("rgba", 53, 37): (7844, 0), ("yuyv", 53, 37): (3996, 0), ("p010", 53, 37): (3922, 2052),
                     ("rgba", 1, 1): (4, 0), ("yuyv", 1, 1): (4, 0), ("p010", 1, 1): (2, 4),
                     ("rgba", 2, 3): (24, 0), ("yuyv", 2, 3): (12, 0), ("p010", 2, 3): (12, 8)}


@pytest.mark.parametrize("fmt", PACKED + ["p010"])
@pytest.mark.parametrize("w,h", [(53, 37), (1, 1), (2, 3)])
def test_cli_raw_file_reader_reads_good_names_of_every_format(tmp_path, reader, fmt, w, h):
    n0, n1 = raw_sizes(fmt, w, h)
    like = "rgba" if fmt in RGBX else ("yuyv" if fmt in YUV422 else "p010")
    assert (n0, n1) == SIZES_WRITTEN_OUT[like, w, h]
    raw = np.random.default_rng(w * 100 + h).integers(0, 256, n0 + n1, dtype=np.uint8)
    good = tmp_path / f"clip_a_{w}x{h}.{fmt}"
    good.write_bytes(raw.tobytes())
    p, gw, gh, g0, g1, why = reader(good, fmt)
    assert p is not None and (gw, gh, g0, g1) == (w, h, n0, n1) and why == ""
    assert np.array_equal(np.frombuffer(p, np.uint8), raw)


@pytest.mark.parametrize("fmt", PACKED + ["p010"])
def test_cli_raw_file_reader_refuses_bad_names_extensions_and_lengths(tmp_path, reader, fmt):
    w, h = 53, 37
    n = sum(raw_sizes(fmt, w, h))
    raw = np.random.default_rng(1).integers(0, 256, n, dtype=np.uint8)
    other = (PACKED + ["p010"])[(PACKED + ["p010"]).index(fmt) - 1]
    for name in (f"clip.{fmt}", f"clip_53x.{fmt}", "clip_53x37.yuv", f"clip_53x37.{other}", "clip_53x37.nv12", "clip_53x37.i422",
                 f"clip_53x37.{fmt}.bak", f"clip_0x37.{fmt}", f"53x37.{fmt}", f"clip_32769x37.{fmt}", f"clip_53x37.{fmt.upper()}"):
        bad = tmp_path / name
        bad.write_bytes(raw.tobytes())
        p, _, _, _, _, why = reader(bad, fmt)
        assert p is None and f"_<W>x<H>.{fmt}" in why and name in why, name
    for delta in (-1, 1):
        bad = tmp_path / f"len{delta}_53x37.{fmt}"
        bad.write_bytes(np.resize(raw, n + delta).tobytes())
        p, _, _, _, _, why = reader(bad, fmt)
        assert p is None and "_<W>x<H>" not in why, why
        assert f"holds {n} bytes, the file holds {'more than ' + str(n) if delta > 0 else n - 1}" in why, why
    p, _, _, _, _, why = reader(tmp_path / f"missing_53x37.{fmt}", fmt)
    assert p is None and "cannot open" in why
