"""CPU checks behind the planar frame input path (mi355_frames_planar_letterbox_minmax / _quantize, network_frames_planar_input_gpu):
the ctypes mirror of the new C-ABI struct, the exported symbols, the CLI's raw-file reader and the refusals of the host entry point,
which come before it touches a device.  No kernel is launched here."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from frames_util import ROOT
from yolo_quantization_amd import binding

FORMATS = ["i420", "yv12", "i422", "i444", "rgb", "bgr"]


def planar_sizes(fmt, w, h):
    """(bytes of plane 0, bytes of each of planes 1 and 2) of a tightly packed frame"""
    cw = w if fmt in ("i444", "rgb", "bgr") else (w + 1) // 2
    ch = (h + 1) // 2 if fmt in ("i420", "yv12") else h
    return w * h, cw * ch


def test_planar_struct_mirror_matches_the_c_header(tmp_path):
    names = [f[0] for f in binding.FramePlanar._fields_]
    src = "#include <stddef.h>\n#include <stdio.h>\n#include \"mi355_yolo_int8.h\"\nint main(void) {\n"
    src += '    printf("%zu", sizeof(mi355_frame_planar));\n'
    for n in names:
        src += f'    printf(" %zu", offsetof(mi355_frame_planar, {n}));\n'
    src += ('    printf(" %d %d %d %d %d %d %d %zu %zu\\n", MI355_PLANAR_I420, MI355_PLANAR_YV12, MI355_PLANAR_I422, MI355_PLANAR_I444,'
            ' MI355_PLANAR_RGB, MI355_PLANAR_BGR, MI355_ABI_VERSION, sizeof(mi355_frame_u8), sizeof(mi355_frame_yuv));\n    return 0;\n}\n')
    c = tmp_path / "layout.c"
    c.write_text(src)
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    vals = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    nf = len(names)
    assert names == ["plane", "w", "h", "pitch", "format", "matrix", "reserved"]
    assert vals[0] == C.sizeof(binding.FramePlanar) == 64
    assert vals[1:1 + nf] == [getattr(binding.FramePlanar, n).offset for n in names]
    assert sum(C.sizeof(t) for _, t in binding.FramePlanar._fields_) == C.sizeof(binding.FramePlanar)  # no hidden padding
    assert vals[1 + nf:7 + nf] == [binding.PLANAR_FORMAT[k] for k in FORMATS] == [0, 1, 2, 3, 4, 5]
    assert vals[7 + nf] == binding.ABI_VERSION == 6  # a new struct and new calls do not bump the ABI
    assert vals[8 + nf] == C.sizeof(binding.FrameU8) == 32 and vals[9 + nf] == C.sizeof(binding.FrameYUV) == 48  # the others are as they were


def test_new_entry_points_are_exported():
    for n in ("mi355_frames_planar_letterbox_minmax", "mi355_frames_planar_letterbox_quantize"):
        assert hasattr(binding.shim(), n), n
    assert hasattr(binding.host(), "network_frames_planar_input_gpu")
    assert hasattr(binding.Net, "prepare_from_frames_planar")


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
    fwrite(raw, 1, bytes[0] + 2 * bytes[1], stdout);
    free(raw);
    return 0;
}
"""


@pytest.fixture(scope="module")
def reader(tmp_path_factory):
    """the CLI's raw-file reader (host/raw_frame_file.c, linked into ./darknet only) behind a main of the test's: no device, no library"""
    d = tmp_path_factory.mktemp("planar_reader")
    host = os.path.join(ROOT, "yolo_quantization_amd", "host")
    (d / "main.c").write_text(READER_MAIN)
    exe = d / "reader"
    subprocess.run(["gcc", "-O1", "-Wall", "-Wextra", "-Werror", "-I", host, str(d / "main.c"), os.path.join(host, "raw_frame_file.c"), "-o",
                    str(exe)], check=True)

    def load(path, fmt):
        """(bytes, w, h, plane 0 bytes, chroma plane bytes, message)"""
        r = subprocess.run([str(exe), str(path), str(fmt if isinstance(fmt, int) else FORMATS.index(fmt))], capture_output=True)
        if r.returncode:
            assert r.returncode == 1 and not r.stdout
            return None, -1, -1, -1, -1, r.stderr.decode()
        head, _, body = r.stdout.partition(b"\n")
        w, h, n0, n1 = (int(v) for v in head.split())
        return body, w, h, n0, n1, r.stderr.decode()
    return load


@pytest.mark.parametrize("fmt", FORMATS[:4])
@pytest.mark.parametrize("w,h", [(7, 5), (8, 6), (1, 1), (6, 3)], ids=["odd_odd", "even_even", "one_pixel", "even_odd"])
def test_cli_raw_file_reader_reads_good_names_of_every_format(tmp_path, reader, fmt, w, h):
    n0, n1 = planar_sizes(fmt, w, h)
    if (w, h) == (7, 5):  # the sizes written out: 4:2:0 rounds both sides up, 4:2:2 the width only
        assert (n0, n1) == {"i420": (35, 12), "yv12": (35, 12), "i422": (35, 20), "i444": (35, 35)}[fmt]
    raw = np.random.default_rng(w * 100 + h).integers(0, 256, n0 + 2 * n1, dtype=np.uint8)
    good = tmp_path / f"clip_a_{w}x{h}.{fmt}"
    good.write_bytes(raw.tobytes())
    p, gw, gh, g0, g1, why = reader(good, fmt)
    assert p is not None and (gw, gh, g0, g1) == (w, h, n0, n1) and why == ""
    assert np.array_equal(np.frombuffer(p, np.uint8), raw)


@pytest.mark.parametrize("fmt", FORMATS[:4])
def test_cli_raw_file_reader_refuses_bad_names_extensions_and_lengths(tmp_path, reader, fmt):
    w, h = 7, 5
    n0, n1 = planar_sizes(fmt, w, h)
    n = n0 + 2 * n1
    raw = np.random.default_rng(1).integers(0, 256, n, dtype=np.uint8)
    other = FORMATS[(FORMATS.index(fmt) + 1) % 4]
    # no size, half a size, other suffixes (another planar format's and NV12's among them), a zero side, no underscore; blanks and
    # signs are no digits; sides beyond 32768 and digit strings that would overflow an int are refused, not wrapped
    for name in (f"clip.{fmt}", f"clip_7x.{fmt}", "clip_7x5.yuv", f"clip_7x5.{other}", "clip_7x5.nv12", f"clip_7x5.{fmt}.bak", f"clip_0x5.{fmt}",
                 f"7x5.{fmt}", f"clip_ 7x5.{fmt}", f"clip_7x+5.{fmt}", f"clip_-7x5.{fmt}", f"clip_7x5 .{fmt}", f"clip_32769x5.{fmt}",
                 f"clip_7x4294967301.{fmt}", "clip_" + "9" * 40 + f"x5.{fmt}", f"clip_7x5.{fmt.upper()}"):
        bad = tmp_path / name
        bad.write_bytes(raw.tobytes())
        p, _, _, _, _, why = reader(bad, fmt)
        assert p is None and f"_<W>x<H>.{fmt}" in why and name in why, name
    for delta in (-1, 1):
        bad = tmp_path / f"len{delta}_7x5.{fmt}"
        bad.write_bytes(np.resize(raw, n + delta).tobytes())
        p, _, _, _, _, why = reader(bad, fmt)
        assert p is None and f"holds {n} bytes" in why and "_<W>x<H>" not in why, why
    if fmt != "i444":  # the length of another format under this format's name
        m0, m1 = planar_sizes("i444", w, h)
        bad = tmp_path / f"as444_7x5.{fmt}"
        bad.write_bytes(np.resize(raw, m0 + 2 * m1).tobytes())
        p, _, _, _, _, why = reader(bad, fmt)
        assert p is None and f"holds {n} bytes, the file holds more than {n}" in why
    p, _, _, _, _, why = reader(tmp_path / f"missing_7x5.{fmt}", fmt)
    assert p is None and "cannot open" in why
    good = tmp_path / f"ok_7x5.{fmt}"
    good.write_bytes(raw.tobytes())
    for no_format in (-1, 4):  # planar RGB has no raw-file form
        p, _, _, _, _, why = reader(good, no_format)
        assert p is None and "i420, yv12, i422 or i444" in why


REFUSAL = """
import ctypes as C, sys
sys.path.insert(0, {root!r})
import numpy as np
from yolo_quantization_amd import binding
net = binding.Net({cfg!r}, None, batch=1)
w, h = 9, 7
planes = [np.zeros((h, w), np.uint8), np.zeros({chroma!r}, np.uint8), np.zeros({chroma!r}, np.uint8)]
ptr = [(C.c_void_p * 1)(p.ctypes.data) for p in planes]
pitch = [(C.c_int * 1)(p.shape[1]) for p in planes]
{change}
net.H.network_frames_planar_input_gpu(net.h, ptr[0], ptr[1], ptr[2], (C.c_int * 1)(w), (C.c_int * 1)(h), pitch[0], pitch[1], pitch[2],
                                      {fmt}, {matrix}, 0)
print("returned")
"""

# what, format id, matrix id, chroma plane shape of a 9 x 7 frame, the change to a good call, the message
REFUSALS = [("null_plane", 0, 0, (4, 5), "ptr[2][0] = None", "null plane"),
            ("chroma_pitch_one_below_minimum_i420", 0, 0, (4, 5), "pitch[1][0] = 4", "need pitch >= the width of its plane"),
            ("chroma_pitch_one_below_minimum_i422", 2, 0, (7, 5), "pitch[2][0] = 4", "need pitch >= the width of its plane"),
            ("chroma_pitch_one_below_minimum_i444", 3, 0, (7, 9), "pitch[2][0] = 8", "need pitch >= the width of its plane"),
            ("luma_pitch_one_below_minimum", 0, 0, (4, 5), "pitch[0][0] = 8", "need pitch >= the width of its plane"),
            ("unknown_format", 6, 0, (4, 5), "", "unknown format"),
            ("negative_format", -1, 0, (4, 5), "", "unknown format"),
            ("unknown_matrix", 0, 4, (4, 5), "", "unknown matrix"),
            ("matrix_with_rgb", 4, 1, (7, 9), "", "matrix must be 0 with MI355_PLANAR_RGB / _BGR"),
            ("matrix_with_bgr", 5, 3, (7, 9), "", "matrix must be 0 with MI355_PLANAR_RGB / _BGR")]


@pytest.mark.parametrize("what,fmt,matrix,chroma,change,message", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_host_entry_refuses_before_it_touches_a_device(what, fmt, matrix, chroma, change, message):
    """error() of the host library: its message and exit(-1), with or without a device in the box"""
    code = REFUSAL.format(root=ROOT, cfg=os.path.join(ROOT, "cfg", "tiny_unit.cfg"), chroma=chroma, change=change, fmt=fmt, matrix=matrix)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 255 and "returned" not in r.stdout, (r.returncode, r.stderr[-500:])
    assert "network_frames_planar_input_gpu: " + message in r.stderr, r.stderr[-500:]
