"""CPU checks behind the NV12 / NV21 frame input path (mi355_frames_yuv_letterbox_minmax / _quantize, network_frames_nv12_input_gpu):
the ctypes mirror of the new C-ABI struct, the soundness of the integer conversion formulas over all 2^24 (Y, U, V) triples, and the
CLI's raw-file reader.  No kernel is launched here."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from frames_util import COEF, ROOT, yuv_to_rgb
from yolo_quantization_amd import binding

# the standards themselves: (Kr, Kb, limited range)
REAL = {0: (0.299, 0.114, True), 1: (0.299, 0.114, False), 2: (0.2126, 0.0722, True), 3: (0.2126, 0.0722, False)}


def test_yuv_struct_mirror_matches_the_c_header(tmp_path):
    names = [f[0] for f in binding.FrameYUV._fields_]
    src = "#include <stddef.h>\n#include <stdio.h>\n#include \"mi355_yolo_int8.h\"\nint main(void) {\n"
    src += '    printf("%zu", sizeof(mi355_frame_yuv));\n'
    for n in names:
        src += f'    printf(" %zu", offsetof(mi355_frame_yuv, {n}));\n'
    src += ('    printf(" %d %d %d %d %d %d %d %zu\\n", MI355_YUV_NV12, MI355_YUV_NV21, MI355_YUV_BT601, MI355_YUV_BT601_FULL, MI355_YUV_BT709,'
            ' MI355_YUV_BT709_FULL, MI355_ABI_VERSION, sizeof(mi355_frame_u8));\n    return 0;\n}\n')
    c = tmp_path / "layout.c"
    c.write_text(src)
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    vals = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    nf = len(names)
    assert names == ["y", "uv", "w", "h", "pitch_y", "pitch_uv", "layout", "matrix", "reserved"]
    assert vals[0] == C.sizeof(binding.FrameYUV) == 48
    assert vals[1:1 + nf] == [getattr(binding.FrameYUV, n).offset for n in names]
    assert sum(C.sizeof(t) for _, t in binding.FrameYUV._fields_) == C.sizeof(binding.FrameYUV)  # explicit padding only
    assert vals[1 + nf:1 + nf + 2] == [binding.YUV_LAYOUT["nv12"], binding.YUV_LAYOUT["nv21"]] == [0, 1]
    assert vals[3 + nf:7 + nf] == [binding.YUV_MATRIX[k] for k in ("bt601", "bt601f", "bt709", "bt709f")] == [0, 1, 2, 3]
    assert vals[7 + nf] == binding.ABI_VERSION == 6  # a new struct and new calls do not bump the ABI
    assert vals[8 + nf] == C.sizeof(binding.FrameU8) == 32  # the u8 struct is as it was


def test_new_entry_points_are_exported():
    for n in ("mi355_frames_yuv_letterbox_minmax", "mi355_frames_yuv_letterbox_quantize"):
        assert hasattr(binding.shim(), n), n
    assert hasattr(binding.host(), "network_frames_nv12_input_gpu")


@pytest.mark.parametrize("matrix", [0, 1, 2, 3], ids=["bt601", "bt601_full", "bt709", "bt709_full"])
def test_integer_formulas_agree_with_the_real_valued_standard(matrix):
    """all 2^24 triples: the 16.16 integer conversion against clamp(rint(real formula)) in float64 on the un-rounded coefficients.
    Never more than 1 apart in a channel, and apart at all in at most 0.1 % of the triples (rounding of the coefficients and the
    floor(x + .5) against round-half-even)."""
    kr, kb, limited = REAL[matrix]
    kg = 1.0 - kr - kb
    ys, cs, yoff = (255.0 / 219.0, 255.0 / 224.0, 16.0) if limited else (1.0, 1.0, 0.0)
    real = (ys, 2 * (1 - kr) * cs, 2 * (1 - kb) * kb / kg * cs, 2 * (1 - kr) * kr / kg * cs, 2 * (1 - kb) * cs)
    assert COEF[matrix][0] == yoff and [int(round(x * 65536)) for x in real] == list(COEF[matrix][1:])  # the table itself
    u, v = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    u, v = u.ravel(), v.ravel()
    cu, cv = u.astype(np.float64) - 128, v.astype(np.float64) - 128
    chroma = np.stack([real[1] * cv, -real[2] * cu - real[3] * cv, real[4] * cu], axis=-1)  # [65536][3]
    worst, differ = 0, np.zeros(65536, np.int64)
    for y in range(256):
        got = yuv_to_rgb(np.full(65536, y), u, v, matrix).astype(np.int16)
        want = np.clip(np.rint(real[0] * (y - yoff) + chroma), 0, 255).astype(np.int16)
        d = np.abs(got - want)
        worst = max(worst, int(d.max()))
        differ += d.any(axis=-1)
    frac = differ.sum() / 2.0 ** 24
    print(f"matrix {matrix}: worst difference {worst}, triples that differ {100 * frac:.4f} %")
    assert worst <= 1
    assert frac <= 0.001


READER_MAIN = r"""
#include <stdio.h>
#include <stdlib.h>
#include "raw_frame_file.h"
int main(int argc, char **argv)
{
    int w = -1, h = -1;
    size_t bytes[2] = {0, 0};
    char why[1024] = "";
    uint8_t *raw = load_raw_frame_file(argv[1], RAW_FRAME_NV12, &w, &h, bytes, why, sizeof(why));
    if (!raw) { fprintf(stderr, "%s", why); return 1; }
    printf("%d %d\n", w, h);
    fwrite(raw, 1, (size_t)w * h + (size_t)((h + 1) / 2) * 2 * ((w + 1) / 2), stdout);
    free(raw);
    return 0;
}
"""


@pytest.fixture(scope="module")
def reader(tmp_path_factory):
    """the CLI's raw-file reader (host/raw_frame_file.c, linked into ./darknet only) behind a main of the test's: no device, no library"""
    d = tmp_path_factory.mktemp("nv12_reader")
    host = os.path.join(ROOT, "yolo_quantization_amd", "host")
    (d / "main.c").write_text(READER_MAIN)
    exe = d / "reader"
    subprocess.run(["gcc", "-O1", "-Wall", "-I", host, str(d / "main.c"), os.path.join(host, "raw_frame_file.c"), "-o", str(exe)], check=True)

    def load(path):
        r = subprocess.run([str(exe), str(path)], capture_output=True)
        if r.returncode:
            assert r.returncode == 1 and not r.stdout
            return None, -1, -1, r.stderr.decode()
        head, _, body = r.stdout.partition(b"\n")
        w, h = (int(v) for v in head.split())
        return body, w, h, r.stderr.decode()
    return load


def test_cli_raw_file_reader_extracts_the_size_and_refuses_bad_names_and_lengths(tmp_path, reader):
    rng = np.random.default_rng(1)
    w, h = 7, 5  # odd: 35 luma bytes, 3 rows of 4 pairs
    n = w * h + ((h + 1) // 2) * 2 * ((w + 1) // 2)
    assert n == 35 + 24
    raw = rng.integers(0, 256, n, dtype=np.uint8)
    good = tmp_path / "clip_a_7x5.nv12"
    good.write_bytes(raw.tobytes())
    p, gw, gh, why = reader(good)
    assert p is not None and (gw, gh) == (w, h) and why == ""
    assert np.array_equal(np.frombuffer(p, np.uint8), raw)
    # no size, half a size, another suffix, a zero side, no underscore; blanks and signs are no digits; sides beyond 32768 and digit
    # strings that would overflow an int are refused, not wrapped
    for name in ("clip.nv12", "clip_7x.nv12", "clip_7x5.yuv", "clip_7x5.nv12.bak", "clip_0x5.nv12", "7x5.nv12", "clip_ 7x5.nv12",
                 "clip_7x+5.nv12", "clip_-7x5.nv12", "clip_7x5 .nv12", "clip_32769x5.nv12", "clip_7x4294967301.nv12",
                 "clip_" + "9" * 40 + "x5.nv12"):
        bad = tmp_path / name
        bad.write_bytes(raw.tobytes())
        p, _, _, why = reader(bad)
        assert p is None and "_<W>x<H>.nv12" in why and name in why, name
    for delta in (-1, 1):
        bad = tmp_path / f"len{delta}_7x5.nv12"
        bad.write_bytes(np.resize(raw, n + delta).tobytes())
        p, _, _, why = reader(bad)
        assert p is None and f"holds {n} bytes" in why and "_<W>x<H>" not in why, why
    p, _, _, why = reader(tmp_path / "missing_7x5.nv12")
    assert p is None and "cannot open" in why
