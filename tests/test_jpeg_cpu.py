"""CPU checks of the JPEG input path: the host entropy decoder (yolo_quantization_amd/host/jpeg.c through binding.jpeg_info /
jpeg_coefficients) followed by the numpy restatement of the device half (jpeg_ref) reproduces, byte for byte, the pixels the compiled
reference loaded from every fixture (tests/golden/jpeg_expected.npz, written by tests/golden/make_golden_jpeg.py); where oracle/_ref is
built the reference itself is asked again (the pin); every refusal returns its own message; the headers are reported as written; the
C structs match their ctypes mirrors; and the decoder survives hostile bytes under AddressSanitizer + UBSan as a stand-alone program.
No kernel is launched here."""
import ctypes as C
import glob
import os
import struct
import subprocess

import numpy as np
import pytest

import jpeg_ref
import refdrv
from yolo_quantization_amd import binding

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
JPEG_DIR = os.path.join(ROOT, "tests", "golden", "jpeg")
REFUSED = ("progressive", "cmyk")
REAL_IMAGE = "/root/reference/test_image/000044.jpg"


@pytest.fixture(scope="module")
def expected():
    with np.load(os.path.join(ROOT, "tests", "golden", "jpeg_expected.npz")) as z:
        return {k: z[k] for k in z.files}


def fixture_names():
    return sorted(n for n in (os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(JPEG_DIR, "*.jpg"))) if n not in REFUSED)


def path_of(name):
    return os.path.join(JPEG_DIR, name + ".jpg")


def data_of(name):
    with open(path_of(name), "rb") as f:
        return f.read()


def test_every_fixture_has_an_expectation(expected):
    names = fixture_names()
    assert len(names) >= 40 and sorted(expected) == names
    for n in names:
        assert os.path.getsize(path_of(n)) < 16384 and max(expected[n].shape[:2]) <= 64


@pytest.mark.parametrize("name", fixture_names())
def test_host_decode_and_numpy_device_half_reproduce_the_reference(expected, name):
    d = binding.jpeg_coefficients(data_of(name))
    got = jpeg_ref.decode(d)  # raises OverflowError if a fixture left stb's 32-bit arithmetic
    want = expected[name]
    assert got.shape == want.shape == (d["h"], d["w"], 3)
    assert np.array_equal(got, want)


def test_fixtures_cover_the_cases():
    seen = set()
    for n in fixture_names():
        d = binding.jpeg_coefficients(path_of(n))
        wl = lambda c: -(-d["w"] // c["hs"])
        for c in d["components"]:
            seen.add((c["hs"], c["vs"]))
            if c["hs"] == 2:
                seen.add(("w_lores", c["vs"], min(wl(c), 3)))
        seen.add(d["mode"])
        seen.add(("scans", d["nscans"]))
        seen.add(("restart", d["restart_interval"]))
        seen.add(("sof", d["sof"]))
        if d["w"] == 1 or d["h"] == 1:
            seen.add(("thin", d["w"] == 1, d["h"] == 1))
    for want in [(1, 1), (2, 1), (1, 2), (2, 2), (4, 1), (4, 2), (3, 1), (1, 4), (1, 3), "ycbcr", "rgb", "grey", ("scans", 1), ("scans", 3), ("restart", 0),
                 ("restart", 1), ("restart", 2), ("sof", 0xC0), ("sof", 0xC1), ("w_lores", 1, 1), ("w_lores", 1, 2), ("w_lores", 2, 1),
                 ("w_lores", 2, 2), ("w_lores", 1, 3), ("w_lores", 2, 3), ("thin", True, True), ("thin", True, False), ("thin", False, True)]:
        assert want in seen, want


def test_a_quantiser_table_redefined_later_does_not_reach_back():
    d = binding.jpeg_coefficients(path_of("444_requant_29x19"))
    q = [c["quant"] for c in d["components"]]
    assert all(c["tq"] == 1 for c in d["components"][1:])
    assert np.array_equal(q[0], q[2]) and not np.array_equal(q[1], q[2])  # Cb was decoded before table 1 became table 0's copy


def test_sixteen_bit_quantiser_table():
    d = binding.jpeg_coefficients(path_of("444_dqt16_48x32"))
    assert d["components"][0]["quant"][2] == 300  # the sixth value of the zigzag sequence is natural position 2


@pytest.mark.skipif(not refdrv.available(), reason="oracle/_ref is not built")
def test_the_reference_reproduces_the_committed_expectations(expected):
    for n in fixture_names():
        f = refdrv.load_image_color(path_of(n))
        by = np.rint(f * 255).astype(np.uint8)
        assert np.array_equal(f, (by / 255.).astype(np.float32)), n
        assert np.array_equal(by.transpose(1, 2, 0), expected[n]), n


@pytest.mark.skipif(not (refdrv.available() and os.path.exists(REAL_IMAGE)), reason="needs oracle/_ref and the reference's test image")
def test_a_real_photograph_decodes_like_the_reference():
    f = refdrv.load_image_color(REAL_IMAGE)
    want = np.rint(f * 255).astype(np.uint8).transpose(1, 2, 0)
    assert np.array_equal(jpeg_ref.decode(binding.jpeg_coefficients(REAL_IMAGE)), want)


def test_jpeg_info_matches_the_headers():
    info = binding.jpeg_info(data_of("420_51x37"))
    assert (info["w"], info["h"], info["ncomp"], info["mode"], info["h_max"], info["v_max"], info["sof"]) == (51, 37, 3, "ycbcr", 2, 2, 0xC0)
    assert info["jfif"] and info["adobe_transform"] == -1 and info["restart_interval"] == 0
    y, cb, cr = info["components"]
    assert (y["h"], y["v"], y["hs"], y["vs"], y["w"], y["rows"], y["blocks_w"], y["blocks_h"]) == (2, 2, 1, 1, 51, 37, 8, 6)
    for c in (cb, cr):
        assert (c["h"], c["v"], c["hs"], c["vs"], c["w"], c["rows"], c["blocks_w"], c["blocks_h"]) == (1, 1, 2, 2, 26, 19, 4, 3)
    assert (y["id"], cb["id"], cr["id"]) == (1, 2, 3) and y["tq"] == 0 and cb["tq"] == cr["tq"] == 1
    assert binding.jpeg_info(path_of("422_restart2_51x37"))["restart_interval"] == 2
    grey = binding.jpeg_info(path_of("grey_51x37"))
    assert (grey["ncomp"], grey["mode"], grey["components"][0]["blocks_w"], grey["components"][0]["blocks_h"]) == (1, "grey", 7, 5)
    adobe = binding.jpeg_info(path_of("rgb_adobe0_48x32"))
    assert adobe["mode"] == "rgb" and adobe["adobe_transform"] == 0 and not adobe["jfif"]
    ids = binding.jpeg_info(path_of("rgb_ids_48x32"))
    assert ids["mode"] == "rgb" and [c["id"] for c in ids["components"]] == [ord(c) for c in "RGB"]
    # the info call and the full decode agree on everything both report
    full = binding.jpeg_coefficients(path_of("410_61x27"))
    head = binding.jpeg_info(path_of("410_61x27"))
    assert all(full[k] == head[k] for k in head if k != "components")
    assert [{k: c[k] for k in hc} for c, hc in zip(full["components"], head["components"])] == head["components"]


def _sof(data):
    pos = 2
    while data[pos + 1] not in (0xC0, 0xC1):
        pos += 2 + struct.unpack(">H", data[pos + 2:pos + 4])[0]
    return pos


def _patched(data, at, value):
    b = bytearray(data)
    b[at] = value
    return bytes(b)


def test_every_refusal_has_its_own_message():
    base = data_of("420_51x37")
    s = _sof(base)
    cases = {
        "progressive": (data_of("progressive"), "progressive"),
        "cmyk": (data_of("cmyk"), "4 components (CMYK / YCCK)"),
        "arithmetic": (_patched(base, s + 1, 0xC9), "arithmetic"),
        "lossless": (_patched(base, s + 1, 0xC3), "lossless / hierarchical"),
        "hierarchical": (_patched(base, s + 1, 0xC5), "lossless / hierarchical"),
        "twelve bit": (_patched(base, s + 4, 12), "only 8-bit"),
        "zero height": (base[:s + 5] + b"\x00\x00" + base[s + 7:], "no header height"),
        "zero width": (base[:s + 7] + b"\x00\x00" + base[s + 9:], "0 width"),
        "sampling 3 of 2": (_patched(_patched(base, s + 11, 0x31), s + 14, 0x21), "do not divide"),
        "bad H": (_patched(base, s + 11, 0x52), "bad H"),
        "bad V": (_patched(base, s + 11, 0x20), "bad V"),
        "bad TQ": (_patched(base, s + 12, 4), "bad TQ"),
        "bad component count": (_patched(base, s + 9, 2), "bad component count"),
        "bad SOF len": (_patched(base, s + 3, 10), "bad SOF len"),
        "not a jpeg": (b"P6\n1 1\n255\n\x00\x00\x00", "no SOI"),
        "png": (b"\x89PNG\r\n\x1a\n" + bytes(32), "no SOI"),
        "empty": (b"", "no SOI"),
        "soi alone": (b"\xff\xd8", "no SOF"),
        "truncated": (base[:len(base) // 2], "expected marker"),
        "unknown marker": (base[:2] + b"\xff\xc8\x00\x02" + base[2:], "unknown marker"),
        "bad DRI len": (base[:2] + b"\xff\xdd\x00\x05\x00\x00\x00" + base[2:], "bad DRI len"),
        "bad DQT type": (base[:2] + b"\xff\xdb\x00\x43\x20" + bytes(64) + base[2:], "bad DQT type"),
        "bad DQT table": (base[:2] + b"\xff\xdb\x00\x43\x04" + bytes(64) + base[2:], "bad DQT table"),
        "bad DHT header": (base[:2] + b"\xff\xc4\x00\x13\x24" + bytes(16) + base[2:], "bad DHT header"),
        "bad code lengths": (base[:2] + b"\xff\xc4\x00\x16\x00\x03" + bytes(15) + b"\x00\x01\x02" + base[2:], "bad code lengths"),
        "bad COM len": (base[:2] + b"\xff\xfe\x00\x01" + base[2:], "bad COM len"),
        "bad APP len": (base[:2] + b"\xff\xe1\x00\x00" + base[2:], "bad APP len"),
    }
    sos = base.index(b"\xff\xda")
    cases["bad SOS component count"] = (_patched(base, sos + 4, 5), "bad SOS component count")
    cases["bad SOS len"] = (_patched(base, sos + 3, 13), "bad SOS len")
    cases["bad DC huff"] = (_patched(base, sos + 6, 0x40), "bad DC huff")
    cases["bad AC huff"] = (_patched(base, sos + 6, 0x04), "bad AC huff")
    cases["bad SOS"] = (_patched(base, sos + 11, 1), "bad SOS")
    cases["undefined huffman table"] = (_patched(base, sos + 6, 0x33), "undefined huffman table")
    cases["SOS before SOF"] = (base[:2] + base[sos:], "SOS before SOF")
    for what, (data, message) in cases.items():
        for call in (binding.jpeg_coefficients, binding.jpeg_info):
            if call is binding.jpeg_info and what in ("truncated", "bad SOS component count", "bad SOS len", "bad DC huff", "bad AC huff",
                                                      "bad SOS", "undefined huffman table"):
                continue  # the headers end at the first SOS
            with pytest.raises(binding.JpegError, match=message.replace("(", r"\(").replace(")", r"\)")):
                call(data)
    messages = {m for _, m in cases.values()}
    assert len(messages) >= 30


def test_struct_mirrors_match_the_c_headers(tmp_path):
    src = ['#include <stddef.h>\n#include <stdio.h>\n#include "mi355_yolo_int8.h"\n#include "jpeg.h"\nint main(void) {\n']
    mirrors = [("mi355_jpeg_plane", binding.JpegPlane, 48), ("mi355_jpeg_component", binding.JpegComponent, 24), ("mi355_jpeg_image", binding.JpegImage, 96),
               ("dnq_jpeg_comp", binding.DnqJpegComp, None), ("dnq_jpeg", binding.DnqJpeg, None)]
    for name, py, _ in mirrors:
        src.append(f'    printf("%zu", sizeof({name}));\n')
        src += [f'    printf(" %zu", offsetof({name}, {f[0]}));\n' for f in py._fields_]
        src.append('    printf("\\n");\n')
    src.append('    printf("%d %d %d %d %d %d %d\\n", MI355_JPEG_YCBCR, MI355_JPEG_RGB, MI355_JPEG_GREY, DNQ_JPEG_YCBCR, DNQ_JPEG_RGB, DNQ_JPEG_GREY, MI355_ABI_VERSION);\n')
    src.append("    return 0;\n}\n")
    c = tmp_path / "layout.c"
    c.write_text("".join(src))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "yolo_quantization_amd", "host"), str(c), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    for (name, py, size), line in zip(mirrors, lines):
        vals = [int(v) for v in line.split()]
        assert vals[0] == C.sizeof(py), name
        assert size is None or vals[0] == size
        assert vals[1:] == [getattr(py, f[0]).offset for f in py._fields_], name
    assert [int(v) for v in lines[-1].split()] == [0, 1, 2, 0, 1, 2, 6]  # new structs and new calls do not bump the ABI
    assert binding.JPEG_MODES == ("ycbcr", "rgb", "grey")


def test_jpeg_ref_flags_an_overflow_of_the_32_bit_arithmetic():
    big = np.zeros(64, np.int16)
    big[[1, 3, 5, 7]] = 32767
    big[[8, 24, 40, 56]] = 32767
    big[[9, 27, 45, 63]] = 32767
    with pytest.raises(OverflowError):
        jpeg_ref.idct_blocks(big, np.ones(64, np.uint16))
    assert jpeg_ref.dequantise(np.array([300, -300, 1]), np.array([300, 300, 65535])).tolist() == [24464, -24464, -1]


def test_decoder_survives_hostile_input_under_sanitizers(tmp_path):
    """the stand-alone fuzz program (tests/jpeg_fuzz_main.c + host/jpeg.c) built with ASan + UBSan: every fixture as it is, every
    truncation of three of them, 4000 seeded single-byte corruptions; it must exit 0 without a report.  The sanitizer runtimes are
    linked into the program, so it does not depend on the order in which the loader finds libraries"""
    exe = tmp_path / "jpeg_fuzz"
    host = os.path.join(ROOT, "yolo_quantization_amd", "host")
    subprocess.run(["gcc", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all", "-I", host, os.path.join(ROOT, "tests", "jpeg_fuzz_main.c"),
                    os.path.join(host, "jpeg.c"), "-o", str(exe)], check=True)
    first = ["420_51x37", "422_restart2_51x37", "444_noninterleaved_29x19"]
    files = [path_of(n) for n in first + [n for n in fixture_names() if n not in first]]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe), "4000"] + files, capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-3000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.stdout.startswith("jpeg_fuzz:")
