"""CPU checks behind the 8-bit frame input path (mi355_frames_u8_letterbox_minmax / _quantize, network_frames_u8_input_gpu): the
byte -> float claim the kernels rest on, and the ctypes mirror of the new C-ABI struct.  No kernel is launched here."""
import ctypes as C
import os
import subprocess

import numpy as np

from yolo_quantization_amd import binding

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def test_byte_to_float_forms_agree_for_all_256_values():
    """(float)byte / 255.f (the kernels, the CLI's PPM reader) == (float)(byte / 255.) (load_image_color, ref: src/image.c:1386) ==
    (float)(byte * (1 / 255.)) for every byte: the frames path may start from bytes and still produce the float path's floats."""
    b = np.arange(256)
    f32_div = b.astype(np.float32) / np.float32(255)
    f64_div = (b.astype(np.float64) / np.float64(255)).astype(np.float32)
    f64_mul = (b.astype(np.float64) * (np.float64(1) / np.float64(255))).astype(np.float32)
    assert f32_div.dtype == np.float32
    assert np.array_equal(f32_div.view(np.uint32), f64_div.view(np.uint32))
    assert np.array_equal(f32_div.view(np.uint32), f64_mul.view(np.uint32))
    assert f32_div[0] == 0 and f32_div[255] == 1 and np.all(np.diff(f32_div) > 0)


def test_frame_struct_mirror_matches_the_c_header(tmp_path):
    """binding.FrameU8 has mi355_frame_u8's size and offsets (the method of test_ctypes_structs_match_the_c_header), and no hidden padding:
    the table is uploaded as raw bytes and read by the kernels."""
    names = [f[0] for f in binding.FrameU8._fields_]
    src = "#include <stddef.h>\n#include <stdio.h>\n#include \"mi355_yolo_int8.h\"\nint main(void) {\n"
    src += '    printf("%zu", sizeof(mi355_frame_u8));\n'
    for n in names:
        src += f'    printf(" %zu", offsetof(mi355_frame_u8, {n}));\n'
    src += '    printf(" %d %d %d\\n", MI355_FRAME_RGB, MI355_FRAME_BGR, MI355_ABI_VERSION);\n    return 0;\n}\n'
    c = tmp_path / "layout.c"
    c.write_text(src)
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    vals = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    nf = len(names)
    assert vals[0] == C.sizeof(binding.FrameU8) == 32
    assert vals[1:1 + nf] == [getattr(binding.FrameU8, n).offset for n in names]
    assert sum(C.sizeof(t) for _, t in binding.FrameU8._fields_) == C.sizeof(binding.FrameU8)  # explicit padding only
    assert vals[1 + nf:1 + nf + 2] == [binding.FRAME_ORDER["rgb"], binding.FRAME_ORDER["bgr"]]
    assert vals[-1] == binding.ABI_VERSION == 6  # a new struct and new calls do not bump the ABI


def test_new_entry_points_are_exported():
    for n in ("mi355_frames_u8_letterbox_minmax", "mi355_frames_u8_letterbox_quantize"):
        assert hasattr(binding.shim(), n), n
    assert hasattr(binding.host(), "network_frames_u8_input_gpu")
