"""The inflate on the device without a device: the host half (png_scan_host) against the files, and the kernel's text run on the CPU
(png_inflate_emulate_host: host/png_inflate_core.h in the kernel's rounds) against the host decoder -- png_decode_host on all fixtures
and on the refusal files, png_inflate_host and zlib.decompress on real zlib streams and on the built streams of png_inflate_streams --
and a sanitizer-built stand-alone program that runs scan + emulation over hostile input."""
import ctypes as C
import glob
import os
import subprocess
import zlib

import pytest

import png_inflate_streams as pis
import png_streams as ps
from yolo_quantization_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PNG_DIR = os.path.join(ROOT, "tests", "golden", "png")
HEADER_MESSAGES = {"bad_zlib_header": "bad zlib header", "preset_dict": "no preset dict"}


def fixture_names():
    return sorted(n for n in (os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(PNG_DIR, "*.png")))
                  if not n.startswith("refuse_"))


def data_of(name):
    with open(os.path.join(PNG_DIR, name + ".png"), "rb") as f:
        return f.read()


# ------------------------------------------------------------------------------------------------------------------ the contract
def test_the_new_symbols_are_exported():
    assert hasattr(binding.shim(), "mi355_png_inflate")
    for name in ("png_scan_host", "png_scan_free", "png_inflate_emulate_host", "png_inflate_reason", "set_png_inflate_on_device"):
        assert hasattr(binding.host(), name), name
    for code, words in binding.PNG_INFLATE_ERRORS.items():
        assert binding.host().png_inflate_reason(code).decode() == words
    assert callable(binding.Net.set_png_inflate_on_device) and callable(binding.png_inflate_device)


def test_struct_mirrors_match_the_c_headers(tmp_path):
    src = ['#include <stddef.h>\n#include <stdio.h>\n#include "mi355_yolo_int8.h"\n#include "png_scan.h"\nint main(void) {\n']
    mirrors = [("mi355_png_stream", binding.PngStream, 88), ("dnq_png_scan", binding.DnqPngScan, None)]
    for name, py, _ in mirrors:
        src.append(f'    printf("%zu", sizeof({name}));\n')
        src += [f'    printf(" %zu", offsetof({name}, {f[0]}));\n' for f in py._fields_]
        src.append('    printf("\\n");\n')
    codes = ["EBLOCK", "ECORRUPT", "ELENGTHS", "EHUFF", "EDIST", "EPREMATURE", "EPAST", "EPIXELS", "EFILTER"]
    src.append('    printf("%d' + " %d" * len(codes) + '\\n", MI355_ABI_VERSION, ' + ", ".join("MI355_PNG_" + c for c in codes) + ");\n")
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
    assert [int(v) for v in lines[-1].split()] == [6] + sorted(binding.PNG_INFLATE_ERRORS)  # a new struct and a new call: the ABI stays


# ------------------------------------------------------------------------------------------------------------------ the scan
def test_scan_returns_the_idat_payloads_behind_the_zlib_header():
    names = fixture_names()
    assert len(names) >= 87
    counts = {}
    for n in names:
        data = data_of(n)
        sc, info = binding.png_scan(data), binding.png_info(data)
        assert sc["z"] == ps.idat_of(data)[2:], n
        for k, v in info.items():
            assert (sc[k] == v).all() if k == "palette" else sc[k] == v, (n, k)
        counts[n] = [k for k, _ in ps.chunks_of(data)].count(b"IDAT")
    assert counts["rgb8_idat_1byte_17x9"] > 50  # the header's two bytes come from two chunks
    kinds = [k for k, _ in ps.chunks_of(data_of("rgb8_ancillary_51x37"))]
    assert b"tIME" in kinds[kinds.index(b"IDAT"):kinds.index(b"IEND")] and counts["rgb8_ancillary_51x37"] > 1


def test_scan_refuses_what_png_info_refuses_in_the_same_words():
    files = ps.refusal_files()
    seen = set()
    for name, (data, message) in files.items():
        try:
            binding.png_info(data)
            info_err = None
        except binding.PngError as e:
            info_err = str(e)
        if info_err is not None:
            with pytest.raises(binding.PngError) as e:
                binding.png_scan(data)
            assert str(e.value) == info_err and message in info_err, name
        elif name in HEADER_MESSAGES:
            with pytest.raises(binding.PngError) as e:
                binding.png_scan(data)
            assert str(e.value) == HEADER_MESSAGES[name] == message
            seen.add(name)
        else:
            binding.png_scan(data)  # what only the inflate finds
    assert seen == set(HEADER_MESSAGES)
    good = data_of("rgb8_plain_51x37")
    at = good.index(b"IDAT") + 4
    with pytest.raises(binding.PngError, match="bad compression"):
        binding.png_scan(good[:at] + b"\x09\x15" + good[at + 2:])  # CM 9, FCHECK right
    with pytest.raises(binding.PngError, match="bad compression"):
        binding.png_scanlines(good[:at] + b"\x09\x15" + good[at + 2:])
    one = ps.SIG + ps.ihdr(3, 2, 8, 2) + ps.chunk(b"IDAT", b"\x78") + ps.chunk(b"IEND")  # one byte of IDAT: no header
    for fn in (binding.png_scan, binding.png_scanlines):
        with pytest.raises(binding.PngError, match="bad zlib header"):
            fn(one)
    for cut in (0, 7, 8, 20, 33, 60, len(good) - 13, len(good) - 12):
        with pytest.raises(binding.PngError) as e:
            binding.png_scan(good[:cut])
        with pytest.raises(binding.PngError) as h:
            binding.png_info(good[:cut])
        assert str(e.value) == str(h.value)


# ------------------------------------------------------------------------------------------------------------------ the emulation
def test_emulation_gives_the_host_decoders_bytes_on_every_fixture():
    names = fixture_names()
    scans = [binding.png_scan(data_of(n)) for n in names]
    args = [binding.png_stream_of(sc) for sc in scans]
    outs, status = binding.png_inflate_emulate([a[0] for a in args], [a[1] for a in args], [a[2] for a in args])
    assert status == [0] * len(names)
    for n, out in zip(names, outs):
        data = data_of(n)
        assert out == binding.png_scanlines(data)["filtered"].tobytes(), n
        assert out == zlib.decompress(ps.idat_of(data))[:len(out)], n


def test_emulation_gives_the_host_decoders_verdict_and_reason_on_the_refusal_files():
    reached = {}
    for name, (data, message) in ps.refusal_files().items():
        try:
            sc = binding.png_scan(data)
        except binding.PngError:
            continue
        with pytest.raises(binding.PngError) as e:
            binding.png_scanlines(data)
        z, cap, passes = binding.png_stream_of(sc)
        _, status = binding.png_inflate_emulate([z], [cap], [passes])
        assert status[0] and binding.PNG_INFLATE_ERRORS[status[0]] == str(e.value) and message in str(e.value), name
        reached[name] = status[0]
    assert set(reached) == {"bad_block_type", "bad_codelengths", "bad_dist", "not_enough_pixels", "invalid_filter"}
    assert sorted(reached.values()) == [1, 3, 5, 8, 9]


def test_emulation_on_real_zlib_streams():
    cases = pis.zlib_cases()
    assert len(cases) == 12
    outs, status = binding.png_inflate_emulate([c.z for c in cases], [c.cap for c in cases])
    pis.check(cases, outs, status)
    for c, out in zip(cases, outs):
        assert out == zlib.decompressobj(-15).decompress(c.z)[:c.cap], c.name
    assert any((c.z[0] >> 1) & 3 == 2 for c in cases) and any((c.z[0] >> 1) & 3 == 1 for c in cases)


def test_emulation_on_hand_chosen_repeat_codes():
    cases = pis.repeat_code_cases()
    assert [c.reason for c in cases] == [None, None, "bad codelengths", "bad codelengths", "bad codelengths"]
    outs, status = binding.png_inflate_emulate([c.z for c in cases], [c.cap for c in cases])
    pis.check(cases, outs, status)
    for c, out in zip(cases[:2], outs):
        assert out == zlib.decompressobj(-15).decompress(c.z), c.name  # zlib reads the writer's headers as we do


@pytest.mark.parametrize("group", ["token_round_cases", "match_cases", "ring_cases", "cap_cases", "block_cases", "error_cases"])
def test_emulation_on_built_streams(group):
    cases = getattr(pis, group)()
    outs, status = binding.png_inflate_emulate([c.z for c in cases], [c.cap for c in cases], [c.passes for c in cases])
    pis.check(cases, outs, status)
    for c, out in zip(cases, outs):  # the built streams that zlib takes too give zlib's bytes
        if c.reason is None and not c.name.startswith(("garbage", "truncated", "one_code", "cap_", "flush_edge", "ring_")):
            assert out == zlib.decompressobj(-15).decompress(c.z)[:c.cap], c.name


def test_error_cases_cover_every_status():
    by_reason = {c.reason for c in pis.error_cases() + pis.cap_cases() + pis.block_cases()}
    assert by_reason == set(binding.PNG_INFLATE_ERRORS.values()) | {None}


def test_emulation_refuses_what_the_call_refuses():
    good = pis.good_case()
    for kw, words in ((dict(caps=[0]), "cap"), (dict(passes=[[(1, good.cap)]]), "add up"), (dict(passes=[[(1, 1)] * 8]), "npasses"),
                      (dict(passes=[[]]), "npasses")):
        a = dict(streams=[good.z], caps=[good.cap], passes=[None])
        a.update(kw)
        with pytest.raises(binding.MI355Error, match="png_inflate: .*" + words):
            binding.png_inflate_emulate(a["streams"], a["caps"], a["passes"])
    table, status = (binding.PngStream * 1)(), (C.c_int * 1)()
    t = table[0]
    t.z, t.out, t.nbytes, t.npasses, t.rows[0] = 4096, 8192, 16, 1, 1  # never followed: the table is refused
    for cap, nbytes, words in ((1 << 31, 16, "cap"), (64, (1 << 28) + 1, "2\\^28")):
        t.cap, t.row_bytes[0], t.nbytes = cap, cap - 1, nbytes
        assert binding.host().png_inflate_emulate_host(table, 1, status) == -1
        assert words.replace("\\", "") in binding.host().png_inflate_emulate_why().decode()
    assert binding.host().png_inflate_emulate_host(table, 0, status) == -1 and binding.host().png_inflate_emulate_host(table, 65536, status) == -1


# ------------------------------------------------------------------------------------------------------------- hostile input
def test_scan_and_emulation_survive_hostile_input_under_sanitizers(tmp_path):
    """the stand-alone program (tests/png_inflate_fuzz_main.c + host/png.c, png_scan.c, png_inflate_emulate.c) built with ASan +
    UBSan: every fixture as it is, every truncation of three of them, 4000 seeded single-byte corruptions; the stream lies in a heap
    block of exactly the bytes the kernel may read and the output between guard bytes; the verdict must be the host decoder's.  It
    must exit 0 without a report.  The sanitizer runtimes are linked into the program."""
    exe = tmp_path / "png_inflate_fuzz"
    host = os.path.join(ROOT, "yolo_quantization_amd", "host")
    subprocess.run(["gcc", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all",
                    "-I", host, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "png_inflate_fuzz_main.c"),
                    os.path.join(host, "png.c"), os.path.join(host, "png_scan.c"), os.path.join(host, "png_inflate_emulate.c"), "-o", str(exe)],
                   check=True)
    first = ["rgb8_plain_51x37", "pal4_adam7_51x37", "rgb8_idat_uneven_51x37"]
    files = [os.path.join(PNG_DIR, n + ".png") for n in first + [n for n in fixture_names() if n not in first]]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe), "4000"] + files, capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-3000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.stdout.startswith("png_inflate_fuzz:")
