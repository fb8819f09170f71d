"""CPU checks of the device entropy decode's host side: the scan lister (yolo_quantization_amd/host/jpeg_scan.c through
binding.jpeg_scan) reports what the host decoder reports and copies out the bytes the file holds; the emulation of mi355_jpeg_entropy
(jpeg_entropy_emulate_host: the kernel's four phases, the lanes run one after another through the routine the kernel's lanes run)
gives jpeg_decode_host's coefficients, bit for bit, on every fixture and on built streams; a stream whose bits do not tell the slot
inside the unit settles one lane a step and still decodes right; hostile bytes survive AddressSanitizer + UBSan as a stand-alone
program; the new structs match their ctypes mirrors.  No kernel is launched here."""
import ctypes as C
import glob
import os
import struct
import subprocess

import numpy as np
import pytest

import jpeg_streams
from yolo_quantization_amd import binding

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
JPEG_DIR = os.path.join(ROOT, "tests", "golden", "jpeg")
REFUSED = ("progressive", "cmyk")
SUBSEQ_BITS = (32, 64, 1024, 8192)


def fixture_names():
    return sorted(n for n in (os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(JPEG_DIR, "*.jpg"))) if n not in REFUSED)


def data_of(name):
    with open(os.path.join(JPEG_DIR, name + ".jpg"), "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def host_decoded():
    """jpeg_decode_host on every fixture, once"""
    return {n: binding.jpeg_coefficients(data_of(n)) for n in fixture_names()}


@pytest.fixture(scope="module")
def built():
    """the built streams and what jpeg_decode_host makes of them, once"""
    files = {}
    files.update(jpeg_streams.round_edge_streams())
    files.update(jpeg_streams.symbol_edge_streams())
    files.update(jpeg_streams.unit_grid_streams())
    files["restart_300"] = jpeg_streams.restart_stream()
    return {n: (d, binding.jpeg_coefficients(d)) for n, d in files.items()}


def scan_data(data):
    """per SOS of the file: the bytes between the scan header and the marker that ends the scan (restart markers are part of them)"""
    out, pos = [], 2
    while pos < len(data):
        assert data[pos] == 0xFF
        m = data[pos + 1]
        if m == 0xD9:
            break
        length = struct.unpack(">H", data[pos + 2:pos + 4])[0]
        pos += 2 + length
        if m == 0xDA:
            end = pos
            while not (data[end] == 0xFF and data[end + 1] != 0 and not 0xD0 <= data[end + 1] <= 0xD7):
                end += 1
            out.append(data[pos:end])
            pos = end
    return out


@pytest.mark.parametrize("name", fixture_names())
def test_scan_reports_what_the_decoder_reports_and_copies_the_files_bytes(host_decoded, name):
    data, want = data_of(name), host_decoded[name]
    got = binding.jpeg_scan(data)
    info = binding.jpeg_info(data)
    assert all(got[k] == want[k] for k in want if k != "components")
    assert all(got[k] == info[k] for k in info if k != "components")
    for g, w in zip(got["components"], want["components"]):
        assert all(g[k] == w[k] for k in w if k not in ("coef", "quant")) and np.array_equal(g["quant"], w["quant"])
    scans = scan_data(data)
    assert len(scans) == got["nscans"] == 1 + max(g["scan"] for g in got["segments"])
    for si, raw in enumerate(scans):
        segs = [g for g in got["segments"] if g["scan"] == si]
        units = segs[0]["units_x"] * segs[0]["units_y"]
        interval = got["restart_interval"] or units
        assert len(segs) == -(-units // interval)
        assert [g["first_unit"] for g in segs] == list(range(0, units, interval))
        assert [g["nunits"] for g in segs] == [min(interval, units - f) for f in range(0, units, interval)]
        again = b""
        for n, g in enumerate(segs):  # stuffed again and joined by the restart markers, the segments are the file's scan
            again += (bytes([0xFF, 0xD0 + (n - 1) % 8]) if n else b"") + g["data"].replace(b"\xff", b"\xff\x00")
        assert again == raw
        for g in segs:  # the geometry parse_scan walks: h x v blocks a unit, or 1 x 1 over the real size in a one-component scan
            comps = [got["components"][c] for c in g["comp"]]
            if g["ncomp"] == 1:
                assert (g["bh"], g["bv"]) == ([1], [1]) and (g["units_x"], g["units_y"]) == (-(-comps[0]["w"] // 8), -(-comps[0]["rows"] // 8))
            else:
                assert g["bh"] == [c["h"] for c in comps] and g["bv"] == [c["v"] for c in comps]
                assert (g["units_x"], g["units_y"]) == (comps[0]["blocks_w"] // comps[0]["h"], comps[0]["blocks_h"] // comps[0]["v"])


def test_scan_refuses_what_the_decoder_refuses_in_its_words():
    base = data_of("420_51x37")
    sos = base.index(b"\xff\xda")
    patch = lambda at, v: base[:at] + bytes([v]) + base[at + 1:]
    cases = [data_of("progressive"), data_of("cmyk"), b"", b"\xff\xd8", base[:len(base) // 2], patch(sos + 4, 5), patch(sos + 3, 13), patch(sos + 6, 0x40),
             patch(sos + 6, 0x04), patch(sos + 11, 1), patch(sos + 6, 0x33), base[:2] + base[sos:], base[:2] + b"\xff\xc8\x00\x02" + base[2:],
             base[:2] + b"\xff\xc4\x00\x16\x00\x03" + bytes(15) + b"\x00\x01\x02" + base[2:]]
    for data in cases:
        with pytest.raises(binding.JpegError) as want:
            binding.jpeg_coefficients(data)
        with pytest.raises(binding.JpegError) as got:
            binding.jpeg_scan(data)
        assert str(got.value) == str(want.value) and str(got.value)


def test_a_huffman_table_redefined_between_scans_does_not_reach_back():
    """three one-component scans; the tables of the second and third are redefined in front of them with other code lengths"""
    comps = [(1, 1, 1), (2, 1, 1), (3, 1, 1)]
    rng = np.random.default_rng(5)
    coef = jpeg_streams._random_planes(rng, 29, 19, comps)
    other_dc = {c: 4 for c in range(12)}
    other_ac = {s: 4 for s in jpeg_streams.AC_LENGTHS if s != 0x0F}
    scans = [{"comps": [0], "dc": [0], "ac": [0]}, {"comps": [1], "dc": [0], "ac": [0], "tables": {("dc", 0): other_dc}},
             {"comps": [2], "dc": [0], "ac": [0], "tables": {("ac", 0): other_ac}}]
    data, _ = jpeg_streams.build(29, 19, comps, coef, scans=scans)
    want = binding.jpeg_coefficients(data)
    got = binding.jpeg_scan(data)
    assert [g["dc"] + g["ac"] for g in got["segments"]] == [[0, 1], [2, 3], [4, 5]]
    assert bytes(got["huff"][0]) != bytes(got["huff"][2]) and bytes(got["huff"][1]) == bytes(got["huff"][3]) != bytes(got["huff"][5])
    (planes,), (status,) = binding.jpeg_entropy([data], subseq_bits=64, emulate=True)
    assert status == [0, 0, 0]
    for a, c, mine in zip(planes, want["components"], coef):
        assert np.array_equal(a, c["coef"]) and np.array_equal(a, mine)


@pytest.mark.parametrize("subseq_bits", SUBSEQ_BITS)
def test_emulation_gives_the_host_decoders_coefficients_on_every_fixture(host_decoded, subseq_bits):
    names = fixture_names()
    planes, status = binding.jpeg_entropy([data_of(n) for n in names], subseq_bits=subseq_bits, emulate=True)
    for n, per, st in zip(names, planes, status):
        assert st == [0] * len(st) and len(st) >= host_decoded[n]["nscans"], n
        for a, c in zip(per, host_decoded[n]["components"]):
            assert np.array_equal(a, c["coef"]), n


@pytest.mark.parametrize("subseq_bits", SUBSEQ_BITS)
def test_emulation_gives_the_host_decoders_coefficients_on_the_built_streams(built, subseq_bits):
    names = sorted(built)
    planes, status = binding.jpeg_entropy([built[n][0] for n in names], subseq_bits=subseq_bits, emulate=True)
    for n, per, st in zip(names, planes, status):
        assert st == [0] * len(st), n
        for a, c in zip(per, built[n][1]["components"]):
            assert np.array_equal(a, c["coef"]), n
    assert len(status[names.index("restart_300")]) == 300


def test_the_built_streams_are_what_they_claim(built):
    for n in jpeg_streams.ROUND_EDGES:  # exactly n subsequences of 32 bits
        (seg,) = binding.jpeg_scan(built[f"subsequences_{n}"][0])["segments"]
        assert -(-8 * len(seg["data"]) // 32) == n
    grid = binding.jpeg_scan(built["noninterleaved_17x9"][0])
    assert (grid["segments"][0]["units_x"], grid["components"][0]["blocks_w"]) == (3, 4)  # the real-size grid is narrower than the plane
    assert sum(b * v for b, v in zip(*[binding.jpeg_scan(built["420_37x21"][0])["segments"][0][k] for k in ("bh", "bv")])) == 6
    assert sum(b * v for b, v in zip(*[binding.jpeg_scan(built["410_70x40"][0])["segments"][0][k] for k in ("bh", "bv")])) == 18
    edge = built["prefix_8"][1]["components"][0]["coef"]
    assert np.abs(edge[0, :, 0].astype(int)).max() >= 32767 and np.abs(edge[0, :, 1].astype(int)).max() >= 16384  # category-15 values


def test_slow_settle_takes_a_step_a_lane_and_decodes_right():
    """the slot inside the unit cannot be read off the bits: an implementation that compares bit positions only stops early and
    hands every component its neighbour's DC differences"""
    data, coef = jpeg_streams.slow_settle()
    want = binding.jpeg_coefficients(data)
    (planes,), (status,) = binding.jpeg_entropy([data], subseq_bits=32, emulate=True)
    ((steps,),) = binding.jpeg_entropy_steps([data], subseq_bits=32)
    assert steps >= 200
    assert status == [0]
    for a, c, mine in zip(planes, want["components"], coef):
        assert np.array_equal(a, c["coef"]) and np.array_equal(a, mine)
    assert sum(a.shape[0] * a.shape[1] for a in planes) >= 1024


def test_damaged_streams_set_their_status_word():
    reasons = {1: "bad huffman code", 2: "bad DC category", 3: "coefficient index past the end of the block"}
    for name, (data, code) in jpeg_streams.damaged_streams().items():
        with pytest.raises(binding.JpegError, match=reasons[code]):
            binding.jpeg_coefficients(data)
        for bits in (32, 1024):
            (planes,), (status,) = binding.jpeg_entropy([data], subseq_bits=bits, emulate=True)
            assert status == [code], name
            assert planes[0][0, :2, 0].tolist() == [1, 0] and planes[0][0, :2, 1].tolist() == [1, 1]  # the blocks in front of the damage
    assert binding.JPEG_ENTROPY_ERRORS == reasons


def test_emulation_refuses_what_the_kernel_refuses():
    data = data_of("grey_8x8")
    for bits in (0, 16, 48, 8224):
        with pytest.raises(binding.MI355Error):
            binding.jpeg_entropy([data], subseq_bits=bits, emulate=True)
    scan = binding.jpeg_scan(data)
    scan["segments"][0]["nunits"] = 2  # a grid of one unit
    with pytest.raises(binding.MI355Error):
        binding.jpeg_entropy([scan], subseq_bits=32, emulate=True)


def test_struct_mirrors_match_the_c_headers(tmp_path):
    src = ['#include <stddef.h>\n#include <stdio.h>\n#include "mi355_yolo_int8.h"\n#include "jpeg_scan.h"\nint main(void) {\n']
    mirrors = [("mi355_jpeg_huff", binding.JpegHuff, 976), ("mi355_jpeg_segment", binding.JpegSegment, 144), ("dnq_jpeg_scan_seg", binding.DnqJpegScanSeg, None),
               ("dnq_jpeg_scan_list", binding.DnqJpegScanList, None)]
    for name, py, _ in mirrors:
        src.append(f'    printf("%zu", sizeof({name}));\n')
        src += [f'    printf(" %zu", offsetof({name}, {f[0]}));\n' for f in py._fields_]
        src.append('    printf("\\n");\n')
    src.append('    printf("%d %d %d %d\\n", MI355_JPEG_EHUFF, MI355_JPEG_EDC, MI355_JPEG_EINDEX, MI355_ABI_VERSION);\n')
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
    assert [int(v) for v in lines[-1].split()] == [1, 2, 3, 6]  # new structs and a new call do not bump the ABI


def test_scan_and_emulation_survive_hostile_input_under_sanitizers(tmp_path):
    """the stand-alone program (tests/jpeg_entropy_fuzz_main.c + jpeg_scan.c + jpeg.c + jpeg_entropy_emulate.c) built with ASan + UBSan,
    the runtimes linked in: every fixture as it is (compared with the host decoder), every truncation of three of them, 4000 seeded
    single-byte corruptions, at 32 and 1024 bits a subsequence; it must exit 0 without a report"""
    exe = tmp_path / "jpeg_entropy_fuzz"
    host = os.path.join(ROOT, "yolo_quantization_amd", "host")
    subprocess.run(["gcc", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all", "-I", host,
                    os.path.join(ROOT, "tests", "jpeg_entropy_fuzz_main.c"), os.path.join(host, "jpeg_scan.c"), os.path.join(host, "jpeg.c"),
                    os.path.join(host, "jpeg_entropy_emulate.c"), "-o", str(exe)], check=True)
    first = ["420_51x37", "422_restart2_51x37", "444_noninterleaved_29x19"]
    files = [os.path.join(JPEG_DIR, n + ".jpg") for n in first + [n for n in fixture_names() if n not in first]]
    extra = []
    for name, (data, _) in jpeg_streams.damaged_streams().items():  # the damaged streams the device tests run
        p = tmp_path / (name + ".jpg")
        p.write_bytes(data)
        extra.append(str(p))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe), "4000"] + files, capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-3000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.stdout.startswith("jpeg_entropy_fuzz:")
    r = subprocess.run([str(exe), "--damaged"] + extra, capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-3000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert "3 scanned" in r.stdout and "6 runs with a status word set" in r.stdout
