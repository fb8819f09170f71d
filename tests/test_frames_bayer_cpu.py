"""CPU checks behind the raw sensor frame input path (mi355_frames_bayer_*, network_frames_bayer_input_gpu): the struct layout and
constants of the C header against their ctypes mirrors, the exported symbols, the numpy restatement of D(frame)
(frames_bayer_util.demosaic) against a literal per-pixel loop of the definition and against properties that pin every parity and
reflection, the sample reductions against a bit-level unpacker, the refusals of the C-ABI calls, the host entry point and the Python
method, which all come before a device is touched, and the CLI's raw-file reader.  No kernel is launched here."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from frames_bayer_util import BAYER, PATTERNS, SAMPLES, TILE, colours, demosaic, mosaic, pack, raw8, row_bytes
from frames_util import ROOT
from yolo_quantization_amd import binding

FIELDS = ["data", "tone", "w", "h", "pitch", "pattern", "sample", "shift", "reserved"]


def _c_values(tmp_path, body):
    src = '#include <stddef.h>\n#include <stdio.h>\n#include "mi355_yolo_int8.h"\nint main(void) {\n' + body + "    return 0;\n}\n"
    c = tmp_path / "layout.c"
    c.write_text(src)
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    return [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]


def test_struct_mirror_matches_the_c_header(tmp_path):
    py = binding.FrameBayer
    names = [f[0] for f in py._fields_]
    assert names == FIELDS
    body = '    printf("%zu", sizeof(mi355_frame_bayer));\n' + "".join(f'    printf(" %zu", offsetof(mi355_frame_bayer, {n}));\n' for n in names)
    body += '    printf(" %d\\n", MI355_ABI_VERSION);\n'
    vals = _c_values(tmp_path, body)
    assert vals[0] == C.sizeof(py) == 48
    assert vals[1:1 + len(names)] == [getattr(py, n).offset for n in names] == [0, 8, 16, 20, 24, 28, 32, 36, 40]
    assert sum(C.sizeof(t) for _, t in py._fields_) == C.sizeof(py)  # no hidden padding
    assert vals[-1] == binding.ABI_VERSION == 6  # a new struct and new calls do not bump the ABI


def test_constants_match_the_c_header(tmp_path):
    body = ('    printf("%d %d %d %d %d %d %d %d %d %d\\n", MI355_BAYER_RGGB, MI355_BAYER_BGGR, MI355_BAYER_GRBG, MI355_BAYER_GBRG,'
            " MI355_BAYER_MONO, MI355_RAW_U8, MI355_RAW_U16, MI355_RAW_MIPI10, MI355_RAW_MIPI12, MI355_ABI_VERSION);\n")
    vals = _c_values(tmp_path, body)
    assert vals[:5] == [binding.BAYER_PATTERN[k] for k in PATTERNS] == [0, 1, 2, 3, 4]
    assert vals[5:9] == [binding.RAW_SAMPLE[k] for k in SAMPLES] == [0, 1, 2, 3]
    assert vals[9] == 6
    assert list(binding.BAYER_PATTERN) == PATTERNS and list(binding.RAW_SAMPLE) == SAMPLES


def test_new_entry_points_are_exported():
    for n in ("mi355_frames_bayer_letterbox_minmax", "mi355_frames_bayer_letterbox_quantize"):
        assert hasattr(binding.shim(), n), n
    assert hasattr(binding.host(), "network_frames_bayer_input_gpu")
    assert hasattr(binding.Net, "prepare_from_frames_bayer")


# ------------------------------------------------------------------------------------- the definition, written out per pixel
def _loop_demosaic(raw, pattern, tone):
    """section by section what mi355_yolo_int8.h says at mi355_frame_bayer, on 8-bit samples"""
    h, w = raw.shape
    names = {"rggb": "RGGB", "bggr": "BGGR", "grbg": "GRBG", "gbrg": "GBRG"}

    def c(x, y):
        return "RGB".index(names[pattern][2 * (y & 1) + (x & 1)])

    def s(x, y):
        x = -x if x < 0 else (2 * (w - 1) - x if x >= w else x)  # -1 -> 1, w -> w - 2
        y = -y if y < 0 else (2 * (h - 1) - y if y >= h else y)
        t = 0 if pattern == "mono" else c(x, y)
        return int(raw[y, x]) if tone is None else int(tone[t][raw[y, x]])
    out = np.zeros((h, w, 3), np.uint8)
    for y in range(h):
        for x in range(w):
            if pattern == "mono":
                out[y, x] = s(x, y)
            elif c(x, y) != 1:
                a = c(x, y)
                out[y, x, a] = s(x, y)
                out[y, x, 1] = (s(x - 1, y) + s(x + 1, y) + s(x, y - 1) + s(x, y + 1) + 2) >> 2
                out[y, x, 2 - a] = (s(x - 1, y - 1) + s(x + 1, y - 1) + s(x - 1, y + 1) + s(x + 1, y + 1) + 2) >> 2
            else:
                hc = c(x ^ 1, y)
                out[y, x, 1] = s(x, y)
                out[y, x, hc] = (s(x - 1, y) + s(x + 1, y) + 1) >> 1
                out[y, x, 2 - hc] = (s(x, y - 1) + s(x, y + 1) + 1) >> 1
    return out


SIZES = [(2, 2), (3, 2), (2, 3), (5, 4), (7, 7)]


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("toned", [False, True])
def test_demosaic_against_a_per_pixel_loop(pattern, w, h, toned):
    rng = np.random.default_rng(100 * w + h)
    raw = rng.integers(0, 256, (h, w), dtype=np.uint8)
    tone = rng.integers(0, 256, (3, 256), dtype=np.uint8) if toned else None
    got = demosaic(raw, pattern, tone=tone)
    assert got.dtype == np.uint8 and got.shape == (h, w, 3)
    assert np.array_equal(got, _loop_demosaic(raw, pattern, tone))


def test_tiles_are_the_patterns_written_out():
    assert {p: ["RGB"[k] for row in TILE[p] for k in row] for p in BAYER} == \
           {"rggb": list("RGGB"), "bggr": list("BGGR"), "grbg": list("GRBG"), "gbrg": list("GBRG")}


@pytest.mark.parametrize("pattern", BAYER)
@pytest.mark.parametrize("w,h", [(2, 2), (3, 5), (6, 4)])
@pytest.mark.parametrize("planes", [(0, 255, 0), (255, 0, 255), (17, 130, 201), (255, 255, 0)])
def test_constant_planes_come_back_exactly(pattern, w, h, planes):
    """every average is over samples of one colour: a parity or reflection mistake mixes planes and shows"""
    rgb = np.empty((h, w, 3), np.uint8)
    rgb[:] = planes
    assert np.array_equal(demosaic(mosaic(rgb, pattern), pattern), rgb)


@pytest.mark.parametrize("pattern", BAYER)
def test_a_sites_own_colour_is_its_sample(pattern):
    rng = np.random.default_rng(5)
    raw = rng.integers(0, 256, (7, 6), dtype=np.uint8)
    tone = rng.integers(0, 256, (3, 256), dtype=np.uint8)
    c = colours(pattern, 7, 6)
    for t in (None, tone):
        s = raw if t is None else t[c, raw]
        assert np.array_equal(np.take_along_axis(demosaic(raw, pattern, tone=t), c[:, :, None], axis=2)[:, :, 0], s)


def test_mono_replicates_and_uses_table_0():
    raw = np.random.default_rng(6).integers(0, 256, (5, 1), dtype=np.uint8)
    assert np.array_equal(demosaic(raw, "mono"), np.repeat(raw[:, :, None], 3, axis=2))
    one = np.array([[9]], np.uint8)
    assert demosaic(one, "mono").tolist() == [[[9, 9, 9]]]
    tone = np.random.default_rng(7).integers(0, 256, (3, 256), dtype=np.uint8)
    assert np.array_equal(demosaic(raw, "mono", tone=tone), np.repeat(tone[0][raw][:, :, None], 3, axis=2))


# ------------------------------------------------------------------------------------------------- the sample reductions
def _bits_unpack(data, bits, w):
    """the full samples of a CSI-2 RAW10 / RAW12 row, bit by bit: n pixels' high bytes, then one byte of their low bits"""
    n = 4 if bits == 10 else 2
    out = []
    for x in range(w):
        g = data[(n + 1) * (x // n):(n + 1) * (x // n + 1)]
        low = (int(g[n]) >> ((bits - 8) * (x % n))) & ((1 << (bits - 8)) - 1)
        out.append((int(g[x % n]) << (bits - 8)) | low)
    return out


@pytest.mark.parametrize("shift", [0, 2, 4, 8])
def test_u16_truncates_by_the_shift_and_saturates(shift):
    top = 255 << shift
    vals = [0, 1, (1 << shift) - 1, 1 << shift, top - 1, top, top | ((1 << shift) - 1), min(top + (1 << shift), 65535), 65535]
    frame = np.array([vals], np.uint16)
    want = [min(v >> shift, 255) for v in vals]
    assert raw8(frame, "u16", shift).tolist() == [want]
    assert want[5] == 255 and want[-1] == 255 and want[2] == 0
    raw = frame.astype("<u2").tobytes()  # the bytes in memory: little-endian
    assert [raw[2 * i] | raw[2 * i + 1] << 8 for i in range(len(vals))] == vals


@pytest.mark.parametrize("sample,w", [("mipi10", 4), ("mipi10", 5), ("mipi10", 6), ("mipi10", 7), ("mipi12", 2), ("mipi12", 3)])
def test_mipi_layouts_against_a_bit_level_unpacker(sample, w):
    bits = 10 if sample == "mipi10" else 12
    h = 3
    assert row_bytes(sample, w) == {("mipi10", 4): 5, ("mipi10", 5): 10, ("mipi10", 6): 10, ("mipi10", 7): 10, ("mipi12", 2): 3,
                                    ("mipi12", 3): 6}[sample, w]
    frame = np.random.default_rng(w).integers(0, 256, (h, row_bytes(sample, w)), dtype=np.uint8)
    want = np.array([[v >> (bits - 8) for v in _bits_unpack(frame[y], bits, w)] for y in range(h)], np.uint8)
    assert np.array_equal(raw8(frame, sample, w=w), want)
    n = 4 if bits == 10 else 2
    other = frame.copy()
    other[:, n::n + 1] ^= 0xFF  # the byte of low bits changes nothing
    assert np.array_equal(raw8(other, sample, w=w), want)
    assert np.array_equal(raw8(pack(want, sample), sample, w=w), want)  # the packer is the reduction's inverse


def test_pack_u16_keeps_the_samples_and_fills_the_low_bits():
    s = np.random.default_rng(8).integers(0, 256, (3, 5), dtype=np.uint8)
    for shift in (0, 2, 4, 6, 8):
        f = pack(s, "u16", shift)
        assert f.dtype == np.uint16 and np.array_equal(raw8(f, "u16", shift), s)
        assert shift == 0 or np.any(f & ((1 << shift) - 1))


@pytest.mark.parametrize("pattern", BAYER)
def test_tone_goes_by_site_colour_and_before_the_averages(pattern):
    """a table that zeroes G and B samples leaves only R-derived values: G and B planes are 0, R is the demosaic of the R samples"""
    raw = np.random.default_rng(9).integers(1, 256, (6, 7), dtype=np.uint8)
    tone = np.zeros((3, 256), np.uint8)
    tone[0] = np.arange(256)[::-1]
    got = demosaic(raw, pattern, tone=tone)
    assert not got[:, :, 1].any() and not got[:, :, 2].any()
    c = colours(pattern, 6, 7)
    only_r = np.where(c == 0, 255 - raw, 0).astype(np.uint8)
    assert np.array_equal(got[:, :, 0], demosaic(only_r, pattern)[:, :, 0])
    # after the averages it would differ: tone((a + b + 1) >> 1) != (tone(a) + tone(b) + 1) >> 1 for a non-linear table
    sq = np.tile((np.arange(256) ** 2 // 255).astype(np.uint8), (3, 1))
    assert not np.array_equal(demosaic(raw, pattern, tone=sq), sq[0][demosaic(raw, pattern)])


# ------------------------------------------------------------------------------------------------ C-ABI refusals
def _entry(**kw):
    e = dict(data=0x1000, tone=None, w=9, h=17, pitch=9, pattern=0, sample=0, shift=0)  # a good 9 x 17 RGGB u8 entry; never dereferenced
    reserved = kw.pop("reserved", (0, 0))
    e.update(kw)
    return binding.FrameBayer(reserved=(C.c_int * 2)(*reserved), **e)


# one case per clause of the contract in mi355_yolo_int8.h: the bad entry and what the message says after the prefix
ABI_REFUSALS = [("null_data", _entry(data=None), "null frame pointer"),
                ("w_zero", _entry(w=0), "need 1 <= w, h <= 32768"),
                ("h_beyond_32768", _entry(h=32769), "need 1 <= w, h <= 32768"),
                ("unknown_pattern", _entry(pattern=5), "unknown pattern"),
                ("negative_pattern", _entry(pattern=-1), "unknown pattern"),
                ("unknown_sample", _entry(sample=4), "unknown sample layout"),
                ("negative_sample", _entry(sample=-1), "unknown sample layout"),
                ("shift_9", _entry(sample=1, pitch=18, shift=9), "shift outside 0..8"),
                ("shift_negative", _entry(sample=1, pitch=18, shift=-1), "shift outside 0..8"),
                ("shift_with_u8", _entry(shift=2), "shift must be 0 without MI355_RAW_U16"),
                ("shift_with_mipi10", _entry(sample=2, pitch=15, shift=2), "shift must be 0 without MI355_RAW_U16"),
                ("reserved_0_set", _entry(reserved=(1, 0)), "reserved must be 0"),
                ("reserved_1_set", _entry(reserved=(0, 1)), "reserved must be 0"),
                ("u8_pitch_one_below_minimum", _entry(pitch=8), "pitch < w"),
                ("u16_pitch_one_below_minimum", _entry(sample=1, pitch=17), "pitch < 2 * w"),
                ("mipi10_pitch_one_below_minimum", _entry(sample=2, pitch=14), "pitch < 5 * ((w + 3) / 4)"),
                ("mipi12_pitch_one_below_minimum", _entry(sample=3, pitch=14), "pitch < 3 * ((w + 1) / 2)"),
                ("bayer_1x9", _entry(w=1, h=9, pitch=1), "a Bayer frame needs w, h >= 2"),
                ("bayer_9x1", _entry(pattern=3, w=9, h=1), "a Bayer frame needs w, h >= 2"),
                ("geometry_mono_1x7", _entry(pattern=4, w=1, h=7, pitch=1), "degenerate aspect (resized side < 2)"),
                ("geometry_2x40", _entry(w=2, h=40, pitch=2), "degenerate aspect (resized side < 2)")]


@pytest.mark.parametrize("what,bad,message", ABI_REFUSALS, ids=[r[0] for r in ABI_REFUSALS])
def test_c_abi_calls_refuse_from_the_host_table_alone(what, bad, message):
    """table_host is validated before anything is launched, so a refusal needs no device: MI355_EINVAL and the message from both
    calls, for a bad entry behind a good one"""
    S = binding.shim()
    table = (binding.FrameBayer * 2)(_entry(), bad)
    fake = C.c_void_p(0x1000)  # device arguments: checked for null only, a refused call never passes them on
    want = f"invalid argument: frames_bayer: {message}".encode()
    assert S.mi355_frames_bayer_letterbox_minmax(fake, table, 2, 12, 12, fake, None) == -22
    assert S.mi355_last_error().startswith(want), S.mi355_last_error()
    assert S.mi355_frames_bayer_letterbox_quantize(fake, table, 2, 12, 12, fake, fake, fake, None) == -22
    assert S.mi355_last_error().startswith(want), S.mi355_last_error()
    assert S.mi355_frames_bayer_letterbox_minmax(None, table, 2, 12, 12, fake, None) == -22
    assert S.mi355_last_error().startswith(b"invalid argument: frames_bayer: letterbox_minmax: null")
    assert S.mi355_frames_bayer_letterbox_minmax(fake, table, 65536, 12, 12, fake, None) == -22
    assert S.mi355_last_error().startswith(b"invalid argument: frames_bayer: null table / need 1 <= B <= 65535")


# -------------------------------------------------------------------------------------------------- host refusals
REFUSAL = """
import ctypes as C, sys
sys.path.insert(0, {root!r})
import numpy as np
from yolo_quantization_amd import binding
net = binding.Net({cfg!r}, None, batch=1)
w, h = 9, 7
one = lambda v: (C.c_int * 1)(v)
frame = np.zeros((h, 2 * w), np.uint8)
frames = (C.c_void_p * 1)(frame.ctypes.data)
ws, hs, pitch = one(w), one(h), one({pitch})
pattern, sample, shift = {pattern}, {sample}, {shift}
{change}
net.H.network_frames_bayer_input_gpu(net.h, frames, ws, hs, pitch, pattern, sample, shift, None, 0)
print("returned")
"""

# what, pattern, sample, shift, the pitch of a 9 x 7 frame, the change to a good call, the message
REFUSALS = [("null_frame", 0, 0, 0, 9, "frames[0] = None", "null frame"),
            ("null_array", 0, 0, 0, 9, "hs = None", "null frames / sizes"),
            ("w_zero", 0, 0, 0, 9, "ws = one(0)", "need 1 <= w, h <= 32768"),
            ("h_beyond_32768", 4, 0, 0, 9, "hs = one(32769)", "need 1 <= w, h <= 32768"),
            ("unknown_pattern", 5, 0, 0, 9, "", "unknown pattern"),
            ("unknown_sample", 0, 4, 0, 9, "", "unknown sample layout"),
            ("shift_9", 0, 1, 9, 18, "", "shift outside 0..8"),
            ("shift_with_u8", 0, 0, 2, 9, "", "shift must be 0 without MI355_RAW_U16"),
            ("u8_pitch_one_below_minimum", 0, 0, 0, 8, "", "need pitch >= w (U8)"),
            ("u16_pitch_one_below_minimum", 0, 1, 2, 17, "", "need pitch >= w (U8), 2 * w (U16)"),
            ("mipi10_pitch_one_below_minimum", 0, 2, 0, 14, "", "need pitch >= w (U8)"),
            ("mipi12_pitch_one_below_minimum", 0, 3, 0, 14, "", "need pitch >= w (U8)"),
            ("bayer_below_2x2", 2, 0, 0, 9, "hs = one(1)", "a Bayer frame needs w, h >= 2")]


@pytest.mark.parametrize("what,pattern,sample,shift,pitch,change,message", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_host_entry_refuses_before_it_touches_a_device(what, pattern, sample, shift, pitch, change, message):
    """error() of the host library: its message and exit(-1), with or without a device in the box"""
    code = REFUSAL.format(root=ROOT, cfg=os.path.join(ROOT, "cfg", "tiny_unit.cfg"), pattern=pattern, sample=sample, shift=shift,
                          pitch=pitch, change=change)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 255 and "returned" not in r.stdout, (r.returncode, r.stderr[-500:])
    assert "network_frames_bayer_input_gpu: " + message in r.stderr, r.stderr[-500:]


def test_python_method_refuses_malformed_frames():
    """raised by the binding before the host library is called: no device is needed"""
    net = binding.Net(os.path.join(ROOT, "cfg", "tiny_unit.cfg"), None, batch=1)
    z = np.zeros
    tone = z((3, 256), np.uint8)
    bad = [(dict(pattern="rgbg"), z((7, 9), np.uint8)),                        # no such pattern
           (dict(sample="u10"), z((7, 9), np.uint8)),                          # no such layout
           (dict(shift=2), z((7, 9), np.uint8)),                               # a shift without u16
           (dict(sample="u16", shift=9), z((7, 9), np.uint16)),                # a shift beyond 8
           (dict(sample="u16"), z((7, 9), np.uint8)),                          # bytes where 16-bit samples are named
           (dict(), z((7, 9), np.uint16)),                                     # 16-bit samples where bytes are named
           (dict(), z((7, 9, 1), np.uint8)),                                   # not [h][w]
           (dict(), z((7, 9, 3), np.uint8)),                                   # an RGB frame
           (dict(), (z((7, 9), np.uint8), 9)),                                 # a width beside a plain frame
           (dict(sample="mipi10"), z((7, 15), np.uint8)),                      # a MIPI frame without its width
           (dict(sample="mipi10"), (z((7, 14), np.uint8), 9)),                 # rows too short for nine pixels
           (dict(sample="mipi12"), (z((7, 14), np.uint8), 9)),
           (dict(sample="mipi12"), (z((7, 15), np.uint8), 0)),                 # no pixels
           (dict(), z((1, 9), np.uint8)),                                      # a Bayer frame below 2 x 2
           (dict(pattern="gbrg"), z((9, 1), np.uint8)),
           (dict(tone=z((3, 255), np.uint8)), z((7, 9), np.uint8)),            # a short table
           (dict(tone=z((3, 256), np.int8)), z((7, 9), np.uint8)),             # no bytes
           (dict(tone=[tone, tone]), z((7, 9), np.uint8)),                     # two tables for one frame
           (dict(on_device=True), z((7, 9), np.uint8))]                        # a host array named a device tensor
    for kw, f in bad:
        with pytest.raises(ValueError):
            net.prepare_from_frames_bayer([f], **kw)

    class Tensor:  # what the binding asks of a device tensor; refused before its address is used
        def __init__(self, shape, dtype, item):
            self.shape, self.dtype, self._item = shape, dtype, item

        def data_ptr(self):
            return 0x1000

        def element_size(self):
            return self._item

        def stride(self, k):
            return int(np.prod(self.shape[k + 1:]))
    with pytest.raises(ValueError):
        net.prepare_from_frames_bayer([Tensor((7, 9), "torch.int8", 1)], on_device=True)  # one byte an element, but no uint8
    with pytest.raises(ValueError):
        net.prepare_from_frames_bayer([Tensor((7, 9), "torch.float16", 2)], sample="u16", on_device=True)
    with pytest.raises(ValueError):
        net.prepare_from_frames_bayer([Tensor((7, 9), "torch.uint8", 1)])  # a device tensor without on_device
    with pytest.raises(ValueError):
        net.prepare_from_frames_bayer([Tensor((7, 9), "torch.uint8", 1)], tone=tone, on_device=True)  # a host table beside it


# ---------------------------------------------------------------------------------------------- the CLI's raw-file reader
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
    fwrite(raw, 1, bytes[0] + bytes[1], stdout);
    free(raw);
    return 0;
}
"""


@pytest.fixture(scope="module")
def reader(tmp_path_factory):
    """the CLI's raw-file reader (host/raw_frame_file.c, linked into ./darknet only) behind a main of the test's: no device, no library"""
    d = tmp_path_factory.mktemp("bayer_reader")
    host = os.path.join(ROOT, "yolo_quantization_amd", "host")
    (d / "main.c").write_text(READER_MAIN)
    exe = d / "reader"
    subprocess.run(["gcc", "-O1", "-Wall", "-Wextra", "-Werror", "-I", host, str(d / "main.c"), os.path.join(host, "raw_frame_file.c"), "-o",
                    str(exe)], check=True)

    def load(path, kind):
        """(bytes, w, h, plane 0 bytes, next plane's bytes, message)"""
        r = subprocess.run([str(exe), str(path), str(kind)], capture_output=True)
        if r.returncode:
            assert r.returncode == 1 and not r.stdout
            return None, -1, -1, -1, -1, r.stderr.decode()
        head, _, body = r.stdout.partition(b"\n")
        w, h, n0, n1 = (int(v) for v in head.split())
        return body, w, h, n0, n1, r.stderr.decode()
    return load


def _kind(sample, pattern):
    return 64 + 8 * SAMPLES.index(sample) + PATTERNS.index(pattern)  # raw_frame_file.h


LENGTHS_WRITTEN_OUT = {("u8", 53, 37): 1961, ("u16", 53, 37): 3922, ("mipi10", 53, 37): 2590, ("mipi12", 53, 37): 2997,
                       ("u8", 2, 2): 4, ("u16", 2, 2): 8, ("mipi10", 2, 2): 10, ("mipi12", 2, 2): 6}


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("sample", SAMPLES)
@pytest.mark.parametrize("w,h", [(53, 37), (2, 2)])
def test_cli_raw_file_reader_reads_every_pattern_and_layout(tmp_path, reader, pattern, sample, w, h):
    n = row_bytes(sample, w) * h
    assert n == LENGTHS_WRITTEN_OUT[sample, w, h]
    raw = np.random.default_rng(w * 100 + h).integers(0, 256, n, dtype=np.uint8)
    good = tmp_path / f"cam_0_{w}x{h}.{pattern}"
    good.write_bytes(raw.tobytes())
    p, gw, gh, g0, g1, why = reader(good, _kind(sample, pattern))
    assert p is not None and (gw, gh, g0, g1) == (w, h, n, 0) and why == ""
    assert np.array_equal(np.frombuffer(p, np.uint8), raw)


@pytest.mark.parametrize("sample", SAMPLES)
def test_cli_raw_file_reader_refuses_bad_names_extensions_and_lengths(tmp_path, reader, sample):
    w, h, pattern = 53, 37, PATTERNS[SAMPLES.index(sample)]
    n = row_bytes(sample, w) * h
    kind = _kind(sample, pattern)
    raw = np.random.default_rng(1).integers(0, 256, n, dtype=np.uint8)
    other = PATTERNS[SAMPLES.index(sample) - 1]
    for name in (f"cam.{pattern}", f"cam_53x.{pattern}", "cam_53x37.raw", f"cam_53x37.{other}", "cam_53x37.nv12", f"cam_53x37.{pattern}.bak",
                 f"cam_0x37.{pattern}", f"53x37.{pattern}", f"cam_32769x37.{pattern}", f"cam_53x37.{pattern.upper()}"):
        bad = tmp_path / name
        bad.write_bytes(raw.tobytes())
        p, _, _, _, _, why = reader(bad, kind)
        assert p is None and f"_<W>x<H>.{pattern}" in why and name in why, name
    for delta in (-1, 1):
        bad = tmp_path / f"len{delta}_53x37.{pattern}"
        bad.write_bytes(np.resize(raw, n + delta).tobytes())
        p, _, _, _, _, why = reader(bad, kind)
        assert p is None and "_<W>x<H>" not in why, why
        assert f"holds {n} bytes, the file holds {'more than ' + str(n) if delta > 0 else n - 1}" in why, why
    p, _, _, _, _, why = reader(tmp_path / f"missing_53x37.{pattern}", kind)
    assert p is None and "cannot open" in why
    for no_kind in (64 + 5, 64 + 7, 64 + 32, 63):  # a pattern past MONO, a layout past MIPI12, the id below the first
        p, _, _, _, _, why = reader(tmp_path / f"cam_53x37.{pattern}", no_kind)
        assert p is None
