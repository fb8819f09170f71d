"""Times the input step alone: from the batch's first upload to the network's uint8 input being ready on the device.

yolov3-tiny @416, batch 64, 640 x 480 RGB frames (synthetic bytes, every frame its own range), nine variants:
  float   the float entry points: per frame one upload of the planar float image (byte / 255, converted before the clock starts)
          and one network_letterbox_input_gpu, then network_quantize_input_gpu (min / max, host sync, quantise)
  frames  network_frames_u8_input_gpu: the bytes go up as they are, two launches for the whole batch
  nv12    network_frames_nv12_input_gpu: the same frames as NV12 planes (made before the clock starts: BT.601 limited-range RGB -> YUV
          in numpy, chroma of the top-left pixel of every 2 x 2 block), half the bytes go up, converted inside the two launches
  i420    network_frames_planar_input_gpu: the same planes with the chroma de-interleaved into a U and a V plane (made before the
          clock starts), the same number of bytes as nv12 in three host arrays per frame
  bgra    network_frames_packed_input_gpu: the RGB frames as B G R A pixels, alpha 255 (made before the clock starts): 4 bytes a pixel
  yuyv    network_frames_packed_input_gpu: the NV12 planes as Y0 U Y1 V macropixels, every chroma row written twice (made before the
          clock starts): 2 bytes a pixel
  p010    network_frames_p010_input_gpu: the NV12 planes as 16-bit samples, the byte at the top (made before the clock starts): 3 bytes
          a pixel
  bayer   network_frames_bayer_input_gpu: the mosaic an RGGB sensor samples from the RGB frames, 8-bit samples, no tone table (made
          before the clock starts): 1 byte a pixel, demosaiced inside the two launches
  bayer_mipi10  the same samples as CSI-2 RAW10 rows, four pixels in five bytes: 1.25 bytes a pixel
each in shared-scale and per-image mode.  A step is timed twice: HIP events on the network's stream around it, and the host clock
from before the first upload to after a stream synchronise.  The variants alternate within a repeat; the same batch is fed every step
(steady state: layer 0 is not re-derived, the per-image bank serves every key from its cache).  Before timing, the float and frames
variants' uint8 inputs, scales and zero points are compared for equality, and the nv12 variant's with those of the frames entry point
fed the RGB frames a numpy restatement of the integer YUV -> RGB formulas makes of the NV12 planes; the i420, yuyv and p010 variants' are compared with the nv12 variant's, the bgra variant's with the frames variant's, and the two bayer variants' with those of the frames entry point fed D(frame), the
numpy restatement of the bilinear demosaic (tests/frames_bayer_util.py).  `host_convert_ms` is the byte -> planar float conversion the float variant
needs before its first upload, done with numpy here: an indication only, not part of either timed step.

--on-device adds, per scale mode, the comparison of the synchronous input step with the one that derives scales and layer-0 constants on
the device (Net.set_input_on_device): every frame variant four times -- synchronous and on-device, with host frames and with the same
frames already in HBM (uploaded before the clock starts, frames_on_device = 1) -- and the float variant twice, all alternating within
a repeat in this one process.  Each reports the two medians above and `call_ms`, the time the host thread spends inside the call; each
on-device network's input, scales and zero points are compared with its synchronous twin's first, and its host_waits() counted over the
timed steps.

--jpeg times the JPEG input path instead: batch 64 of 640 x 480 4:2:0 baseline files (smooth pictures with noise, written with Pillow at
quality 85 before the clock starts), per scale mode three variants alternating within a repeat:
  jpeg    network_frames_jpeg_input_gpu: host entropy decode of the batch, one upload of coefficients and tables, mi355_jpeg_idct,
          mi355_jpeg_to_rgb, then the u8 step on the frames where they lie
  u8      network_frames_u8_input_gpu on the decoded RGB frames in host memory (what a caller with its own JPEG decoder would feed)
  jpeg_device  the same call with set_jpeg_entropy_on_device: host scan + unstuff, one upload of bytes and tables, mi355_jpeg_entropy,
          one wait for its status words, then as above (alternating with `jpeg` in one process; its input, scales and zero points are
          compared with the jpeg network's first).  `stages_jpeg_device`: host_scan_ms, upload_ms / upload_bytes, entropy_ms per
          subseq_bits between device events, and the settle steps of the slowest round (host emulation of the first 8 files)
and, once, the stages of the jpeg variant on their own through the same calls: `host_entropy_ms` (jpeg_decode_host over the batch, host
clock, one thread), `upload_ms`, `idct_ms`, `to_rgb_ms` (HIP events around one copy of all coefficients and tables and around each
launch; medians of `iters`).  Before timing, the jpeg network's uint8 input, scales and zero points are compared with the u8 network's.

--png times the PNG input path in the same way: batch 64 of 640 x 480 8-bit RGB files (the same pictures, filtered with Paeth and
deflated by zlib at its default level before the clock starts), per scale mode three variants alternating within a repeat:
  png     network_frames_png_input_gpu: host chunk parse + inflate of the batch, one upload of tables and filtered bytes,
          mi355_png_unfilter, mi355_png_to_rgb, then the u8 step on the frames where they lie
  u8      network_frames_u8_input_gpu on the decoded RGB frames in host memory
  png_device  the same call with set_png_inflate_on_device: host chunk walk + gather of the IDAT payloads, one upload of tables and
          compressed bytes, mi355_png_inflate, one wait for its status words, then the same two launches and the u8 step (its input,
          scales and zero points are compared with the png network's first).  `stages_png_device`: host_scan_ms, upload_ms /
          upload_bytes, inflate_ms (mi355_png_inflate between device events)
and, once, the stages on their own: `host_inflate_ms` (png_decode_host over the batch, host clock, one thread), `upload_ms`,
`unfilter_ms`, `to_rgb_ms` (HIP events around one copy of all filtered bytes and around each launch; medians of `iters`).  Before
timing, the png network's uint8 input, scales and zero points are compared with the u8 network's.

--views times frame views (network_set_frame_views): twelve tiles (4 x 3, overlap 64) of ONE 3840 x 2160 frame as the slots of a batch of
12, per-image scales, five variants alternating within a repeat:
  u8_view_orient1 / _orient6      the frame in every slot under twelve views (it goes up once), as stored and turned a quarter clockwise
  nv12_view_orient1 / _orient6    the same frame as NV12 planes
  u8_crops                        the twelve rectangles handed over as separate u8 frames by pointer and pitch (twelve uploads)
with the bytes uploaded by each form.  Before timing, every view variant's input, scales and zero points are compared with the u8 step
on the materialised tiles, and u8_view_orient1's with u8_crops'.  A record, not a claim: under orient 6 a wave reads a frame column.
Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from frames_bayer_util import demosaic, mosaic, pack  # noqa: E402  (numpy only: the definition of the Bayer source)
from yolo_quantization_amd import binding, synth  # noqa: E402

CFG = os.path.join(ROOT, "cfg", "yolov3-tiny_quant.cfg")


def make_frames(B, w, h):
    rng = np.random.default_rng(7)
    return [rng.integers(b % 40, 256 - (3 * b) % 90, (h, w, 3), dtype=np.uint8) for b in range(B)]


def rgb_to_nv12(f):
    """BT.601 limited-range RGB -> (y [h][w], uv [(h + 1) // 2][(w + 1) // 2][2]); any fixed formula serves: the planes are the input"""
    r, g, b = (f[..., k].astype(np.float64) for k in range(3))
    y = 16 + (65.481 * r + 128.553 * g + 24.966 * b) / 255
    u = 128 + (-37.797 * r - 74.203 * g + 112.0 * b) / 255
    v = 128 + (112.0 * r - 93.786 * g - 18.214 * b) / 255
    q = [np.clip(np.rint(p), 0, 255).astype(np.uint8) for p in (y, u, v)]
    return q[0], np.ascontiguousarray(np.stack([q[1][::2, ::2], q[2][::2, ::2]], axis=-1))


def nv12_to_rgb(y, uv):
    """the NV12 path's specification (MI355_YUV_BT601): int32, floor shift, clamp; nearest chroma"""
    h, w = y.shape
    c = uv[(np.arange(h) // 2)[:, None], (np.arange(w) // 2)[None, :]].astype(np.int32) - 128
    yy = 76309 * (y.astype(np.int32) - 16)
    rgb = [(yy + 104597 * c[..., 1] + 32768) >> 16, (yy - 25675 * c[..., 0] - 53279 * c[..., 1] + 32768) >> 16,
           (yy + 132201 * c[..., 0] + 32768) >> 16]
    return np.ascontiguousarray(np.stack([np.clip(p, 0, 255).astype(np.uint8) for p in rgb], axis=-1))


class Events:
    def __init__(self):
        self.a, self.b = C.c_void_p(), C.c_void_p()
        binding.check(binding.shim().mi355_event_create(C.byref(self.a)), "event")
        binding.check(binding.shim().mi355_event_create(C.byref(self.b)), "event")

    def ms(self):
        out = C.c_float()
        binding.check(binding.shim().mi355_event_elapsed_ms(self.a, self.b, C.byref(out)), "elapsed")
        return out.value


class FloatVariant:
    def __init__(self, net, frames):
        self.net = net
        self.planes = [np.ascontiguousarray(f.transpose(2, 0, 1)).astype(np.float32) / np.float32(255) for f in frames]
        self.bufs = [binding.DevBuf(p.nbytes) for p in self.planes]

    def step(self):
        net, S = self.net, binding.shim()
        for slot, (p, buf) in enumerate(zip(self.planes, self.bufs)):
            binding.check(S.mi355_h2d(buf.ptr, p.ctypes.data, p.nbytes, net.stream()), "h2d")
            net.H.network_letterbox_input_gpu(net.h, slot, buf.ptr, p.shape[2], p.shape[1])
        net.H.network_quantize_input_gpu(net.h)


def _addr(a, hbm, keep):
    """the address of a plane: the host array's, or (hbm) that of a device copy made now, kept in `keep`"""
    if not hbm:
        return a.ctypes.data
    keep.append(binding.DevBuf.from_numpy(a))
    return keep[-1].ptr.value


class FramesVariant:
    def __init__(self, net, frames, hbm=False):
        B = len(frames)
        self.net, self.frames, self.hbm, self.keep = net, frames, int(hbm), []
        self.ptrs, self.w, self.h = (C.c_void_p * B)(), (C.c_int * B)(), (C.c_int * B)()
        for b, f in enumerate(frames):
            self.ptrs[b], self.h[b], self.w[b] = _addr(f, hbm, self.keep), f.shape[0], f.shape[1]

    def step(self):
        self.net.H.network_frames_u8_input_gpu(self.net.h, self.ptrs, self.w, self.h, None, 0, self.hbm)


class NV12Variant:
    def __init__(self, net, planes, hbm=False):
        B = len(planes)
        self.net, self.planes, self.hbm, self.keep = net, planes, int(hbm), []
        self.y, self.uv, self.w, self.h = (C.c_void_p * B)(), (C.c_void_p * B)(), (C.c_int * B)(), (C.c_int * B)()
        for b, (y, uv) in enumerate(planes):
            self.y[b], self.uv[b], self.h[b], self.w[b] = _addr(y, hbm, self.keep), _addr(uv, hbm, self.keep), y.shape[0], y.shape[1]

    def step(self):
        self.net.H.network_frames_nv12_input_gpu(self.net.h, self.y, self.uv, self.w, self.h, None, None, 0, 0, self.hbm)


class I420Variant:
    def __init__(self, net, planes, hbm=False):
        B = len(planes)
        self.net, self.hbm, self.keep = net, int(hbm), []
        self.planes = [(y, np.ascontiguousarray(uv[..., 0]), np.ascontiguousarray(uv[..., 1])) for y, uv in planes]
        self.p = [(C.c_void_p * B)() for _ in range(3)]
        self.w, self.h = (C.c_int * B)(), (C.c_int * B)()
        for b, yuv in enumerate(self.planes):
            for k in range(3):
                self.p[k][b] = _addr(yuv[k], hbm, self.keep)
            self.h[b], self.w[b] = yuv[0].shape

    def step(self):
        self.net.H.network_frames_planar_input_gpu(self.net.h, self.p[0], self.p[1], self.p[2], self.w, self.h, None, None, None, 0, 0, self.hbm)


class PackedVariant:
    """frames: uint8 [h][row_bytes] arrays of one packed plane; fmt: MI355_PACKED_*"""

    def __init__(self, net, frames, w, fmt, hbm=False):
        B = len(frames)
        self.net, self.frames, self.fmt, self.hbm, self.keep = net, frames, fmt, int(hbm), []
        self.ptrs, self.w, self.h = (C.c_void_p * B)(), (C.c_int * B)(), (C.c_int * B)()
        for b, f in enumerate(frames):
            self.ptrs[b], self.h[b], self.w[b] = _addr(f, hbm, self.keep), f.shape[0], w

    def step(self):
        self.net.H.network_frames_packed_input_gpu(self.net.h, self.ptrs, self.w, self.h, None, self.fmt, 0, self.hbm)


class BayerVariant:
    """frames: uint8 [h][row_bytes] arrays of raw samples behind an RGGB filter; sample: MI355_RAW_*"""

    def __init__(self, net, frames, w, sample, hbm=False):
        B = len(frames)
        self.net, self.frames, self.sample, self.hbm, self.keep = net, frames, sample, int(hbm), []
        self.ptrs, self.w, self.h = (C.c_void_p * B)(), (C.c_int * B)(), (C.c_int * B)()
        for b, f in enumerate(frames):
            self.ptrs[b], self.h[b], self.w[b] = _addr(f, hbm, self.keep), f.shape[0], w

    def step(self):
        self.net.H.network_frames_bayer_input_gpu(self.net.h, self.ptrs, self.w, self.h, None, 0, self.sample, 0, None, self.hbm)


def rgb_to_bgra(f):
    return np.ascontiguousarray(np.concatenate([f[..., ::-1], np.full(f.shape[:2] + (1,), 255, np.uint8)], axis=-1)).reshape(f.shape[0], -1)


def nv12_to_yuyv(y, uv):
    """Y0 U Y1 V macropixels of an even-width NV12 frame: row r takes chroma row r // 2, so nearest sampling reads the same samples"""
    h, w = y.shape
    c = uv[np.arange(h) // 2]
    return np.ascontiguousarray(np.stack([y[:, 0::2], c[..., 0], y[:, 1::2], c[..., 1]], axis=-1)).reshape(h, 2 * w)


class P010Variant(NV12Variant):
    def __init__(self, net, planes, hbm=False):
        super().__init__(net, [((y.astype(np.uint16) << 8), (uv.astype(np.uint16) << 8)) for y, uv in planes], hbm)

    def step(self):
        self.net.H.network_frames_p010_input_gpu(self.net.h, self.y, self.uv, self.w, self.h, None, None, 0, self.hbm)


class JpegVariant:
    def __init__(self, net, files):
        B = len(files)
        self.net, self.files = net, files
        self.ptrs, self.sizes = (C.c_char_p * B)(*files), (C.c_size_t * B)(*[len(f) for f in files])
        self.w, self.h = (C.c_int * B)(), (C.c_int * B)()

    def step(self):
        if self.net.H.network_frames_jpeg_input_gpu(self.net.h, self.ptrs, self.sizes, self.w, self.h) != 0:
            sys.exit(self.net.H.network_jpeg_last_error().decode())


def make_jpegs(B, w, h):
    import io
    from PIL import Image
    files = []
    y, x = np.mgrid[0:h, 0:w]
    for b in range(B):
        rng = np.random.default_rng(100 + b)
        base = np.stack([(x * 255) // (w - 1), (y * 255) // (h - 1), ((x + y + 7 * b) * 255 // (w + h)) % 256], axis=-1)
        pic = np.clip(base + rng.integers(-25, 26, (h, w, 3)), 0, 255).astype(np.uint8)
        buf = io.BytesIO()
        Image.fromarray(pic).save(buf, "JPEG", quality=85, subsampling=2)
        files.append(buf.getvalue())
    return files


def jpeg_stages(files, ev, iters):
    """the stages of one batch on the default stream: host entropy decode, one upload, the two launches"""
    S, H = binding.shim(), binding.host()
    host_ms = []
    for _ in range(max(3, iters // 4)):
        t0 = time.perf_counter()
        for f in files:
            j = binding.DnqJpeg()
            if H.jpeg_decode_host(f, len(f), C.byref(j), None, 0) != 0:
                sys.exit("a generated file was refused")
            H.jpeg_free(C.byref(j))
        host_ms.append((time.perf_counter() - t0) * 1e3)
    dec = [binding.jpeg_coefficients(f) for f in files]
    comps = [c for d in dec for c in d["components"]]
    stage = np.concatenate([c["coef"].ravel().view(np.uint8) for c in comps] + [c["quant"].view(np.uint8) for c in comps])
    dev = binding.DevBuf(stage.nbytes)
    planes = binding.DevBuf(sum(64 * c["blocks_w"] * c["blocks_h"] for c in comps))
    tp = (binding.JpegPlane * len(comps))()
    ti = (binding.JpegImage * len(dec))()
    at, out_at, first, k = 0, 0, 0, 0
    quant_at = sum(c["coef"].nbytes for c in comps)
    rgb = []
    for b, d in enumerate(dec):
        pitch = (3 * d["w"] + 3) & ~3
        rgb.append(binding.DevBuf(d["h"] * pitch))
        ti[b].rgb, ti[b].w, ti[b].h, ti[b].pitch, ti[b].mode = rgb[-1].ptr, d["w"], d["h"], pitch, binding.JPEG_MODES.index(d["mode"])
        for i, c in enumerate(d["components"]):
            blocks = c["blocks_w"] * c["blocks_h"]
            tp[k].coef, tp[k].quant, tp[k].out = dev.ptr.value + at, dev.ptr.value + quant_at + 128 * k, planes.ptr.value + out_at
            tp[k].blocks_w, tp[k].blocks_h, tp[k].first_block = c["blocks_w"], c["blocks_h"], first
            ti[b].comp[i].plane, ti[b].comp[i].pitch, ti[b].comp[i].rows = tp[k].out, 8 * c["blocks_w"], c["rows"]
            ti[b].comp[i].hs, ti[b].comp[i].vs = c["hs"], c["vs"]
            at, out_at, first, k = at + 128 * blocks, out_at + 64 * blocks, first + blocks, k + 1
    tpd = binding.DevBuf.from_numpy(np.frombuffer(bytes(tp), np.uint8))
    tid = binding.DevBuf.from_numpy(np.frombuffer(bytes(ti), np.uint8))
    calls = {"upload_ms": lambda: S.mi355_h2d(dev.ptr, stage.ctypes.data, stage.nbytes, None),
             "idct_ms": lambda: S.mi355_jpeg_idct(tpd.ptr, tp, len(comps), None),
             "to_rgb_ms": lambda: S.mi355_jpeg_to_rgb(tid.ptr, ti, len(dec), None)}
    res = {"host_entropy_ms": round(float(np.median(host_ms)), 4), "coefficient_bytes": int(stage.nbytes), "blocks": int(first),
           "file_bytes": int(sum(len(f) for f in files))}
    for name, call in calls.items():
        ms = []
        for _ in range(iters + 2):
            binding.check(S.mi355_stream_sync(None), "sync")
            binding.check(S.mi355_event_record(ev.a, None), "record")
            binding.check(call(), name)
            binding.check(S.mi355_event_record(ev.b, None), "record")
            binding.check(S.mi355_stream_sync(None), "sync")
            ms.append(ev.ms())
        res[name] = round(float(np.median(ms[2:])), 4)
    frames = []
    for b, d in enumerate(dec):
        pitch = (3 * d["w"] + 3) & ~3
        frames.append(rgb[b].to_numpy(np.uint8, d["h"] * pitch).reshape(d["h"], pitch)[:, :3 * d["w"]].reshape(d["h"], d["w"], 3).copy())
    for b in rgb + [dev, planes, tpd, tid]:
        b.free()
    return res, frames


class PngVariant(JpegVariant):
    def step(self):
        if self.net.H.network_frames_png_input_gpu(self.net.h, self.ptrs, self.sizes, self.w, self.h) != 0:
            sys.exit(self.net.H.network_png_last_error().decode())


def make_pngs(B, w, h):
    """the pictures of make_jpegs as 8-bit RGB PNG files, every row under the Paeth filter; and the pictures"""
    import struct
    import zlib

    def chunk(kind, data):
        return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data))

    files, pics = [], []
    y, x = np.mgrid[0:h, 0:w]
    for b in range(B):
        rng = np.random.default_rng(100 + b)
        base = np.stack([(x * 255) // (w - 1), (y * 255) // (h - 1), ((x + y + 7 * b) * 255 // (w + h)) % 256], axis=-1)
        pic = np.clip(base + rng.integers(-25, 26, (h, w, 3)), 0, 255).astype(np.uint8)
        r = pic.reshape(h, 3 * w).astype(np.int32)
        a, up, c = np.zeros_like(r), np.zeros_like(r), np.zeros_like(r)
        a[:, 3:], up[1:], c[1:, 3:] = r[:, :-3], r[:-1], r[:-1, :-3]
        pa, pb, pc = np.abs(up - c), np.abs(a - c), np.abs(a + up - 2 * c)
        pred = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, up, c))
        rows = np.concatenate([np.full((h, 1), 4, np.uint8), ((r - pred) & 255).astype(np.uint8)], axis=1)
        files.append(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(rows.tobytes()))
                     + chunk(b"IEND", b""))
        pics.append(pic)
    return files, pics


def png_stages(files, ev, iters):
    """the stages of one batch on the default stream: host parse + inflate, one upload, the two launches"""
    S, H = binding.shim(), binding.host()
    host_ms = []
    for _ in range(max(3, iters // 4)):
        t0 = time.perf_counter()
        for f in files:
            p = binding.DnqPng()
            if H.png_decode_host(f, len(f), C.byref(p), None, 0) != 0:
                sys.exit("a generated file was refused")
            H.png_free(C.byref(p))
        host_ms.append((time.perf_counter() - t0) * 1e3)
    dec = [binding.png_scanlines(f) for f in files]
    stage = np.concatenate([d["filtered"] for d in dec])
    dev = binding.DevBuf(stage.nbytes)
    nseg = sum(len(d["passes"]) for d in dec)
    rows = binding.DevBuf(sum(q["rows"] * q["row_bytes"] for d in dec for q in d["passes"]))
    ts = (binding.PngSegment * nseg)()
    ti = (binding.PngImage * len(dec))()
    at, out_at, k, rgb = 0, 0, 0, []
    for b, d in enumerate(dec):
        pitch = (3 * d["w"] + 3) & ~3
        rgb.append(binding.DevBuf(d["h"] * pitch))
        ti[b].rgb, ti[b].w, ti[b].h, ti[b].pitch = rgb[-1].ptr, d["w"], d["h"], pitch
        ti[b].depth, ti[b].color, ti[b].interlace = d["depth"], d["color"], d["interlace"]
        for q in d["passes"]:
            ts[k].filtered, ts[k].out = dev.ptr.value + at + q["offset"], rows.ptr.value + out_at
            ts[k].row_bytes, ts[k].rows, ts[k].bpp = q["row_bytes"], q["rows"], d["bpp"]
            ti[b].pass_[q["index"]] = ts[k].out
            out_at, k = out_at + q["rows"] * q["row_bytes"], k + 1
        at += d["filtered_bytes"]
    tsd = binding.DevBuf.from_numpy(np.frombuffer(bytes(ts), np.uint8))
    tid = binding.DevBuf.from_numpy(np.frombuffer(bytes(ti), np.uint8))
    calls = {"upload_ms": lambda: S.mi355_h2d(dev.ptr, stage.ctypes.data, stage.nbytes, None),
             "unfilter_ms": lambda: S.mi355_png_unfilter(tsd.ptr, ts, nseg, None),
             "to_rgb_ms": lambda: S.mi355_png_to_rgb(tid.ptr, ti, len(dec), None)}
    res = {"host_inflate_ms": round(float(np.median(host_ms)), 4), "filtered_bytes": int(stage.nbytes), "segments": int(nseg),
           "file_bytes": int(sum(len(f) for f in files))}
    for name, call in calls.items():
        ms = []
        for _ in range(iters + 2):
            binding.check(S.mi355_stream_sync(None), "sync")
            binding.check(S.mi355_event_record(ev.a, None), "record")
            binding.check(call(), name)
            binding.check(S.mi355_event_record(ev.b, None), "record")
            binding.check(S.mi355_stream_sync(None), "sync")
            ms.append(ev.ms())
        res[name] = round(float(np.median(ms[2:])), 4)
    frames = []
    for b, d in enumerate(dec):
        pitch = (3 * d["w"] + 3) & ~3
        frames.append(rgb[b].to_numpy(np.uint8, d["h"] * pitch).reshape(d["h"], pitch)[:, :3 * d["w"]].reshape(d["h"], d["w"], 3).copy())
    for b in rgb + [dev, rows, tsd, tid]:
        b.free()
    return res, frames


def inflate_stages(files, ev, iters):
    """the stages of the png_device variant on their own, on the default stream: host scan (chunk walk + gather of the IDAT payloads),
    one upload of the stream table and the compressed bytes, mi355_png_inflate between device events"""
    S, H = binding.shim(), binding.host()
    scan_ms = []
    for _ in range(max(3, iters // 4)):
        t0 = time.perf_counter()
        for f in files:
            sc = binding.DnqPngScan()
            if H.png_scan_host(f, len(f), C.byref(sc), None, 0) != 0:
                sys.exit("a generated file was refused")
            H.png_scan_free(C.byref(sc))
        scan_ms.append((time.perf_counter() - t0) * 1e3)
    scans = [binding.png_scan(f) for f in files]
    want = [binding.png_scanlines(f)["filtered"].tobytes() for f in files]
    n = len(scans)
    table = (binding.PngStream * n)()
    zat, oat, ztot, otot = [], [], 0, 0
    for sc in scans:
        zat.append(ztot)
        ztot += (((len(sc["z"]) + 3) & ~3) + 8 + 255) & ~255
        oat.append(otot)
        otot += (sc["filtered_bytes"] + 255) & ~255
    stage = np.zeros(C.sizeof(table) + ztot, np.uint8)
    for sc, at in zip(scans, zat):
        stage[C.sizeof(table) + at:C.sizeof(table) + at + len(sc["z"])] = np.frombuffer(sc["z"], np.uint8)
    dev, out, st = binding.DevBuf(stage.nbytes), binding.DevBuf(otot), binding.DevBuf(4 * n)
    for i, sc in enumerate(scans):
        t = table[i]
        t.z, t.out, t.nbytes, t.cap = dev.ptr.value + C.sizeof(table) + zat[i], out.ptr.value + oat[i], len(sc["z"]), sc["filtered_bytes"]
        t.npasses = len(sc["passes"])
        for k, q in enumerate(sc["passes"]):
            t.rows[k], t.row_bytes[k] = q["rows"], q["row_bytes"]
    stage[:C.sizeof(table)] = np.frombuffer(bytes(table), np.uint8)
    res = {"host_scan_ms": round(float(np.median(scan_ms)), 4), "upload_bytes": int(stage.nbytes), "stream_bytes": int(sum(len(sc["z"]) for sc in scans)),
           "streams": n}
    calls = {"upload_ms": lambda: S.mi355_h2d(dev.ptr, stage.ctypes.data, stage.nbytes, None),
             "inflate_ms": lambda: S.mi355_png_inflate(dev.ptr, table, n, st.ptr, None)}
    for name, call in calls.items():
        ms = []
        for _ in range(iters + 2):
            binding.check(S.mi355_stream_sync(None), "sync")
            binding.check(S.mi355_event_record(ev.a, None), "record")
            binding.check(call(), name)
            binding.check(S.mi355_event_record(ev.b, None), "record")
            binding.check(S.mi355_stream_sync(None), "sync")
            ms.append(ev.ms())
        res[name] = round(float(np.median(ms[2:])), 4)
    status = st.to_numpy(np.int32, n)
    got = out.to_numpy(np.uint8, otot)
    res["filtered_bytes_identical_to_png_decode_host"] = bool(not status.any() and all(
        got[oat[i]:oat[i] + len(w)].tobytes() == w for i, w in enumerate(want)))
    for b in (dev, out, st):
        b.free()
    return res


def png_main(a, wts, ev):
    sw, sh = (int(v) for v in a.src.split("x"))
    files, pics = make_pngs(a.batch, sw, sh)
    res = {}
    res["stages"], frames = png_stages(files, ev, a.iters)
    res["stages_png_device"] = inflate_stages(files, ev, a.iters)
    res["frames_identical_to_the_pictures"] = bool(all(np.array_equal(f, p) for f, p in zip(frames, pics)))
    for mode in ("shared", "per_image"):
        nets = {k: binding.Net(CFG, wts, batch=a.batch) for k in ("png", "png_device", "u8")}
        for n in nets.values():
            n.set_input_per_image(mode == "per_image")
        nets["png_device"].set_png_inflate_on_device(True)
        var = {"png": PngVariant(nets["png"], files), "png_device": PngVariant(nets["png_device"], files), "u8": FramesVariant(nets["u8"], frames)}
        for _ in range(a.warmup):
            for v in var.values():
                v.step()
        out = {k: {"device_ms": [], "wall_ms": [], "call_ms": []} for k in var}
        same = same_input(nets["png"], nets["u8"])
        out["png_device_identical_to_png"] = same_input(nets["png_device"], nets["png"])
        for _ in range(a.repeats):
            for k, v in var.items():  # alternating
                for name, x in zip(("device_ms", "wall_ms", "call_ms"), timed(v, ev, a.iters)):
                    out[k][name].append(round(x, 4))
        for k in var:
            out[k]["median"] = {m: float(np.median(out[k][m])) for m in ("device_ms", "wall_ms", "call_ms")}
        out["png_identical_to_u8_on_the_decoded_frames"] = same
        res[mode] = out
        for n in nets.values():
            n.close()
    cpu = "unknown"
    try:
        with open("/proc/cpuinfo") as f:
            cpu = next(line.split(":", 1)[1].strip() for line in f if line.startswith("model name"))
    except (OSError, StopIteration):
        pass
    res["config"] = {"cfg": "yolov3-tiny_quant.cfg", "batch": a.batch, "src": a.src, "format": "RGB 8-bit, Paeth on every row, zlib level 6",
                     "iters": a.iters, "warmup": a.warmup, "repeats": a.repeats, "host_cpu": cpu,
                     "values": "per repeat the median of `iters` steps: device_ms between HIP events around the step, wall_ms host clock to the "
                               "end of a stream synchronise after it, call_ms host clock inside the call; `median` over the repeats; stages: "
                               "see the module text"}
    print(json.dumps(res))


SUBSEQ_BITS = (128, 256, 512, 1024, 2048, 4096, 8192)


def entropy_stages(files, ev, iters, steps_files=8):
    """the stages of the jpeg_device variant on their own, on the default stream: host scan + unstuff, one upload of the unstuffed
    bytes and tables, mi355_jpeg_entropy at every SUBSEQ_BITS; and, from the host emulation, the settle steps of the slowest round"""
    S, H = binding.shim(), binding.host()
    scan_ms = []
    for _ in range(max(3, iters // 4)):
        t0 = time.perf_counter()
        for f in files:
            j, sl = binding.DnqJpeg(), binding.DnqJpegScanList()
            if H.jpeg_scan_host(f, len(f), C.byref(j), C.byref(sl), None, 0) != 0:
                sys.exit("a generated file was refused")
            H.jpeg_scan_free(C.byref(sl))
        scan_ms.append((time.perf_counter() - t0) * 1e3)
    job = binding.JpegEntropyJob(files)
    want = [binding.jpeg_coefficients(f) for f in files]
    planes, status, _ = job.run(1024)
    exact = all(not any(st) for st in status) and all(np.array_equal(a, c["coef"]) for per, d in zip(planes, want) for a, c in zip(per, d["components"]))
    stage = np.zeros(job.stream_bytes + job.huff_bytes + C.sizeof(job.table), np.uint8)
    dev = binding.DevBuf(stage.nbytes)
    res = {"host_scan_ms": round(float(np.median(scan_ms)), 4), "upload_bytes": int(stage.nbytes), "stream_bytes": job.stream_bytes,
           "segments": job.nseg, "coefficients_identical_to_jpeg_decode_host": bool(exact), "entropy_ms": {}}

    def timed_call(call, name):
        ms = []
        for _ in range(iters + 2):
            binding.check(S.mi355_stream_sync(None), "sync")
            binding.check(S.mi355_event_record(ev.a, None), "record")
            binding.check(call(), name)
            binding.check(S.mi355_event_record(ev.b, None), "record")
            binding.check(S.mi355_stream_sync(None), "sync")
            ms.append(ev.ms())
        return round(float(np.median(ms[2:])), 4)

    res["upload_ms"] = timed_call(lambda: S.mi355_h2d(dev.ptr, stage.ctypes.data, stage.nbytes, None), "upload")
    for bits in SUBSEQ_BITS:
        res["entropy_ms"][str(bits)] = timed_call(lambda: job.launch(bits), "mi355_jpeg_entropy")
    job.free()
    dev.free()
    emu = binding.JpegEntropyJob(files[:steps_files], emulate=True)
    res["settle_steps_of_the_slowest_round"] = {"files": min(steps_files, len(files))}
    for bits in SUBSEQ_BITS:
        steps = [s for per in emu.run(bits)[2] for s in per]
        res["settle_steps_of_the_slowest_round"][str(bits)] = {"max": int(max(steps)), "median": float(np.median(steps))}
    return res


def jpeg_main(a, wts, ev):
    sw, sh = (int(v) for v in a.src.split("x"))
    files = make_jpegs(a.batch, sw, sh)
    res = {}
    res["stages"], frames = jpeg_stages(files, ev, a.iters)
    res["stages_jpeg_device"] = entropy_stages(files, ev, a.iters)
    for mode in ("shared", "per_image"):
        nets = {k: binding.Net(CFG, wts, batch=a.batch) for k in ("jpeg", "jpeg_device", "u8")}
        for n in nets.values():
            n.set_input_per_image(mode == "per_image")
        nets["jpeg_device"].set_jpeg_entropy_on_device(True, subseq_bits=a.subseq_bits)
        var = {"jpeg": JpegVariant(nets["jpeg"], files), "jpeg_device": JpegVariant(nets["jpeg_device"], files), "u8": FramesVariant(nets["u8"], frames)}
        for _ in range(a.warmup):
            for v in var.values():
                v.step()
        out = {k: {"device_ms": [], "wall_ms": [], "call_ms": []} for k in var}
        same = same_input(nets["jpeg"], nets["u8"])
        out["jpeg_device_identical_to_jpeg"] = same_input(nets["jpeg_device"], nets["jpeg"])
        for _ in range(a.repeats):
            for k, v in var.items():  # alternating
                for name, x in zip(("device_ms", "wall_ms", "call_ms"), timed(v, ev, a.iters)):
                    out[k][name].append(round(x, 4))
        for k in var:
            out[k]["median"] = {m: float(np.median(out[k][m])) for m in ("device_ms", "wall_ms", "call_ms")}
        out["jpeg_identical_to_u8_on_the_decoded_frames"] = same
        res[mode] = out
        for n in nets.values():
            n.close()
    cpu = "unknown"
    try:
        with open("/proc/cpuinfo") as f:
            cpu = next(line.split(":", 1)[1].strip() for line in f if line.startswith("model name"))
    except (OSError, StopIteration):
        pass
    res["config"] = {"cfg": "yolov3-tiny_quant.cfg", "batch": a.batch, "src": a.src, "sampling": "4:2:0", "quality": 85, "iters": a.iters,
                     "subseq_bits": a.subseq_bits,
                     "warmup": a.warmup, "repeats": a.repeats, "host_cpu": cpu,
                     "values": "per repeat the median of `iters` steps: device_ms between HIP events around the step, wall_ms host clock to the "
                               "end of a stream synchronise after it, call_ms host clock inside the call; `median` over the repeats; stages: "
                               "see the module text"}
    print(json.dumps(res))


class CropsVariant:
    """the views' rectangles of one host frame handed over as separate u8 frames, by pointer and pitch (orient 1 only: a pointer cannot turn)"""

    def __init__(self, net, frame, views):
        B = len(views)
        self.net, self.frame = net, frame
        self.ptrs, self.w, self.h, self.pitch = (C.c_void_p * B)(), (C.c_int * B)(), (C.c_int * B)(), (C.c_int * B)()
        for b, (x0, y0, w, h, _) in enumerate(views):
            self.ptrs[b] = frame.ctypes.data + y0 * frame.strides[0] + 3 * x0
            self.w[b], self.h[b], self.pitch[b] = w, h, frame.strides[0]
        self.uploaded = sum((h - 1) * frame.strides[0] + 3 * w for _, _, w, h, _ in views)

    def step(self):
        self.net.H.network_frames_u8_input_gpu(self.net.h, self.ptrs, self.w, self.h, self.pitch, 0, 0)


def views_main(a, wts, ev):
    """--views: twelve tiles (4 x 3, overlap 64) of ONE 3840 x 2160 frame at the network's size, per-image scales: the frame under twelve views
    (u8_view, nv12_view; uploaded once), at orient 1 and at orient 6, and the twelve crops as separate u8 frames by pointer and pitch."""
    W, H, B = 3840, 2160, 12
    frame = make_frames(1, W, H)[0]
    y, uv = rgb_to_nv12(frame)
    converted = nv12_to_rgb(y, uv)
    tiles = {o: binding.tile_views(W, H, 4, 3, 64, o) for o in (1, 6)}
    names = ["u8_view_orient1", "u8_view_orient6", "nv12_view_orient1", "nv12_view_orient6", "u8_crops"]
    nets = {k: binding.Net(CFG, wts, batch=B) for k in names + ["check"]}
    for n in nets.values():
        n.set_input_per_image(True)
    for o in (1, 6):
        nets[f"u8_view_orient{o}"].set_frame_views(tiles[o])
        nets[f"nv12_view_orient{o}"].set_frame_views(tiles[o])
    var = {f"u8_view_orient{o}": FramesVariant(nets[f"u8_view_orient{o}"], [frame] * B) for o in (1, 6)}
    var.update({f"nv12_view_orient{o}": NV12Variant(nets[f"nv12_view_orient{o}"], [(y, uv)] * B) for o in (1, 6)})
    var["u8_crops"] = CropsVariant(nets["u8_crops"], frame, tiles[1])
    for v in var.values():
        for _ in range(a.warmup):
            v.step()
    same = {"u8_view_orient1_identical_to_crops": same_input(nets["u8_view_orient1"], nets["u8_crops"])}
    for o in (1, 6):  # against the u8 path on the materialised tiles
        for kind, rgb in (("u8", frame), ("nv12", converted)):
            mat = [np.ascontiguousarray({1: lambda t: t, 6: lambda t: np.rot90(t, -1)}[o](rgb[y0:y0 + h, x0:x0 + w])) for x0, y0, w, h, _ in tiles[o]]
            FramesVariant(nets["check"], mat).step()
            same[f"{kind}_view_orient{o}_identical_to_u8_on_materialised_tiles"] = same_input(nets[f"{kind}_view_orient{o}"], nets["check"])
    runs = {k: [] for k in names}
    for _ in range(a.repeats):
        for k in names:
            d, wl, c = timed(var[k], ev, a.iters)
            runs[k].append({"device_ms": round(d, 4), "wall_ms": round(wl, 4), "call_ms": round(c, 4)})
    uploaded = {"u8_view": frame.nbytes, "nv12_view": y.nbytes + uv.nbytes, "u8_crops": var["u8_crops"].uploaded}
    print(json.dumps({"views": {"frame": f"{W}x{H}", "tiles": "4x3, overlap 64", "tile": list(tiles[1][0][2:4]), "batch": B, "identical": same,
                                "bytes_uploaded": uploaded, "runs": runs,
                                "note": "median of --iters steps per entry, variants alternating within a repeat; a record, not a claim"}}))


def same_input(a, b):
    same = np.array_equal(pull_input(a), pull_input(b))
    qa, qb = a.input_quantization(), b.input_quantization()
    return bool(same and np.array_equal(qa[0].view(np.uint32), qb[0].view(np.uint32)) and np.array_equal(qa[1], qb[1]))


def timed(variant, ev, iters):
    net, S = variant.net, binding.shim()
    dev, wall, call = [], [], []
    for _ in range(iters):
        net.sync()
        t0 = time.perf_counter()
        binding.check(S.mi355_event_record(ev.a, net.stream()), "record")
        t1 = time.perf_counter()
        variant.step()
        call.append((time.perf_counter() - t1) * 1e3)
        binding.check(S.mi355_event_record(ev.b, net.stream()), "record")
        net.sync()
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(ev.ms())
    return float(np.median(dev)), float(np.median(wall)), float(np.median(call))


def pull_input(net):
    net.sync()
    out = np.empty(net.batch * net.inputs, np.uint8)
    binding.check(binding.shim().mi355_d2h(out.ctypes.data, net.input_gpu_ptr(), out.nbytes, None), "d2h")
    binding.check(binding.shim().mi355_stream_sync(None), "sync")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--src", default="640x480")
    ap.add_argument("--on-device", action="store_true", help="compare the synchronous step with the on-device one instead (see the module text)")
    ap.add_argument("--jpeg", action="store_true", help="time the JPEG input path beside the u8 path on the decoded frames instead (see the module text)")
    ap.add_argument("--png", action="store_true", help="time the PNG input path beside the u8 path on the decoded frames instead (see the module text)")
    ap.add_argument("--views", action="store_true", help="time twelve tiles of one 3840 x 2160 frame as views and as separate crops instead (see views_main)")
    ap.add_argument("--subseq-bits", type=int, default=1024, help="--jpeg: bits a lane decodes per round in the jpeg_device variant")
    a = ap.parse_args()
    binding.init(0)  # raises without a gfx950: nothing is timed on a CPU
    wts = "/tmp/input_path_bench.weights"
    synth.synth_weights(CFG, wts, seed=5)
    if a.jpeg:
        jpeg_main(a, wts, Events())
        return
    if a.png:
        png_main(a, wts, Events())
        return
    if a.views:
        views_main(a, wts, Events())
        return
    sw, sh = (int(v) for v in a.src.split("x"))
    if sw % 2:
        sys.exit("--src: the yuyv variant is made from the NV12 planes and needs an even width")
    frames = make_frames(a.batch, sw, sh)
    t0 = time.perf_counter()
    for f in frames:
        np.ascontiguousarray(f.transpose(2, 0, 1)).astype(np.float32) / np.float32(255)
    convert_ms = (time.perf_counter() - t0) * 1e3
    planes = [rgb_to_nv12(f) for f in frames]
    converted = [nv12_to_rgb(y, uv) for y, uv in planes]
    bgra, yuyv = [rgb_to_bgra(f) for f in frames], [nv12_to_yuyv(y, uv) for y, uv in planes]
    mosaics = [mosaic(f, "rggb") for f in frames]
    raw10, demosaiced = [pack(m, "mipi10") for m in mosaics], [demosaic(m, "rggb") for m in mosaics]
    ev = Events()
    res = {}
    if a.on_device:
        sources = {"frames": (FramesVariant, (frames,)), "nv12": (NV12Variant, (planes,)), "i420": (I420Variant, (planes,)),
                   "bgra": (PackedVariant, (bgra, sw, 1)), "yuyv": (PackedVariant, (yuyv, sw, 4)), "p010": (P010Variant, (planes,))}
        for mode in ("shared", "per_image"):
            var = {}
            for k, (cls, args) in sources.items():
                for where in ("host", "hbm"):
                    for how in ("sync", "device"):
                        net = binding.Net(CFG, wts, batch=a.batch)
                        net.set_input_per_image(mode == "per_image")
                        net.set_input_on_device(how == "device")
                        var[f"{k}/{where}/{how}"] = cls(net, *args, hbm=where == "hbm")
            for how in ("sync", "device"):
                net = binding.Net(CFG, wts, batch=a.batch)
                net.set_input_per_image(mode == "per_image")
                net.set_input_on_device(how == "device")
                var[f"float/host/{how}"] = FloatVariant(net, frames)
            for _ in range(a.warmup):
                for v in var.values():
                    v.step()
            out = {k: {"device_ms": [], "wall_ms": [], "call_ms": []} for k in var}
            for k in var:
                if k.endswith("/device"):
                    out[k]["identical_to_sync"] = same_input(var[k].net, var[k[:-len("device")] + "sync"].net)
            waits = {k: v.net.host_waits() for k, v in var.items()}
            for _ in range(a.repeats):
                for k, v in var.items():  # alternating
                    for name, x in zip(("device_ms", "wall_ms", "call_ms"), timed(v, ev, a.iters)):
                        out[k][name].append(round(x, 4))
            for k, v in var.items():
                out[k]["host_waits_per_step"] = (v.net.host_waits() - waits[k]) / (a.repeats * a.iters)
                out[k]["median"] = {m: float(np.median(out[k][m])) for m in ("device_ms", "wall_ms", "call_ms")}
            res[mode] = out
            for v in var.values():
                v.net.close()
        res["config"] = {"cfg": "yolov3-tiny_quant.cfg", "batch": a.batch, "src": a.src, "iters": a.iters, "warmup": a.warmup, "repeats": a.repeats,
                         "keys": "<source>/<host: frames uploaded by the call | hbm: frames already on the device>/<sync | device>",
                         "values": "per repeat the median of `iters` steps: device_ms between HIP events around the step, wall_ms host clock "
                                   "to the end of a stream synchronise after it, call_ms host clock inside the call; `median` over the repeats"}
        print(json.dumps(res))
        return
    for mode in ("shared", "per_image"):
        nets = {k: binding.Net(CFG, wts, batch=a.batch) for k in ("float", "frames", "nv12", "i420", "bgra", "yuyv", "p010", "bayer", "bayer_mipi10")}
        if mode == "per_image":
            for n in nets.values():
                n.set_input_per_image(True)
        var = {"float": FloatVariant(nets["float"], frames), "frames": FramesVariant(nets["frames"], frames),
               "nv12": NV12Variant(nets["nv12"], planes), "i420": I420Variant(nets["i420"], planes),
               "bgra": PackedVariant(nets["bgra"], bgra, sw, 1), "yuyv": PackedVariant(nets["yuyv"], yuyv, sw, 4),
               "p010": P010Variant(nets["p010"], planes), "bayer": BayerVariant(nets["bayer"], mosaics, sw, 0),
               "bayer_mipi10": BayerVariant(nets["bayer_mipi10"], raw10, sw, 2)}
        for _ in range(a.warmup):
            for v in var.values():
                v.step()
        same = same_input(nets["float"], nets["frames"])
        same_bgra = same_input(nets["bgra"], nets["frames"])
        FramesVariant(nets["frames"], converted).step()  # the frames entry point on the numpy conversion of the NV12 planes
        same_nv12 = same_input(nets["nv12"], nets["frames"])
        same_i420 = same_input(nets["i420"], nets["nv12"])
        same_yuyv, same_p010 = same_input(nets["yuyv"], nets["nv12"]), same_input(nets["p010"], nets["nv12"])
        FramesVariant(nets["frames"], demosaiced).step()  # the frames entry point on D(frame) of the mosaics
        same_bayer, same_raw10 = same_input(nets["bayer"], nets["frames"]), same_input(nets["bayer_mipi10"], nets["frames"])
        for _ in range(a.warmup):
            var["frames"].step()
        runs = {k: {"device_ms": [], "wall_ms": []} for k in var}
        for _ in range(a.repeats):
            for k, v in var.items():  # alternating
                d, w, _ = timed(v, ev, a.iters)
                runs[k]["device_ms"].append(round(d, 4))
                runs[k]["wall_ms"].append(round(w, 4))
        med = {k: {m: float(np.median(r[m])) for m in r} for k, r in runs.items()}
        res[mode] = {"identical_input": same, "nv12_identical_to_frames_on_converted_rgb": same_nv12,
                     "i420_identical_to_nv12": same_i420, "float": runs["float"], "frames": runs["frames"], "nv12": runs["nv12"],
                     "i420": runs["i420"],
                     "bgra_identical_to_frames": same_bgra, "yuyv_identical_to_nv12": same_yuyv, "p010_identical_to_nv12": same_p010,
                     "bgra": runs["bgra"], "yuyv": runs["yuyv"], "p010": runs["p010"],
                     "bayer_identical_to_frames_on_demosaiced_rgb": same_bayer,
                     "bayer_mipi10_identical_to_frames_on_demosaiced_rgb": same_raw10,
                     "bayer": runs["bayer"], "bayer_mipi10": runs["bayer_mipi10"],
                     "bayer_over_frames_device": round(med["frames"]["device_ms"] / med["bayer"]["device_ms"], 3),
                     "bayer_mipi10_over_frames_device": round(med["frames"]["device_ms"] / med["bayer_mipi10"]["device_ms"], 3),
                     "bgra_over_frames_device": round(med["frames"]["device_ms"] / med["bgra"]["device_ms"], 3),
                     "yuyv_over_nv12_device": round(med["nv12"]["device_ms"] / med["yuyv"]["device_ms"], 3),
                     "p010_over_nv12_device": round(med["nv12"]["device_ms"] / med["p010"]["device_ms"], 3),
                     "speedup_device": round(med["float"]["device_ms"] / med["frames"]["device_ms"], 3),
                     "speedup_wall": round(med["float"]["wall_ms"] / med["frames"]["wall_ms"], 3),
                     "nv12_over_frames_device": round(med["frames"]["device_ms"] / med["nv12"]["device_ms"], 3),
                     "nv12_over_frames_wall": round(med["frames"]["wall_ms"] / med["nv12"]["wall_ms"], 3),
                     "i420_over_nv12_device": round(med["nv12"]["device_ms"] / med["i420"]["device_ms"], 3),
                     "i420_over_nv12_wall": round(med["nv12"]["wall_ms"] / med["i420"]["wall_ms"], 3)}
        for n in nets.values():
            n.close()
    res["host_convert_ms_numpy"] = round(convert_ms, 3)
    res["config"] = {"cfg": "yolov3-tiny_quant.cfg", "batch": a.batch, "src": a.src, "iters": a.iters, "warmup": a.warmup,
                     "repeats": a.repeats, "values": "median of `iters` steps per repeat; speedup = median over repeats, float / frames; "
                               "nv12_over_frames = frames / nv12; i420_over_nv12 = nv12 / i420; bgra_over_frames, yuyv_over_nv12, p010_over_nv12, bayer_over_frames, bayer_mipi10_over_frames likewise"}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
