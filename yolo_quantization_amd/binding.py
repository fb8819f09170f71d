"""ctypes bindings over the two product libraries:

  lib/libmi355yolo.so   HIP kernels + C-ABI   (include/mi355_yolo_int8.h)
  lib/libdarknet_q.so   plain-C darknet host   (include/darknet_q.h + host/capi.c accessors)

There is no fallback: if a library is missing or the device is not a gfx950, loading / init raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_DIR = os.environ.get("MI355_LIB_DIR") or os.path.join(_HERE, "lib")   # override: A/B runs against another build of the libraries

ACT = {"relu": 1, "linear": 3, "relu6": 8, "leaky": 9}
STORE_WRAP, STORE_SATURATE = 0, 1
ACC_EXACT, ACC_REF_F32 = 0, 1


class MI355Error(RuntimeError):
    pass


class Tensor(C.Structure):
    _fields_ = [("data", C.c_void_p), ("B", C.c_int), ("H", C.c_int), ("W", C.c_int), ("C", C.c_int),
                ("cs", C.c_int), ("lead", C.c_int), ("tail", C.c_int)]


class ConvDesc(C.Structure):
    _fields_ = [("n", C.c_int), ("c", C.c_int), ("ksize", C.c_int), ("stride", C.c_int), ("pad", C.c_int),
                ("activation", C.c_int), ("store_mode", C.c_int), ("accum_mode", C.c_int),
                ("zp_in", C.c_uint8), ("zp_act", C.c_uint8), ("s_act", C.c_float), ("plan", C.c_int), ("epilogue_packed", C.c_int)]


class FrameU8(C.Structure):
    """mi355_frame_u8: one entry of the frame table of mi355_frames_u8_letterbox_minmax / _quantize (data: a DEVICE pointer)."""
    _fields_ = [("data", C.c_void_p), ("w", C.c_int), ("h", C.c_int), ("pitch", C.c_int), ("order", C.c_int), ("reserved", C.c_int * 2)]


FRAME_ORDER = {"rgb": 0, "bgr": 1}  # MI355_FRAME_RGB / MI355_FRAME_BGR


class FrameYUV(C.Structure):
    """mi355_frame_yuv: one entry of the frame table of mi355_frames_yuv_letterbox_minmax / _quantize (y, uv: DEVICE pointers)."""
    _fields_ = [("y", C.c_void_p), ("uv", C.c_void_p), ("w", C.c_int), ("h", C.c_int), ("pitch_y", C.c_int), ("pitch_uv", C.c_int),
                ("layout", C.c_int), ("matrix", C.c_int), ("reserved", C.c_int * 2)]


YUV_LAYOUT = {"nv12": 0, "nv21": 1}  # MI355_YUV_NV12 / MI355_YUV_NV21
YUV_MATRIX = {"bt601": 0, "bt601f": 1, "bt709": 2, "bt709f": 3}  # MI355_YUV_BT601, _BT601_FULL, _BT709, _BT709_FULL



class FramePlanar(C.Structure):
    """mi355_frame_planar: one entry of the frame table of mi355_frames_planar_letterbox_minmax / _quantize (plane: DEVICE pointers)."""
    _fields_ = [("plane", C.c_void_p * 3), ("w", C.c_int), ("h", C.c_int), ("pitch", C.c_int * 3), ("format", C.c_int),
                ("matrix", C.c_int), ("reserved", C.c_int * 3)]


PLANAR_FORMAT = {"i420": 0, "yv12": 1, "i422": 2, "i444": 3, "rgb": 4, "bgr": 5}  # MI355_PLANAR_I420 .. MI355_PLANAR_BGR


class FramePacked(C.Structure):
    """mi355_frame_packed: one entry of the frame table of mi355_frames_packed_letterbox_minmax / _quantize (data: a DEVICE pointer)."""
    _fields_ = [("data", C.c_void_p), ("w", C.c_int), ("h", C.c_int), ("pitch", C.c_int), ("format", C.c_int), ("matrix", C.c_int),
                ("reserved", C.c_int)]


PACKED_FORMAT = {"rgba": 0, "bgra": 1, "argb": 2, "abgr": 3, "yuyv": 4, "uyvy": 5, "yvyu": 6}  # MI355_PACKED_RGBA .. MI355_PACKED_YVYU
PACKED_RGBX = ("rgba", "bgra", "argb", "abgr")  # four bytes a pixel; the others: four bytes a macropixel of two pixels (4:2:2)


class FrameP010(C.Structure):
    """mi355_frame_p010: one entry of the frame table of mi355_frames_p010_letterbox_minmax / _quantize (y, uv: DEVICE pointers);
    mi355_frame_yuv's field layout, `layout` reserved and zero."""
    _fields_ = [("y", C.c_void_p), ("uv", C.c_void_p), ("w", C.c_int), ("h", C.c_int), ("pitch_y", C.c_int), ("pitch_uv", C.c_int),
                ("layout", C.c_int), ("matrix", C.c_int), ("reserved", C.c_int * 2)]


class FrameBayer(C.Structure):
    """mi355_frame_bayer: one entry of the frame table of mi355_frames_bayer_letterbox_minmax / _quantize (data, tone: DEVICE
    pointers; tone may be NULL)."""
    _fields_ = [("data", C.c_void_p), ("tone", C.c_void_p), ("w", C.c_int), ("h", C.c_int), ("pitch", C.c_int), ("pattern", C.c_int),
                ("sample", C.c_int), ("shift", C.c_int), ("reserved", C.c_int * 2)]


class FrameView(C.Structure):
    """mi355_frame_view: what a batch slot looks at -- the rectangle [x0, x0 + w) x [y0, y0 + h) of its frame under EXIF orientation
    `orient` (1..8).  One per slot, beside the frame table, in the mi355_frames_<kind>_view_letterbox_minmax / _quantize calls."""
    _fields_ = [("x0", C.c_int), ("y0", C.c_int), ("w", C.c_int), ("h", C.c_int), ("orient", C.c_int), ("reserved", C.c_int * 3)]


class Box(C.Structure):
    """box of darknet_q.h"""
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("w", C.c_float), ("h", C.c_float)]


BAYER_PATTERN = {"rggb": 0, "bggr": 1, "grbg": 2, "gbrg": 3, "mono": 4}  # MI355_BAYER_RGGB .. MI355_BAYER_MONO
RAW_SAMPLE = {"u8": 0, "u16": 1, "mipi10": 2, "mipi12": 3}  # MI355_RAW_U8 .. MI355_RAW_MIPI12


def raw_row_bytes(sample, w):
    """The bytes of a row of w raw samples of layout `sample` (a key of RAW_SAMPLE)."""
    return {"u8": w, "u16": 2 * w, "mipi10": 5 * ((w + 3) // 4), "mipi12": 3 * ((w + 1) // 2)}[sample]


class YoloHead(C.Structure):
    """mi355_yolo_head: one yolo layer of mi355_yolo_detections_batch (yolo_out, anchors, mask: DEVICE pointers)."""
    _fields_ = [("yolo_out", C.c_void_p), ("anchors", C.c_void_p), ("mask", C.c_void_p), ("n", C.c_int), ("H", C.c_int), ("W", C.c_int),
                ("reserved", C.c_int)]


YOLO_MAX_HEADS = 8  # MI355_YOLO_MAX_HEADS

_shim = None
_host = None


class JpegPlane(C.Structure):
    """mi355_jpeg_plane: one component plane of mi355_jpeg_idct's table (device pointers)."""
    _fields_ = [("coef", C.c_void_p), ("quant", C.c_void_p), ("out", C.c_void_p), ("blocks_w", C.c_int), ("blocks_h", C.c_int),
                ("first_block", C.c_int), ("reserved", C.c_int * 3)]


class JpegComponent(C.Structure):
    _fields_ = [("plane", C.c_void_p), ("pitch", C.c_int), ("rows", C.c_int), ("hs", C.c_int), ("vs", C.c_int)]


class JpegImage(C.Structure):
    """mi355_jpeg_image: one image of mi355_jpeg_to_rgb's table (device pointers)."""
    _fields_ = [("rgb", C.c_void_p), ("w", C.c_int), ("h", C.c_int), ("pitch", C.c_int), ("mode", C.c_int), ("comp", JpegComponent * 3)]


class DnqJpegComp(C.Structure):
    _fields_ = [("id", C.c_int), ("h", C.c_int), ("v", C.c_int), ("hs", C.c_int), ("vs", C.c_int), ("w", C.c_int), ("rows", C.c_int),
                ("blocks_w", C.c_int), ("blocks_h", C.c_int), ("tq", C.c_int), ("scans", C.c_int), ("coef", C.POINTER(C.c_int16)),
                ("quant", C.c_uint16 * 64)]


class DnqJpeg(C.Structure):
    """dnq_jpeg (yolo_quantization_amd/host/jpeg.h): what the host half of the JPEG decoder returns."""
    _fields_ = [("w", C.c_int), ("h", C.c_int), ("ncomp", C.c_int), ("mode", C.c_int), ("h_max", C.c_int), ("v_max", C.c_int),
                ("sof", C.c_int), ("jfif", C.c_int), ("adobe_transform", C.c_int), ("restart_interval", C.c_int), ("nscans", C.c_int),
                ("comp", DnqJpegComp * 3)]


class JpegHuff(C.Structure):
    """mi355_jpeg_huff: one Huffman table as mi355_jpeg_entropy reads it."""
    _fields_ = [("look", C.c_uint16 * 256), ("maxcode", C.c_int32 * 17), ("mincode", C.c_int32 * 17), ("first", C.c_int32 * 17),
                ("nvalues", C.c_int32), ("values", C.c_uint8 * 256)]


class JpegSegment(C.Structure):
    """mi355_jpeg_segment: one restart interval (or whole scan) of mi355_jpeg_entropy's table."""
    _fields_ = [("bits", C.c_void_p), ("huff", C.c_void_p), ("coef", C.c_void_p * 3), ("nbytes", C.c_uint32), ("ncomp", C.c_int),
                ("bh", C.c_int * 3), ("bv", C.c_int * 3), ("blocks_w", C.c_int * 3), ("blocks_h", C.c_int * 3), ("dc", C.c_int * 3),
                ("ac", C.c_int * 3), ("units_x", C.c_int), ("units_y", C.c_int), ("first_unit", C.c_int), ("nunits", C.c_int),
                ("nhuff", C.c_int), ("reserved", C.c_int)]


class DnqJpegScanSeg(C.Structure):
    """dnq_jpeg_scan_seg (yolo_quantization_amd/host/jpeg_scan.h)."""
    _fields_ = [("ncomp", C.c_int), ("comp", C.c_int * 3), ("bh", C.c_int * 3), ("bv", C.c_int * 3), ("dc", C.c_int * 3), ("ac", C.c_int * 3),
                ("units_x", C.c_int), ("units_y", C.c_int), ("first_unit", C.c_int), ("nunits", C.c_int), ("scan", C.c_int),
                ("nbytes", C.c_uint32), ("offset", C.c_size_t)]


class DnqJpegScanList(C.Structure):
    """dnq_jpeg_scan_list: what jpeg_scan_host returns beside the headers."""
    _fields_ = [("nsegs", C.c_int), ("nhuff", C.c_int), ("segs", C.POINTER(DnqJpegScanSeg)), ("huff", C.POINTER(JpegHuff)),
                ("bytes", C.POINTER(C.c_uint8)), ("nbytes", C.c_size_t), ("cap_segs", C.c_int), ("cap_huff", C.c_int), ("cap_bytes", C.c_size_t)]


class PngSegment(C.Structure):
    """mi355_png_segment: one pass of one image of mi355_png_unfilter's table (device pointers)."""
    _fields_ = [("filtered", C.c_void_p), ("out", C.c_void_p), ("row_bytes", C.c_int), ("rows", C.c_int), ("bpp", C.c_int),
                ("reserved", C.c_int)]


class PngImage(C.Structure):
    """mi355_png_image: one image of mi355_png_to_rgb's table (device pointers)."""
    _fields_ = [("rgb", C.c_void_p), ("palette", C.c_void_p), ("pass_", C.c_void_p * 7), ("w", C.c_int), ("h", C.c_int),
                ("pitch", C.c_int), ("depth", C.c_int), ("color", C.c_int), ("interlace", C.c_int), ("pal_len", C.c_int),
                ("reserved", C.c_int)]


class DnqPngPass(C.Structure):
    _fields_ = [("w", C.c_int), ("rows", C.c_int), ("row_bytes", C.c_int), ("index", C.c_int), ("offset", C.c_size_t)]


class DnqPng(C.Structure):
    """dnq_png (yolo_quantization_amd/host/png.h): what the host half of the PNG decoder returns."""
    _fields_ = [("w", C.c_int), ("h", C.c_int), ("depth", C.c_int), ("color", C.c_int), ("interlace", C.c_int), ("channels", C.c_int),
                ("bpp", C.c_int), ("pal_len", C.c_int), ("has_trns", C.c_int), ("npasses", C.c_int), ("pass_", DnqPngPass * 7),
                ("palette", C.c_uint8 * 768), ("filtered_bytes", C.c_size_t), ("filtered", C.POINTER(C.c_uint8))]


class PngStream(C.Structure):
    """mi355_png_stream: the deflate stream of one image of mi355_png_inflate's table (device pointers)."""
    _fields_ = [("z", C.c_void_p), ("out", C.c_void_p), ("nbytes", C.c_uint32), ("cap", C.c_uint32), ("npasses", C.c_int),
                ("rows", C.c_int * 7), ("row_bytes", C.c_int * 7), ("reserved", C.c_int)]


class DnqPngScan(C.Structure):
    """dnq_png_scan (yolo_quantization_amd/host/png_scan.h): what png_scan_host returns."""
    _fields_ = [("im", DnqPng), ("z", C.POINTER(C.c_uint8)), ("nbytes", C.c_size_t), ("zcap", C.c_size_t)]


PNG_MAX_DIM = 32768  # DNQ_PNG_MAX_DIM
PNG_INFLATE_ERRORS = {1: "bad block type", 2: "zlib corrupt", 3: "bad codelengths", 4: "bad huffman code", 5: "bad dist",
                      6: "premature end of the zlib data", 7: "read past buffer", 8: "not enough pixels", 9: "invalid filter"}
JPEG_MODES = ("ycbcr", "rgb", "grey")
JPEG_ENTROPY_ERRORS = {1: "bad huffman code", 2: "bad DC category", 3: "coefficient index past the end of the block"}


def shim():
    global _shim
    if _shim is None:
        path = os.path.join(LIB_DIR, "libmi355yolo.so")
        if not os.path.exists(path):
            raise MI355Error(f"{path} is missing: build it with yolo_quantization_amd/csrc/build.sh "
                             "(__graft_entry__.build()); there is no CPU fallback")
        L = C.CDLL(path, mode=C.RTLD_GLOBAL)
        vp, ci, sz = C.c_void_p, C.c_int, C.c_size_t
        L.mi355_last_error.restype = C.c_char_p
        L.mi355_alloc.argtypes = [C.POINTER(vp), sz]
        L.mi355_free.argtypes = [vp]
        L.mi355_memset.argtypes = [vp, ci, sz, vp]
        for n in ("mi355_h2d", "mi355_d2h", "mi355_d2d"):
            getattr(L, n).argtypes = [vp, vp, sz, vp]
        L.mi355_stream_create.argtypes = [C.POINTER(vp)]
        L.mi355_stream_acquire.argtypes = [C.POINTER(vp)]
        L.mi355_stream_release.argtypes = [vp]
        L.mi355_stream_destroy.argtypes = [vp]
        L.mi355_stream_sync.argtypes = [vp]
        L.mi355_event_create.argtypes = [C.POINTER(vp)]
        L.mi355_event_destroy.argtypes = [vp]
        L.mi355_event_record.argtypes = [vp, vp]
        L.mi355_event_elapsed_ms.argtypes = [vp, vp, C.POINTER(C.c_float)]
        L.mi355_graph_begin.argtypes = [vp]
        L.mi355_graph_end.argtypes = [vp, C.POINTER(vp)]
        L.mi355_graph_launch.argtypes = [vp, vp]
        L.mi355_graph_destroy.argtypes = [vp]
        L.mi355_tensor_describe.restype = sz
        L.mi355_tensor_describe.argtypes = [C.POINTER(Tensor), ci, ci, ci, ci]
        L.mi355_tensor_fill.argtypes = [C.POINTER(Tensor), C.c_uint8, vp]
        L.mi355_nchw_to_tensor.argtypes = [vp, C.POINTER(Tensor), vp]
        L.mi355_tensor_to_nchw.argtypes = [C.POINTER(Tensor), vp, vp]
        L.mi355_conv_pack_size.restype = sz
        L.mi355_conv_pack_size.argtypes = [ci, ci, ci]
        L.mi355_conv_pack.argtypes = [ci, ci, ci, vp, vp, vp, vp, vp, vp]
        if hasattr(L, "mi355_conv_pack_epilogue"):  # (absent from older A/B builds under build_ab/; conv_pack(..., activation) then raises)
            L.mi355_conv_pack_epilogue.argtypes = [ci, ci, ci, ci, ci, vp]
        L.mi355_conv_forward.argtypes = [C.POINTER(ConvDesc), C.POINTER(Tensor), vp, vp, vp, C.POINTER(Tensor), vp, vp, vp]
        L.mi355_conv_set_tile.argtypes = [ci, ci]
        L.mi355_conv_pool_forward.argtypes = [C.POINTER(ConvDesc), C.POINTER(Tensor), vp, C.POINTER(Tensor), C.POINTER(Tensor), vp]
        L.mi355_debug_flags.argtypes = [ci]
        L.mi355_last_conv_kernel.argtypes = []
        L.mi355_last_conv_kernel.restype = ci
        if hasattr(L, "mi355_last_conv_launch"):  # (absent from older A/B builds under build_ab/)
            L.mi355_last_conv_launch.argtypes = [C.POINTER(ci), C.POINTER(ci), C.POINTER(ci)]
        L.mi355_conv_shortcut_forward.argtypes = [C.POINTER(ConvDesc), C.POINTER(Tensor), vp, C.POINTER(Tensor), C.POINTER(Tensor),
                                                  C.c_int32, C.c_int32, C.c_uint8, C.c_uint8, vp]
        L.mi355_conv_yolo_forward.argtypes = [C.POINTER(ConvDesc), C.POINTER(Tensor), vp, C.POINTER(Tensor), vp, vp, ci, vp]
        L.mi355_conv_upsample_forward.argtypes = [C.POINTER(ConvDesc), C.POINTER(Tensor), vp, C.POINTER(Tensor), ci, vp]
        L.mi355_maxpool_forward.argtypes = [C.POINTER(Tensor), C.POINTER(Tensor), ci, ci, ci, vp]
        L.mi355_upsample_forward.argtypes = [C.POINTER(Tensor), C.POINTER(Tensor), ci, vp]
        L.mi355_route_forward.argtypes = [C.POINTER(C.POINTER(Tensor)), ci, C.POINTER(Tensor), vp]
        L.mi355_yolo_forward.argtypes = [vp, vp, ci, ci, ci, ci, ci, vp]
        L.mi355_dequant_forward.argtypes = [C.POINTER(Tensor), ci, ci, C.c_uint8, C.c_float, vp, ci, ci, vp]
        L.mi355_shortcut_multiplier.argtypes = [C.c_float, C.c_float, vp]
        L.mi355_shortcut_forward.argtypes = [C.POINTER(Tensor), C.POINTER(Tensor), C.POINTER(Tensor), C.c_int32, C.c_int32,
                                             C.c_uint8, C.c_uint8, C.c_uint8, vp]
        L.mi355_image_minmax.argtypes = [vp, C.c_long, vp, vp]
        L.mi355_letterbox_forward.argtypes = [vp, ci, ci, ci, vp, ci, ci, vp]
        L.mi355_image_quantize.argtypes = [vp, C.c_long, C.c_float, ci, vp, vp]
        L.mi355_image_minmax_batched.argtypes = [vp, ci, C.c_long, vp, vp]
        L.mi355_image_quantize_per_image.argtypes = [vp, ci, C.c_long, vp, vp, vp, vp]
        L.mi355_input_pairs.argtypes = [vp, ci, ci, vp, vp, vp, vp, vp]
        L.mi355_l0_derive.argtypes = [vp, vp, vp, sz, ci, ci, vp, vp, vp, vp, vp, vp]
        L.mi355_conv_forward_per_image.argtypes = [C.POINTER(ConvDesc), C.POINTER(Tensor), vp, C.c_size_t, vp, vp, vp, vp,
                                                   C.POINTER(Tensor), vp, vp, vp]
        L.mi355_conv_pool_forward_per_image.argtypes = [C.POINTER(ConvDesc), C.POINTER(Tensor), vp, C.c_size_t, vp, vp,
                                                        C.POINTER(Tensor), C.POINTER(Tensor), vp]
        if hasattr(L, "mi355_jpeg_idct"):  # MI355_LIB_DIR may name an older build of the libraries (A/B runs): calling them there raises
            L.mi355_jpeg_idct.argtypes = [vp, C.POINTER(JpegPlane), ci, vp]
            L.mi355_jpeg_to_rgb.argtypes = [vp, C.POINTER(JpegImage), ci, vp]
        if hasattr(L, "mi355_png_unfilter"):
            L.mi355_png_unfilter.argtypes = [vp, C.POINTER(PngSegment), ci, vp]
            L.mi355_png_to_rgb.argtypes = [vp, C.POINTER(PngImage), ci, vp]
        if hasattr(L, "mi355_jpeg_entropy"):
            L.mi355_jpeg_entropy.argtypes = [vp, C.POINTER(JpegSegment), ci, ci, vp, vp]
        if hasattr(L, "mi355_png_inflate"):
            L.mi355_png_inflate.argtypes = [vp, C.POINTER(PngStream), ci, vp, vp]
        L.mi355_frames_u8_letterbox_minmax.argtypes = [vp, C.POINTER(FrameU8), ci, ci, ci, vp, vp]
        L.mi355_frames_u8_letterbox_quantize.argtypes = [vp, C.POINTER(FrameU8), ci, ci, ci, vp, vp, vp, vp]
        L.mi355_frames_yuv_letterbox_minmax.argtypes = [vp, C.POINTER(FrameYUV), ci, ci, ci, vp, vp]
        L.mi355_frames_yuv_letterbox_quantize.argtypes = [vp, C.POINTER(FrameYUV), ci, ci, ci, vp, vp, vp, vp]
        L.mi355_frames_planar_letterbox_minmax.argtypes = [vp, C.POINTER(FramePlanar), ci, ci, ci, vp, vp]
        L.mi355_frames_planar_letterbox_quantize.argtypes = [vp, C.POINTER(FramePlanar), ci, ci, ci, vp, vp, vp, vp]
        L.mi355_frames_packed_letterbox_minmax.argtypes = [vp, C.POINTER(FramePacked), ci, ci, ci, vp, vp]
        L.mi355_frames_packed_letterbox_quantize.argtypes = [vp, C.POINTER(FramePacked), ci, ci, ci, vp, vp, vp, vp]
        L.mi355_frames_p010_letterbox_minmax.argtypes = [vp, C.POINTER(FrameP010), ci, ci, ci, vp, vp]
        L.mi355_frames_p010_letterbox_quantize.argtypes = [vp, C.POINTER(FrameP010), ci, ci, ci, vp, vp, vp, vp]
        if hasattr(L, "mi355_frames_bayer_letterbox_minmax"):  # as above: an older build has no Bayer calls
            L.mi355_frames_bayer_letterbox_minmax.argtypes = [vp, C.POINTER(FrameBayer), ci, ci, ci, vp, vp]
            L.mi355_frames_bayer_letterbox_quantize.argtypes = [vp, C.POINTER(FrameBayer), ci, ci, ci, vp, vp, vp, vp]
        for kind, struct in (("u8", FrameU8), ("yuv", FrameYUV), ("planar", FramePlanar), ("packed", FramePacked), ("p010", FrameP010),
                             ("bayer", FrameBayer)):
            pre = [vp, C.POINTER(struct), vp, C.POINTER(FrameView), ci, ci, ci]
            getattr(L, f"mi355_frames_{kind}_view_letterbox_minmax").argtypes = pre + [vp, vp]
            getattr(L, f"mi355_frames_{kind}_view_letterbox_quantize").argtypes = pre + [vp, vp, vp, vp]
        L.mi355_yolo_detections_sizes.argtypes = [vp, ci, ci, ci, ci, ci, vp, vp, ci, ci, vp, vp, C.c_float, ci, vp, ci, vp, vp]
        L.mi355_yolo_detections_batch_work_ints.restype = C.c_long
        L.mi355_yolo_detections_batch_work_ints.argtypes = [C.POINTER(YoloHead), ci, ci]
        L.mi355_yolo_detections_batch.argtypes = [C.POINTER(YoloHead), ci, ci, ci, ci, ci, vp, vp, C.c_float, ci, ci, vp, vp, vp, vp,
                                                  C.c_long, vp]
        _shim = L
    return _shim


def check(rc, what=""):
    if rc != 0:
        raise MI355Error(f"{what}: code {rc}: {shim().mi355_last_error().decode()}")


ABI_VERSION = 6  # include/mi355_yolo_int8.h MI355_ABI_VERSION: the struct mirrors above are this version's


def init(device=0):
    got = shim().mi355_abi_version()
    if got != ABI_VERSION:
        raise MI355Error(f"libmi355yolo.so speaks ABI {got}, binding.py mirrors ABI {ABI_VERSION}")
    check(shim().mi355_init(device), "mi355_init")


# ------------------------------------------------------------------------------------- thin device helpers
class DevBuf:
    """Owned device allocation (shim allocator)."""

    def __init__(self, nbytes):
        self.ptr = C.c_void_p()
        self.nbytes = int(nbytes)
        check(shim().mi355_alloc(C.byref(self.ptr), self.nbytes), "alloc")

    @classmethod
    def from_numpy(cls, a):
        a = np.ascontiguousarray(a)
        b = cls(max(a.nbytes, 16))
        check(shim().mi355_h2d(b.ptr, a.ctypes.data, a.nbytes, None), "h2d")
        check(shim().mi355_stream_sync(None), "sync")
        return b

    def to_numpy(self, dtype, count):
        out = np.empty(count, dtype=dtype)
        check(shim().mi355_stream_sync(None), "sync")
        check(shim().mi355_d2h(out.ctypes.data, self.ptr, out.nbytes, None), "d2h")
        check(shim().mi355_stream_sync(None), "sync")
        return out

    def free(self):
        if self.ptr:
            shim().mi355_free(self.ptr)
            self.ptr = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class DevTensor:
    """PHWC activation tensor on the device."""

    def __init__(self, B, H, W, Cc, zero_point=0):
        self.t = Tensor()
        nbytes = shim().mi355_tensor_describe(C.byref(self.t), B, H, W, Cc)
        if not nbytes:
            raise MI355Error("bad tensor dims")
        self.buf = DevBuf(nbytes)
        self.t.data = self.buf.ptr
        check(shim().mi355_tensor_fill(C.byref(self.t), zero_point, None), "fill")

    @classmethod
    def from_nchw(cls, x, zero_point=0):
        x = np.ascontiguousarray(x, np.uint8)
        B, Cc, H, W = x.shape
        t = cls(B, H, W, Cc, zero_point)
        src = DevBuf.from_numpy(x)
        check(shim().mi355_nchw_to_tensor(src.ptr, C.byref(t.t), None), "nchw_to_tensor")
        check(shim().mi355_stream_sync(None), "sync")
        return t

    def to_nchw(self):
        n = self.t.B * self.t.C * self.t.H * self.t.W
        dst = DevBuf(n)
        check(shim().mi355_tensor_to_nchw(C.byref(self.t), dst.ptr, None), "tensor_to_nchw")
        return dst.to_numpy(np.uint8, n).reshape(self.t.B, self.t.C, self.t.H, self.t.W)

    def ref(self):
        return C.byref(self.t)


def conv_pack(wq, zp_w, c, ksize, biases_int32, M_value, shift_value, activation=None, zp_act=None, pad=None):
    """Host-side packing -> numpy uint8 blob.  With activation / zp_act the blob also gets the conv + maxpool kernels' epilogue
    table (mi355_conv_pack_epilogue); without, those kernels derive the constants per workgroup (same bytes).  The packing
    depends on (n, c, ksize) only: `pad` is accepted for symmetry with conv_forward and not used."""
    wq = np.ascontiguousarray(wq, np.uint8)
    n = wq.shape[0]
    sz = shim().mi355_conv_pack_size(n, c, ksize)
    if not sz:
        raise MI355Error(f"unsupported conv shape n={n} c={c} k={ksize}")
    blob = np.zeros(sz, np.uint8)
    zp_w = np.ascontiguousarray(zp_w, np.uint8)
    b = np.ascontiguousarray(biases_int32, np.int32)
    mv = np.ascontiguousarray(M_value, np.float64)
    sv = np.ascontiguousarray(shift_value, np.float64)
    check(shim().mi355_conv_pack(n, c, ksize, wq.ctypes.data, zp_w.ctypes.data, b.ctypes.data, mv.ctypes.data,
                                 sv.ctypes.data, blob.ctypes.data), "conv_pack")
    if activation is not None:
        check(shim().mi355_conv_pack_epilogue(n, c, ksize, int(activation), int(zp_act), blob.ctypes.data), "conv_pack_epilogue")
    return blob


def last_conv_kernel():
    """mi355_last_conv_kernel: the kernel family that served this thread's most recent conv call"""
    return int(shim().mi355_last_conv_kernel())


def last_conv_launch():
    """mi355_last_conv_launch: (workgroups, threads per workgroup, dynamic LDS bytes) of this thread's most recent conv kernel launch"""
    g, t, l = C.c_int(), C.c_int(), C.c_int()
    shim().mi355_last_conv_launch(C.byref(g), C.byref(t), C.byref(l))
    return g.value, t.value, l.value


def _pack_blob(wq, zp_w, c, ksize, biases_int32, M_value, shift_value, activation, zp_act, epilogue):
    """device blob; epilogue=True adds the epilogue table for (activation, zp_act), as the darknet host always does"""
    ept = (activation, zp_act) if epilogue else ()
    return DevBuf.from_numpy(conv_pack(wq, zp_w, c, ksize, biases_int32, M_value, shift_value, *ept))


def conv_forward(x: DevTensor, wq, zp_w, ksize, biases_int32, M_value, shift_value, zp_in, zp_act, s_act,
                 activation, store=STORE_WRAP, accum=ACC_EXACT, want_acc=True, want_f32=False, stride=1, pad=None,
                 plan=0, epilogue=False):
    """One quantized conv layer through the C-ABI. Returns dict(u8 NCHW, int32 [B,n,HW], f32).  pad=None: ksize // 2.
    plan: mi355_conv_desc.plan (0 latency, 1 throughput).  epilogue: pack the blob's epilogue table for (activation, zp_act)
    and set desc.epilogue_packed, as the darknet host does (host/layers.c)."""
    n = wq.shape[0]
    c = x.t.C
    blob = _pack_blob(wq, zp_w, c, ksize, biases_int32, M_value, shift_value, activation, zp_act, epilogue)
    wraw = DevBuf.from_numpy(np.ascontiguousarray(wq, np.uint8))
    zraw = DevBuf.from_numpy(np.ascontiguousarray(zp_w, np.uint8))
    if pad is None:
        pad = ksize // 2
    OH, OW = (x.t.H + 2 * pad - ksize) // stride + 1, (x.t.W + 2 * pad - ksize) // stride + 1
    y = DevTensor(x.t.B, OH, OW, n, zp_act)
    cnt = x.t.B * n * OH * OW
    acc = DevBuf(cnt * 4) if want_acc else None
    f32 = DevBuf(cnt * 4) if want_f32 else None
    d = ConvDesc(n, c, ksize, stride, pad, activation, store, accum, zp_in, zp_act, float(s_act), int(plan), int(bool(epilogue)))
    check(shim().mi355_conv_forward(C.byref(d), x.ref(), blob.ptr, wraw.ptr, zraw.ptr, y.ref(),
                                    acc.ptr if acc else None, f32.ptr if f32 else None, None), "conv_forward")
    check(shim().mi355_stream_sync(None), "sync")
    out = {"u8": y.to_nchw(), "tensor": y}
    if acc:
        out["int32"] = acc.to_numpy(np.int32, cnt).reshape(x.t.B, n, OH * OW)
    if f32:
        out["f32"] = f32.to_numpy(np.float32, cnt).reshape(x.t.B, n, OH * OW)
    return out


FUSED = ("pool2", "pool1", "upsample", "yolo", "shortcut")


def conv_fused_forward(x: DevTensor, wq, zp_w, ksize, biases_int32, M_value, shift_value, zp_in, zp_act, s_act, activation, fuse,
                       store=STORE_WRAP, plan=0, epilogue=False, keep_y=False, classes=80, up=2, res=None, Ka=0, Kb=0,
                       zp_from=0, zp_out=0):
    """A conv fused with the layer after it, through the C-ABI entry point the darknet host uses for it (stride 1, pad ksize // 2):
      pool2     2x2 / stride-2 maxpool (mi355_conv_pool_forward, pooled map)        -> out["u8"] = the pooled tensor
      pool1     2x2 / stride-1 maxpool (mi355_conv_pool_forward, the conv's map)    -> out["u8"] = the pooled tensor
      upsample  nearest x `up` (mi355_conv_upsample_forward)                        -> out["u8"] = the upsampled tensor
      yolo      quant_stop head + yolo layer (mi355_conv_yolo_forward, `classes`)   -> out["u8"], out["f32"], out["yolo"]
      shortcut  quantized residual add of DevTensor `res` (mi355_conv_shortcut_forward, Ka, Kb, zp_from, zp_out) -> out["u8"] = the sum
    keep_y (pools): the conv's own tensor is stored as well, out["y"].  plan / epilogue as in conv_forward.  A refused call raises
    MI355Error (code -22)."""
    assert fuse in FUSED, fuse
    n = wq.shape[0]
    c = x.t.C
    B, H, W = x.t.B, x.t.H, x.t.W
    blob = _pack_blob(wq, zp_w, c, ksize, biases_int32, M_value, shift_value, activation, zp_act, epilogue)
    d = ConvDesc(n, c, ksize, 1, ksize // 2, activation, store, ACC_EXACT, zp_in, zp_act, float(s_act), int(plan), int(bool(epilogue)))
    S = shim()
    out = {}
    if fuse in ("pool2", "pool1"):
        y = DevTensor(B, H, W, n, zp_act) if keep_y else None
        yp = DevTensor(B, H // 2, W // 2, n, zp_act) if fuse == "pool2" else DevTensor(B, H, W, n, zp_act)
        check(S.mi355_conv_pool_forward(C.byref(d), x.ref(), blob.ptr, y.ref() if y else None, yp.ref(), None), "conv_pool_forward")
        res_t = yp
        if y:
            out["y"] = y.to_nchw()
    elif fuse == "upsample":
        res_t = DevTensor(B, H * up, W * up, n, zp_act)
        check(S.mi355_conv_upsample_forward(C.byref(d), x.ref(), blob.ptr, res_t.ref(), up, None), "conv_upsample_forward")
    elif fuse == "yolo":
        res_t = DevTensor(B, H, W, n, zp_act)
        cnt = B * n * H * W
        f32, yo = DevBuf(cnt * 4), DevBuf(cnt * 4)
        check(S.mi355_conv_yolo_forward(C.byref(d), x.ref(), blob.ptr, res_t.ref(), f32.ptr, yo.ptr, classes, None), "conv_yolo_forward")
        out["f32"] = f32.to_numpy(np.float32, cnt).reshape(B, n, H * W)
        out["yolo"] = yo.to_numpy(np.float32, cnt).reshape(B, n, H * W)
    else:
        res_t = DevTensor(B, H, W, n, zp_out)
        check(S.mi355_conv_shortcut_forward(C.byref(d), x.ref(), blob.ptr, res.ref(), res_t.ref(), int(Ka), int(Kb), int(zp_from),
                                            int(zp_out), None), "conv_shortcut_forward")
    check(S.mi355_stream_sync(None), "sync")
    out["u8"] = res_t.to_nchw()
    out["tensor"] = res_t
    return out


# ------------------------------------------------------------------------------------------- darknet host
def host():
    global _host
    if _host is None:
        shim()  # resolve the dependency first, RTLD_GLOBAL
        path = os.path.join(LIB_DIR, "libdarknet_q.so")
        if not os.path.exists(path):
            raise MI355Error(f"{path} is missing: run `make -C yolo_quantization_amd/host`")
        L = C.CDLL(path)
        vp, ci = C.c_void_p, C.c_int
        L.load_network.restype = vp
        L.load_network.argtypes = [C.c_char_p, C.c_char_p, ci]
        L.parse_network_cfg.restype = vp
        L.parse_network_cfg.argtypes = [C.c_char_p, ci]
        L.set_batch_network.argtypes = [vp, ci]
        L.network_replica.restype = vp
        L.network_replica.argtypes = [vp]
        L.free_network.argtypes = [vp]
        L.quantization_weights_and_activations.argtypes = [vp]
        L.quantization_weights_and_activations_fixed_input.argtypes = [vp, C.c_float, C.c_uint8]
        L.quantization_weights_and_activations_gpu.argtypes = [vp, vp]
        L.network_letterbox_input_gpu.argtypes = [vp, ci, vp, ci, ci]
        L.network_quantize_input_gpu.argtypes = [vp]
        L.network_frames_u8_input_gpu.argtypes = [vp, C.POINTER(vp), C.POINTER(ci), C.POINTER(ci), C.POINTER(ci), ci, ci]
        L.network_frames_nv12_input_gpu.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(ci), C.POINTER(ci), C.POINTER(ci),
                                                    C.POINTER(ci), ci, ci, ci]
        L.network_frames_planar_input_gpu.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(ci), C.POINTER(ci),
                                                      C.POINTER(ci), C.POINTER(ci), C.POINTER(ci), ci, ci, ci]
        L.network_frames_packed_input_gpu.argtypes = [vp, C.POINTER(vp), C.POINTER(ci), C.POINTER(ci), C.POINTER(ci), ci, ci, ci]
        L.network_frames_p010_input_gpu.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(ci), C.POINTER(ci), C.POINTER(ci),
                                                    C.POINTER(ci), ci, ci]
        if hasattr(L, "jpeg_decode_host"):  # as above: an older build has no JPEG entry points
            L.jpeg_decode_host.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(DnqJpeg), C.c_char_p, C.c_size_t]
            L.jpeg_info_host.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(DnqJpeg), C.c_char_p, C.c_size_t]
            L.jpeg_free.argtypes = [C.POINTER(DnqJpeg)]
            L.jpeg_free.restype = None
            L.network_jpeg_decode_gpu.argtypes = [vp, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), ci, C.POINTER(vp), C.POINTER(ci),
                                                  C.POINTER(ci), C.POINTER(ci)]
            L.network_frames_jpeg_input_gpu.argtypes = [vp, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.POINTER(ci), C.POINTER(ci)]
            L.network_jpeg_last_error.restype = C.c_char_p
        if hasattr(L, "png_decode_host"):
            L.png_decode_host.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(DnqPng), C.c_char_p, C.c_size_t]
            L.png_info_host.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(DnqPng), C.c_char_p, C.c_size_t]
            L.png_free.argtypes = [C.POINTER(DnqPng)]
            L.png_free.restype = None
            L.png_inflate_host.argtypes = [C.c_char_p, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_size_t), C.c_char_p, C.c_size_t]
            L.network_png_decode_gpu.argtypes = [vp, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), ci, C.POINTER(vp), C.POINTER(ci),
                                                 C.POINTER(ci), C.POINTER(ci)]
            L.network_frames_png_input_gpu.argtypes = [vp, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.POINTER(ci), C.POINTER(ci)]
            L.network_png_last_error.restype = C.c_char_p
        if hasattr(L, "jpeg_scan_host"):
            L.jpeg_scan_host.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(DnqJpeg), C.POINTER(DnqJpegScanList), C.c_char_p, C.c_size_t]
            L.jpeg_scan_free.argtypes = [C.POINTER(DnqJpegScanList)]
            L.jpeg_scan_free.restype = None
            L.jpeg_entropy_emulate_host.argtypes = [C.POINTER(JpegSegment), ci, ci, C.POINTER(ci), C.POINTER(ci)]
            L.set_jpeg_entropy_on_device.argtypes = [vp, ci]
            L.set_jpeg_entropy_on_device.restype = None
            L.set_jpeg_entropy_subseq_bits.argtypes = [vp, ci]
            L.set_jpeg_entropy_subseq_bits.restype = None
        if hasattr(L, "png_scan_host"):
            L.png_scan_host.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(DnqPngScan), C.c_char_p, C.c_size_t]
            L.png_scan_free.argtypes = [C.POINTER(DnqPngScan)]
            L.png_scan_free.restype = None
            L.png_inflate_emulate_host.argtypes = [C.POINTER(PngStream), ci, C.POINTER(ci)]
            L.png_inflate_emulate_why.restype = C.c_char_p
            L.png_inflate_reason.argtypes = [ci]
            L.png_inflate_reason.restype = C.c_char_p
            L.set_png_inflate_on_device.argtypes = [vp, ci]
            L.set_png_inflate_on_device.restype = None
        if hasattr(L, "network_frames_bayer_input_gpu"):  # as above
            L.network_frames_bayer_input_gpu.argtypes = [vp, C.POINTER(vp), C.POINTER(ci), C.POINTER(ci), C.POINTER(ci), ci, ci, ci,
                                                         C.POINTER(vp), ci]
        L.quantization_prep_host.argtypes = [vp, C.c_float, C.c_uint8]
        L.forward_network_gpu.argtypes = [vp]
        L.network_predict.restype = vp
        L.network_predict.argtypes = [vp, vp]
        L.push_network_input_uint8.argtypes = [vp, vp]
        L.pull_layer_output.argtypes = [vp, ci]
        L.network_profile_begin.argtypes = [vp, ci]
        L.network_profile_read.argtypes = [vp, vp]
        L.network_yolo_detections_gpu.argtypes = [vp, ci, ci, ci, C.c_float, ci, vp, ci, vp]
        L.network_profile_set_stride.argtypes = [vp, ci]
        L.network_profile_set_phase.argtypes = [vp, ci]
        L.network_selfcheck.argtypes = [vp, ci]
        L.network_selfcheck_result.argtypes = [vp]
        L.network_packed_size.restype = C.c_size_t
        L.network_packed_size.argtypes = [vp]
        L.network_export_packed.argtypes = [vp, vp]
        L.network_import_packed.argtypes = [vp, vp, C.c_size_t]
        L.network_import_packed_gpu.argtypes = [vp, vp, C.c_size_t]
        L.network_import_packed_host.argtypes = [vp, vp, C.c_size_t]
        L.quant_multi_smaller_than_one_to_scale_and_shift.argtypes = [C.c_float, vp, vp]
        L.quant_image_with_min_max.argtypes = [ci, vp, vp, vp, vp]
        for n in ("dnq_net_n", "dnq_net_batch", "dnq_net_inputs"):
            getattr(L, n).argtypes = [vp]
        for n in ("dnq_net_stream", "dnq_net_input_gpu", "dnq_net_input_host", "dnq_net_input_float"):
            getattr(L, n).restype = vp
            getattr(L, n).argtypes = [vp]
        L.dnq_net_set.argtypes = [vp, C.c_char_p, ci]
        L.dnq_layer_info.argtypes = [vp, ci, vp]
        for n in ("dnq_layer_u8", "dnq_layer_int32", "dnq_layer_f32", "dnq_layer_f32_gpu"):
            getattr(L, n).restype = vp
            getattr(L, n).argtypes = [vp, ci]
        L.dnq_layer_prep.argtypes = [vp, ci] + [vp] * 6
        L.dnq_layer_is_fused.argtypes = [vp, ci]
        L.dnq_layer_fuses_next.argtypes = [vp, ci]
        L.dnq_layer_shortcut.argtypes = [vp, ci, vp]
        L.dnq_layer_plan.argtypes = [vp, ci, vp]
        L.network_save_packed.argtypes = [vp, C.c_char_p]
        L.network_load_packed.argtypes = [vp, C.c_char_p]
        L.dnq_layer_conv_kernel.argtypes = [vp, ci]
        L.dnq_layer_conv_kernel.restype = ci
        L.set_input_quantization_per_image.argtypes = [vp, ci]
        L.set_input_quantization_per_image.restype = ci
        L.network_input_quantization.argtypes = [vp, vp, vp]
        L.network_yolo_detections_gpu_sizes.argtypes = [vp, ci, vp, vp, C.c_float, ci, vp, ci, vp]
        L.dnq_net_pi_packed.argtypes = [vp]
        L.dnq_net_pi_entry_bytes.argtypes = [vp]
        L.dnq_net_pi_entry_bytes.restype = C.c_long
        L.network_layer0_entry.argtypes = [vp, C.c_float, C.c_uint8, vp]
        L.set_input_quantization_on_device.argtypes = [vp, ci]
        L.set_input_quantization_on_device.restype = ci
        L.network_input_status.argtypes = [vp, vp]
        L.network_input_status.restype = ci
        L.network_input_bank_entry.argtypes = [vp, ci, vp]
        L.network_host_waits.argtypes = [vp]
        L.network_host_waits.restype = C.c_long
        L.network_layer0_consts.argtypes = [vp, vp]
        L.network_layer0_consts.restype = C.c_size_t
        L.dnq_net_graph.argtypes = [vp]
        L.dnq_net_graph.restype = vp
        L.dnq_net_detb_counts.argtypes = [vp]
        L.dnq_net_detb_counts.restype = vp
        L.network_detections_batch_shape.argtypes = [vp, C.POINTER(ci), C.POINTER(ci), C.POINTER(ci)]
        L.network_yolo_detections_batch_gpu.argtypes = [vp, vp, vp, C.c_float, ci, ci, vp, vp, vp]
        L.network_detections_batch.argtypes = [vp, vp, vp, C.c_float, ci, C.c_float, ci, C.POINTER(vp), C.POINTER(ci)]
        L.free_detections_batch.argtypes = [C.POINTER(vp), C.POINTER(ci), ci]
        L.detections_from_records.argtypes = [vp, vp, ci, ci, C.c_float, C.POINTER(vp), C.POINTER(ci)]
        L.detections_to_arrays.argtypes = [vp, ci, ci, vp, vp, vp]
        L.do_nms_sort_arrays.argtypes = [vp, vp, vp, ci, ci, C.c_float]
        L.network_set_frame_views.argtypes = [vp, C.POINTER(FrameView)]
        L.network_set_frame_views.restype = None
        L.network_tile_views.argtypes = [ci, ci, ci, ci, ci, ci, C.POINTER(FrameView)]
        L.network_view_box_to_frame.argtypes = [C.POINTER(FrameView), ci, ci, C.POINTER(Box)]
        L.network_view_box_to_frame.restype = None
        L.network_detections_views.argtypes = [vp, vp, vp, vp, C.c_float, C.c_float, ci, C.POINTER(vp), C.POINTER(ci)]
        L.detections_views_merge.argtypes = [C.POINTER(vp), C.POINTER(ci), ci, C.POINTER(FrameView), vp, vp, vp, ci, C.c_float,
                                             C.POINTER(vp), C.POINTER(ci)]
        L.jpeg_exif_orientation_host.argtypes = [C.c_char_p, C.c_size_t]
        _host = L
    return _host


INFO_KEYS = ["type", "out_c", "out_h", "out_w", "c", "h", "w", "n", "size", "stride", "pad", "activation",
             "batch_normalize", "quantized", "quant_stop", "outputs"]
PLAN_KEYS = ["route_elided", "out_view", "view_offset", "fuse_next_pool", "fuse_next_upsample", "fuse_next_shortcut", "fuse_next_yolo",
             "fuse_pool_keep"]
T_CONV, T_MAXPOOL, T_ROUTE, T_SHORTCUT, T_YOLO, T_UPSAMPLE = 0, 3, 8, 13, 23, 26


def frame_view(v, frame_w=None, frame_h=None):
    """FrameView of `v`: a FrameView, an (x0, y0, w, h, orient) tuple, or None -- the whole frame_w x frame_h frame, orient 1"""
    if isinstance(v, FrameView):
        return v
    if v is None:
        v = (0, 0, frame_w, frame_h, 1)
    x0, y0, w, h, orient = (int(t) for t in v)
    return FrameView(x0, y0, w, h, orient, (C.c_int * 3)(0, 0, 0))


def tile_views(frame_w, frame_h, cols, rows, overlap=0, orient=1):
    """network_tile_views: cols * rows (x0, y0, w, h, orient) tuples that cover the frame, row by row"""
    n = max(int(cols), 0) * max(int(rows), 0)
    out = (FrameView * max(n, 1))()
    rc = host().network_tile_views(int(frame_w), int(frame_h), int(cols), int(rows), int(overlap), int(orient), out)
    if rc < 0:
        raise ValueError(f"network_tile_views refuses {cols} x {rows} tiles with overlap {overlap}, orient {orient} of a {frame_w} x {frame_h} frame")
    return [(v.x0, v.y0, v.w, v.h, v.orient) for v in out[:rc]]


def view_box_to_frame(view, frame_w, frame_h, box):
    """network_view_box_to_frame: (x, y, w, h) relative to the view (its oriented size) -> relative to the frame, float32 values"""
    b = Box(*(float(t) for t in box))
    host().network_view_box_to_frame(C.byref(frame_view(view, frame_w, frame_h)), int(frame_w), int(frame_h), C.byref(b))
    return np.array([b.x, b.y, b.w, b.h], np.float32)


def jpeg_exif_orientation(data):
    """jpeg_exif_orientation_host: the EXIF orientation 1..8 of a JPEG file's bytes; 1 when there is none to be read"""
    data = bytes(data)
    return int(host().jpeg_exif_orientation_host(data, len(data)))


def _as(ptr, n, dt):
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(dt)), shape=(n,))


def _byte_rows(a, keep):
    """(address, pitch) of a uint8 array [rows][...]: its row stride serves as the pitch where a row's bytes are contiguous and the stride
    is at least the row, anything else is copied first.  `keep` keeps what the address points into alive over the call."""
    if not a[:1].flags["C_CONTIGUOUS"] or a.strides[0] < a[:1].size:
        a = np.ascontiguousarray(a)
    keep.append(a)
    return a.ctypes.data, a.strides[0]


def _sample_rows(f, sample_bytes, inner, keep, what):
    """(address, pitch in bytes, shape, on_device) of a frame plane [rows][...] + inner of `sample_bytes`-byte samples: a host array
    (through _byte_rows, as bytes) or a device tensor (anything with data_ptr(), shape, stride() and element_size(), as a torch
    tensor has; its samples must be contiguous inside a row, rows may be padded; where it has a dtype, that must be the unsigned
    integer of the sample's size, as a host array's)."""
    if hasattr(f, "data_ptr"):
        shape = tuple(f.shape)
        nd = len(shape)
        want = 1
        dtype = str(getattr(f, "dtype", "")).rsplit(".", 1)[-1]  # "torch.uint8" -> "uint8"
        ok = f.element_size() == sample_bytes and nd >= 2 and shape[nd - len(inner):] == inner and dtype in ("", f"uint{8 * sample_bytes}")
        for k in range(nd - 1, 0, -1):  # strides are in samples
            ok = ok and f.stride(k) == want
            want *= shape[k]
        if not ok or f.stride(0) < want:
            raise ValueError(f"{what}: a device tensor must hold uint{8 * sample_bytes} samples, contiguous inside its rows")
        return f.data_ptr(), f.stride(0) * sample_bytes, shape, True
    a = np.asarray(f)
    if a.dtype.itemsize != sample_bytes or a.dtype.kind != "u" or a.ndim < 2 or a.shape[a.ndim - len(inner):] != inner:
        raise ValueError(f"{what}: a plane must be an array of uint{8 * sample_bytes}")
    if sample_bytes > 1:
        a = a.astype(a.dtype.newbyteorder("<"), copy=False)  # little-endian samples (a no-op on little-endian hosts)
        if a.strides[-1] != sample_bytes:
            a = np.ascontiguousarray(a)
        a = a.view(np.uint8)
    ptr, pitch = _byte_rows(a, keep)
    return ptr, pitch, tuple(np.asarray(f).shape), False


class JpegError(ValueError):
    """A JPEG the decoder refuses; the message is the decoder's (with "jpeg slot <b>: " in front where a batch was decoded)."""


def _jpeg_bytes(item):
    """bytes of an item that is bytes-like or a path"""
    if isinstance(item, (bytes, bytearray, memoryview)):
        return bytes(item)
    with open(item, "rb") as f:
        return f.read()


def _jpeg_host(data, headers_only):
    j = DnqJpeg()
    err = C.create_string_buffer(256)
    fn = host().jpeg_info_host if headers_only else host().jpeg_decode_host
    if fn(data, len(data), C.byref(j), err, len(err)) != 0:
        raise JpegError(err.value.decode())
    return j


def _jpeg_dict(j):
    return {"w": j.w, "h": j.h, "ncomp": j.ncomp, "mode": JPEG_MODES[j.mode], "h_max": j.h_max, "v_max": j.v_max, "sof": j.sof,
            "jfif": bool(j.jfif), "adobe_transform": j.adobe_transform, "restart_interval": j.restart_interval, "nscans": j.nscans,
            "components": [{k: getattr(j.comp[i], k) for k in ("id", "h", "v", "hs", "vs", "w", "rows", "blocks_w", "blocks_h", "tq")}
                           for i in range(j.ncomp)]}


def jpeg_info(data):
    """The headers of a JPEG (bytes or a path) as a dict: size, components with their sampling factors and plane sizes, colour mode
    ("ycbcr" | "rgb" | "grey").  Host only; raises JpegError with the decoder's message for a file it refuses."""
    j = _jpeg_host(_jpeg_bytes(data), True)
    d = _jpeg_dict(j)
    del d["nscans"]
    return d


def jpeg_coefficients(data):
    """The host half of the decoder on a JPEG (bytes or a path): jpeg_info's dict, plus per component "coef", int16
    [blocks_h][blocks_w][64] quantised coefficients in natural order, and "quant", uint16 [64], the table its scan was decoded with.
    Host only."""
    j = _jpeg_host(_jpeg_bytes(data), False)
    try:
        d = _jpeg_dict(j)
        for i, c in enumerate(d["components"]):
            n = c["blocks_w"] * c["blocks_h"] * 64
            c["coef"] = np.ctypeslib.as_array(j.comp[i].coef, shape=(n,)).reshape(c["blocks_h"], c["blocks_w"], 64).copy()
            c["quant"] = np.array(j.comp[i].quant, np.uint16)
        return d
    finally:
        host().jpeg_free(C.byref(j))


def jpeg_scan(data):
    """jpeg_scan_host on a JPEG (bytes or a path): jpeg_coefficients' dict without "coef" (the same headers, "quant" included), plus
    "segments", one dict per restart interval of every scan -- "ncomp", "comp", "bh", "bv", "dc", "ac" (lists in scan order), the unit
    grid, "first_unit", "nunits", "scan" and "data", the segment's unstuffed bytes -- and "huff", the JpegHuff tables "dc" / "ac" index.
    Host only."""
    data = _jpeg_bytes(data)
    j, sl = DnqJpeg(), DnqJpegScanList()
    err = C.create_string_buffer(256)
    if host().jpeg_scan_host(data, len(data), C.byref(j), C.byref(sl), err, len(err)) != 0:
        raise JpegError(err.value.decode())
    try:
        d = _jpeg_dict(j)
        for i, c in enumerate(d["components"]):
            c["quant"] = np.array(j.comp[i].quant, np.uint16)
        raw = bytes(np.ctypeslib.as_array(sl.bytes, shape=(sl.nbytes,))) if sl.nbytes else b""
        d["segments"] = []
        for i in range(sl.nsegs):
            g = sl.segs[i]
            assert g.offset % 4 == 0 and not any(raw[g.offset + g.nbytes:g.offset + ((g.nbytes + 3) & ~3) + 8])
            seg = {k: list(getattr(g, k))[:g.ncomp] for k in ("comp", "bh", "bv", "dc", "ac")}
            seg.update({k: getattr(g, k) for k in ("ncomp", "units_x", "units_y", "first_unit", "nunits", "scan")})
            seg["data"] = raw[g.offset:g.offset + g.nbytes]
            d["segments"].append(seg)
        d["huff"] = [JpegHuff.from_buffer_copy(sl.huff[i]) for i in range(sl.nhuff)]
        return d
    finally:
        host().jpeg_scan_free(C.byref(sl))


class JpegEntropyJob:
    """Every segment of every item (a JPEG, or a jpeg_scan dict) in one mi355_jpeg_segment table: device buffers and device pointers,
    or, with emulate, numpy arrays and host pointers for jpeg_entropy_emulate_host.  run() is one call for all of them."""

    def __init__(self, items, emulate=False):
        self.emulate = emulate
        self.scans = scans = [it if isinstance(it, dict) else jpeg_scan(it) for it in items]
        self.nseg = nseg = sum(len(d["segments"]) for d in scans)
        self.table = table = (JpegSegment * max(nseg, 1))()
        huffs = [h for d in scans for h in d["huff"]]
        huff_np = np.frombuffer(b"".join(bytes(h) for h in huffs), np.uint8).copy() if huffs else np.zeros(C.sizeof(JpegHuff), np.uint8)
        chunks = [g["data"] + bytes(((len(g["data"]) + 3) & ~3) + 8 - len(g["data"])) for d in scans for g in d["segments"]]
        bits_np = np.frombuffer(b"".join(chunks), np.uint8).copy() if chunks else np.zeros(8, np.uint8)
        self.stream_bytes, self.huff_bytes = int(bits_np.nbytes), int(huff_np.nbytes)
        self.planes = [[np.zeros((c["blocks_h"], c["blocks_w"], 64), np.int16) for c in d["components"]] for d in scans]
        self.keep, self.plane_bufs = [huff_np, bits_np], []
        if emulate:
            huff_ptr, bits_ptr = huff_np.ctypes.data, bits_np.ctypes.data
            plane_ptr = [[a.ctypes.data for a in per] for per in self.planes]
        else:
            hb, bb = DevBuf.from_numpy(huff_np), DevBuf.from_numpy(bits_np)
            self.plane_bufs = [[DevBuf.from_numpy(a.ravel()) for a in per] for per in self.planes]  # zero: only non-zeros are stored
            self.keep += [hb, bb] + [b for bufs in self.plane_bufs for b in bufs]
            huff_ptr, bits_ptr = hb.ptr.value, bb.ptr.value
            plane_ptr = [[b.ptr.value for b in bufs] for bufs in self.plane_bufs]
        i, at, huff_at = 0, 0, 0
        for n, d in enumerate(scans):
            for g in d["segments"]:
                t = table[i]
                t.bits, t.huff, t.nbytes, t.ncomp, t.nhuff = bits_ptr + at, huff_ptr, len(g["data"]), g["ncomp"], len(huffs)
                for c in range(g["ncomp"]):
                    comp = d["components"][g["comp"][c]]
                    t.coef[c] = plane_ptr[n][g["comp"][c]]
                    t.bh[c], t.bv[c], t.blocks_w[c], t.blocks_h[c] = g["bh"][c], g["bv"][c], comp["blocks_w"], comp["blocks_h"]
                    t.dc[c], t.ac[c] = huff_at + g["dc"][c], huff_at + g["ac"][c]
                t.units_x, t.units_y, t.first_unit, t.nunits = g["units_x"], g["units_y"], g["first_unit"], g["nunits"]
                at += ((len(g["data"]) + 3) & ~3) + 8
                i += 1
            huff_at += len(d["huff"])
        self.status, self.steps = (C.c_int * max(nseg, 1))(), (C.c_int * max(nseg, 1))()
        if not emulate:
            self.tdev, self.sdev = DevBuf.from_numpy(np.frombuffer(bytes(table), np.uint8)), DevBuf(4 * max(nseg, 1))
            self.keep += [self.tdev, self.sdev]

    def launch(self, subseq_bits):
        """mi355_jpeg_entropy on the default stream; the return code"""
        return shim().mi355_jpeg_entropy(self.tdev.ptr, self.table, self.nseg, subseq_bits, self.sdev.ptr, None)

    def run(self, subseq_bits):
        """(planes, status per item, settle steps per item | None)"""
        if self.emulate:
            if host().jpeg_entropy_emulate_host(self.table, self.nseg, subseq_bits, self.status, self.steps) != 0:
                raise MI355Error("jpeg_entropy_emulate_host refused its arguments")
        else:
            check(self.launch(subseq_bits), "mi355_jpeg_entropy")
            check(shim().mi355_stream_sync(None), "sync")
            st = self.sdev.to_numpy(np.int32, max(self.nseg, 1))
            for k in range(self.nseg):
                self.status[k] = int(st[k])
            for per, bufs in zip(self.planes, self.plane_bufs):
                for a, b in zip(per, bufs):
                    a[...] = b.to_numpy(np.int16, a.size).reshape(a.shape)
        out_status, out_steps, i = [], [], 0
        for d in self.scans:
            k = len(d["segments"])
            out_status.append([self.status[i + x] for x in range(k)])
            out_steps.append([self.steps[i + x] for x in range(k)])
            i += k
        return self.planes, out_status, (out_steps if self.emulate else None)

    def free(self):
        for b in self.keep:
            if isinstance(b, DevBuf):
                b.free()
        self.keep = []


def _jpeg_entropy_run(items, subseq_bits, emulate):
    job = JpegEntropyJob(items, emulate)
    try:
        return job.run(subseq_bits)
    finally:
        job.free()


def jpeg_entropy(items, subseq_bits=1024, emulate=False):
    """mi355_jpeg_entropy on every segment of every item (JPEG bytes, a path, or a jpeg_scan dict) in ONE launch, or, with emulate,
    jpeg_entropy_emulate_host (no device).  Returns (coef, status): per item, the int16 [blocks_h][blocks_w][64] planes of its
    components (jpeg_coefficients' "coef") and the status word of each of its segments."""
    planes, status, _ = _jpeg_entropy_run(list(items), subseq_bits, emulate)
    return planes, status


def jpeg_entropy_steps(items, subseq_bits=1024):
    """Per item, per segment: the settle steps of the segment's slowest round (jpeg_entropy_emulate_host; no device)."""
    return _jpeg_entropy_run(list(items), subseq_bits, True)[2]


def jpeg_idct(planes):
    """mi355_jpeg_idct on built inputs: planes is a list of (coef int16 [blocks_h][blocks_w][64], quant uint16 [64]); one launch for
    all of them.  Returns the uint8 planes [8 * blocks_h][8 * blocks_w]."""
    L = shim()
    table = (JpegPlane * len(planes))()
    keep, first = [], 0
    for i, (coef, quant) in enumerate(planes):
        coef = np.ascontiguousarray(coef, np.int16)
        bh, bw = coef.shape[:2]
        bufs = (DevBuf.from_numpy(coef), DevBuf.from_numpy(np.ascontiguousarray(quant, np.uint16)), DevBuf(64 * bh * bw))
        keep.append(bufs)
        table[i].coef, table[i].quant, table[i].out = bufs[0].ptr, bufs[1].ptr, bufs[2].ptr
        table[i].blocks_w, table[i].blocks_h, table[i].first_block = bw, bh, first
        first += bw * bh
    tdev = DevBuf.from_numpy(np.frombuffer(bytes(table), np.uint8))
    check(L.mi355_jpeg_idct(tdev.ptr, table, len(planes), None), "mi355_jpeg_idct")
    check(L.mi355_stream_sync(None), "sync")
    out = [b[2].to_numpy(np.uint8, 64 * table[i].blocks_h * table[i].blocks_w).reshape(8 * table[i].blocks_h, 8 * table[i].blocks_w)
           for i, b in enumerate(keep)]
    for bufs in keep:
        for b in bufs:
            b.free()
    tdev.free()
    return out


def jpeg_to_rgb(images, pitch_pad=0):
    """mi355_jpeg_to_rgb on built inputs: images is a list of dicts {"w", "h", "mode" ("ycbcr" | "rgb" | "grey"), "components":
    [{"plane": uint8 [rows][pitch], "hs", "vs", "rows" (default: the plane's)}]}; one launch for all of them.  pitch_pad: bytes added
    to every output row's 3 * w.  Returns uint8 [h][w][3] per image; the pad bytes must come back as they were (0xA5)."""
    L = shim()
    table = (JpegImage * len(images))()
    keep = []
    for i, im in enumerate(images):
        w, h = im["w"], im["h"]
        pitch = 3 * w + pitch_pad
        out = DevBuf.from_numpy(np.full(h * pitch, 0xA5, np.uint8))
        bufs = [out]
        table[i].rgb, table[i].w, table[i].h, table[i].pitch, table[i].mode = out.ptr, w, h, pitch, JPEG_MODES.index(im["mode"])
        for k, c in enumerate(im["components"]):
            plane = np.ascontiguousarray(c["plane"], np.uint8)
            b = DevBuf.from_numpy(plane)
            bufs.append(b)
            table[i].comp[k].plane, table[i].comp[k].pitch = b.ptr, plane.shape[1]
            table[i].comp[k].rows, table[i].comp[k].hs, table[i].comp[k].vs = c.get("rows", plane.shape[0]), c["hs"], c["vs"]
        keep.append(bufs)
    tdev = DevBuf.from_numpy(np.frombuffer(bytes(table), np.uint8))
    check(L.mi355_jpeg_to_rgb(tdev.ptr, table, len(images), None), "mi355_jpeg_to_rgb")
    check(L.mi355_stream_sync(None), "sync")
    res = []
    for i, bufs in enumerate(keep):
        w, h, pitch = table[i].w, table[i].h, table[i].pitch
        raw = bufs[0].to_numpy(np.uint8, h * pitch).reshape(h, pitch)
        if pitch_pad and not (raw[:, 3 * w:] == 0xA5).all():
            raise MI355Error("mi355_jpeg_to_rgb wrote into the padding of a row")
        res.append(raw[:, :3 * w].reshape(h, w, 3).copy())
        for b in bufs:
            b.free()
    tdev.free()
    return res


def _file_args(items):
    datas = [_jpeg_bytes(it) for it in items]
    n = len(datas)
    ptrs, sizes = (C.c_char_p * n)(*datas), (C.c_size_t * n)(*[len(d) for d in datas])
    return datas, ptrs, sizes


def _decode_on_net(net, items, decode, last_error, exc):
    """network_jpeg_decode_gpu / network_png_decode_gpu (`decode`) on the items, the frames pulled back: [uint8 [h][w][3], ...]"""
    datas, ptrs, sizes = _file_args(items)
    n = len(items)
    rgb, ws, hs, ps = (C.c_void_p * n)(), (C.c_int * n)(), (C.c_int * n)(), (C.c_int * n)()
    if decode(net.h, ptrs, sizes, n, rgb, ws, hs, ps) != 0:
        raise exc(last_error().decode())
    net.sync()
    out = []
    for b in range(n):
        raw = np.empty(hs[b] * ps[b], np.uint8)
        check(shim().mi355_d2h(raw.ctypes.data, rgb[b], raw.nbytes, None), "d2h")
        check(shim().mi355_stream_sync(None), "sync")
        out.append(raw.reshape(hs[b], ps[b])[:, :3 * ws[b]].reshape(hs[b], ws[b], 3).copy())
    return out


def jpeg_decode(data, net=None):
    """Decode a JPEG (bytes or a path) to uint8 [h][w][3], the pixels the reference's stbi_load(.., 3) returns: entropy decode on the
    host, everything else on the device.  A list of items is decoded as one batch (two launches) and a list comes back.  net: a Net
    whose buffers and stream serve the call (network_jpeg_decode_gpu); without one the C-ABI calls run on the default stream."""
    many = isinstance(data, (list, tuple))
    items = list(data) if many else [data]
    if net is not None:
        out = _decode_on_net(net, items, net.H.network_jpeg_decode_gpu, net.H.network_jpeg_last_error, JpegError)
        return out if many else out[0]
    decoded = []
    for b, it in enumerate(items):
        try:
            decoded.append(jpeg_coefficients(it))
        except JpegError as e:
            raise JpegError(f"jpeg slot {b}: {e}") from None
    planes = jpeg_idct([(c["coef"], c["quant"]) for d in decoded for c in d["components"]])
    images, at = [], 0
    for d in decoded:
        comps = [{"plane": planes[at + k], "hs": c["hs"], "vs": c["vs"], "rows": c["rows"]} for k, c in enumerate(d["components"])]
        at += d["ncomp"]
        images.append({"w": d["w"], "h": d["h"], "mode": d["mode"], "components": comps})
    out = jpeg_to_rgb(images)
    return out if many else out[0]


class PngError(ValueError):
    """A PNG the decoder refuses; the message is the decoder's (with "png slot <b>: " in front where a batch was decoded)."""


def _png_host(data, headers_only):
    p = DnqPng()
    err = C.create_string_buffer(256)
    fn = host().png_info_host if headers_only else host().png_decode_host
    if fn(data, len(data), C.byref(p), err, len(err)) != 0:
        raise PngError(err.value.decode())
    return p


def _png_dict(p):
    return {"w": p.w, "h": p.h, "depth": p.depth, "color": p.color, "interlace": p.interlace, "channels": p.channels, "bpp": p.bpp,
            "pal_len": p.pal_len, "has_trns": bool(p.has_trns), "palette": np.array(p.palette, np.uint8).reshape(256, 3),
            "filtered_bytes": p.filtered_bytes,
            "passes": [{k: getattr(p.pass_[i], k) for k in ("w", "rows", "row_bytes", "index", "offset")} for i in range(p.npasses)]}


def png_info(data):
    """The headers of a PNG (bytes or a path) as a dict: size, depth, colour type, interlace flag, channels, filter unit "bpp", the
    palette ([256][3], zero beyond "pal_len") and "passes", the layout of the filtered stream: per pass that holds pixels its width,
    rows, row bytes, Adam7 index and offset.  Host only, nothing is inflated; raises PngError with the decoder's message."""
    return _png_dict(_png_host(_jpeg_bytes(data), True))


def png_scanlines(data):
    """The host half of the decoder on a PNG (bytes or a path): png_info's dict plus "filtered", the inflated bytes (uint8
    [filtered_bytes]: per pass, rows of one filter byte and row_bytes bytes).  Host only."""
    p = _png_host(_jpeg_bytes(data), False)
    try:
        d = _png_dict(p)
        d["filtered"] = np.ctypeslib.as_array(p.filtered, shape=(p.filtered_bytes,)).copy()
        return d
    finally:
        host().png_free(C.byref(p))


def png_inflate(z, cap, passes=None):
    """Two calls under one name.  png_inflate(z: bytes, cap: int): png_inflate_host, the host decoder's inflate on a ZLIB stream, at
    most cap bytes of output; host only.  png_inflate(streams: list, caps: list, passes): mi355_png_inflate on built inputs, see
    png_inflate_device."""
    if not isinstance(z, (bytes, bytearray, memoryview)):
        return png_inflate_device(z, cap, passes)
    out = np.empty(max(cap, 1), np.uint8)
    n = C.c_size_t(0)
    err = C.create_string_buffer(256)
    if host().png_inflate_host(bytes(z), len(z), out.ctypes.data, cap, C.byref(n), err, len(err)) != 0:
        raise PngError(err.value.decode())
    return out[:n.value].tobytes()


def png_scan(data):
    """png_scan_host on a PNG (bytes or a path): png_info's dict plus "z", the raw deflate data (the IDAT payloads behind the two-byte
    zlib header).  Host only, nothing is inflated; raises PngError with the decoder's message."""
    data = _jpeg_bytes(data)
    sc = DnqPngScan()
    err = C.create_string_buffer(256)
    if host().png_scan_host(data, len(data), C.byref(sc), err, len(err)) != 0:
        raise PngError(err.value.decode())
    try:
        d = _png_dict(sc.im)
        raw = bytes(np.ctypeslib.as_array(sc.z, shape=(sc.zcap,)))
        assert sc.zcap == ((sc.nbytes + 3) & ~3) + 8 and not any(raw[sc.nbytes:])
        d["z"] = raw[:sc.nbytes]
        return d
    finally:
        host().png_scan_free(C.byref(sc))


PNG_INFLATE_GUARD = 256  # guard bytes around every output of png_inflate_device / png_inflate_emulate
_STATUS_GUARD = 16       # guard words around the status words


def _png_inflate_run(streams, caps, passes, emulate):
    """One call of mi355_png_inflate (or of the emulation) for all streams.  Every output lies between guard bytes (0xA5), the status
    words between guard words; MI355Error if a guard changed.  passes[i]: [(rows, row_bytes), ...] of stream i; None: one row of
    caps[i] - 1 bytes.  Returns (outputs: bytes of caps[i] each, statuses)."""
    n = len(streams)
    assert n == len(caps) and n >= 1
    passes = [None] * n if passes is None else list(passes)
    G = PNG_INFLATE_GUARD
    table = (PngStream * n)()
    zat, oat, ztot, otot = [], [], 0, G
    for z, cap in zip(streams, caps):
        zat.append(ztot)
        ztot += (((len(z) + 3) & ~3) + 8 + 255) & ~255
        oat.append(otot)
        otot += ((cap + 3) & ~3) + G
    znp = np.zeros(max(ztot, 16), np.uint8)
    for z, at in zip(streams, zat):
        znp[at:at + len(z)] = np.frombuffer(bytes(z), np.uint8)
    onp = np.full(otot, 0xA5, np.uint8)
    snp = np.full(n + 2 * _STATUS_GUARD, 0x5A5A5A5A, np.int32)
    if emulate:
        zptr, optr, keep = znp.ctypes.data, onp.ctypes.data, []
    else:
        zb, ob, sb = DevBuf.from_numpy(znp), DevBuf.from_numpy(onp), DevBuf.from_numpy(snp)
        zptr, optr, keep = zb.ptr.value, ob.ptr.value, [zb, ob, sb]
    for i, (z, cap) in enumerate(zip(streams, caps)):
        t = table[i]
        t.z, t.out, t.nbytes, t.cap = zptr + zat[i], optr + oat[i], len(z), cap
        ps = passes[i] if passes[i] is not None else [(1, cap - 1)]
        t.npasses = len(ps)
        for k, (rows, rb) in enumerate(ps[:7]):
            t.rows[k], t.row_bytes[k] = rows, rb
    try:
        if emulate:
            status = (C.c_int * n)()
            if host().png_inflate_emulate_host(table, n, status) != 0:
                raise MI355Error("png_inflate_emulate_host: " + host().png_inflate_emulate_why().decode())
            snp[_STATUS_GUARD:_STATUS_GUARD + n] = list(status)
        else:
            tdev = DevBuf.from_numpy(np.frombuffer(bytes(table), np.uint8))
            keep.append(tdev)
            check(shim().mi355_png_inflate(tdev.ptr, table, n, sb.ptr.value + 4 * _STATUS_GUARD, None), "mi355_png_inflate")
            check(shim().mi355_stream_sync(None), "sync")
            onp = ob.to_numpy(np.uint8, otot)
            snp = sb.to_numpy(np.int32, n + 2 * _STATUS_GUARD)
    finally:
        for b in keep:
            b.free()
    if not ((snp[:_STATUS_GUARD] == 0x5A5A5A5A).all() and (snp[_STATUS_GUARD + n:] == 0x5A5A5A5A).all()):
        raise MI355Error("mi355_png_inflate wrote outside its status words")
    outs, at = [], 0
    for i, cap in enumerate(caps):
        if not (onp[at:oat[i]] == 0xA5).all():
            raise MI355Error(f"mi355_png_inflate wrote in front of stream {i}'s output")
        outs.append(onp[oat[i]:oat[i] + cap].tobytes())
        at = oat[i] + cap
    if not (onp[at:] == 0xA5).all():
        raise MI355Error("mi355_png_inflate wrote behind the last stream's output")
    return outs, [int(v) for v in snp[_STATUS_GUARD:_STATUS_GUARD + n]]


def png_inflate_device(streams, caps, passes=None):
    """mi355_png_inflate on built inputs: streams[i] is raw deflate data (no zlib header), caps[i] its stop mark, passes[i] its
    [(rows, row_bytes), ...] (None: one row of caps[i] - 1 bytes, so only the first byte is checked against 4); ONE launch for all of
    them.  Returns (outputs, statuses): caps[i] bytes per stream (0xA5 where nothing was stored) and its status word (0, or a key of
    PNG_INFLATE_ERRORS).  Guard bytes before, between and behind the outputs and guard words around the status words must come back
    as they were.  A table the call refuses raises MI355Error with its message."""
    return _png_inflate_run(list(streams), list(caps), passes, False)


def png_inflate_emulate(streams, caps, passes=None):
    """png_inflate_device's arguments and results from png_inflate_emulate_host: the kernel's rounds on the CPU, no device."""
    return _png_inflate_run(list(streams), list(caps), passes, True)


def png_stream_of(scan):
    """(stream, cap, passes) of a png_scan dict, as png_inflate_device takes them"""
    return scan["z"], scan["filtered_bytes"], [(q["rows"], q["row_bytes"]) for q in scan["passes"]]


def png_unfilter(segments, src_offset=0, dst_offset=0):
    """mi355_png_unfilter on built inputs: segments is a list of (filtered uint8 [rows][1 + row_bytes], bpp); one launch for all of
    them.  src_offset / dst_offset: bytes by which every segment's source / destination is moved off its allocation's alignment.
    Returns the reconstructed uint8 [rows][row_bytes] per segment; the bytes around a destination must come back as they were."""
    L = shim()
    table = (PngSegment * len(segments))()
    keep = []
    for i, (filt, bpp) in enumerate(segments):
        filt = np.ascontiguousarray(filt, np.uint8)
        rows, rb = filt.shape[0], filt.shape[1] - 1
        src = DevBuf.from_numpy(np.concatenate([np.zeros(src_offset, np.uint8), filt.ravel()]))
        dst = DevBuf.from_numpy(np.full(dst_offset + rows * rb + 16, 0xA5, np.uint8))
        keep.append((src, dst))
        table[i].filtered, table[i].out = src.ptr.value + src_offset, dst.ptr.value + dst_offset
        table[i].row_bytes, table[i].rows, table[i].bpp = rb, rows, bpp
    tdev = DevBuf.from_numpy(np.frombuffer(bytes(table), np.uint8))
    try:
        check(L.mi355_png_unfilter(tdev.ptr, table, len(segments), None), "mi355_png_unfilter")
        check(L.mi355_stream_sync(None), "sync")
        res = []
        for i, (src, dst) in enumerate(keep):
            n = table[i].rows * table[i].row_bytes
            raw = dst.to_numpy(np.uint8, dst_offset + n + 16)
            if not ((raw[:dst_offset] == 0xA5).all() and (raw[dst_offset + n:] == 0xA5).all()):
                raise MI355Error("mi355_png_unfilter wrote outside a segment's rows")
            res.append(raw[dst_offset:dst_offset + n].reshape(table[i].rows, table[i].row_bytes).copy())
        return res
    finally:
        for src, dst in keep:
            src.free()
            dst.free()
        tdev.free()


def png_to_rgb(images, pitch_pad=0):
    """mi355_png_to_rgb on built inputs: images is a list of dicts {"w", "h", "depth", "color", "interlace", "passes": {index: uint8
    [rows][row_bytes] reconstructed rows} (a plain image: {0: ...}), "palette": uint8 [n][3] (colour type 3), "pal_len" (default: n)};
    one launch for all of them.  pitch_pad: bytes added to every output row's 3 * w.  Returns uint8 [h][w][3] per image; the pad bytes
    must come back as they were (0xA5)."""
    L = shim()
    table = (PngImage * len(images))()
    keep = []
    for i, im in enumerate(images):
        w, h = im["w"], im["h"]
        pitch = 3 * w + pitch_pad
        out = DevBuf.from_numpy(np.full(max(h * pitch, 1), 0xA5, np.uint8))
        bufs = [out]
        t = table[i]
        t.rgb, t.w, t.h, t.pitch = out.ptr, w, h, pitch
        t.depth, t.color, t.interlace = im["depth"], im["color"], im.get("interlace", 0)
        if im.get("palette") is not None:
            pal = np.zeros((256, 3), np.uint8)
            src = np.asarray(im["palette"], np.uint8).reshape(-1, 3)
            pal[:len(src)] = src
            b = DevBuf.from_numpy(pal)
            bufs.append(b)
            t.palette, t.pal_len = b.ptr, im.get("pal_len", len(src))
        for k, rows in im["passes"].items():
            b = DevBuf.from_numpy(np.ascontiguousarray(rows, np.uint8))
            bufs.append(b)
            t.pass_[k] = b.ptr
        keep.append(bufs)
    tdev = DevBuf.from_numpy(np.frombuffer(bytes(table), np.uint8))
    try:
        check(L.mi355_png_to_rgb(tdev.ptr, table, len(images), None), "mi355_png_to_rgb")
        check(L.mi355_stream_sync(None), "sync")
        res = []
        for i, bufs in enumerate(keep):
            w, h, pitch = table[i].w, table[i].h, table[i].pitch
            raw = bufs[0].to_numpy(np.uint8, h * pitch).reshape(h, pitch)
            if pitch_pad and not (raw[:, 3 * w:] == 0xA5).all():
                raise MI355Error("mi355_png_to_rgb wrote into the padding of a row")
            res.append(raw[:, :3 * w].reshape(h, w, 3).copy())
        return res
    finally:
        for bufs in keep:
            for b in bufs:
                b.free()
        tdev.free()


def png_decode(data, net=None):
    """Decode a PNG (bytes or a path) to uint8 [h][w][3], the pixels the reference's stbi_load(.., 3) returns: chunk parse and inflate
    on the host, everything else on the device.  A list of items is decoded as one batch (two launches) and a list comes back.  net: a
    Net whose buffers and stream serve the call (network_png_decode_gpu); without one the C-ABI calls run on the default stream."""
    many = isinstance(data, (list, tuple))
    items = list(data) if many else [data]
    if net is not None:
        out = _decode_on_net(net, items, net.H.network_png_decode_gpu, net.H.network_png_last_error, PngError)
        return out if many else out[0]
    decoded = []
    for b, it in enumerate(items):
        try:
            decoded.append(png_scanlines(it))
        except PngError as e:
            raise PngError(f"png slot {b}: {e}") from None
    segs = []
    for d in decoded:
        for q in d["passes"]:
            n = q["rows"] * (q["row_bytes"] + 1)
            segs.append((d["filtered"][q["offset"]:q["offset"] + n].reshape(q["rows"], q["row_bytes"] + 1), d["bpp"]))
    rows = png_unfilter(segs)
    images, at = [], 0
    for d in decoded:
        passes = {q["index"]: rows[at + k] for k, q in enumerate(d["passes"])}
        at += len(d["passes"])
        images.append({"w": d["w"], "h": d["h"], "depth": d["depth"], "color": d["color"], "interlace": d["interlace"], "passes": passes,
                       "palette": d["palette"] if d["color"] == 3 else None, "pal_len": d["pal_len"]})
    out = png_to_rgb(images)
    return out if many else out[0]


class Net:
    """The darknet host network (libdarknet_q.so): load_network -> prep -> forward_network_gpu."""

    def __init__(self, cfg, weights=None, batch=1, gpu=0, accum=ACC_EXACT, store=STORE_WRAP, dump_int32=False,
                 use_graph=False, fuse_maxpool=True, keep_head_float=True):
        """keep_head_float: the head convs fused with their yolo layers also store their own float tensors (the library's default is
        not to: nothing but the yolo layer reads them; parity pulls want them)"""
        H = host()
        self.H = H
        self.h = H.load_network(cfg.encode(), weights.encode() if weights else None, 0)
        H.dnq_net_set(self.h, b"gpu_index", gpu)
        H.dnq_net_set(self.h, b"accum_mode", accum)
        H.dnq_net_set(self.h, b"store_mode", store)
        H.dnq_net_set(self.h, b"dump_int32", int(dump_int32))
        H.dnq_net_set(self.h, b"use_graph", int(use_graph))
        H.dnq_net_set(self.h, b"fuse_maxpool", int(fuse_maxpool))
        H.dnq_net_set(self.h, b"keep_head_float", int(keep_head_float))
        self.keep_head_float = bool(keep_head_float)
        if batch != H.dnq_net_batch(self.h):
            H.set_batch_network(self.h, batch)
        self.n = H.dnq_net_n(self.h)
        self.batch = batch
        self.inputs = H.dnq_net_inputs(self.h)
        self.info = []
        for i in range(self.n):
            a = (C.c_int * 16)()
            H.dnq_layer_info(self.h, i, a)
            self.info.append(dict(zip(INFO_KEYS, list(a))))

    def set(self, key, val):
        assert self.H.dnq_net_set(self.h, key.encode(), int(val)) == 0

    def replica(self, default_stream=False):
        """network_replica: a second executor of this prepared model on the same device (own activations, input and HIP
        stream; this network's packed weights).  This network must outlive it.  default_stream: the replica launches on the
        device's default stream (HIP's fourth hardware queue: darknet_q.h replica_default_stream)."""
        if default_stream:
            self.set("replica_default_stream", 1)
        r = object.__new__(Net)
        r.H = self.H
        r.h = self.H.network_replica(self.h)
        r.keep_head_float = self.keep_head_float
        r.n, r.batch, r.inputs, r.info = self.n, self.batch, self.inputs, self.info
        r._parent = self  # keeps the parent alive
        r.per_image = getattr(self, "per_image", False)
        r.input_on_device = getattr(self, "input_on_device", False)
        return r

    def prepare_fixed(self, in_scale=1.0 / 255.0, in_zp=0):
        self.H.quantization_weights_and_activations_fixed_input(self.h, np.float32(in_scale), in_zp)

    def prepare_host_only(self, in_scale=1.0 / 255.0, in_zp=0):
        self.H.quantization_prep_host(self.h, np.float32(in_scale), in_zp)

    def set_input_per_image(self, on=True):
        """Per-image input quantisation (darknet_q.h set_input_quantization_per_image): every image of a batch gets its own
        scale / zero point and layer-0 constants.  Off (the default): image 0 defines the scale of the batch.  Raises
        MI355Error when layer 0 cannot be served per image.  While it is on, the prepare_from_* calls return
        (uint8 input, scale[batch], zero_point[batch])."""
        rc = self.H.set_input_quantization_per_image(self.h, int(bool(on)))
        if rc != 0:
            raise MI355Error(f"set_input_quantization_per_image: code {rc} (layer 0 is not served per image)")
        self.per_image = bool(on)

    def set_input_on_device(self, on=True):
        """Input quantisation on the device (darknet_q.h set_input_quantization_on_device): the device input paths derive the
        (scale, zero point) of every image and layer 0's constants in HBM, without a copy back or a wait; combines with
        set_input_per_image either way.  Raises MI355Error under set_input_per_image's conditions.  While it is on, a
        prepare_from_frames_* call with frames on the device only enqueues work and returns None: input_quantization(),
        input_status() and input_bank_entry() are the explicit (waiting) reads."""
        rc = self.H.set_input_quantization_on_device(self.h, int(bool(on)))
        if rc != 0:
            raise MI355Error(f"set_input_quantization_on_device: code {rc} (layer 0 is not served from a bank)")
        self.input_on_device = bool(on)

    def input_status(self):
        """uint32[batch] MI355_INPUT_* bits of the last on-device input step (0: the image was quantised with its own pair; else it kept
        the pair and layer-0 entry of its previous batch).  Waits for the network's stream."""
        st = np.zeros(self.batch, np.uint32)
        self.H.network_input_status(self.h, st.ctypes.data)
        return st

    def input_bank_entry(self, b):
        """Image b's layer-0 bank entry as the device holds it (bank_entry_bytes() bytes).  Waits for the network's stream."""
        out = np.zeros(self.bank_entry_bytes(), np.uint8)
        self.H.network_input_bank_entry(self.h, b, out.ctypes.data)
        return out

    def layer0_consts(self):
        """Layer 0's constant table for mi355_l0_derive as bytes (network_layer0_consts; host only)."""
        out = np.zeros(self.H.network_layer0_consts(self.h, None), np.uint8)
        self.H.network_layer0_consts(self.h, out.ctypes.data)
        return out

    def host_waits(self):
        """How often the host library has waited for the device on this network's behalf so far (network_host_waits)."""
        return int(self.H.network_host_waits(self.h))

    def _enqueued_only(self, on_device):
        return bool(on_device) and getattr(self, "input_on_device", False)

    def input_quantization(self):
        """(scale[batch] float32, zero_point[batch] uint8) the last batch was quantised with."""
        s = np.zeros(self.batch, np.float32)
        z = np.zeros(self.batch, np.uint8)
        self.H.network_input_quantization(self.h, s.ctypes.data, z.ctypes.data)
        return s, z

    def _prepared(self, xq):
        if getattr(self, "per_image", False):
            s, z = self.input_quantization()
            return xq, s, z
        return xq

    def prepare_from_float(self, x_float):
        """Reference flow: dynamic layer-0 quantiser on the float image(s) (src/blas.c:279)."""
        x = np.ascontiguousarray(x_float, np.float32).ravel()
        assert x.size == self.batch * self.inputs
        C.memmove(self.H.dnq_net_input_float(self.h), x.ctypes.data, x.nbytes)
        self.H.quantization_weights_and_activations(self.h)
        return self._prepared(_as(self.H.dnq_net_input_host(self.h), self.batch * self.inputs, C.c_uint8).copy())

    def prepare_from_float_gpu(self, x_float):
        """The same with the quantiser on the device: the floats are uploaded as they are, min / max and the per-element
        quantiser run in HBM (quantization_weights_and_activations_gpu).  Returns the uint8 input the device produced."""
        x = np.ascontiguousarray(x_float, np.float32).ravel()
        assert x.size == self.batch * self.inputs
        buf = DevBuf.from_numpy(x)
        self.H.quantization_weights_and_activations_gpu(self.h, buf.ptr)
        self.sync()
        out = np.empty(x.size, np.uint8)
        check(shim().mi355_d2h(out.ctypes.data, self.input_gpu_ptr(), out.nbytes, None), "d2h")
        check(shim().mi355_stream_sync(None), "sync")
        buf.free()
        return self._prepared(out)

    def prepare_from_images_gpu(self, images):
        """Device input path: every image (float32 [c][h][w], any size) is uploaded, letterboxed into its batch slot and
        the batch quantised on the device.  Returns the uint8 network input the device produced."""
        assert len(images) == self.batch
        bufs = []
        for slot, im in enumerate(images):
            im = np.ascontiguousarray(im, np.float32)
            b = DevBuf.from_numpy(im)
            bufs.append(b)
            self.H.network_letterbox_input_gpu(self.h, slot, b.ptr, im.shape[2], im.shape[1])
        self.H.network_quantize_input_gpu(self.h)
        self.sync()
        out = np.empty(self.batch * self.inputs, np.uint8)
        check(shim().mi355_d2h(out.ctypes.data, self.input_gpu_ptr(), out.nbytes, None), "d2h")
        check(shim().mi355_stream_sync(None), "sync")
        for b in bufs:
            b.free()
        return self._prepared(out)

    def prepare_from_frames_u8(self, frames, order="rgb"):
        """8-bit frame input path (network_frames_u8_input_gpu): every frame (uint8 [h][w][3], any size, interleaved `order` = "rgb" |
        "bgr") goes up as bytes; letterbox, min / max and the quantiser run on the device for the whole batch in two launches.  Rows
        need not be contiguous: a frame whose pixels are 3 contiguous bytes and whose row stride is at least 3 * w is passed with that
        stride as its pitch (anything else is copied first).  Returns what prepare_from_images_gpu returns."""
        assert len(frames) == self.batch
        B = self.batch
        keep = []
        ptrs, ws, hs, ps = (C.c_void_p * B)(), (C.c_int * B)(), (C.c_int * B)(), (C.c_int * B)()
        for b, f in enumerate(frames):
            a = np.asarray(f)
            if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
                raise ValueError("prepare_from_frames_u8: every frame must be a uint8 [h][w][3] array")
            ptrs[b], ps[b] = _byte_rows(a, keep)
            hs[b], ws[b] = a.shape[:2]
        self.H.network_frames_u8_input_gpu(self.h, ptrs, ws, hs, ps, FRAME_ORDER[order], 0)
        return self._prepared(self._pull_input())

    def set_jpeg_entropy_on_device(self, on=True, subseq_bits=None):
        """JPEG scans are entropy-decoded on the device (set_jpeg_entropy_on_device): the input the network sees is unchanged; the
        JPEG calls then wait once, for the segments' status words.  subseq_bits: the bits a lane decodes per round."""
        self.H.set_jpeg_entropy_on_device(self.h, 1 if on else 0)
        if subseq_bits is not None:
            self.H.set_jpeg_entropy_subseq_bits(self.h, int(subseq_bits))

    def set_png_inflate_on_device(self, on=True):
        """PNG streams are inflated on the device (set_png_inflate_on_device): the input the network sees is unchanged; the PNG calls
        then wait once, for the streams' status words."""
        self.H.set_png_inflate_on_device(self.h, 1 if on else 0)

    def prepare_from_jpeg(self, items):
        """JPEG input path (network_frames_jpeg_input_gpu): every item (the bytes of a JPEG file, or a path) is entropy-decoded on the
        host and finished on the device; the RGB frames stay there and feed the 8-bit frame path.  Returns [(w, h), ...], the images'
        sizes for the detection calls.  Raises JpegError naming the slot when an image is refused; nothing has been launched then."""
        return self._prepare_from_files(items, self.H.network_frames_jpeg_input_gpu, self.H.network_jpeg_last_error, JpegError)

    def prepare_from_png(self, items):
        """PNG input path (network_frames_png_input_gpu): every item (the bytes of a PNG file, or a path) is parsed and inflated on the
        host and finished on the device; the RGB frames stay there and feed the 8-bit frame path.  Returns [(w, h), ...], the images'
        sizes for the detection calls.  Raises PngError naming the slot when an image is refused; nothing has been launched then."""
        return self._prepare_from_files(items, self.H.network_frames_png_input_gpu, self.H.network_png_last_error, PngError)

    def _prepare_from_files(self, items, frames_input, last_error, exc):
        assert len(items) == self.batch
        B = self.batch
        datas, ptrs, sizes = _file_args(items)
        ws, hs = (C.c_int * B)(), (C.c_int * B)()
        if frames_input(self.h, ptrs, sizes, ws, hs) != 0:
            raise exc(last_error().decode())
        return [(ws[b], hs[b]) for b in range(B)]

    def _pull_input(self):
        self.sync()
        out = np.empty(self.batch * self.inputs, np.uint8)
        check(shim().mi355_d2h(out.ctypes.data, self.input_gpu_ptr(), out.nbytes, None), "d2h")
        check(shim().mi355_stream_sync(None), "sync")
        return out

    def prepare_from_frames_nv12(self, frames, layout="nv12", matrix="bt601", on_device=False):
        """NV12 / NV21 frame input path (network_frames_nv12_input_gpu): frames[b] is a pair (y, uv) of uint8 arrays, [h][w] and
        [(h + 1) // 2][(w + 1) // 2][2] (`layout` = "nv12": pairs are (U, V) | "nv21": (V, U)); both planes go up as they are and are
        converted with `matrix` = "bt601" | "bt601f" | "bt709" | "bt709f" (f: full range) on the device, inside the letterbox.  Row
        strides are passed through as pitches where the samples of a row are contiguous and the stride is at least the row
        (anything else is copied first).  on_device: frames[b] is (y_ptr, uv_ptr, w, h, pitch_y, pitch_uv) with device addresses
        instead, used in place.  Returns what prepare_from_frames_u8 returns."""
        assert len(frames) == self.batch
        B = self.batch
        keep = []
        ys, uvs = (C.c_void_p * B)(), (C.c_void_p * B)()
        ws, hs, py, puv = (C.c_int * B)(), (C.c_int * B)(), (C.c_int * B)(), (C.c_int * B)()
        for b, f in enumerate(frames):
            if on_device:
                ys[b], uvs[b], ws[b], hs[b], py[b], puv[b] = f
                continue
            y, uv = np.asarray(f[0]), np.asarray(f[1])
            if y.dtype != np.uint8 or y.ndim != 2 or uv.dtype != np.uint8 or uv.ndim != 3 or uv.shape[2] != 2:
                raise ValueError("prepare_from_frames_nv12: every frame must be (uint8 [h][w], uint8 [(h + 1) // 2][(w + 1) // 2][2])")
            h, w = y.shape
            if uv.shape[:2] != ((h + 1) // 2, (w + 1) // 2):
                raise ValueError("prepare_from_frames_nv12: the chroma plane must be [(h + 1) // 2][(w + 1) // 2][2]")
            (ys[b], py[b]), (uvs[b], puv[b]), hs[b], ws[b] = _byte_rows(y, keep), _byte_rows(uv, keep), h, w
        self.H.network_frames_nv12_input_gpu(self.h, ys, uvs, ws, hs, py, puv, YUV_LAYOUT[layout], YUV_MATRIX[matrix], int(on_device))
        if self._enqueued_only(on_device):
            return None
        return self._prepared(self._pull_input())

    def prepare_from_frames_planar(self, frames, format="i420", matrix="bt601", on_device=False):
        """Planar frame input path (network_frames_planar_input_gpu): frames[b] is a tuple of three 2-D uint8 arrays in the order
        `format` names them -- "i420": (Y, U, V), "yv12": (Y, V, U), chroma [(h + 1) // 2][(w + 1) // 2]; "i422": (Y, U, V), chroma
        [h][(w + 1) // 2]; "i444": (Y, U, V), "rgb": (R, G, B), "bgr": (B, G, R), all [h][w].  For "rgb" / "bgr" a single [3][h][w]
        array is accepted too and split along axis 0.  The planes go up as they are; the YUV formats are converted with `matrix` =
        "bt601" | "bt601f" | "bt709" | "bt709f" on the device, inside the letterbox (leave it at its default with "rgb" / "bgr").
        A plane's row stride is passed through as its pitch where the row's bytes are contiguous and the stride is at least the row
        (anything else is copied first).  on_device: frames[b] is (ptr0, ptr1, ptr2, w, h, pitch0, pitch1, pitch2) with device
        addresses instead, used in place -- or, for "rgb" / "bgr", a uint8 [3][h][w] device tensor (anything with data_ptr(), shape
        and stride(), as a torch tensor has) whose rows are contiguous; the work that wrote it must have finished, and its memory
        must belong to the HIP runtime this library is linked to.  Returns what prepare_from_frames_u8 returns."""
        assert len(frames) == self.batch
        B = self.batch
        rgb = format in ("rgb", "bgr")
        keep = []
        ptr = [(C.c_void_p * B)() for _ in range(3)]
        pitch = [(C.c_int * B)() for _ in range(3)]
        ws, hs = (C.c_int * B)(), (C.c_int * B)()
        for b, f in enumerate(frames):
            if on_device:
                if hasattr(f, "data_ptr"):
                    if not rgb or tuple(f.shape[:1]) != (3,) or len(f.shape) != 3 or f.element_size() != 1 or f.stride(2) != 1 or f.stride(1) < f.shape[2]:
                        raise ValueError("prepare_from_frames_planar: a device tensor must be uint8 [3][h][w] with contiguous rows, format rgb / bgr")
                    f = tuple(f.data_ptr() + k * f.stride(0) for k in range(3)) + (f.shape[2], f.shape[1]) + (f.stride(1),) * 3
                ptr[0][b], ptr[1][b], ptr[2][b], ws[b], hs[b], pitch[0][b], pitch[1][b], pitch[2][b] = f
                continue
            planes = [np.asarray(a) for a in f] if isinstance(f, (tuple, list)) else np.asarray(f)
            if not isinstance(planes, list):
                if not rgb or planes.ndim != 3 or planes.shape[0] != 3:
                    raise ValueError("prepare_from_frames_planar: a single array must be [3][h][w], format rgb / bgr")
                planes = [planes[k] for k in range(3)]
            if len(planes) != 3 or any(a.dtype != np.uint8 or a.ndim != 2 for a in planes):
                raise ValueError("prepare_from_frames_planar: every frame must be three 2-D uint8 arrays")
            h, w = planes[0].shape
            chroma = (h, w) if rgb or format == "i444" else ((h, (w + 1) // 2) if format == "i422" else ((h + 1) // 2, (w + 1) // 2))
            if planes[1].shape != chroma or planes[2].shape != chroma:
                raise ValueError(f"prepare_from_frames_planar: planes 1 and 2 of a {w} x {h} {format} frame must be {chroma[1]} x {chroma[0]}")
            for k, a in enumerate(planes):
                ptr[k][b], pitch[k][b] = _byte_rows(a, keep)
            hs[b], ws[b] = h, w
        self.H.network_frames_planar_input_gpu(self.h, ptr[0], ptr[1], ptr[2], ws, hs, pitch[0], pitch[1], pitch[2],
                                               PLANAR_FORMAT[format], YUV_MATRIX[matrix], int(on_device))
        if self._enqueued_only(on_device):
            return None
        return self._prepared(self._pull_input())

    def prepare_from_frames_packed(self, frames, format="bgra", matrix="bt601"):
        """Packed frame input path (network_frames_packed_input_gpu), one plane of 4-byte groups.  `format` = "rgba" | "bgra" | "argb" |
        "abgr": frames[b] is uint8 [h][w][4], the byte that is not R, G or B is never looked at; leave `matrix` at its default.
        `format` = "yuyv" (YUY2) | "uyvy" | "yvyu" (4:2:2, a macropixel of two pixels in four bytes): frames[b] is uint8 [h][row_bytes]
        and w = row_bytes / 2, or a tuple (array, w) -- the only way to name an odd width, whose rows still hold (w + 1) / 2 whole
        macropixels --; converted with `matrix` = "bt601" | "bt601f" | "bt709" | "bt709f" on the device, inside the letterbox.  A
        frame is a host array or a device tensor (anything with data_ptr(), shape, stride() and element_size(), as a torch tensor
        has; used in place: the work that wrote it must have finished, and its memory must belong to the HIP runtime this library
        is linked to), all frames of a batch the same.  Row strides are passed through as the pitch, as prepare_from_frames_u8 does.
        Returns what prepare_from_frames_u8 returns."""
        assert len(frames) == self.batch
        B = self.batch
        rgbx = format in PACKED_RGBX
        if format not in PACKED_FORMAT:
            raise ValueError(f"prepare_from_frames_packed: format is one of {', '.join(PACKED_FORMAT)}")
        if rgbx and matrix != "bt601":
            raise ValueError("prepare_from_frames_packed: matrix goes with yuyv / uyvy / yvyu only")
        keep, where = [], set()
        ptrs, ws, hs, ps = (C.c_void_p * B)(), (C.c_int * B)(), (C.c_int * B)(), (C.c_int * B)()
        for b, f in enumerate(frames):
            f, w = f if isinstance(f, (tuple, list)) else (f, None)
            if rgbx:
                if w is not None:
                    raise ValueError("prepare_from_frames_packed: (array, w) goes with yuyv / uyvy / yvyu only")
                ptrs[b], ps[b], shape, dev = _sample_rows(f, 1, (4,), keep, "prepare_from_frames_packed")
                if len(shape) != 3:
                    raise ValueError(f"prepare_from_frames_packed: a {format} frame must be uint8 [h][w][4]")
                hs[b], ws[b] = shape[:2]
            else:
                ptrs[b], ps[b], shape, dev = _sample_rows(f, 1, (), keep, "prepare_from_frames_packed")
                if len(shape) != 2 or (w is None and shape[1] % 4) or (w is not None and (w < 1 or shape[1] < 4 * ((w + 1) // 2))):
                    raise ValueError(f"prepare_from_frames_packed: a {format} frame must be uint8 [h][row_bytes] holding (w + 1) // 2 "
                                     "macropixels of 4 bytes a row; give (array, w) for an odd w")
                hs[b], ws[b] = shape[0], shape[1] // 2 if w is None else w
            where.add(dev)
        if len(where) != 1:
            raise ValueError("prepare_from_frames_packed: the frames of a batch are all host arrays or all device tensors")
        on_device = where.pop()
        self.H.network_frames_packed_input_gpu(self.h, ptrs, ws, hs, ps, PACKED_FORMAT[format], 0 if rgbx else YUV_MATRIX[matrix],
                                               int(on_device))
        if self._enqueued_only(on_device):
            return None
        return self._prepared(self._pull_input())

    def prepare_from_frames_p010(self, frames, matrix="bt601"):
        """P010 / P012 / P016 frame input path (network_frames_p010_input_gpu): frames[b] is a pair (y, uv) of uint16 little-endian
        planes, [h][w] and [(h + 1) // 2][(w + 1) // 2][2] with (U, V) pairs, the significant bits of a sample at the top -- host
        arrays or device tensors (see prepare_from_frames_packed), all frames of a batch the same.  Both planes go up as they are; the
        device reads the high byte of every sample (sample >> 8: truncation, not rounding) and converts with `matrix` = "bt601" |
        "bt601f" | "bt709" | "bt709f" inside the letterbox, as prepare_from_frames_nv12 does for (y >> 8, uv >> 8).  Row strides are
        passed through as pitches.  Returns what prepare_from_frames_u8 returns."""
        assert len(frames) == self.batch
        B = self.batch
        keep, where = [], set()
        ys, uvs = (C.c_void_p * B)(), (C.c_void_p * B)()
        ws, hs, py, puv = (C.c_int * B)(), (C.c_int * B)(), (C.c_int * B)(), (C.c_int * B)()
        for b, f in enumerate(frames):
            if not isinstance(f, (tuple, list)) or len(f) != 2:
                raise ValueError("prepare_from_frames_p010: every frame must be a pair (y, uv)")
            ys[b], py[b], sy, dev_y = _sample_rows(f[0], 2, (), keep, "prepare_from_frames_p010")
            uvs[b], puv[b], suv, dev_uv = _sample_rows(f[1], 2, (2,), keep, "prepare_from_frames_p010")
            if len(sy) != 2 or len(suv) != 3 or suv[:2] != ((sy[0] + 1) // 2, (sy[1] + 1) // 2):
                raise ValueError("prepare_from_frames_p010: every frame must be (uint16 [h][w], uint16 [(h + 1) // 2][(w + 1) // 2][2])")
            hs[b], ws[b] = sy
            where |= {dev_y, dev_uv}
        if len(where) != 1:
            raise ValueError("prepare_from_frames_p010: the planes of a batch are all host arrays or all device tensors")
        on_device = where.pop()
        self.H.network_frames_p010_input_gpu(self.h, ys, uvs, ws, hs, py, puv, YUV_MATRIX[matrix], int(on_device))
        if self._enqueued_only(on_device):
            return None
        return self._prepared(self._pull_input())

    def prepare_from_frames_bayer(self, frames, pattern="rggb", sample="u8", shift=0, tone=None, on_device=False):
        """Raw sensor frame input path (network_frames_bayer_input_gpu): one sample per pixel behind a Bayer filter, `pattern` = "rggb" |
        "bggr" | "grbg" | "gbrg" (the 2 x 2 tile from the top left corner), or behind none, "mono".  `sample` = "u8": frames[b] is
        uint8 [h][w]; "u16": uint16 [h][w], little-endian, every sample reduced to min(v >> shift, 255) with `shift` in 0..8 (2, 4, 6 for
        LSB-aligned 10-, 12-, 14-bit samples, 8 for MSB-aligned or 16-bit ones); "mipi10" | "mipi12" (CSI-2 RAW10: four pixels in five
        bytes, RAW12: two in three): a tuple (uint8 [h][row_bytes], w).  `tone`: None, one uint8 [3][256] array for all frames, or a
        sequence of one per frame (None: identity) -- the (R, G, B) tables every sample goes through by the colour of its site before
        anything is averaged (black level, white balance, transfer curve; "mono" uses table 0).  The frames go up as they are and are
        demosaiced bilinearly on the device, inside the letterbox, as mi355_yolo_int8.h defines at mi355_frame_bayer.  on_device:
        frames and tone tables are device tensors (see prepare_from_frames_packed) used in place; otherwise host arrays.  Row strides
        are passed through as the pitch, as prepare_from_frames_u8 does.  Returns what prepare_from_frames_u8 returns."""
        me = "prepare_from_frames_bayer"
        assert len(frames) == self.batch
        B = self.batch
        if pattern not in BAYER_PATTERN:
            raise ValueError(f"{me}: pattern is one of {', '.join(BAYER_PATTERN)}")
        if sample not in RAW_SAMPLE:
            raise ValueError(f"{me}: sample is one of {', '.join(RAW_SAMPLE)}")
        if not isinstance(shift, int) or not 0 <= shift <= 8 or (shift and sample != "u16"):
            raise ValueError(f"{me}: shift is 0..8 and goes with sample u16 only")
        mipi = sample in ("mipi10", "mipi12")
        keep, where = [], set()
        ptrs, ws, hs, ps = (C.c_void_p * B)(), (C.c_int * B)(), (C.c_int * B)(), (C.c_int * B)()
        for b, f in enumerate(frames):
            f, w = f if isinstance(f, (tuple, list)) else (f, None)
            if mipi != (w is not None):
                raise ValueError(f"{me}: a frame is (uint8 [h][row_bytes], w) with mipi10 / mipi12 and a plain [h][w] array otherwise")
            ptrs[b], ps[b], shape, dev = _sample_rows(f, 2 if sample == "u16" else 1, (), keep, me)
            if len(shape) != 2 or (mipi and (not isinstance(w, int) or w < 1 or shape[1] < raw_row_bytes(sample, w))):
                raise ValueError(f"{me}: a {sample} frame must be [h][w]" + (f" bytes holding {raw_row_bytes(sample, max(w, 1))} a row" if mipi else ""))
            hs[b], ws[b] = shape[0], w if mipi else shape[1]
            if pattern != "mono" and (hs[b] < 2 or ws[b] < 2):
                raise ValueError(f"{me}: a Bayer frame needs w, h >= 2")
            where.add(dev)
        tones = None
        if tone is not None:
            per_frame = isinstance(tone, (tuple, list))
            if per_frame and len(tone) != B:
                raise ValueError(f"{me}: tone is None, one uint8 [3][256] table or one per frame")
            tones = (C.c_void_p * B)()
            for b, t in enumerate(tone if per_frame else [tone] * B):
                if t is None:
                    continue
                if hasattr(t, "data_ptr"):
                    if tuple(t.shape) != (3, 256) or t.element_size() != 1 or t.stride(1) != 1 or t.stride(0) != 256:
                        raise ValueError(f"{me}: a tone table must be a contiguous uint8 [3][256]")
                    tones[b] = t.data_ptr()
                    where.add(True)
                else:
                    a = np.asarray(t)
                    if a.dtype != np.uint8 or a.shape != (3, 256):
                        raise ValueError(f"{me}: a tone table must be a contiguous uint8 [3][256]")
                    if not per_frame and b:  # the one table of all frames: one address, so it goes up once
                        tones[b] = tones[0]
                        continue
                    a = np.ascontiguousarray(a)
                    keep.append(a)
                    tones[b] = a.ctypes.data
                    where.add(False)
        if where != {bool(on_device)}:
            raise ValueError(f"{me}: frames and tone tables are all host arrays, or all device tensors with on_device=True")
        self.H.network_frames_bayer_input_gpu(self.h, ptrs, ws, hs, ps, BAYER_PATTERN[pattern], RAW_SAMPLE[sample], shift, tones,
                                              int(bool(on_device)))
        if self._enqueued_only(on_device):
            return None
        return self._prepared(self._pull_input())

    def push_input(self, x_u8):
        x = np.ascontiguousarray(x_u8, np.uint8).ravel()
        assert x.size == self.batch * self.inputs
        self._keep = x
        self.H.push_network_input_uint8(self.h, x.ctypes.data)

    def input_gpu_ptr(self):
        return self.H.dnq_net_input_gpu(self.h)

    def stream(self):
        return self.H.dnq_net_stream(self.h)

    def forward(self):
        self.H.forward_network_gpu(self.h)

    def sync(self):
        check(shim().mi355_stream_sync(self.stream()), "sync")

    def pull(self, i):
        self.H.pull_layer_output(self.h, i)
        cnt = self.batch * self.info[i]["outputs"]
        out = {}
        ty = self.info[i]["type"]
        if ty != T_YOLO:
            out["u8"] = _as(self.H.dnq_layer_u8(self.h, i), cnt, C.c_uint8).copy()
        if ty == T_CONV:
            out["int32"] = _as(self.H.dnq_layer_int32(self.h, i), cnt, C.c_int32).copy()
        if ty == T_YOLO or (self.info[i]["quant_stop"] and (self.keep_head_float or ty != T_CONV or not self.fuses_next(i))):
            out["f32"] = _as(self.H.dnq_layer_f32(self.h, i), cnt, C.c_float).copy()
        return out

    def conv_kernel(self, i):
        """mi355_last_conv_kernel code of the kernel that served conv layer i in the last forward pass (5 = conv_rows / conv_igemm)"""
        return int(self.H.dnq_layer_conv_kernel(self.h, i))

    def is_fused(self, i):
        """conv i runs fused with the layer after it and its own uint8 tensor is not stored."""
        return bool(self.H.dnq_layer_is_fused(self.h, i))

    def fuses_next(self, i):
        """layer i + 1 runs inside conv i's kernel (conv i's own tensor may be stored too: a conv + pool whose output a route reads)."""
        return bool(self.H.dnq_layer_fuses_next(self.h, i))

    def plan(self, i):
        """The planner's decisions for layer i as they stand now (dnq_layer_plan): after a forward pass the fuse flags a launcher
        refused are 0."""
        a = (C.c_int * 8)()
        assert self.H.dnq_layer_plan(self.h, i, a) == 0
        return dict(zip(PLAN_KEYS, list(a)))

    def prep(self, i):
        n = max(self.info[i]["n"], 1)
        b = np.zeros(n, np.int32); mv = np.zeros(n, np.float64); sv = np.zeros(n, np.float64)
        m0 = np.zeros(n, np.int32); sh = np.zeros(n, np.int32); q = np.zeros(4, np.float32)
        self.H.dnq_layer_prep(self.h, i, b.ctypes.data, mv.ctypes.data, sv.ctypes.data, m0.ctypes.data,
                              sh.ctypes.data, q.ctypes.data)
        return dict(biases_int32=b, M_value=mv, shift_value=sv, M0=m0, shift=sh, s_in=q[0], zp_in=int(q[1]),
                    s_act=q[2], zp_act=int(q[3]))

    def detections(self, i, classes, imw, imh, thresh, relative, max_recs):
        """Box decode of yolo layer i on the device: (counts [B], records [B][max_recs][6 + classes], reference order)."""
        recs = np.zeros((self.batch, max_recs, 6 + classes), np.float32)
        counts = np.zeros(self.batch, np.int32)
        self.H.network_yolo_detections_gpu(self.h, i, imw, imh, C.c_float(thresh), int(relative), recs.ctypes.data, max_recs,
                                           counts.ctypes.data)
        return counts, recs

    def detections_sizes(self, i, classes, imw, imh, thresh, relative, max_recs):
        """detections() with one source image size per batch slot: imw, imh are sequences of `batch` ints."""
        recs = np.zeros((self.batch, max_recs, 6 + classes), np.float32)
        counts = np.zeros(self.batch, np.int32)
        w = np.ascontiguousarray(imw, np.int32)
        h = np.ascontiguousarray(imh, np.int32)
        assert w.size == self.batch and h.size == self.batch
        self.H.network_yolo_detections_gpu_sizes(self.h, i, w.ctypes.data, h.ctypes.data, C.c_float(thresh), int(relative),
                                                 recs.ctypes.data, max_recs, counts.ctypes.data)
        return counts, recs

    def detections_shape(self):
        """(number of yolo layers, their common class count, candidates per image) of the batched decode; raises MI355Error for a
        network it refuses (no yolo layer, more than YOLO_MAX_HEADS, differing class counts)."""
        nh, cl, ca = C.c_int(), C.c_int(), C.c_int()
        rc = self.H.network_detections_batch_shape(self.h, C.byref(nh), C.byref(cl), C.byref(ca))
        if rc != 0:
            raise MI355Error(f"network_detections_batch_shape: code {rc} (the yolo layers of this network cannot be decoded together)")
        return nh.value, cl.value, ca.value

    def _sizes(self, imw, imh):
        w = np.ascontiguousarray(np.broadcast_to(np.asarray(imw, np.int32), (self.batch,)))
        h = np.ascontiguousarray(np.broadcast_to(np.asarray(imh, np.int32), (self.batch,)))
        return w, h

    def detections_batch(self, imw, imh, thresh, relative=1, max_per_image=None):
        """Box decode of every yolo layer and every image in one call (network_yolo_detections_batch_gpu): (counts [B, nheads] found per
        image and layer, offsets [B + 1], records [total, 6 + classes]); image b's records are recs[offsets[b]:offsets[b + 1]], yolo
        layers in network order, rank ascending inside a layer.  imw / imh: scalars or length-B sequences.  max_per_image: an image
        keeps its first max_per_image records (None: all)."""
        nh, classes, cand = self.detections_shape()
        w, h = self._sizes(imw, imh)
        cap = cand if max_per_image is None or max_per_image <= 0 else min(int(max_per_image), cand)
        recs = np.zeros((self.batch * cap, 6 + classes), np.float32)
        counts = np.zeros((self.batch, nh), np.int32)
        offsets = np.zeros(self.batch + 1, np.int32)
        rc = self.H.network_yolo_detections_batch_gpu(self.h, w.ctypes.data, h.ctypes.data, C.c_float(thresh), int(relative), cap,
                                                      recs.ctypes.data, counts.ctypes.data, offsets.ctypes.data)
        if rc != 0:
            raise MI355Error(f"network_yolo_detections_batch_gpu: code {rc} (refused: see stderr)")
        return counts, offsets, recs[:offsets[-1]].copy()

    def detect(self, imw, imh, thresh=.5, nms=.45, relative=True, max_per_image=None):
        """Final boxes of every image of the batch (network_detections_batch, then the host's do_nms_sort on each image): a list of
        dicts, one per image: boxes [k, 4] (x, y, w, h), objectness [k], probs [k, classes] with the scores NMS suppressed set to 0,
        rows in the reference's order (yolo layers in network order, rank ascending); found = candidates above thresh, kept = k."""
        nh, classes, cand = self.detections_shape()
        w, h = self._sizes(imw, imh)
        B = self.batch
        dets, num = (C.c_void_p * B)(), (C.c_int * B)()
        rc = self.H.network_detections_batch(self.h, w.ctypes.data, h.ctypes.data, C.c_float(thresh), int(bool(relative)), C.c_float(0.0),
                                             0 if max_per_image is None else int(max_per_image), dets, num)
        if rc != 0:
            raise MI355Error(f"network_detections_batch: code {rc} (refused: see stderr)")
        counts = self._last_counts()
        out = []
        for b in range(B):
            k = num[b]
            boxes, obj, probs = np.zeros((k, 4), np.float32), np.zeros(k, np.float32), np.zeros((k, classes), np.float32)
            self.H.detections_to_arrays(dets[b], k, classes, boxes.ctypes.data, obj.ctypes.data, probs.ctypes.data)
            if nms and nms > 0:  # rows keep their place, suppressed scores become 0
                self.H.do_nms_sort_arrays(boxes.ctypes.data, probs.ctypes.data, obj.ctypes.data, k, classes, C.c_float(nms))
            out.append(dict(boxes=boxes, objectness=obj, probs=probs, found=int(counts[b].sum()), kept=int(k)))
        self.H.free_detections_batch(dets, num, B)
        return out

    def set_frame_views(self, views, sizes=None):
        """network_set_frame_views: one view per batch slot for the prepare_from_frames_* / _jpeg / _png calls that follow --
        (x0, y0, w, h, orient) tuples or FrameView; None for a slot means its whole frame, orient 1, and needs sizes[b] = (w, h) of that
        frame.  views = None clears: every slot is its whole frame as stored again."""
        if views is None:
            self.H.network_set_frame_views(self.h, None)
            return
        if len(views) != self.batch:
            raise ValueError(f"set_frame_views: {len(views)} views for a batch of {self.batch}")
        if any(v is None for v in views) and sizes is None:
            raise ValueError("set_frame_views: a None view needs sizes, the (w, h) of every slot's frame")
        table = (FrameView * self.batch)()
        for b, v in enumerate(views):
            table[b] = frame_view(v, *(sizes[b] if v is None else (None, None)))
        self.H.network_set_frame_views(self.h, table)

    def detect_views(self, frame_w, frame_h, frame_of_slot=None, thresh=.5, nms=.45, max_per_image=None):
        """network_detections_views: the detections of a batch of views per FRAME.  frame_w, frame_h: the frame sizes per slot (or one
        for all); frame_of_slot[b]: which frame slot b looks at (default: frame 0 for every slot).  Boxes are relative to the frame;
        the slots of a frame are concatenated and go through one do_nms_sort.  Returns {frame: dict(boxes [k, 4], objectness [k],
        probs [k, classes])} in the NMS's order, suppressed scores 0."""
        classes = self.detections_shape()[1]
        w, h = self._sizes(frame_w, frame_h)
        B = self.batch
        fos = np.ascontiguousarray(np.zeros(B, np.int32) if frame_of_slot is None else frame_of_slot, np.int32)
        if fos.shape != (B,):
            raise ValueError("detect_views: frame_of_slot needs one entry per slot")
        dets, num = (C.c_void_p * B)(), (C.c_int * B)()
        rc = self.H.network_detections_views(self.h, w.ctypes.data, h.ctypes.data, fos.ctypes.data, C.c_float(thresh), C.c_float(nms or 0.0),
                                             0 if max_per_image is None else int(max_per_image), dets, num)
        if rc != 0:
            raise MI355Error(f"network_detections_views: code {rc} (refused: see stderr)")
        out = {}
        for f in sorted(set(fos.tolist())):
            k = num[f]
            boxes, obj, probs = np.zeros((k, 4), np.float32), np.zeros(k, np.float32), np.zeros((k, classes), np.float32)
            self.H.detections_to_arrays(dets[f], k, classes, boxes.ctypes.data, obj.ctypes.data, probs.ctypes.data)
            out[f] = dict(boxes=boxes, objectness=obj, probs=probs)
        self.H.free_detections_batch(dets, num, B)
        return out

    def _last_counts(self):
        """counts [B, nheads] of the last batched decode (the host's staging copy)"""
        nh = self.detections_shape()[0]
        p = self.H.dnq_net_detb_counts(self.h)
        return _as(p, self.batch * nh, C.c_int).copy().reshape(self.batch, nh)

    def layer0_entry(self, scale, zp):
        """Host-side bank entry of layer 0 for one (input scale, zero point): the bytes the per-image path uploads for it."""
        info = self.info[0]
        out = np.zeros(int(shim().mi355_conv_pack_size(info["n"], info["c"], info["size"])), np.uint8)
        self.H.network_layer0_entry(self.h, C.c_float(scale), int(zp), out.ctypes.data)
        return out

    def bank_entry_bytes(self):
        """per-image mode: byte stride of the layer-0 bank (0 before the first per-image batch)"""
        return int(self.H.dnq_net_pi_entry_bytes(self.h))

    def graph_handle(self):
        """the captured graph of the layer loop, or None (use_graph networks capture on their first forward)"""
        return self.H.dnq_net_graph(self.h)

    def bank_packed(self):
        """per-image mode: bank entries packed by the last batch (the others were cached)"""
        return int(self.H.dnq_net_pi_packed(self.h))

    def selfcheck(self, passes):
        """queue `passes` forward passes over the resident input with a device-side checksum of the yolo outputs after each
        (nothing is synchronised); selfcheck_result() -> number of passes that differ from the first"""
        self.H.network_selfcheck(self.h, passes)

    def selfcheck_result(self):
        return int(self.H.network_selfcheck_result(self.h))

    def profile_begin(self, max_steps, stride=1, phase=0):
        """record per-layer events on the forward passes whose index (from now) % stride == phase, at most max_steps of them"""
        self.H.network_profile_set_stride(self.h, stride)
        self.H.network_profile_set_phase(self.h, phase)
        self.H.network_profile_begin(self.h, max_steps)

    def profile_read(self):
        ms = np.zeros(self.n + 1, np.float32)
        steps = self.H.network_profile_read(self.h, ms.ctypes.data)
        return steps, ms

    def packed_size(self):
        return self.H.network_packed_size(self.h)

    def export_packed(self):
        buf = np.zeros(self.packed_size(), np.uint8)
        self.H.network_export_packed(self.h, buf.ctypes.data)
        return buf

    def save_packed(self, path):
        self.H.network_save_packed(self.h, path.encode())

    def load_packed(self, path):
        """Packed file -> host blobs -> device (the on-disk twin of import_packed)."""
        self.H.network_load_packed(self.h, path.encode())

    def shortcut_multipliers(self, i):
        k = (C.c_int32 * 3)()
        assert self.H.dnq_layer_shortcut(self.h, i, k) == 0
        return int(k[0]), int(k[1])

    def shortcut_from(self, i):
        k = (C.c_int32 * 3)()
        assert self.H.dnq_layer_shortcut(self.h, i, k) == 0
        return int(k[2])

    def import_packed(self, buf):
        buf = np.ascontiguousarray(buf, np.uint8)
        self.H.network_import_packed(self.h, buf.ctypes.data, buf.nbytes)

    def import_packed_host(self, buf):
        buf = np.ascontiguousarray(buf, np.uint8)
        self.H.network_import_packed_host(self.h, buf.ctypes.data, buf.nbytes)

    def import_packed_gpu(self, dev_ptr, nbytes):
        self.H.network_import_packed_gpu(self.h, dev_ptr, nbytes)

    def close(self):
        if self.h:
            self.H.free_network(self.h)
            self.h = None
