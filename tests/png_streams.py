"""A small PNG writer and a deflate stream builder for the PNG tests and tests/golden/make_golden_png.py: the filter of every row,
the interlace flag, the chunking and the shape of the deflate stream are chosen here (struct + zlib; nothing else can choose them)."""
import struct
import zlib

import numpy as np

import png_ref

SIG = b"\x89PNG\r\n\x1a\n"


def chunk(kind, data=b""):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data))


def ihdr(w, h, depth, color, interlace=0, comp=0, filt=0):
    return chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, color, comp, filt, interlace))


def filtered_stream(samples, depth, color, interlace, filters):
    """samples: int [h][w][channels]; filters: a function (pass index, row) -> 0..4.  The bytes a PNG encoder deflates."""
    s = np.asarray(samples)
    bpp = png_ref.filter_unit(depth, color)
    out = []
    for k, p in (png_ref.adam7_split(s).items() if interlace else [(0, s)]):
        rows = png_ref.pack_samples(p, depth)
        out.append(png_ref.filter_rows(rows, [filters(k, y) for y in range(rows.shape[0])], bpp).tobytes())
    return b"".join(out)


def split(data, sizes):
    """data cut into pieces of the sizes given, cyclically"""
    out, at, i = [], 0, 0
    while at < len(data):
        n = sizes[i % len(sizes)]
        out.append(data[at:at + n])
        at += n
        i += 1
    return out


def write_png(samples, depth, color, interlace=0, filters=lambda k, y: 0, palette=None, trns=None, idat_sizes=None, before=(), between=(),
              deflate=lambda raw: zlib.compress(raw, 9), trailing=b""):
    """The file's bytes.  palette: uint8 [n][3]; trns: the tRNS chunk's data; idat_sizes: cut the zlib stream into IDAT chunks of these
    sizes (cyclically); before / between: whole chunks put before the first IDAT / between the IDAT chunks; trailing: bytes appended to
    the filtered stream before it is deflated."""
    s = np.asarray(samples)
    h, w = s.shape[:2]
    z = deflate(filtered_stream(s, depth, color, interlace, filters) + trailing)
    parts = [SIG, ihdr(w, h, depth, color, interlace)]
    parts += list(before)
    if palette is not None:
        parts.append(chunk(b"PLTE", np.asarray(palette, np.uint8).tobytes()))
    if trns is not None:
        parts.append(chunk(b"tRNS", bytes(trns)))
    pieces = split(z, idat_sizes) if idat_sizes else [z]
    for i, piece in enumerate(pieces):
        parts.append(chunk(b"IDAT", piece))
        if i + 1 < len(pieces) and i < len(between):
            parts.append(between[i])
    parts.append(chunk(b"IEND"))
    return b"".join(parts)


def chunks_of(data):
    """[(type, data)] of a PNG file's chunks"""
    out, pos = [], 8
    while pos + 8 <= len(data):
        n, kind = struct.unpack(">I4s", data[pos:pos + 8])
        out.append((kind, data[pos + 8:pos + 8 + n]))
        pos += 12 + n
    return out


def idat_of(data):
    return b"".join(d for k, d in chunks_of(data) if k == b"IDAT")


# ---- deflate ---------------------------------------------------------------------------------------------------------
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
             16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
FIXED_LITLEN = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def canonical(lengths):
    """{symbol: (code, length)} of the canonical Huffman code with these lengths (RFC 1951 3.2.2)"""
    count = [0] * 16
    for n in lengths:
        count[n] += 1
    count[0] = 0
    code, nxt = 0, [0] * 16
    for bits in range(1, 16):
        code = (code + count[bits - 1]) << 1
        nxt[bits] = code
    out = {}
    for sym, n in enumerate(lengths):
        if n:
            out[sym] = (nxt[n], n)
            nxt[n] += 1
    return out


def length_symbol(n):
    if n == 258:
        return 28
    return max(i for i in range(28) if LEN_BASE[i] <= n)


def dist_symbol(d):
    return max(i for i in range(30) if DIST_BASE[i] <= d)


class Deflate:
    """A deflate stream put together block by block.  Tokens: an int is a literal, (length, distance) a match."""

    def __init__(self):
        self.acc, self.n, self.out, self.raw = 0, 0, bytearray(), bytearray()

    def bits(self, value, n):
        """n bits, least significant first (header fields, extra bits)"""
        self.acc |= (value & ((1 << n) - 1)) << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, pair):
        """a Huffman code, most significant bit first"""
        c, n = pair
        self.bits(int(format(c, "0%db" % n)[::-1], 2), n)

    def _track(self, tokens):
        for t in tokens:
            if isinstance(t, tuple):
                for _ in range(t[0]):
                    self.raw.append(self.raw[-t[1]] if t[1] <= len(self.raw) else 0)  # (a distance too far: refusal files only)
            else:
                self.raw.append(t)

    def stored(self, data, final=False):
        self.bits(1 if final else 0, 1)
        self.bits(0, 2)
        if self.n:
            self.bits(0, 8 - self.n)
        self.out += struct.pack("<HH", len(data), len(data) ^ 0xFFFF) + bytes(data)
        self.raw += bytes(data)

    def _tokens(self, tokens, lit, dist):
        for t in tokens:
            if isinstance(t, tuple):
                ls, ds = length_symbol(t[0]), dist_symbol(t[1])
                self.code(lit[257 + ls])
                self.bits(t[0] - LEN_BASE[ls], LEN_EXTRA[ls])
                self.code(dist[ds])
                self.bits(t[1] - DIST_BASE[ds], DIST_EXTRA[ds])
            else:
                self.code(lit[t])
        self.code(lit[256])
        self._track(tokens)

    def fixed(self, tokens, final=False):
        self.bits(1 if final else 0, 1)
        self.bits(1, 2)
        self._tokens(tokens, canonical(FIXED_LITLEN), canonical(FIXED_DIST))

    def dynamic(self, tokens, litlen, dist, final=False):
        """litlen: code lengths of symbols 0 .. (at least 257 of them), dist: of the distance symbols (at least one).  The code
        lengths go out one by one under a complete code-length code of 4- and 5-bit codes: no repeat codes."""
        self.bits(1 if final else 0, 1)
        self.bits(2, 2)
        self.bits(len(litlen) - 257, 5)
        self.bits(len(dist) - 1, 5)
        self.bits(19 - 4, 4)
        cl = [4] * 13 + [5] * 6  # a complete code over the 19 symbols (zlib refuses an incomplete code-length code)
        by_symbol = canonical(cl)
        for s in CL_ORDER:
            self.bits(cl[s], 3)
        for n in list(litlen) + list(dist):
            self.code(by_symbol[n])
        self._tokens(tokens, canonical(litlen), canonical(dist))

    def finish(self):
        if self.n:
            self.bits(0, 8 - self.n)
        return bytes(self.out)

    def zlib(self):
        """the stream in a zlib wrapper (no preset dictionary, Adler-32 of what it inflates to)"""
        return b"\x78\x01" + self.finish() + struct.pack(">I", zlib.adler32(bytes(self.raw)))


def lengths_for(symbols, total, long_symbol=None):
    """Code lengths of a complete code over `symbols` (a set of used symbols among 0 .. total - 1): a chain 1, 2, 3, .. n - 1, n - 1
    where that fits in 15 bits, else a balanced code.  long_symbol, where given, takes one of the two longest codes."""
    syms = sorted(symbols)
    if long_symbol is not None:
        syms.remove(long_symbol)
        syms.append(long_symbol)
    out = [0] * total
    n = len(syms)
    if n == 1:
        out[syms[0]] = 1
        return out
    if n <= 16:
        for i, s in enumerate(syms):
            out[s] = min(i + 1, n - 1)
        return out
    bits = (n - 1).bit_length()
    short = (1 << bits) - n  # codes that can be one bit shorter
    for i, s in enumerate(syms):
        out[s] = bits - 1 if i < short else bits
    return out


# ---- files the decoder refuses ----------------------------------------------------------------------------------------
def _rgb(w=3, h=2):
    return np.arange(h * w * 3).reshape(h, w, 3) % 256


def _idat(raw):
    return chunk(b"IDAT", zlib.compress(raw))


def refusal_files():
    """{name: (file bytes, the message the decoder gives)}: one file per refusal of yolo_quantization_amd/host/png.c"""
    raw = filtered_stream(_rgb(), 8, 2, 0, lambda k, y: 0)  # 2 rows of 1 + 9 bytes
    head, end = SIG + ihdr(3, 2, 8, 2), chunk(b"IEND")
    pal_head = SIG + ihdr(3, 2, 8, 3)
    pal_raw = bytes([0, 0, 1, 2, 0, 1, 0, 1])
    plte = chunk(b"PLTE", bytes(range(9)))

    def with_ihdr(**kw):
        a = dict(w=3, h=2, depth=8, color=2, interlace=0, comp=0, filt=0)
        a.update(kw)
        return SIG + ihdr(a["w"], a["h"], a["depth"], a["color"], a["interlace"], a["comp"], a["filt"]) + _idat(raw) + end

    def with_zlib(z):
        return head + chunk(b"IDAT", z) + end

    good = zlib.compress(raw)
    bad_filter = bytearray(raw)
    bad_filter[10] = 5
    d_type3 = Deflate()
    d_type3.bits(1, 1)
    d_type3.bits(3, 2)
    d_dist = Deflate()
    d_dist.fixed([1, 2, (3, 5)] + [0] * 20, final=True)  # a match that reaches before the start of the output
    d_lens = Deflate()  # dynamic block whose code-length code is over-subscribed
    d_lens.bits(1, 1); d_lens.bits(2, 2); d_lens.bits(0, 5); d_lens.bits(0, 5); d_lens.bits(15, 4)
    for i in range(19):
        d_lens.bits((1, 2, 2, 2)[i] if i < 4 else 0, 3)  # one code of 1 bit and three of 2
    files = {
        "no_signature": (b"\x89PNX\r\n\x1a\n" + ihdr(3, 2, 8, 2) + _idat(raw) + end, "bad png sig"),
        "first_not_ihdr": (SIG + chunk(b"gAMA", struct.pack(">I", 45455)) + ihdr(3, 2, 8, 2) + _idat(raw) + end, "first not IHDR"),
        "multiple_ihdr": (head + ihdr(3, 2, 8, 2) + _idat(raw) + end, "multiple IHDR"),
        "bad_ihdr_len": (SIG + chunk(b"IHDR", struct.pack(">IIBBBBBB", 3, 2, 8, 2, 0, 0, 0, 0)) + _idat(raw) + end, "bad IHDR len"),
        "depth_3": (with_ihdr(depth=3), "1/2/4/8/16-bit only"),
        "ctype_7": (with_ihdr(color=7), "bad ctype"),
        "ctype_5": (with_ihdr(color=5), "bad ctype"),
        "palette_16": (with_ihdr(color=3, depth=16), "bad ctype"),
        "comp_method": (with_ihdr(comp=1), "bad comp method"),
        "filter_method": (with_ihdr(filt=1), "bad filter method"),
        "interlace_2": (with_ihdr(interlace=2), "bad interlace method"),
        "zero_width": (with_ihdr(w=0), "0-pixel image"),
        "invalid_plte": (head + chunk(b"PLTE", bytes(10)) + _idat(raw) + end, "invalid PLTE"),
        "trns_after_idat": (pal_head + plte + _idat(pal_raw) + chunk(b"tRNS", b"\x00") + end, "tRNS after IDAT"),
        "trns_before_plte": (pal_head + chunk(b"tRNS", b"\x00") + plte + _idat(pal_raw) + end, "tRNS before PLTE"),
        "bad_trns_len_palette": (pal_head + plte + chunk(b"tRNS", bytes(4)) + _idat(pal_raw) + end, "bad tRNS len"),
        "bad_trns_len_rgb": (head + chunk(b"tRNS", bytes(2)) + _idat(raw) + end, "bad tRNS len"),
        "trns_with_alpha": (SIG + ihdr(3, 2, 8, 6) + chunk(b"tRNS", bytes(8)) + _idat(bytes(26)) + end, "tRNS with alpha"),
        "no_plte": (pal_head + _idat(pal_raw) + end, "no PLTE"),
        "no_idat": (head + end, "no IDAT"),
        "unknown_critical": (head + chunk(b"ABCD", b"xy") + _idat(raw) + end, "ABCD PNG chunk not known"),
        "bad_zlib_header": (with_zlib(b"\x78\x02" + good[2:]), "bad zlib header"),
        "preset_dict": (with_zlib(b"\x78\x20" + good[2:]), "no preset dict"),
        "bad_block_type": (with_zlib(b"\x78\x01" + d_type3.finish() + bytes(8)), "bad block type"),
        "bad_codelengths": (with_zlib(b"\x78\x01" + d_lens.finish() + bytes(8)), "bad codelengths"),
        "bad_dist": (with_zlib(b"\x78\x01" + d_dist.finish() + bytes(4)), "bad dist"),
        "not_enough_pixels": (head + _idat(raw[:-1]) + end, "not enough pixels"),
        "invalid_filter": (head + _idat(bytes(bad_filter)) + end, "invalid filter"),
        "too_wide": (with_ihdr(w=32769), "width or height above 32768"),
        "cgbi": (SIG + chunk(b"CgBI", bytes(4)) + ihdr(3, 2, 8, 2) + _idat(raw) + end, "CgBI"),
    }
    return files
