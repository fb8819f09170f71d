"""A coefficient-level baseline JPEG encoder for the entropy-decode tests: chosen coefficients, sampling factors, scan layout, restart
interval and CHOSEN CODE LENGTHS of the Huffman tables go in, a file jpeg_decode_host accepts comes out.  numpy and plain Python; the
streams the tests build are a few kilobytes.  (tests/golden/make_golden_jpeg.py's write_coefficient_jpeg is the shape.)"""
import struct

import numpy as np

ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56,
          57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]

# DC categories 0..11 in 1..12 bits and category 15 in 16; AC symbols of 2..10 bits and (0, 15) in 16: short codes, codes behind the
# 8-bit lookup, and 31-bit symbols (a 16-bit code and 15 value bits)
DC_LENGTHS = {**{c: c + 1 for c in range(12)}, 15: 16}
AC_LENGTHS = {0x00: 2, 0x01: 2, 0x02: 3, 0x11: 4, 0x03: 5, 0x21: 6, 0xF0: 7, 0x04: 8, 0x31: 9, 0x12: 10, 0x0F: 16}


def table(lengths):
    """{symbol: code length} -> (counts[16], values, {symbol: (code, length)}): the canonical codes of T.81 C.2, symbols of one length
    in the order given"""
    order = sorted(lengths, key=lambda s: lengths[s])  # stable
    counts = [sum(1 for s in order if lengths[s] == l) for l in range(1, 17)]
    code, codes, k = 0, {}, 0
    for l in range(1, 17):
        for _ in range(counts[l - 1]):
            codes[order[k]] = (code, l)
            code += 1
            k += 1
        assert code <= 1 << l, "these lengths are no prefix code"
        code <<= 1
    return counts, order, codes


class Bits:
    def __init__(self):
        self.bits = []  # (value, n)
        self.n = 0

    def put(self, v, n):
        if n:
            self.bits.append((v, n))
            self.n += n

    def flush(self):
        """the bytes, padded with 1-bits, stuffed"""
        acc = 0
        for v, n in self.bits:
            acc = acc << n | v
        pad = -self.n % 8
        acc = acc << pad | ((1 << pad) - 1)
        raw = acc.to_bytes((self.n + pad) // 8, "big") if self.n else b""
        return raw.replace(b"\xff", b"\xff\x00"), raw


def magnitude(v):
    size = int(abs(v)).bit_length()
    return size, (v if v >= 0 else v + (1 << size) - 1)


def encode_block(bw, blk, pred, dc, ac):
    """blk: 64 coefficients, natural order.  The DC difference is taken modulo 2^16 into -32767 .. 32767."""
    diff = (int(blk[0]) - pred + 32768) % 65536 - 32768
    size, bits = magnitude(diff)
    bw.put(*dc[size])
    bw.put(bits, size)
    zz = [int(blk[ZIGZAG[k]]) for k in range(64)]
    last = max([k for k in range(1, 64) if zz[k]], default=0)
    run = 0
    for k in range(1, last + 1):
        if zz[k] == 0:
            run += 1
            continue
        while run > 15:
            bw.put(*ac[0xF0])
            run -= 16
        size, bits = magnitude(zz[k])
        bw.put(*ac[run << 4 | size])
        bw.put(bits, size)
        run = 0
    if last < 63:
        bw.put(*ac[0x00])
    return int(blk[0])


def build(w, h, comps, coef, scans=None, tables=None, restart=0, raw=None):
    """comps: [(id, h, v)]; coef: per component int [blocks_h][blocks_w][64], natural order, the MCU-padded planes; scans: a list of
    {"comps": [component index, ..], "dc": [table id, ..], "ac": [..], "tables": {("dc" | "ac", id): lengths} written in front of it}
    (default: one scan of all components on tables 0); tables: those written in front of the first scan (default DC_LENGTHS /
    AC_LENGTHS as table 0); raw: {scan index: Bits}, hand-made bits that stand for the whole scan's data (damaged streams).  Returns
    the file and, per scan, the unstuffed bytes of each restart interval."""
    tables = tables if tables is not None else {("dc", 0): DC_LENGTHS, ("ac", 0): AC_LENGTHS}
    scans = scans or [{"comps": list(range(len(comps))), "dc": [0] * len(comps), "ac": [0] * len(comps)}]
    hmax, vmax = max(c[1] for c in comps), max(c[2] for c in comps)
    mx, my = -(-w // (8 * hmax)), -(-h // (8 * vmax))
    current = {}

    def dht(tabs):
        seg = b""
        for (kind, tid), lengths in tabs.items():
            counts, values, codes = table(lengths)
            current[(kind, tid)] = codes
            seg += b"\xff\xc4" + struct.pack(">H", 19 + len(values)) + bytes([(kind == "ac") << 4 | tid]) + bytes(counts) + bytes(values)
        return seg

    out = bytearray(b"\xff\xd8\xff\xe0" + struct.pack(">H", 16) + b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    out += b"\xff\xdb" + struct.pack(">H", 67) + b"\x00" + bytes([1] * 64)
    out += b"\xff\xc0" + struct.pack(">HBHHB", 8 + 3 * len(comps), 8, h, w, len(comps))
    for cid, ch, cv in comps:
        out += bytes([cid, ch << 4 | cv, 0])
    if restart:
        out += b"\xff\xdd" + struct.pack(">HH", 4, restart)
    out += dht(tables)
    segments = []
    for si, scan in enumerate(scans):
        out += dht(scan.get("tables", {}))
        ns = len(scan["comps"])
        out += b"\xff\xda" + struct.pack(">HB", 6 + 2 * ns, ns)
        for ci, d, a in zip(scan["comps"], scan["dc"], scan["ac"]):
            out += bytes([comps[ci][0], d << 4 | a])
        out += b"\x00\x3f\x00"
        units = []  # per unit: [(component, by, bx)]
        if ns == 1:  # the component's own blocks in raster order, over its real size
            ci = scan["comps"][0]
            cw, chh = -(-(w * comps[ci][1]) // hmax), -(-(h * comps[ci][2]) // vmax)
            units = [[(0, by, bx)] for by in range(-(-chh // 8)) for bx in range(-(-cw // 8))]
        else:
            for uy in range(my):
                for ux in range(mx):
                    units.append([(i, uy * comps[ci][2] + yy, ux * comps[ci][1] + xx) for i, ci in enumerate(scan["comps"])
                                  for yy in range(comps[ci][2]) for xx in range(comps[ci][1])])
        interval = restart or len(units)
        if raw and si in raw:
            stuffed, unstuffed = raw[si].flush()
            out += stuffed
            segments.append([unstuffed])
            continue
        mine = []
        for n, first in enumerate(range(0, len(units), interval)):
            if n:
                out += bytes([0xFF, 0xD0 + (n - 1) % 8])
            bw, pred = Bits(), [0] * ns
            for unit in units[first:first + interval]:
                for i, by, bx in unit:
                    ci = scan["comps"][i]
                    pred[i] = encode_block(bw, coef[ci][by, bx], pred[i], current[("dc", scan["dc"][i])], current[("ac", scan["ac"][i])])
            stuffed, plain = bw.flush()
            out += stuffed
            mine.append(plain)
        segments.append(mine)
    out += b"\xff\xd9"
    return bytes(out), segments


def planes(w, h, comps):
    """zero coefficient planes of the MCU-padded sizes"""
    hmax, vmax = max(c[1] for c in comps), max(c[2] for c in comps)
    mx, my = -(-w // (8 * hmax)), -(-h // (8 * vmax))
    return [np.zeros((my * cv, mx * ch, 64), np.int32) for _, ch, cv in comps]


def random_block(rng, dc, ac_lengths=AC_LENGTHS, most=12):
    """a block of up to `most` AC symbols, all of them in ac_lengths and below 15 bits"""
    blk = np.zeros(64, np.int32)
    blk[0] = dc
    syms = [s for s in ac_lengths if s & 15 and (s & 15) < 15]
    k = 1
    for _ in range(int(rng.integers(0, most + 1))):
        s = syms[int(rng.integers(len(syms)))]
        run, size = s >> 4, s & 15
        if k + run > 63:
            break
        k += run
        mag = int(rng.integers(1 << (size - 1), 1 << size))
        blk[ZIGZAG[k]] = mag if rng.integers(2) else -mag
        k += 1
    return blk


def block_bits(blk, pred, dc_lengths=DC_LENGTHS, ac_lengths=AC_LENGTHS):
    bw = Bits()
    encode_block(bw, blk, pred, table(dc_lengths)[2], table(ac_lengths)[2])
    return bw.n


def grey_stream(blocks, tables=None, restart=0):
    """one grey component, one row of len(blocks) blocks (8 n x 8 pixels), one scan"""
    n = len(blocks)
    coef = [np.asarray(blocks, np.int32).reshape(1, n, 64)]
    return build(8 * n, 8, [(1, 1, 1)], coef, tables=tables, restart=restart)


def grey_stream_of_bits(rng, nbits):
    """a grey stream of exactly nbits bits of entropy-coded data: random blocks, then blocks of 3 bits (DC difference 0, end of block) and
    5 bits (difference +-1, end of block) up to the bit"""
    assert nbits >= 8
    blocks, pred, have = [], 0, 0
    while nbits - have > 120:
        blk = random_block(rng, int(np.clip(pred + rng.integers(-40, 41), -900, 900)))
        have += block_bits(blk, pred)
        pred = int(blk[0])
        blocks.append(blk)
    left = nbits - have
    fives = next(b for b in range(3) if (left - 5 * b) % 3 == 0 and left - 5 * b >= 0)
    for i in range(fives):
        blk = np.zeros(64, np.int32)
        pred += 1 if i % 2 == 0 else -1
        blk[0] = pred
        blocks.append(blk)
    for _ in range((left - 5 * fives) // 3):
        blk = np.zeros(64, np.int32)
        blk[0] = pred
        blocks.append(blk)
    data, segs = grey_stream(blocks)
    assert len(segs[0][0]) == -(-nbits // 8)
    return data, blocks


def slow_settle(units=342):
    """three components at 1 x 1 on ONE DC and ONE AC table, every block 8 bits: a 3-bit DC code of category 2, 2 value bits, a 3-bit
    end of block.  At 32-bit subsequences the bits do not tell the slot inside the unit, so a lane is right only once its predecessor
    is.  The DC differences differ per component (2, 3, -2)."""
    dc = {2: 3, 0: 3, 1: 3}
    ac = {0x00: 3, 0x01: 3}
    side = int(np.ceil(np.sqrt(units)))
    mx, my = side, -(-units // side)
    comps = [(1, 1, 1), (2, 1, 1), (3, 1, 1)]
    coef = planes(8 * mx, 8 * my, comps)
    for c, d in enumerate((2, 3, -2)):
        coef[c][:, :, 0] = (d * (np.arange(mx * my) + 1)).reshape(my, mx)
    data, segs = build(8 * mx, 8 * my, comps, coef, tables={("dc", 0): dc, ("ac", 0): ac})
    assert len(segs[0][0]) == 3 * mx * my
    return data, coef


# ---- the streams both test files run ---------------------------------------------------------------------------------------------
ROUND_EDGES = (1, 2, 255, 256, 257, 511, 512, 513)


def round_edge_streams(seed=11):
    """one-segment grey streams of exactly n 32-bit subsequences (4 n bytes, the last four bits padding), n around the round of 256"""
    rng = np.random.default_rng(seed)
    return {f"subsequences_{n}": grey_stream_of_bits(rng, 32 * n - 4)[0] for n in ROUND_EDGES}


def symbol_edge_streams():
    """32 grey streams of 64-bit blocks -- a DC of category 15 on a 16-bit code (31 bits), an AC (0, 15) on a 16-bit code (31 bits), a
    2-bit end of block -- behind a prefix of 8 .. 39 bits: over the 32 streams every symbol starts at every offset of a 32-bit
    subsequence, and the symbols around bit 8192 lie across the edge of the first round at every offset"""
    out = {}
    for prefix in range(8, 40):
        fives = next(b for b in range(3) if (prefix - 5 * b) % 3 == 0 and prefix - 5 * b >= 0)
        blocks, pred = [], 0
        for i in range(fives + (prefix - 5 * fives) // 3):
            blk = np.zeros(64, np.int32)
            pred += (1 if i % 2 == 0 else -1) if i < fives else 0
            blk[0] = pred
            blocks.append(blk)
        for i in range(132):
            blk = np.zeros(64, np.int32)
            pred = pred + 32767 if i % 2 == 0 else pred - 32767
            blk[0] = pred
            blk[1] = (16384 + 37 * i) * (1 if i % 3 else -1)
            blocks.append(blk)
        out[f"prefix_{prefix}"] = grey_stream(blocks)[0]
    return out


def restart_stream(n=300, seed=12):
    """n grey blocks at restart interval 1: n segments, the DC prediction starts at zero in each"""
    rng = np.random.default_rng(seed)
    return grey_stream([random_block(rng, int(rng.integers(-1000, 1001)), most=4) for _ in range(n)], restart=1)[0]


def _random_planes(rng, w, h, comps):
    coef = planes(w, h, comps)
    for c in coef:
        dc = np.clip(np.cumsum(rng.integers(-30, 31, c.shape[0] * c.shape[1])), -900, 900)
        for n, (by, bx) in enumerate(np.ndindex(c.shape[0], c.shape[1])):
            c[by, bx] = random_block(rng, int(dc[n]), most=6)
    return coef


def unit_grid_streams(seed=13):
    """a one-component scan whose real size is narrower than its MCU-padded plane (17 x 9 at 2 x 2: a grid of 3 x 2 units in a plane 4
    blocks wide), and interleaved scans of 6 (4:2:0) and 18 (4 x 4 luma) blocks a unit at sizes that are no multiple of the unit"""
    rng = np.random.default_rng(seed)
    out = {}
    c420 = [(1, 2, 2), (2, 1, 1), (3, 1, 1)]
    one = [{"comps": [i], "dc": [0], "ac": [0]} for i in range(3)]
    out["noninterleaved_17x9"] = build(17, 9, c420, _random_planes(rng, 17, 9, c420), scans=one)[0]
    out["420_37x21"] = build(37, 21, c420, _random_planes(rng, 37, 21, c420))[0]
    c410 = [(1, 4, 4), (2, 1, 1), (3, 1, 1)]
    out["410_70x40"] = build(70, 40, c410, _random_planes(rng, 70, 40, c410))[0]
    out["420_restart3_37x21"] = build(37, 21, c420, _random_planes(rng, 37, 21, c420), restart=3)[0]
    return out


def damaged_streams():
    """{name: (file, status word)}: grey streams of 6 blocks whose third block holds a symbol that decodes to nothing -- a code no
    symbol has, a DC category of 16, a run that leaves the block.  jpeg_decode_host refuses each of them with that reason."""
    out = {}
    for name, dc_len, ac_len, code in (("no_code", DC_LENGTHS, AC_LENGTHS, 1), ("dc_category_16", {0: 1, 1: 2, 16: 3}, {0x00: 2, 0x01: 2}, 2),
                                       ("index_past_63", {0: 1, 1: 2}, {0x00: 2, 0x01: 2, 0xF1: 3}, 3)):
        dc, ac = table(dc_len)[2], table(ac_len)[2]
        bw = Bits()
        for sign in (1, 0):  # two good blocks: DC difference +1, -1, one AC coefficient of 1, end of block
            bw.put(*dc[1]); bw.put(sign, 1); bw.put(*ac[0x01]); bw.put(1, 1); bw.put(*ac[0x00])
        if name == "no_code":
            bw.put(0xFFFF, 16)
        elif name == "dc_category_16":
            bw.put(*dc[16])
        else:
            bw.put(*dc[0])
            for _ in range(4):
                bw.put(*ac[0xF1]); bw.put(1, 1)
        bw.put(0, 40)
        file, _ = build(48, 8, [(1, 1, 1)], planes(48, 8, [(1, 1, 1)]), tables={("dc", 0): dc_len, ("ac", 0): ac_len}, raw={0: bw})
        out[name] = (file, code)
    return out
