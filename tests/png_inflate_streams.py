"""Built deflate streams for the tests of the inflate on the device (mi355_png_inflate and its host emulation): the shapes at which a
round-based, ring-buffered decoder can go wrong, each as a Case the CPU tests give to the emulation and the GPU tests to the kernel.
The oracle is the host decoder, png_inflate_host through binding.png_inflate(zlib stream, cap), followed by the two checks
png_decode_host makes behind it (length, filter bytes).  Also the writer for hand-chosen repeat codes 16 / 17 / 18, which
png_streams.Deflate.dynamic never writes."""
import zlib

import numpy as np

import png_streams as ps
from yolo_quantization_amd import binding

REASONS = binding.PNG_INFLATE_ERRORS


class Case:
    """name; z: raw deflate data; cap; passes ([(rows, row_bytes)] or None: one row); reason: None (accepted) or the words expected"""

    def __init__(self, name, z, cap, reason=None, passes=None):
        if not isinstance(z, (bytes, bytearray)):
            z = z.finish()
        self.name, self.z, self.cap, self.reason, self.passes = name, bytes(z), cap, reason, passes

    def rows(self):
        return self.passes if self.passes is not None else [(1, self.cap - 1)]


def oracle(case):
    """(reason | None, bytes | None) of the host decoder on the case: png_inflate_host, then "not enough pixels", then the filter bytes"""
    try:
        got = binding.png_inflate(b"\x78\x01" + case.z, case.cap)
    except binding.PngError as e:
        return str(e), None
    if len(got) < case.cap:
        return "not enough pixels", None
    at = 0
    for rows, rb in case.rows():
        for _ in range(rows):
            if got[at] > 4:
                return "invalid filter", None
            at += rb + 1
    assert at == case.cap
    return None, got


def check(cases, outs, statuses):
    """what a launch (or the emulation) gave for the cases, against the oracle and against the reasons the cases name"""
    assert len(outs) == len(statuses) == len(cases)
    for c, out, st in zip(cases, outs, statuses):
        reason, want = oracle(c)
        assert reason == c.reason, (c.name, "the oracle says", reason)
        if reason is None:
            assert st == 0, (c.name, REASONS.get(st, st))
            assert out == want, (c.name, "first difference at", next(i for i in range(c.cap) if out[i] != want[i]))
        else:
            assert st != 0 and REASONS[st] == reason, (c.name, REASONS.get(st, st), reason)


def filler(n, seed=1):
    """n bytes that do not repeat at short distances; byte 0 is a valid filter byte"""
    a = np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)
    if n:
        a[0] = 0
    return a.tobytes()


def stored_bulk(d, data):
    for at in range(0, len(data), 65535):
        d.stored(data[at:at + 65535])


# ---- hand-chosen repeat codes ----------------------------------------------------------------------------------------------------
CL = [4] * 13 + [5] * 6  # the complete code-length code png_streams.Deflate.dynamic uses


def dynamic_header(d, hlit, hdist, items, final=False):
    """The header of a dynamic block with the code-length symbols given one by one: an int 0..15 is a length, (16, n) repeats the
    previous length n = 3..6 times, (17, n) is n = 3..10 zeros, (18, n) is n = 11..138 zeros.  Nothing is checked: refusals are built
    with it."""
    d.bits(1 if final else 0, 1)
    d.bits(2, 2)
    d.bits(hlit - 257, 5)
    d.bits(hdist - 1, 5)
    d.bits(19 - 4, 4)
    by_symbol = ps.canonical(CL)
    for s in ps.CL_ORDER:
        d.bits(CL[s], 3)
    for it in items:
        if isinstance(it, tuple):
            sym, n = it
            d.code(by_symbol[sym])
            d.bits(n - (3, 3, 11)[sym - 16], (2, 3, 7)[sym - 16])
        else:
            d.code(by_symbol[it])


def expand(items):
    out = []
    for it in items:
        if isinstance(it, tuple):
            out += [out[-1] if it[0] == 16 else 0] * it[1]
        else:
            out.append(it)
    return out


def repeat_code_cases():
    cases = []
    # a repeat that runs from the literal lengths into the distance lengths: 259 literal/length symbols and 8 distance symbols;
    # 0..7 get 4 bits, 8..254 none, 255 gets 3 bits and (16, 6) repeats that over 256, 257, 258 and the distance symbols 0, 1, 2
    # (complete codes on both trees, so that zlib reads the stream too)
    items = [4] * 8 + [(18, 138), (18, 109)] + [3, (16, 6), 3, (16, 4)]
    lens = expand(items)
    assert len(lens) == 259 + 8 and lens[255:] == [3] * 12
    d = ps.Deflate()
    dynamic_header(d, 259, 8, items, final=True)
    lit, dist = ps.canonical(lens[:259]), ps.canonical(lens[259:])
    d._tokens([0, 1, 2, 3, 4, 5, 6, 7, (4, 4), (3, 1), 255, (4, 3), (3, 2)], lit, dist)
    cases.append(Case("repeat_into_distance_lengths", d, len(d.raw)))
    # every repeat code with its smallest and its largest count
    items = [(17, 3), 4, (16, 3), (16, 6), (17, 10), 4, 4, (18, 11), (18, 138)]
    items += [0] * (256 - len(expand(items))) + [3, 3, 1]
    lens = expand(items)
    assert len(lens) == 259 and lens[3:13] == [4] * 10
    d = ps.Deflate()
    dynamic_header(d, 258, 1, items, final=True)
    d._tokens([3, 4, 12, 23, 3, (3, 1)], ps.canonical(lens[:258]), ps.canonical(lens[258:]))
    cases.append(Case("repeat_counts_at_their_ends", d, len(d.raw)))
    d = ps.Deflate()
    dynamic_header(d, 257, 1, [(16, 3)] + [0] * 255, final=True)
    cases.append(Case("repeat_16_first", d.finish() + bytes(8), 8, "bad codelengths"))
    d = ps.Deflate()
    dynamic_header(d, 257, 1, [1] * 250 + [(17, 10)], final=True)  # 260 > 258
    cases.append(Case("repeat_overshoots", d.finish() + bytes(8), 8, "bad codelengths"))
    d = ps.Deflate()
    dynamic_header(d, 257, 1, [0] * 250 + [(18, 138)], final=True)
    cases.append(Case("repeat_18_overshoots", d.finish() + bytes(8), 8, "bad codelengths"))
    return cases


# ---- the shapes -----------------------------------------------------------------------------------------------------------------
def lits(n, first=0):
    return [first] + [(7 * i + 3) % 251 for i in range(1, n)] if n else []


def token_round_cases():
    cases = []
    for n in (1, 63, 64, 65, 129):  # 64: the block ends exactly on a round edge, its end-of-block symbol opens an empty round
        d = ps.Deflate()
        d.fixed(lits(n))
        d.fixed([9, (3, 1), 8], final=True)
        cases.append(Case(f"tokens_{n}", d, len(d.raw)))
    d = ps.Deflate()
    d.fixed([0, 1])
    d.fixed([])  # 256 alone
    lit = ps.lengths_for({65, 66, 256}, 257)
    d.dynamic([], lit, [1])
    d.fixed([2, (4, 2)])
    d.stored(b"")
    d.fixed([], final=True)
    cases.append(Case("empty_blocks", d, len(d.raw)))
    d = ps.Deflate()
    d.fixed(lits(60) + [(258, 7), (3, 60), 1, 2])  # 64 tokens, matches among them, then the edge
    d.fixed(lits(64, 5) + lits(64, 6), final=True)  # 128: two full rounds and an empty one
    cases.append(Case("round_edges", d, len(d.raw)))
    return cases


def match_cases():
    cases = []
    for length in (3, 258):
        for dist in (1, 2, 3, 4, 63, 64, 65, 257, 258, 259):
            d = ps.Deflate()
            d.fixed(lits(259 + dist % 5) + [(length, dist), 77, (length, dist), 78], final=True)
            cases.append(Case(f"match_{length}_{dist}", d, len(d.raw)))
    d = ps.Deflate()
    d.fixed([0, 5])
    d.fixed([(3, 1)] * 64, final=True)  # one round, each match reads the one before
    cases.append(Case("64_distance_1_matches", d, len(d.raw)))
    d = ps.Deflate()
    d.fixed(lits(40) + [(10, 10), (10, 10), (20, 20), 3, (3, 3)], final=True)  # the source ends just before the match
    cases.append(Case("source_ends_before_match", d, len(d.raw)))
    d = ps.Deflate()
    d.fixed(lits(5) + [(258, 1), (258, 2), (258, 3), (100, 5), (258, 259), (258, 258), (258, 257), 4, (4, 1)] * 7, final=True)  # 63 tokens + 5
    cases.append(Case("long_matches_chained", d, len(d.raw)))
    return cases


def ring_cases():
    cases = []
    for n in (32767, 32768, 32769, 65535, 65536, 65537):
        d = ps.Deflate()
        stored_bulk(d, filler(n - 100, n))
        d.fixed(lits(100, 9))
        assert len(d.raw) == n
        far = min(n, 32768)
        d.fixed([(258, far), (3, 32768 if n + 258 >= 32768 else far), 11], final=True)
        cases.append(Case(f"ring_{n}_exact", d, n))  # the stream goes on behind cap
        cases.append(Case(f"ring_{n}_far_match", d, len(d.raw)))
    for seam in (32768, 65536, 131072):
        d = ps.Deflate()
        stored_bulk(d, filler(seam - 10, seam))
        d.fixed([(20, 7), 1, 2])  # the destination straddles the seam
        stored_bulk(d, filler(100, 3)[1:])
        d.fixed([(40, 131 + 10), (258, 32768), 3], final=True)  # the source straddles it; then the whole window back
        cases.append(Case(f"seam_{seam}", d, len(d.raw)))
    for cap in (16383, 16384, 16385, 32767, 32769):  # a flush edge (16 KiB of stored bytes, or of tokens) at cap - 1, cap, cap + 1
        d = ps.Deflate()
        d.stored(filler(16384, cap))
        d.fixed(lits(20, 4))
        stored_bulk(d, filler(16384, 5))
        d.fixed(lits(20, 4), final=True)
        cases.append(Case(f"flush_edge_{cap}", d, cap))
    d = ps.Deflate()
    d.fixed([0] + [(258, 1)] * 200, final=True)  # 16 KiB of tokens without a stored block: flushes between rounds
    cases.append(Case("flush_tokens", d, len(d.raw)))
    cases.append(Case("flush_tokens_cap", d, 16385 + 64))
    return cases


def cap_cases():
    cases = []
    d = ps.Deflate()
    d.fixed(lits(50) + [(258, 50), 1, 2, 3])
    d.stored(filler(500, 2))
    d.fixed([4, 5, (30, 3)], final=True)
    total = len(d.raw)
    z = d.finish()
    cases.append(Case("cap_mid_match", z, 50 + 100))
    cases.append(Case("cap_end_of_match", z, 50 + 258))
    cases.append(Case("cap_by_literal", z, 50 + 258 + 2))
    cases.append(Case("cap_mid_stored", z, 50 + 258 + 3 + 77))
    cases.append(Case("cap_end_of_stored", z, 50 + 258 + 3 + 500))
    cases.append(Case("cap_all", z, total))
    cases.append(Case("cap_one_more", z, total + 1, "not enough pixels"))
    cut = z[:len(z) // 2]
    cases.append(Case("garbage_beyond_cap", cut + bytes(range(255, 0, -1)) * 2, 60))
    cases.append(Case("truncated_beyond_cap", z[:40], 20))
    return cases


def block_cases():
    cases = []
    offsets = set()
    for n in (0, 1, 255, 65535):
        for lead in range(8):
            d = ps.Deflate()
            d.fixed([0] + [200] * lead)  # 3 + 8 + 9 * lead + 7 bits: the stored header starts at every bit offset
            offsets.add(d.n)
            d.stored(filler(n, n + lead)[::-1])
            d.fixed([1, (5, 1)], final=True)
            cases.append(Case(f"stored_{n}_at_bit_{d.n}_{lead}", d, len(d.raw)))
    assert offsets == set(range(8))
    d = ps.Deflate()
    d.fixed([0])
    for i in range(300):
        used = {256, 65 + i % 20, 97 + i % 7, 257 + i % 3}
        d.dynamic([65 + i % 20, 97 + i % 7, (3 + i % 3, 1 + i % 2)], ps.lengths_for(used, 260), [1, 1])
    d.fixed([], final=True)
    cases.append(Case("300_dynamic_blocks", d, len(d.raw)))
    d = ps.Deflate()
    d.fixed(list(range(256)) + [(258, 256), (3, 1), (4, 200)])
    d.fixed([143, 144, 255, (115, 5), (227, 300)], final=True)
    cases.append(Case("fixed_blocks", d, len(d.raw)))
    d = ps.Deflate()
    lit = ps.lengths_for({0, 68, 69, 256, 257}, 258)
    for i in range(6):
        d.stored(bytes([i, i + 1, i + 2]))
        d.fixed([66, (3, 2)])
        d.dynamic([68, 69, (3, 2)], lit, [0, 1])
    d.stored(b"", final=True)
    cases.append(Case("block_types_in_turn", d, len(d.raw)))
    d = ps.Deflate()
    used = list(range(66, 80)) + [256, 265]
    lit = ps.lengths_for(used, 266, long_symbol=265)
    dist = ps.lengths_for(range(16), 16, long_symbol=15)
    assert max(lit) == 15 and lit[265] == 15 and max(dist) == 15 and dist[15] == 15
    d.stored(filler(300, 8))
    d.dynamic([79, 66, (11, 193), 78, (12, 255), 79, (11, 1), (12, 200)] * 5, lit, dist, final=True)
    cases.append(Case("15_bit_codes_on_both_trees", d, len(d.raw)))
    d = ps.Deflate()
    lit = ps.lengths_for(set(range(97, 105)) | {0, 256, 257, 260}, 261)
    d.dynamic([0, 97, 98, 99, 100, (3, 4), (6, 4), 101, (3, 4)], lit, [0, 0, 0, 1], final=True)
    cases.append(Case("one_code_distance_tree", d, len(d.raw)))
    # a 15-bit literal/length code, 5 extra bits, a 15-bit distance code and 13 extra bits behind k one-bit literals: every part
    # starts at, and straddles, every bit offset of a dword
    used = [0] + list(range(70, 83)) + [256, 257 + 27]
    lit = ps.lengths_for(used, 285, long_symbol=284)
    dist = ps.lengths_for(range(14, 30), 30, long_symbol=29)
    assert lit[0] == 1 and lit[284] == 15 and dist[29] == 15
    for k in range(32):
        d = ps.Deflate()
        stored_bulk(d, filler(33000, k))
        d.dynamic([0] * k + [(227 + 9 + k % 22, 24577 + 8191 - 40 * k), 71, 0, (227 + 30, 32768), 72], lit, dist, final=True)
        cases.append(Case(f"straddle_{k}", d, len(d.raw)))
    cases.append(Case("one_byte_stream", b"\x03", 4, "premature end of the zlib data"))
    return cases


def _raw_fixed(tokens_then):
    """a fixed block, final, of literals, then the bits given as (value, n) pairs written as they are"""
    d = ps.Deflate()
    d.bits(1, 1)
    d.bits(1, 2)
    fixed = ps.canonical(ps.FIXED_LITLEN)
    for t in tokens_then[0]:
        d.code(fixed[t])
    for code, n, msb in tokens_then[1]:
        if msb:
            d.code((code, n))
        else:
            d.bits(code, n)
    return d


def error_cases():
    """one per status, and per way into it"""
    cases = []
    d = ps.Deflate()
    d.fixed([0, 1])
    d.bits(0, 1)
    d.bits(3, 2)
    cases.append(Case("bad_block_type", d.finish() + bytes(8), 16, "bad block type"))
    d = ps.Deflate()
    d.fixed([0, 1])
    d.bits(1, 1)
    d.bits(0, 2)
    d.bits(0, 8 - d.n)
    d.out += bytes([3, 0, 0xFC, 0xFE]) + b"abc"  # NLEN is not LEN's complement
    cases.append(Case("zlib_corrupt", d.finish(), 16, "zlib corrupt"))
    d = ps.Deflate()  # the refusal file's: a code-length code of one 1-bit and three 2-bit codes
    d.bits(1, 1); d.bits(2, 2); d.bits(0, 5); d.bits(0, 5); d.bits(15, 4)
    for i in range(19):
        d.bits((1, 2, 2, 2)[i] if i < 4 else 0, 3)
    cases.append(Case("oversubscribed_code_length_code", d.finish() + bytes(8), 16, "bad codelengths"))
    d = ps.Deflate()
    dynamic_header(d, 257, 1, [1, 1, 1] + [0] * 253 + [2, 1], final=True)  # three 1-bit literal codes
    cases.append(Case("oversubscribed_literal_lengths", d.finish() + bytes(8), 16, "bad codelengths"))
    d = ps.Deflate()
    dynamic_header(d, 257, 3, [2] + [0] * 255 + [2] + [1, 1, 1], final=True)  # three 1-bit distance codes
    cases.append(Case("oversubscribed_distance_lengths", d.finish() + bytes(8), 16, "bad codelengths"))
    d = ps.Deflate()
    dynamic_header(d, 257, 1, [2] + [0] * 255 + [2] + [1], final=True)  # codes 00 and 01 only
    d.bits(0, 2)  # literal 0
    d.bits(1, 1)  # 1x: no code
    d.bits(0xFFFF, 16)
    cases.append(Case("symbol_no_code_has", d.finish() + bytes(8), 16, "bad huffman code"))
    d = ps.Deflate()
    dynamic_header(d, 258, 2, [2] + [0] * 255 + [2, 2] + [2, 2], final=True)  # distance codes 00 and 01 only
    d.bits(0, 2)  # literal 0
    d.bits(1, 2)  # 257 is code 10, sent MSB first: length 3
    d.bits(3, 2)  # 11: no distance code
    cases.append(Case("distance_no_code_has", d.finish() + bytes(8), 16, "bad huffman code"))
    for sym in (286, 287):
        d = _raw_fixed(([0, 1, 2], [(fixed_code(sym), 8, True), (0, 16, False)]))
        cases.append(Case(f"length_symbol_{sym}", d.finish() + bytes(8), 16, "bad huffman code"))
    for sym in (30, 31):
        d = _raw_fixed(([0, 1, 2], [ps.canonical(ps.FIXED_LITLEN)[257] + (True,), (sym, 5, True), (0, 16, False)]))
        cases.append(Case(f"distance_symbol_{sym}", d.finish() + bytes(8), 16, "bad dist"))
    d = ps.Deflate()
    d.fixed(lits(70) + [(3, 71)], final=True)  # one past the bytes produced, in the second round
    cases.append(Case("distance_one_past", d.finish() + bytes(4), 100, "bad dist"))
    d = ps.Deflate()
    d.fixed([0, (3, 2)], final=True)  # ... and in the first
    cases.append(Case("distance_one_past_first_round", d.finish() + bytes(4), 100, "bad dist"))
    d = ps.Deflate()
    d.fixed(lits(100) + [(258, 90)] * 3, final=True)
    z = d.finish()
    cases.append(Case("ends_inside_a_symbol", z[:60], len(d.raw), "premature end of the zlib data"))
    cases.append(Case("ends_inside_a_match_symbol", z[:-3], len(d.raw), "premature end of the zlib data"))
    d = ps.Deflate()
    d.fixed([0, 1, 2])
    d.stored(filler(100, 4))
    cases.append(Case("ends_inside_a_stored_block", d.finish()[:-30], 200, "read past buffer"))
    cases.append(Case("ends_inside_a_stored_header", d.finish()[:-102], 200, "premature end of the zlib data"))
    d = ps.Deflate()
    d.fixed([0, 1, 2])
    d.stored(filler(10, 4))
    d.fixed([5, 6])
    cases.append(Case("ends_between_blocks", d.finish(), 200, "premature end of the zlib data"))
    d = ps.Deflate()
    d.fixed(lits(30), final=True)
    cases.append(Case("not_enough_pixels", d.finish(), 31, "not enough pixels"))
    d = ps.Deflate()
    d.fixed(lits(30))
    d.stored(b"xy", final=True)
    cases.append(Case("not_enough_pixels_stored", d.finish(), 33, "not enough pixels"))
    rows, rb = 70, 9  # more rows than lanes
    for bad in (0, 35, 64, 69):
        raw = bytearray(filler(rows * (rb + 1), bad))
        raw[::rb + 1] = bytes([y % 5 for y in range(rows)])
        raw[bad * (rb + 1)] = 5
        cases.append(Case(f"filter_5_in_row_{bad}", zlib.compress(bytes(raw), 6)[2:-4], len(raw), "invalid filter", [(rows, rb)]))
    raw = bytearray(filler(rows * (rb + 1), 99))
    raw[::rb + 1] = bytes([y % 5 for y in range(rows)])
    raw[1] = 5  # not a filter byte
    cases.append(Case("filter_bytes_all_valid", zlib.compress(bytes(raw), 6)[2:-4], len(raw), None, [(rows, rb)]))
    return cases


def fixed_code(sym):
    return ps.canonical(ps.FIXED_LITLEN)[sym][0]


def good_case(seed=0):
    raw = filler(600, 40 + seed) + bytes(300) + filler(600, 40 + seed)
    return Case(f"good_{seed}", zlib.compress(raw, 9)[2:-4], len(raw))


def zlib_cases():
    """real zlib streams: levels 1, 6, 9 and the strategies Z_FIXED, Z_HUFFMAN_ONLY, Z_RLE; they carry the repeat codes"""
    rng = np.random.default_rng(7)
    text = bytes(rng.choice(np.frombuffer(b"abcdefgh    \n", np.uint8), 60000))
    noisy = bytes(np.where(rng.random(60000) < 0.9, np.frombuffer(text, np.uint8), rng.integers(0, 256, 60000)).astype(np.uint8))
    raw = b"\x00" + text + noisy + text[:30000] + bytes(5000) + noisy[1000:9000]
    cases = []
    for level, strategy, name in ((1, 0, "level_1"), (6, 0, "level_6"), (9, 0, "level_9"), (6, zlib.Z_FIXED, "fixed"),
                                  (6, zlib.Z_HUFFMAN_ONLY, "huffman_only"), (6, zlib.Z_RLE, "rle")):
        c = zlib.compressobj(level, zlib.DEFLATED, 15, 9, strategy)
        z = c.compress(raw) + c.flush()
        assert zlib.decompress(z) == raw
        cases.append(Case("zlib_" + name, z[2:-4], len(raw)))
        cases.append(Case("zlib_" + name + "_capped", z[2:-4], len(raw) - 12345))
    return cases


def all_built_cases():
    return (token_round_cases() + match_cases() + ring_cases() + cap_cases() + block_cases() + repeat_code_cases() + error_cases())
