"""tests/frame_geometry.py without a device: the restatements against tests/oracle.py, both sides of every label, the invariants of
frame_geometry over a sweep (with the float clauses that no accepted-size source fires, by name), and the refusals through the shim's host-side
check (fake device pointers: a refused call never passes them on; no accepted table is passed here)."""
import ctypes as C

import numpy as np
import pytest

import frame_geometry as fg
import frames_packed_util
import glue_edges as ge
import oracle
from yolo_quantization_amd import binding

SMALL = [c for c in fg.CASES if max(c.imw, c.imh, c.w, c.h) <= 1024 and c.B <= 3]


# ----------------------------------------------------------------------------------------------------- restatements against the oracle
def _probe(imw, imh):
    """planes whose values all lie in (0.6, 1): nothing the letterbox makes of them equals the bars' 0.5"""
    return (np.random.default_rng(imw * 7 + imh).random((2, imh, imw), dtype=np.float32) * np.float32(.39) + np.float32(.6)).astype(np.float32)


@pytest.mark.parametrize("c", fg.GEO_CASES, ids=lambda c: c.name)
def test_geometry_equals_where_the_oracle_puts_the_image(c):
    """ox, oy, new_w, new_h from where the oracle's 0.5 bars end; the last row and column from the source rows and columns they equal"""
    g = fg.geometry1(c.imw, c.imh, c.w, c.h)
    assert g.accepted and fg.frames_check(1, c.w, c.h, [(c.imw, c.imh)]) is None
    im = _probe(c.imw, c.imh)
    want = oracle.letterbox_image(im, c.h, c.w)
    inside = want[0] != np.float32(.5)
    rows, cols = np.flatnonzero(inside.any(axis=1)), np.flatnonzero(inside.any(axis=0))
    assert (rows[0], cols[0], rows.size, cols.size) == (g.oy, g.ox, g.new_h, g.new_w)
    assert inside[g.oy:g.oy + g.new_h, g.ox:g.ox + g.new_w].all(), "a rectangle"
    t = fg.taps(c.imw, c.imh, g)
    row, iy, dy = ge.letterbox_last_row(im, g.new_w, g.new_h)
    assert (iy, dy) == (t.iy[-1], t.dy[-1])
    assert np.array_equal(want[:, g.oy + g.new_h - 1, g.ox:g.ox + g.new_w].view(np.uint32), row.view(np.uint32)), "the last row"
    col = ge.letterbox_last_column(im, g.new_h)
    assert np.array_equal(want[:, g.oy:g.oy + g.new_h, g.ox + g.new_w - 1].view(np.uint32), col.view(np.uint32)), "the source's last column alone"
    if fg.GEO_CLAUSES["geo.last_row_short"](c):  # a near-black line: (1 - dy) times source row imh - 2
        assert 0 < 1 - dy < 1e-5 and want[:, g.oy + g.new_h - 1, g.ox:g.ox + g.new_w].max() < 1e-5
    if fg.GEO_CLAUSES["geo.last_row_exact"](c):
        assert want[:, g.oy + g.new_h - 1, g.ox + g.new_w - 1].tolist() == im[:, -1, -1].tolist()
    if fg.GEO_CLAUSES["geo.identity"](c):
        assert g.w_scale in (0, 1) and g.h_scale in (0, 1) and not t.dx.any() and not t.dy.any()
        assert np.array_equal(want[:, g.oy:g.oy + g.new_h, g.ox:g.ox + g.new_w], im)
    if max(c.imw, c.imh, c.w, c.h) <= 1024:  # the whole image, tap by tap
        assert np.array_equal(fg.letterbox_restated(im, c.w, c.h).view(np.uint32), want.view(np.uint32))


def test_letterbox_restated_equals_the_oracle_on_every_small_case():
    seen = set()
    for c in SMALL:
        if (c.imw, c.imh, c.w, c.h) in seen:
            continue
        seen.add((c.imw, c.imh, c.w, c.h))
        im = fg.planes(fg.frame(c, 0))
        assert np.array_equal(fg.letterbox_restated(im, c.w, c.h).view(np.uint32), oracle.letterbox_image(im, c.h, c.w).view(np.uint32)), c.name
    assert len(seen) >= 50


def test_expected_bytes_restate_the_oracles_quantiser():
    """with the oracle's own pair the quantiser line gives the oracle's bytes; the expectation of a case is cached and shared"""
    for c in fg.GEO_CASES[:12] + fg.STORE_CASES[:8]:
        for want in fg.expected(c.name):
            q, s, z = oracle.quantize_image(want.lb)
            assert (want.scale, want.zp) == (s, z) and np.array_equal(want.q, q), c.name
            assert want.mm.view(np.float32)[0] == max(want.lb.max(), 0) and want.mm[1] == 0x80000000  # no float is negative
    assert fg.expected("identity") is fg.expected("identity")
    z = fg.expected("quant_zero_frame")
    assert all(w.mm.tolist() == [0, 0x80000000] and (w.q == 23).all() for w in z), "max stays +0.0, min stays -0.0"
    for c in fg.QUANT_CASES:  # no quotient leaves what C defines, and none is negative
        for want in fg.expected(c.name):
            assert want.lb.min() >= 0 and (want.lb / want.scale < 2 ** 20).all()
            assert c.data != "ramp" or all(np.unique(want.lb[k]).size == 256 for k in range(3))


# ------------------------------------------------------------------------------------------------------------------------ the tables
def test_every_label_is_reached_on_both_sides_and_the_dead_clauses_are_named():
    tables = ((fg.GEO_CLAUSES, fg.GEO_CASES), (fg.LAUNCH_CLAUSES, fg.STORE_CASES + fg.MINMAX_CASES), (fg.QUANT_CLAUSES, fg.QUANT_CASES + fg.GEO_CASES[:1]),
              (fg.SOURCE_CLAUSES, fg.SOURCE_SIZES))
    missing = [m for clauses, cases in tables for m in fg.Reach(clauses, cases).missing()]
    assert not missing, missing
    assert all(fg.frames_check(1, s.w, s.h, [(s.imw, s.imh)]) is None for s in fg.SOURCE_SIZES) and len(set(fg.SOURCE_SIZES)) == len(fg.SOURCE_SIZES)
    assert len({c.name for c in fg.CASES}) == len(fg.CASES) == len(fg.BY_NAME)
    # the refused side of the size labels
    by = {r[0]: r for r in fg.REFUSED}
    sides = {n: {min(fg.geometry1(imw, imh, w, h).new_w, fg.geometry1(imw, imh, w, h).new_h) for imw, imh in sizes[-1:]}
             for n, _, w, h, sizes, m in fg.REFUSED if m == fg.DEGENERATE}
    assert {v for s in sides.values() for v in s} == {0, 1}, "resized side 1 and resized side 0"
    assert by["source_w_32769"][4][-1][0] == fg.SIDE_MAX + 1 and by["net_w_32769"][2] == fg.SIDE_MAX + 1 and by["B_65536"][1] == fg.B_MAX + 1
    for name, B, w, h, sizes, message in fg.REFUSED:
        assert fg.frames_check(B, w, h, sizes) == message, name
        assert all(fg.frames_check(1, 12, 12, [s]) is None for s in sizes[:-1]), "the frames in front are good ones"
    # one-pixel sources: accepted with the guards, refused by the rule before them; nothing else in the tables changes its verdict
    for c in fg.CASES:
        old = fg.frames_check(c.B, c.w, c.h, [(c.imw, c.imh)], guarded=False)
        assert fg.frames_check(c.B, c.w, c.h, [(c.imw, c.imh)]) is None, c.name
        assert (old == fg.DEGENERATE) == (c.name in fg.ONE_PIXEL) and old in (None, fg.DEGENERATE), c.name
    assert len(fg.ONE_PIXEL) == 9
    for imw, imh in ((1, 7), (7, 1)):  # still refused into 12 x 12: a resized side of 1
        assert not fg.geometry1(imw, imh, 12, 12).sized
    # the store paths by count: every path in the table, both in one launch, the row tail
    total = {"wide": 0, "bytes": 0, "tail": 0}
    for c in fg.STORE_CASES:
        p = fg.store_paths(c.B, c.w, c.h, c.out_off)
        assert sum(p.values()) == c.B * 3 * c.h * ((c.w + 3) // 4)
        for k in total:
            total[k] += p[k]
    assert min(total.values()) > 100, total
    assert fg.store_paths(2, 8, 2, 0) == {"wide": 24, "bytes": 0, "tail": 0} and fg.store_paths(2, 8, 2, 1)["wide"] == 0
    assert fg.store_paths(1, 5, 2, 0) == {"wide": 2, "bytes": 4, "tail": 6}  # w % 4 != 0: every plane-row starts at another alignment
    # launch sizings
    assert [fg.minmax_grid_x(B, 2, 2) for B in (1, 2048, 2049, fg.B_MAX)] == [1, 1, 1, 1]
    assert fg.minmax_grid_x(1, 1024, 513) == 2048 and fg.minmax_trips(1, 1024, 513) == 2 and fg.minmax_grid_x(3, 416, 416) == 676
    assert fg.minmax_grid_x(2048, 416, 416) == 1 and fg.minmax_grid_x(2049, 416, 416) == 1 and fg.minmax_grid_x(1024, 416, 416) == 2
    assert [fg.quantize_grid_x(w, h) for w, h in ((10, 85), (8, 128), (4, 257), (416, 416))] == [1, 1, 2, 169]
    # the quantiser pairs sit where they aim
    e = {c.name: fg.quant_edges(*c.pair) for c in fg.QUANT_CASES if c.data == "ramp"}
    assert e["quant_tie"]["tie"] >= 32 and e["quant_tie3"]["tie"] >= 8, "many bytes on a tie, not one"
    assert e["quant_tie_scale_below"]["above"] >= 32 and e["quant_tie_scale_above"]["below"] >= 32 and e["quant_tie"]["below"] >= 32
    assert (e["quant_unit_zp0"]["255"], e["quant_unit_zp0"]["256"]) == (1, 0) and (e["quant_unit_zp1"]["255"], e["quant_unit_zp1"]["256"]) == (1, 1)
    assert e["quant_unit_zp255"]["far"] == 254 and e["quant_tie_zp255"]["256"] > 0
    # listed, not reached
    names = [n for n, _ in fg.UNREACHED]
    assert set(fg.DEAD_CLAUSES) <= set(names) and "byte_offsets_above_2^31" in names and "float_and_exact_aspects_disagree" in names
    assert not any(c.h * c.w == 257 for c in fg.CASES) and "mm.pixels_257" in names


def test_tables_stay_small():
    for c in fg.CASES:
        assert c.B * 3 * c.h * c.w <= 2 << 20 and c.imw * c.imh * 3 <= 16 << 20, c.name
    assert sum(c.imw * c.imh > 1 << 16 for c in fg.CASES) == 2, "the two frames with a side of 32768"
    assert all(c.B <= 3 or (c.w, c.h) == (2, 2) for c in fg.CASES)


# ---------------------------------------------------------------------------------------------------------------------------- the sweep
def _sweep_pairs():
    """(imw, imh, w, h) arrays: every source up to 24 x 24 into six networks, the issue's sources (1..199, 255..257, 640, 1920, 4096, 32767,
    32768; both sides) into eight networks, and 4000 seeded pairs with log-uniform sides up to the limits"""
    small = np.arange(1, 25)
    nets_small = [(2, 2), (2, 9), (12, 12), (13, 11), (16, 10), (5, 31)]
    a = np.array([(iw, ih, w, h) for iw in small for ih in small for w, h in nets_small])
    side = np.concatenate([np.arange(1, 200), [255, 256, 257, 640, 1920, 4096, 32767, 32768]])
    nets = [(2, 2), (12, 12), (13, 11), (416, 416), (608, 352), (320, 1024), (32768, 2), (2, 32768)]
    iw, ih, n = np.meshgrid(side, side, np.arange(len(nets)), indexing="ij")
    b = np.stack([iw.ravel(), ih.ravel(), np.array(nets)[n.ravel(), 0], np.array(nets)[n.ravel(), 1]], axis=1)
    rng = np.random.default_rng(20240)
    c = np.exp(rng.uniform(0, np.log(32768.999), (4000, 4))).astype(np.int64)
    c[:, 2:] = np.maximum(c[:, 2:], 2)
    return np.concatenate([a, b, c]).T


def test_geometry_invariants_over_the_sweep():
    imw, imh, w, h = _sweep_pairs()
    assert imw.size > 340000
    g, old = fg.geometry(imw, imh, w, h), fg.geometry(imw, imh, w, h, guarded=False)
    s = g.sized
    assert s.sum() > 100000 and (~s).sum() > 10000
    assert (g.new_w[s] <= w[s]).all() and (g.new_h[s] <= h[s]).all() and (g.ox[s] >= 0).all() and (g.oy[s] >= 0).all()
    assert ((g.new_w == w) | (g.new_h == h)).all() and (g.ox + g.new_w <= w)[s].all() and (g.oy + g.new_h <= h)[s].all()
    # the three float clauses: which accepted-size sources fire them
    assert not g.row_last.any(), "clause.row_last: dead"
    assert np.array_equal(g.row_next, s & (imh == 1)) and np.array_equal(g.col_next, s & (imw == 1)), "exactly the one-row / one-column sources"
    assert np.array_equal(g.accepted, s), "with the guards the clauses refuse nothing: clause.row_next, clause.col_next dead"
    assert np.array_equal(old.accepted, s & (imw > 1) & (imh > 1)) and (s & ((imw == 1) | (imh == 1))).sum() > 1000
    assert {"clause.row_last", "clause.row_next", "clause.col_next"} == set(fg.DEAD_CLAUSES)
    # the comparison in float against exact integers: equal over the whole sweep
    exact = w * imh < h * imw
    assert np.array_equal(exact, g.width_bound)
    assert (imw * imh).max() == 1 << 30
    # every tap the kernels read lies inside the frame (checked pair by pair on a seeded subset plus every one-pixel and side-2 pair of it)
    pick = np.flatnonzero(s)
    pick = pick[np.random.default_rng(2).permutation(pick.size)[:3000]]
    edge = np.flatnonzero(s & ((imw == 1) | (imh == 1) | (g.new_w == 2) | (g.new_h == 2)))[::53]
    short = 0
    for k in np.concatenate([pick, edge]).tolist():
        gk = fg.Geo(*(v[k] for v in g))
        t = fg.taps(int(imw[k]), int(imh[k]), gk)
        assert t.ix.min() >= 0 and (t.ix + t.two_x).max() <= imw[k] - 1 and t.iy.min() >= 0 and (t.iy + t.two_y).max() <= imh[k] - 1
        assert t.ix[-1] == imw[k] - 1 and not t.two_x[-1] and not t.two_y[-1] and (t.dx >= 0).all() and (t.dx < 1).all() and (t.dy < 1).all()
        assert t.iy[-1] in (imh[k] - 1, imh[k] - 2) or imh[k] == 1
        short += int(imh[k] > 1 and t.iy[-1] == imh[k] - 2)
    assert short > 50, "the short last row is no rarity"


def test_the_other_frames_tests_helper_states_the_same_rule():
    """frames_packed_util.geometry_accepts, which the packed and Bayer tests size their batches with, mirrors the guards"""
    imw, imh, w, h = _sweep_pairs()
    g = fg.geometry(imw, imh, w, h)
    for k in np.random.default_rng(1).integers(0, imw.size, 2000).tolist() + np.flatnonzero((imw == 1) | (imh == 1))[::97].tolist():
        assert frames_packed_util.geometry_accepts(int(imw[k]), int(imh[k]), int(w[k]), int(h[k])) == bool(g.accepted[k])


def test_float_and_exact_aspect_comparison_part_only_at_5e8_pixels():
    imw, imh, w, h = fg.DISAGREEMENT
    g = fg.geometry1(imw, imh, w, h)
    assert w * imh < h * imw and not g.width_bound, "the smallest disagreeing source found"
    assert (g.new_w, g.new_h) == (w, h) and g.accepted and (g.ox, g.oy) == (0, 0), "new_w is w either way: (imw * h) / imh == w"
    assert imw * imh > 5e8
    # no pair of nearly equal aspects below 4096 x 4096 disagrees: the quotients are 24-bit floats of ratios that differ by more than an ulp
    rng = np.random.default_rng(3)
    sw, sh, nw = (rng.integers(1, 4097, 200000) for _ in range(3))
    nh = np.clip(nw * sh // sw + rng.integers(-1, 2, sw.size), 2, 32768)
    nw = np.maximum(nw, 2)
    assert np.array_equal(fg.geometry(sw, sh, nw, nh).width_bound, nw * sh < nh * sw)


# ---------------------------------------------------------------------------------------------------- refusals through the host-side check
@pytest.mark.parametrize("r", fg.REFUSED, ids=lambda r: r[0])
def test_refusals_through_the_shims_host_side_check(r):
    name, B, w, h, sizes, message = r
    S = binding.shim()
    table = (binding.FrameU8 * len(sizes))()
    for b, (imw, imh) in enumerate(sizes):
        table[b] = binding.FrameU8(0x1000, imw, imh, 3 * max(imw, 1), binding.FRAME_ORDER["rgb"], (C.c_int * 2)(0, 0))
    fake = C.c_void_p(0x1000)  # device arguments: checked for null only, a refused call never passes them on
    want = ("invalid argument: frames_u8: " + message).encode()
    assert S.mi355_frames_u8_letterbox_minmax(fake, table, B, w, h, fake, None) == -22
    assert S.mi355_last_error() == want
    assert S.mi355_frames_u8_letterbox_quantize(fake, table, B, w, h, fake, fake, fake, None) == -22
    assert S.mi355_last_error() == want
