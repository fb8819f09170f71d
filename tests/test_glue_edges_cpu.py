"""tests/glue_edges.py without a device: every plain reference against tests/oracle.py where the oracle is defined, every clause label of the
tables reached on both sides, every shortcut parameter set on its aimed edge by count, no int32 overflow in the shortcut's arithmetic for any
legal input, and the tables' own validity (what a case lets a kernel write, buffer sizes, the sentinel)."""
import itertools

import numpy as np
import pytest

import glue_edges as ge
import oracle


def _per_image(f, x, *args):
    return np.stack([f(x[b], *args) for b in range(x.shape[0])])


# ----------------------------------------------------------------------------------------------------------- references against the oracle
def test_pool_output_size_is_c_division():
    assert [ge.cdiv(a, b) for a, b in ((7, 2), (-7, 2), (-1, 3), (-3, 3), (0, 5), (-4, 3))] == [3, -3, 0, -1, 0, -1]
    assert ge.pool_out(2, 5, 3, 1) == 1 and (2 + 1 - 5) // 3 + 1 == 0, "where truncation and floor part: H + pad < size"
    x = np.arange(1, 1 + 2 * 2 * 2, dtype=np.uint8).reshape(2, 2, 2)
    assert oracle.maxpool_u8(x, 5, 3, 1).shape == (2, 1, 1), "the oracle wrapper sizes its output the C way too"


def test_maxpool_reference_equals_the_oracle():
    outside = 0
    for cs in ge.POOL_CASES:
        full, x = ge.pool_inputs(cs)
        assert x.min() >= (0 if cs.data == "planted" else 1)
        want = ge.maxpool_ref(x, cs.size, cs.stride, cs.pad)
        assert np.array_equal(want, _per_image(oracle.maxpool_u8, x, cs.size, cs.stride, cs.pad)), cs.name
        if ge.pool_has_outside_window(cs) and cs.data != "planted":
            outside += 1
            assert (want == 0).any(), cs.name
    assert outside >= 8
    planted = [cs for cs in ge.POOL_CASES if cs.data == "planted"]
    for cs in planted:  # image 1: every lane gives its own planted byte back (or 0 from a window outside the image), never a neighbour's
        want = ge.maxpool_ref(ge.pool_inputs(cs)[1], cs.size, cs.stride, cs.pad)
        for c in range(cs.C):
            assert set(np.unique(want[1, c]).tolist()) <= {0, ge.PLANT[c % 4]}, cs.name
        assert (want[0] == 0xff).any() and (want[2] == 0xff).any()


def test_upsample_route_dequant_references_equal_the_oracle():
    for cs in ge.UP_CASES:
        x = ge.operand_bytes(cs.name, cs.B, cs.H, cs.W, cs.x, lo=0)[:, cs.x.off:cs.x.off + cs.C]
        assert np.array_equal(ge.upsample_ref(x, cs.stride), _per_image(oracle.upsample_u8, x, cs.stride)), cs.name
    a, b = np.arange(24, dtype=np.uint8).reshape(1, 2, 3, 4), np.arange(100, 112, dtype=np.uint8).reshape(1, 1, 3, 4)
    r = ge.route_ref([a, b])
    assert r.shape == (1, 3, 3, 4) and np.array_equal(r[:, :2], a) and np.array_equal(r[:, 2:], b)
    rng = np.random.default_rng(5)
    for cs in ge.DQ_CASES:
        u = rng.integers(0, 256, (3, cs.nc, 3, 5), dtype=np.uint8)
        u.ravel()[:2] = (0, 255)
        want = ge.dequant_ref(u, cs.zp, cs.scale)
        assert want.dtype == np.float32 and np.array_equal(want.view(np.uint32), oracle.dequant(u, cs.zp, np.float32(cs.scale)).view(np.uint32)), cs.name


def test_shortcut_reference_equals_the_oracle_and_every_set_hits_its_edge():
    a, b = ge.shortcut_pairs()
    assert a.shape == b.shape == (1, 16, 256, 256)
    for k in range(16):  # every lane sees every (a, b) pair exactly once
        assert np.unique(a[0, k].astype(np.int64) * 256 + b[0, k]).size == 65536
    assert (a[0, 0] == np.arange(256)[:, None]).all() and (b[0, 0] == np.arange(256)[None, :]).all()
    for s in ge.SC_SETS + [ge.SC_RAGGED.s]:
        assert np.array_equal(ge.shortcut_ref(a, b, s), oracle.shortcut_u8(a, b, s.Ka, s.Kb, s.za, s.zb, s.zo)), s.name
        counts = ge.shortcut_edge_counts(a, b, s)
        assert len(counts) >= 2 and all(n > 0 for n in counts), (s.name, s.aim, counts)
        if s.aim == "tie":
            assert min(counts) > 10000, (s.name, counts)  # "many pairs": more than 1 % of the launch on either sign
    crossed = [s for s in ge.SC_SETS if s.aim == "corners"]
    assert {(s.Ka, s.Kb) for s in crossed} == set(itertools.product((1, 65536, ge.K_MAX), repeat=2))
    for field in ("za", "zb", "zo"):
        assert {getattr(s, field) for s in ge.SC_SETS} >= {0, 1, 128, 255}, field
    assert {s.aim for s in ge.SC_SETS} >= {"corners", "tie", "clamp_lo", "clamp_hi", "clamp_both", "clamp_far"}


def test_shortcut_int32_arithmetic_never_overflows():
    """Every intermediate of the kernel's int arithmetic is a sum of products in which each of Ka, Kb, za, zb, zo, a, b appears at most once per
    product (multilinear), so over the box of legal inputs it takes its extremes at the corners: all 128 of them, in Python integers."""
    box = ((1, ge.K_MAX), (1, ge.K_MAX), (0, 255), (0, 255), (0, 255), (0, 255), (0, 255))
    worst = 0
    for corner in itertools.product(*box):
        worst = max([worst] + [abs(v) for v in ge.shortcut_int32_intermediates(*corner)])
    assert worst < 2 ** 31, worst
    assert worst > 2 ** 30, "the bound is not idle: the limits of the multipliers use the top bit but one"
    for s in ge.SC_SETS:
        for a, b in itertools.product((0, 255), repeat=2):
            assert max(abs(v) for v in ge.shortcut_int32_intermediates(s.Ka, s.Kb, s.za, s.zb, s.zo, a, b)) < 2 ** 31


def test_quantiser_references_equal_the_oracle():
    for kind in ("mixed", "positive", "negative"):
        for count in (5, 257, 1025):
            x = ge.q_data(count, kind, 0.25, seed=count)
            out, s, z = oracle.quantize_image(x)
            mm = ge.minmax_ref(x).view(np.float32)
            assert np.float32(mm[0] - mm[1]) * (np.float32(1.0) / np.float32(255.0)) == s, (kind, count)
            assert np.array_equal(ge.quantize_ref(x, s, z), out), (kind, count)
            xn = ge.with_nans(x)  # planted NaNs are skipped: the min / max of the elements they did not replace
            assert np.isnan(xn[[0, -1]]).all() and ge.minmax_ref(x[~np.isnan(xn)]).tolist() == ge.minmax_ref(xn).tolist()
    # the seeds' bit patterns
    assert ge.minmax_ref(ge.q_data(7, "positive")).tolist()[1] == 0x80000000
    assert ge.minmax_ref(ge.q_data(7, "negative")).tolist()[0] == 0
    for kind in ("zero", "negzero"):
        assert ge.minmax_ref(ge.q_data(7, kind)).tolist() == [0, 0x80000000]
    assert ge.minmax_ref(np.array([np.nan, -np.nan], np.float32)).tolist() == [0, 0x80000000]
    d = ge.q_data(64, "denormal")
    assert (np.abs(d) < np.finfo(np.float32).tiny).all() and (d > 0).any() and (d < 0).any()
    # round half away from zero, both signs, and both clamps
    x = np.array([0.125, -0.125, 0.375, -0.375, 0.625, 1e4, -1e4, 0.0, -0.0], np.float32)
    assert ge.quantize_ref(x, 0.25, 3).tolist() == [4, 2, 5, 1, 6, 255, 0, 3, 3]
    with pytest.raises(AssertionError):
        ge.quantize_ref(np.array([3e9], np.float32), 1.0, 0)  # outside the contract: not asserted anywhere


def test_letterbox_restatements_equal_the_oracle():
    exact = 0
    for cs in ge.LB_CASES:
        im = ge.letterbox_source(cs)
        want = oracle.letterbox_image(im, cs.h, cs.w)
        new_w, new_h, ox, oy = ge.letterbox_geometry(cs.imw, cs.imh, cs.w, cs.h)
        assert new_w >= 2 and new_h >= 2 and (new_w == cs.w or new_h == cs.h)
        assert np.array_equal(want[:, oy:oy + new_h, ox + new_w - 1], ge.letterbox_last_column(im, new_h)), cs.name
        row, iy, dy = ge.letterbox_last_row(im, new_w, new_h)
        assert np.array_equal(want[:, oy + new_h - 1, ox:ox + new_w], row), cs.name
        if iy == cs.imh - 1 and dy == 0:
            exact += 1
            assert np.array_equal(want[:, oy + new_h - 1, ox + new_w - 1], im[:, -1, -1])
    assert exact >= len(ge.LB_CASES) // 2
    for cs, message in ge.LB_REFUSED:
        if message == ge.LB_DEGENERATE:
            assert min(ge.letterbox_geometry(cs.imw, cs.imh, cs.w, cs.h)[:2]) < 2
            with pytest.raises(AssertionError):
                oracle.letterbox_image(np.zeros((cs.c, cs.imh, cs.imw), np.float32), cs.h, cs.w)


def test_yolo_and_checksum_references():
    import ctypes as C
    for n, classes, hw in ((1, 1, 1), (3, 80, 65), (5, 1, 257)):
        x = ge.yolo_input(ge.YOLO_B, n, classes, hw, seed=n)
        want = ge.yolo_ref(x)
        got = np.empty_like(x)
        for b in range(x.shape[0]):
            oracle.lib().orc_yolo_forward(x[b].ctypes.data, n, classes, 1, hw, got[b].ctypes.data)
        assert np.array_equal(got[:, :, 2:4].view(np.uint32), want[:, :, 2:4].view(np.uint32))
        act = np.ones(classes + 5, bool)
        act[2:4] = False
        assert ge.ulps_apart(got[:, :, act], want[:, :, act]).max() <= 1  # numpy's exp and libm's may differ in the last double place
        exact = np.isin(x[:, :, act], np.array(ge.YOLO_EXACT, np.float32))
        assert exact.sum() >= 3 and np.array_equal(got[:, :, act][exact], want[:, :, act][exact])
    one = np.float32(1.0)
    v = np.zeros((1, 1, 6, 1), np.float32)
    v[0, 0, [0, 1, 4, 5], 0] = (88.0, -104.0, 745.0, -np.inf)
    assert ge.yolo_ref(v)[0, 0, [0, 1, 4, 5], 0].tolist() == [one, 0.0, one, 0.0]
    assert ge.ulps_apart(np.float32([1.0, 0.0]), np.float32([np.nextafter(one, 2 * one), 1e-45])).tolist() == [1, 1]
    for n in (0, 1, 257, 5000):
        w = ge.checksum_words(n)
        wrapped = (w.astype(np.uint64) * (2 * np.arange(n, dtype=np.uint64) + 1)).sum(dtype=np.uint64) if n else 0
        assert ge.checksum_ref(w) == int(wrapped), n


# ------------------------------------------------------------------------------------------------------------------- the tables themselves
def test_every_clause_label_is_reached_on_both_sides():
    tables = ((ge.POOL_CLAUSES, ge.POOL_CASES), (ge.UP_CLAUSES, ge.UP_CASES), (ge.ROUTE_CLAUSES, ge.ROUTE_CASES), (ge.LAY_CLAUSES, ge.LAY_CASES),
              (ge.DQ_CLAUSES, ge.DQ_CASES), (ge.LB_CLAUSES, ge.LB_CASES))
    missing = [m for clauses, cases in tables for m in ge.Reach(clauses, cases).missing()]
    hits = {}
    for launch in ge.q_launches():
        for label, side in ge.q_path_labels(*launch):
            hits.setdefault(label, set()).add(side)
    assert set(hits) == set(ge.Q_LABELS)
    missing += [(k, side) for k in ge.Q_LABELS for side in (True, False) if side not in hits[k]]
    assert not missing, missing
    # the route table reaches both kernels
    assert any(ge.route_aligned(c.Cs) for c in ge.ROUTE_CASES) and any(not ge.route_aligned(c.Cs) for c in ge.ROUTE_CASES)
    assert {c for cs in ge.ROUTE_CASES if not ge.route_aligned(cs.Cs) for c in cs.Cs[:-1]} >= {1, 15, 17, 24}
    assert {cs.Cs[-1] for cs in ge.ROUTE_CASES if ge.route_aligned(cs.Cs)} >= {17, 40}
    assert {len(cs.Cs) for cs in ge.ROUTE_CASES} >= {1, 2, 4, 16}
    assert {cs.C for cs in ge.POOL_CASES} >= set(ge.CHANNELS) and {cs.C for cs in ge.UP_CASES} >= set(ge.CHANNELS)
    assert {cs.C for cs in ge.LAY_CASES} >= {1, 2, 3, 4, 5, 15, 16, 17}
    assert {cs.W for cs in ge.LAY_CASES if ge.layout_fast_path(cs)} >= {4, 8, 12}
    assert {cs.W for cs in ge.LAY_CASES if cs.C == 3 and not ge.layout_fast_path(cs)} >= {5, 6, 7, 8}
    assert {h * w for h, w in ge.YOLO_MAPS} == {1, 63, 64, 65, 257}
    for t in (ge.POOL_CASES, ge.UP_CASES, ge.ROUTE_CASES, ge.LAY_CASES, ge.DQ_CASES, ge.LB_CASES, ge.SC_SETS):
        assert len({c.name for c in t}) == len(t), "names are the test ids and the seeds"


def test_what_the_cases_let_a_kernel_write_is_theirs():
    """the group kernels own [off, off + up16(C)) of a cell: behind a ragged C lie pad bytes C..cs of the wider tensor's own cells, nothing else"""
    for cs in ge.POOL_CASES + ge.UP_CASES:
        assert ge.readable_ok(cs.x, cs.C) and ge.owned_ok(cs.y, cs.C), cs.name
        assert ge.pool_out(cs.H, cs.size, cs.stride, cs.pad) >= 1 if isinstance(cs, ge.Pool) else True
    r = ge.SC_RAGGED
    assert ge.readable_ok(r.a, r.C) and ge.readable_ok(r.b, r.C) and ge.owned_ok(r.y, r.C)
    assert len({r.a.cs, r.b.cs, r.y.cs}) == 3 and len({r.a.lead, r.b.lead, r.y.lead}) == 3 and r.C == 17
    for cs in ge.ROUTE_CASES:
        total, al = sum(cs.Cs), ge.route_aligned(cs.Cs)
        assert cs.y.off + total <= cs.y.wide <= cs.y.cs and cs.y.cs % 16 == 0, cs.name
        seen = {}
        for c, t in zip(cs.Cs, cs.xs):
            assert t.cs % 16 == 0 and t.off + (ge.up16(c) if al else c) <= t.cs and t.off + c <= t.wide, cs.name
            if al:
                assert t.off % 16 == 0, cs.name
            if ge.is_window(t, c):  # windows that share a wide tensor do not overlap
                used = seen.setdefault((t.cs, t.lead, t.wide), set())
                assert not used & set(range(t.off, t.off + c)), cs.name
                used |= set(range(t.off, t.off + c))
        writes = ge.route_writes(cs)
        assert writes[0][0] == cs.y.off and writes[-1][0] + writes[-1][1] <= cs.y.cs
        if al:
            assert cs.y.off % 16 == 0 and (cs.Cs[-1] % 16 == 0 or cs.y.off + total == cs.y.wide), cs.name
        else:
            assert writes[-1][0] + writes[-1][1] == cs.y.off + total
    for _, B, Cc, H, W, t in ge.UNLAY_CASES:
        assert t.off + Cc <= t.wide <= t.cs
    for cs in ge.DQ_CASES:
        assert 0 <= cs.c0 and cs.nc >= 1 and cs.c0 + cs.nc <= cs.C and 0 <= cs.out_c0 and cs.out_c0 + cs.nc <= cs.out_C, cs.name
        assert cs.zp in (0, 1, 77, 128, 255) and cs.scale in ge.DQ_SCALES
    # the sentinel is no zero point, plain or biased, and no fill of a float plane a reference could produce by accident
    assert all(ge.SENTINEL not in (zp, zp ^ 0x80) for zp in ge.ZERO_POINTS)
    assert {cs.zp for cs in ge.LAY_CASES} <= set(ge.ZERO_POINTS)


def test_tables_stay_small():
    worst = 0
    for cs in ge.POOL_CASES:
        OH, OW = ge.pool_out(cs.H, cs.size, cs.stride, cs.pad), ge.pool_out(cs.W, cs.size, cs.stride, cs.pad)
        worst = max(worst, ge.Cells(cs.B, cs.H, cs.W, cs.x.cs, cs.x.lead).nbytes, ge.Cells(cs.B, OH, OW, cs.y.cs, cs.y.lead).nbytes)
        assert max(cs.H, cs.W) <= 20 or cs.name.startswith("threads"), cs.name
    for cs in ge.UP_CASES:
        worst = max(worst, ge.Cells(cs.B, cs.H * cs.stride, cs.W * cs.stride, cs.y.cs, cs.y.lead).nbytes)
    for cs in ge.ROUTE_CASES:
        worst = max(worst, ge.Cells(cs.B, cs.H, cs.W, cs.y.cs, cs.y.lead).nbytes)
    worst = max(worst, ge.Cells(1, 256, 256, 16).nbytes)                         # the shortcut's all-pairs map
    worst = max(worst, 4 * ge.Q_COUNTS[-1], 4 * ge.CK_COUNTS[-1])                # the largest float image and checksum buffer
    worst = max(worst, max(4 * ge.YOLO_B * n * (c + 5) * h * w for n in ge.YOLO_N for c in ge.YOLO_CLASSES for h, w in ge.YOLO_MAPS))
    worst = max(worst, max(4 * cs.c * max(cs.w * cs.h, cs.imw * cs.imh) for cs in ge.LB_CASES))
    assert max(cs.w for cs in ge.LB_CASES) <= 32 and max(cs.h for cs in ge.LB_CASES) <= 32
    assert worst + 2 * ge.GUARD < ge.MAX_TENSOR_BYTES, worst
    assert ge.Q_COUNTS[-1] == 2048 * 256 + 1 and ge.CK_COUNTS[-1] == 1024 * 256 + 1 and ge.Q_B_REFUSED == 65536


def test_cells_restates_the_header():
    c = ge.Cells(2, 3, 4, 16, lead=2)
    assert c.tail == 7 and c.ncells == 2 + 2 * 4 * 5 + 7
    idx = c.interior().reshape(2, 3, 4)
    assert idx[0, 0, 0] == 2 + 5 and idx[1, 2, 3] == 2 + (1 * 4 + 3) * 5 + 3
    raw = np.zeros(c.nbytes, np.uint8)
    x = np.arange(2 * 5 * 3 * 4, dtype=np.uint8).reshape(2, 5, 3, 4)
    c.put(raw, x, 3)
    assert np.array_equal(c.get(raw, 3, 5), x) and raw.reshape(c.ncells, 16)[idx[1, 0, 1], 3] == x[1, 0, 0, 1] ^ 0x80
    k = c.kinds(3, 5).reshape(c.ncells, 16)
    assert (k[idx.ravel(), 3:8] == 0).all() and (k[idx.ravel(), :3] == 1).all() and (k[idx.ravel(), 8:] == 1).all() and (k == 2).sum() == (c.ncells - 24) * 16
    assert (raw.reshape(c.ncells, 16)[k.reshape(c.ncells, 16)[:, 0] == 2] == 0).all(), "put touches no pad cell"
    # a plane of the 4-byte image keeps its bytes plain
    c4 = ge.Cells(1, 2, 2, 4)
    raw = np.zeros(c4.nbytes, np.uint8)
    c4.put(raw, np.full((1, 3, 2, 2), 9, np.uint8))
    assert sorted(np.unique(raw).tolist()) == [0, 9]
    full = ge.nchw_to_cells_ref(np.full((1, 5, 2, 2), 7, np.uint8), 16)
    assert full.shape[1] == 8 and (full[:, 5:] == 0).all()
