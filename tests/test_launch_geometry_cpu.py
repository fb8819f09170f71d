"""The restated launch geometry (tests/launch_geometry.py) on the CPU: its reference against the oracle, the case table's coverage of
every labelled clause and its cost caps, and the launchers' invariants over seeded sweeps of a few thousand shapes each."""
import numpy as np
import pytest

import launch_geometry as lg
import oracle

MB = 1 << 20


# ------------------------------------------------------------------------------------------------------------ the reference
REF_SHAPES = [
    # (B, c, n, H, W, k, stride, zp_in)
    (3, 3, 16, 5, 7, 3, 1, 0), (2, 16, 32, 6, 4, 3, 1, 9), (2, 16, 32, 7, 9, 3, 2, 255), (4, 32, 64, 2, 2, 3, 1, 131), (1, 64, 30, 3, 5, 1, 1, 9),
    (2, 64, 64, 8, 6, 3, 2, 1), (5, 3, 32, 1, 1, 3, 1, 77), (2, 128, 32, 4, 4, 3, 1, 9), (3, 48, 16, 5, 5, 3, 1, 200), (2, 256, 255, 3, 3, 1, 1, 0),
    (2, 16, 16, 9, 11, 3, 2, 9), (3, 32, 32, 6, 10, 3, 1, 254),
]


@pytest.mark.parametrize("shape", REF_SHAPES, ids=lambda s: "B%d_c%d_n%d_%dx%d_k%d_s%d_zp%d" % s)
def test_reference_equals_oracle_image_by_image(shape):
    B, c, n, H, W, k, stride, zp_in = shape
    rng = np.random.default_rng(sum(shape))
    x = rng.integers(0, 256, (B, c, H, W), dtype=np.uint8)
    wq, zp_w, bias, mv, sv = lg.rand_layer(rng, n, c, k)
    assert zp_w[0] == 0 and (n == 1 or zp_w[1] == 255)
    zp_per_image = rng.integers(0, 256, B).astype(np.uint8)
    for zp in (zp_in, zp_per_image):
        for store in (oracle.STORE_WRAP, oracle.STORE_SATURATE):
            got = lg.conv_ref(x, wq, zp_w, k, stride, zp, bias, mv, sv, 23, oracle.ACT["leaky"], store)
            for b in range(B):
                z = int(np.broadcast_to(np.asarray(zp), (B,))[b])
                acc = oracle.conv_acc(x[b], wq, zp_w, k, stride, k // 2, z)
                want = oracle.requant(acc, bias, mv, sv, 23, oracle.ACT["leaky"], store).reshape(got[b].shape)
                assert np.array_equal(got[b], want), (b, store)
                if stride == 1 and H % 2 == 0 and W % 2 == 0:
                    assert np.array_equal(lg.maxpool2(got[b]), oracle.maxpool_u8(want, 2, 2, 1))
                if stride == 1 and H > 1:
                    assert np.array_equal(lg.maxpool1(got[b]), oracle.maxpool_u8(want, 2, 1, 1))


def test_reference_wraps_accumulators_as_the_oracle_does():
    """4096 channels of a 3 x 3 window: 36 864 products of up to 255 x 255 pass 2^31, below it and back.  Built operands (all-255 inputs,
    weights 255 against zero point 0, and the mirror image) put the centre pixel's sum at +-2 397 081 600; the reference must wrap it to int32
    exactly as oracle.conv_acc does"""
    c, k = 4096, 3
    x = np.full((2, c, 3, 3), 255, np.uint8)
    x[1] = np.random.default_rng(5).integers(200, 256, (c, 3, 3), dtype=np.uint8)
    wq = np.stack([np.full(c * k * k, 255, np.uint8), np.zeros(c * k * k, np.uint8)])
    zp_w = np.array([0, 255], np.uint8)
    got, OH, OW = lg.conv_acc_ref(x, wq, zp_w, k, 1, 255)
    exact = c * k * k * 255 * 255
    assert exact > 2 ** 31 and got[0, 4] == exact - 2 ** 32 and got[1, 4] == 2 ** 32 - exact, "the centre pixel of image 0, wrapped"
    for b in range(2):
        want = oracle.conv_acc(x[b], wq, zp_w, k, 1, 1, 255)
        assert np.array_equal(got[:, b * 9:(b + 1) * 9], want)
    assert (np.abs(got.astype(np.int64)) > 2 ** 30).all()


# ------------------------------------------------------------------------------------------------------------ the case table
def _table_trace():
    tot = lg.Trace()
    for cs in lg.CASES:
        tot.merge(lg.trace_case(cs)[0])
    return tot


def test_case_names_are_unique():
    names = [cs.name for cs in lg.CASES]
    assert len(set(names)) == len(names)


def test_every_clause_is_reached_on_both_sides():
    hits = _table_trace().hits
    excused = {**{l: True for l in lg.SIZE_GUARDS}, **{l: side for l, (side, _) in lg.DEAD.items()}, **{l: side for l, (side, _) in lg.OVER_CAP.items()}}
    assert set(excused) <= set(lg.ALL_LABELS)
    missing = []
    for label in lg.ALL_LABELS:
        for side in (True, False):
            if side not in hits.get(label, set()) and excused.get(label) is not side:
                missing.append((label, side))
    assert not missing, f"no case reaches {missing}"
    # what is excused is excused for one side only, with a reason, and the table does not reach it after all
    for label, side in excused.items():
        assert side not in hits.get(label, set()), f"{label} is declared unreached on its {side} side, but a case reaches it"
        assert (not side) in hits.get(label, set()), f"{label}: not even the other side is reached"
    for d in (lg.SIZE_GUARDS, lg.DEAD, lg.OVER_CAP):
        for label, why in d.items():
            assert (why if isinstance(why, str) else why[1]).strip(), label


def test_only_the_named_size_guards_are_left_for_their_size():
    """the guards that need tensors of 2 GiB and more: in_cells * in_cs >= 2^31 / 2^32, the pooled-cell guards, total_p + 256 >= 2^31, grid > 2^31"""
    kinds = ("in_bytes_2^32", "in_bytes_2^31", "in_cells_2^31", "pool_cells_24bit", "pool_bytes_2^32", "total_p_2^31", "ntiles_2^31", "grid_2^31")
    for label in lg.SIZE_GUARDS:
        assert label.split(".", 1)[1] in kinds, label


@pytest.mark.parametrize("cs", lg.CASES, ids=repr)
def test_case_cost_caps(cs):
    for name, nbytes in lg.device_tensors(cs).items():
        assert nbytes <= 64 * MB, (name, nbytes)
    assert lg.macs(cs) <= 6e9


# what the table must hold for every kernel that walks flat tiles: a case whose fullest tile is (nearly) full AND crosses at least this many
# image boundaries.  (family, key) -> (least fill, least crossings).  The row-image kernels' DMA-slot test admits maps at least 3/4 as wide as
# their row slots only, which bounds the images a tile can span there; a 3x3 tile of 384 columns in every workgroup of one round is 7.2e9
# multiply-adds, over the table's cap: those cases fill 73 % and more.
FULL_TILES = {
    ("conv_rows", (1, 128, 16, False)): (0.99, 4), ("conv_rows", (1, 128, 32, False)): (0.99, 1), ("conv_rows", (1, 128, 64, False)): (0.99, 0),
    ("conv_rows", (1, 384, 16, False)): (0.99, 1), ("conv_rows", (1, 384, 32, False)): (0.97, 2), ("conv_rows", (1, 384, 64, False)): (0.94, 1),
    ("conv_rows", (3, 128, 16, False)): (0.99, 2), ("conv_rows", (3, 128, 32, False)): (0.99, 1), ("conv_rows", (3, 128, 64, False)): (0.99, 0),
    ("conv_rows", (3, 256, 16, False)): (0.97, 4), ("conv_rows", (3, 256, 32, False)): (0.98, 2), ("conv_rows", (3, 256, 64, False)): (0.99, 0),
    ("conv_rows", (3, 384, 32, False)): (0.73, 2), ("conv_rows", (3, 384, 64, False)): (0.75, 1),
    ("conv_rows", (3, 128, 16, True)): (0.99, 3), ("conv_rows", (3, 256, 16, True)): (0.96, 5), ("conv_rows", (3, 384, 16, True)): (0.73, 11),
    ("conv_rows", (3, 384, 32, True)): (0.77, 3),
    # aligned tiles of 128 / 256 pixels over 4-pixel images span 32 / 64 of them: 31 / 63 boundaries
    ("conv_igemm", (3, 128)): (1.0, 31), ("conv_igemm", (3, 256)): (1.0, 63), ("conv_igemm", (1, 128)): (1.0, 127),
    ("conv_small", None): (1.0, 31), ("conv_small32", None): (1.0, 42), ("conv_mid", None): (1.0, 7),
    ("conv_ws3", None): (1.0, 63), ("conv1x1", None): (1.0, 63),
}


def test_every_flat_kernel_has_a_full_tile_that_crosses_image_boundaries():
    seen = {}
    for cs in lg.CASES:
        _, g, _ = lg.trace_case(cs)
        if g is None or g["grid"] is None:
            continue
        st = lg.tile_stats(cs, g)
        if st is None:
            continue
        key = {"conv_rows": lambda: (cs.k, g["bn"], g["RS"], g["rows16"]), "conv_igemm": lambda: (cs.k, g["bn"])}.get(g["family"], lambda: None)()
        seen.setdefault((g["family"], key), []).append(st)
    for fk, (fill, cross) in FULL_TILES.items():
        assert any(f >= fill and c >= cross for f, c in seen.get(fk, [])), f"{fk}: no case fills {fill} of a tile across {cross} image boundaries: {seen.get(fk)}"
    # a SERVED row-image launch on each row-slot width right at its threshold (W + 2 = 16, 32, 64 on conv_rows.hip; 17 on conv_rows16.hip's
    # narrow-map variant -- the DMA-slot test refuses every other 17- and 33-cell row: a map must be 3/4 as wide as its slots)
    served = {(cs.W + 2, g["RS"], g["rows16"]) for cs in lg.CASES for g in [lg.trace_case(cs)[1]] if g and g["family"] == "conv_rows"}
    assert {(16, 16, False), (16, 16, True), (32, 32, False), (64, 64, False), (17, 32, True)} <= served
    # the narrow-map 384 variant also with a tile over eight one-row images
    assert any(c >= 7 for f, c in seen[("conv_rows", (3, 384, 32, True))])


# ------------------------------------------------------------------------------------------------------------ sweeps
def _rand_B(rng):
    return int(rng.choice([1, 2, 3, 5, 8, 17, 64, 100, 255, 256, 257, 700, 1024, 4097, 16385, 49153, 65537, 300000]))


def _rand_hw(rng, even=False, hi=70):
    H, W = int(rng.integers(1, hi)), int(rng.integers(1, hi))
    if rng.random() < 0.15:
        W = int(rng.integers(hi, 700))
    if rng.random() < 0.3:
        H, W = int(rng.integers(1, 6)), int(rng.integers(1, 6))
    if even:
        H, W = 2 * ((H + 1) // 2), 2 * ((W + 1) // 2)
    return H, W


def _sweep_conv1x1(sweep_hits):
    rng = np.random.default_rng(1)
    for _ in range(4000):
        c, n = int(rng.choice([64, 128, 256, 512, 1024])), int(rng.choice([1, 30, 32, 64, 100, 255, 256, 512, 768, 1024]))
        B, (H, W), plan = _rand_B(rng), _rand_hw(rng), int(rng.integers(0, 2))
        if lg.in_cells(B, H, W) * c >= 2 ** 32:
            continue
        g = lg.conv1x1(sweep_hits, B, H, W, c, n, plan)
        if g["refused"]:
            continue
        total = B * H * W
        assert g["lds"] <= lg.LDS_MAX
        assert (g["ntiles"] - 1) * g["tp"] < total <= g["ntiles"] * g["tp"], "tiles cover every pixel exactly once"
        assert g["grid"] == g["ntiles"] * g["mtiles"] and g["threads"] <= 512
        assert g["tp"] <= g["gmax"] * 32 or (plan == 1 and g["rounds"] == 1), "the tile limit of gmax groups (the one-round growth is bounded by LDS)"
        if g["rounds"] > 1 or g["grid"] > 256:
            assert g["lds"] <= 96 * lg.KB, "two workgroups per CU beyond one round of the chip"


def _sweep_conv_ws3(sweep_hits):
    rng = np.random.default_rng(2)
    done = 0
    for _ in range(3000):
        c, n = int(rng.choice([128, 256])), int(rng.choice([32, 64, 128, 256, 512, 1024]))
        if not lg.ws3_eligible(n, c, 3):
            continue
        B, (H, W), plan = min(_rand_B(rng), 70000), _rand_hw(rng), int(rng.integers(0, 2))
        S, pm = [(1, 0), (2, 0), (1, 1), (1, 2)][int(rng.integers(0, 4))]
        if pm == 2:
            H, W = 2 * ((H + 1) // 2), 2 * ((W + 1) // 2)
        if pm == 1 and rng.random() < 0.2:  # whole-image tiles of up to 256 pixels, 256 channels: the form that can miss LDS
            c, n, B, H, W = 256, int(rng.choice([128, 256])), 128, int(rng.integers(2, 17)), 16
        if pm == 1 and H < 2:
            continue
        if lg.in_cells(B, H, W) * c >= 2 ** 32:
            continue
        g = lg.conv_ws3(sweep_hits, B, H, W, c, n, S, pm, plan)
        if g["refused"]:
            continue
        done += 1
        total, tp = g["total"], g["tp"]
        assert g["lds"] <= lg.LDS_MAX
        assert (g["ntiles"] - 1) * tp < total <= g["ntiles"] * tp, "tiles cover every unit exactly once"
        assert tp * g["upx"] <= lg.WS3_GMAX * 32, "a tile is at most eight groups of 32 pixels"
        assert g["grid"] == g["mtiles"] * g["nwg"] and g["nwg"] <= max(256 // g["mtiles"], 1)
        if pm:
            assert g["ntiles"] == g["nwg"] or pm == 1, "the stride-2 pool exists for one tile per workgroup"
        if pm == 1:
            assert tp == ((H + 2 - 3) + 1) * ((W + 2 - 3) + 1), "the stride-1 pool needs whole-image tiles"
        # rows_cap against the rows the worst tile spans in the padded layout (H + 1 rows an image, a halo row above and below)
        OH, OW = (H - 1) // S + 1, (W - 1) // S + 1
        t = np.arange(g["ntiles"], dtype=np.int64)
        p0, p1 = t * tp, np.minimum(t * tp + tp, total) - 1
        if pm == 2:
            per, w2 = (OH // 2) * (OW // 2), OW // 2
            first = (p0 // per) * (H + 1) + 2 * ((p0 % per) // w2)
            last = (p1 // per) * (H + 1) + 2 * ((p1 % per) // w2) + 1
        else:
            first = (p0 // (OH * OW)) * (H + 1) + S * ((p0 % (OH * OW)) // OW)
            last = (p1 // (OH * OW)) * (H + 1) + S * ((p1 % (OH * OW)) // OW)
        span = int((last - first).max()) + 3
        assert g["rows_cap"] >= span - (1 if g["alias"] else 0)
        if g["alias"]:
            assert span == H + 2 and tp == OH * OW and S == 1, "only whole-image tiles let the pad rows above and below alias"
    assert done > 300


def _check_flat(g, ppb_cells, what):
    assert g["lds"] <= lg.LDS_MAX
    if g["tiles_x"]:
        assert g["ntiles"] * 128 >= g["total"] and g["tiles_x"] * 16 >= g["OW"] and g["tiles_y"] * 8 >= g["OH"], "patches cover the pooled map"
        assert (g["tiles_x"] - 1) * 16 < g["OW"] and (g["tiles_y"] - 1) * 8 < g["OH"], "no patch lies outside it"
        assert g["rows_cap"] == 18, "8 pooled rows: 16 image rows and a halo row above and below"
    else:
        tp = g["tp"]
        assert (g["ntiles"] - 1) * tp < g["total"] <= g["ntiles"] * tp, "tiles cover every pooled pixel exactly once"
        span = lg.worst_flat_span(tp, g["total"], g["OH"], g["OW"])
        assert g["rows_cap"] >= span, f"{what}: rows_cap {g['rows_cap']} below the {span} rows the worst tile spans ({g})"
        assert g["ncell"] >= 2 * g["OW"] + 2
    assert 64 <= g["rows_cap"] * g["ncell"] <= ppb_cells, "the image fits the DMA instructions a wave issues per piece"


def _sweep_conv_small_and_small32(sweep_hits):
    rng = np.random.default_rng(3)
    done = 0
    for _ in range(5000):
        c, n = int(rng.choice([16, 32])), int(rng.choice([32, 64]))
        B, (H, W), plan = _rand_B(rng), _rand_hw(rng, hi=140), int(rng.integers(0, 2))
        if lg.in_cells(B, H, W) * c >= 2 ** 32 or B * H * W >= 2 ** 32:
            continue
        g = lg.conv_small(sweep_hits, B, H, W, c, n, plan)
        if not g["refused"]:
            done += 1
            _check_flat(g, 4 * lg.SM_KMAX * 64, "conv_small")
            assert g["grid"] <= 768 and g["per_cu"] * g["lds"] <= lg.LDS_MAX
        if (c, n) == (32, 64) and not (H | W) & 1:
            g = lg.conv_small32(sweep_hits, B, H, W)
            if not g["refused"]:
                _check_flat(g, 8 * lg.S32_KDMA * 64, "conv_small32")
                assert 2 * g["lds"] <= lg.LDS_MAX and g["grid"] <= 512
    assert done > 500


def _sweep_conv_mid(sweep_hits):
    rng = np.random.default_rng(4)
    done = 0
    for _ in range(5000):
        n = int(rng.choice([64, 96, 128]))
        B, (H, W), plan = _rand_B(rng), _rand_hw(rng, hi=140), int(rng.integers(0, 2))
        if lg.in_cells(B, H, W) * 64 >= 2 ** 32:
            continue
        g = lg.conv_mid(sweep_hits, B, H, W, n, plan)
        if g["refused"]:
            continue
        done += 1
        _check_flat(g, 10 ** 9, "conv_mid")
        assert g["tp"] <= lg.SM_GMAX * 32, "a tile is at most eight groups of 32 pooled pixels"
        assert g["grid"] == g["ntiles"]
        if g["half"]:
            assert 2 * g["lds"] <= lg.LDS_MAX, "two half workgroups share a CU"
        if plan == 1 and not g["tiles_x"]:
            assert g["tp"] % 32 == 0 and g["tp"] <= 128
    assert done > 500


def _check_xcd_walk(grid, ntiles):
    """conv_pool16 / the pooled first layer keep one tile per lane: no workgroup may be handed more than 64"""
    w = np.arange(grid, dtype=np.int64)
    xw = grid % 8 == 0
    per_x = lg.cdiv(ntiles, 8) if xw else ntiles
    stride = grid // 8 if xw else grid
    base = (w & 7) * per_x if xw else 0 * w
    end = np.minimum(base + per_x, ntiles)
    t0 = base + (w >> 3 if xw else w)
    count = np.maximum(0, -(-(end - t0) // stride))
    assert int(count.sum()) == ntiles, "every tile is walked exactly once ((XCD, residue) pairs are distinct, so the count settles it)"
    assert int(count.max()) <= 64, f"a workgroup of a grid of {grid} walks {int(count.max())} of {ntiles} tiles"


def test_xcd_walk_helper_agrees_with_the_enumeration():
    for grid, ntiles in ((8, 1), (768, 769), (776, 49153), (1032, 65537), (767, 767), (1024, 65536), (20, 20)):
        most, once = lg.xcd_walk_tiles(grid, ntiles)
        assert once and most <= 64
        _check_xcd_walk(grid, ntiles)
    assert lg.xcd_walk_tiles(768, 49153)[0] == 65, "without the widening a workgroup would be handed 65 tiles"
    assert lg.xcd_walk_tiles(1024, 65537)[0] == 65


def _sweep_pool16_and_first_layer(sweep_hits):
    rng = np.random.default_rng(5)
    for _ in range(3000):
        B, (H, W) = _rand_B(rng), _rand_hw(rng, even=True, hi=120)
        if rng.random() < 0.05:
            B, H, W = 1, 2, int(rng.choice([32736, 32738, 32752]))
        if lg.in_cells(B, H, W) * 16 >= 2 ** 31:
            continue
        g = lg.conv_pool16(sweep_hits, B, H, W)
        if not g["refused"]:
            assert g["tiles_x"] <= 1023 and g["tiles_y"] <= 1023
            assert (g["tiles_x"] - 1) * 16 < g["OW"] <= g["tiles_x"] * 16 and (g["tiles_y"] - 1) * 8 < g["OH"] <= g["tiles_y"] * 8
            _check_xcd_walk(g["grid"], g["ntiles"])
        n, pool, pi = int(rng.choice([16, 32])), bool(rng.integers(0, 2)), rng.random() < 0.4
        if pi and rng.random() < 0.3:
            B, H, W = int(rng.choice([1024, 1100, 2048])), 2, int(rng.choice([2050, 2080, 4160]))  # B * tpi > 65 536 with tpi >= 65
        g = lg.conv_first(sweep_hits, B, H, W, n, pool, per_image=pi)
        if g["refused"]:
            continue
        tpi = g["tiles_x"] * g["tiles_y"]
        if pi:
            most, once = lg.per_image_walk_tiles(B, tpi, g["wpi"])
            assert once and most <= 64 and g["grid"] == g["wpi"] * B and 1 <= g["wpi"] <= tpi
        elif pool:
            _check_xcd_walk(g["grid"], g["ntiles"])
        else:
            assert g["grid"] == min(g["ntiles"], 1024), "the form without a pool walks its tiles in a loop: no 64-tile limit, no widening"


def _sweep_conv_igemm(sweep_hits):
    rng = np.random.default_rng(6)
    rows = cfgs = 0
    for _ in range(5000):
        c, n = int(rng.choice([16, 32, 48, 64, 128, 192, 256, 512])), int(rng.choice([16, 30, 32, 48, 64, 128, 200, 255, 256, 512]))
        B, (H, W), plan = min(_rand_B(rng), 5000), _rand_hw(rng), int(rng.integers(0, 2))
        k, S, pool = [(1, 1, False), (3, 1, False), (3, 2, False), (3, 1, True)][int(rng.integers(0, 4))]
        if pool:
            H, W = 2 * ((H + 1) // 2), 2 * ((W + 1) // 2)
        if lg.in_cells(B, H, W) * c >= 2 ** 32:
            continue
        g = lg.conv_igemm(sweep_hits, B, H, W, c, n, k, S, pool, plan)
        if g["refused"]:
            continue
        assert g["lds"] <= lg.LDS_MAX
        if g["family"] == "conv_rows":
            rows += 1
            assert g["tile_q"] + (1 if g["tile_r"] else 0) <= g["bn"], "no tile holds more pixels than the kernel's columns"
            assert g["ntiles"] * g["tile_q"] + g["tile_r"] == g["total"], "tiles cover every pixel exactly once"
            span = lg.worst_rows_span(g, H, W)
            assert g["rows_cap"] >= span, f"rows_cap {g['rows_cap']} below the {span} rows the worst tile spans ({g})"
            assert W + 2 <= g["RS"], "a padded row fits its LDS slots"
            assert g["grid"] == g["ntiles"] * g["mtiles"]
        else:
            cfgs += 1
            assert g["threads"] in (256, 512)
    assert rows > 500 and cfgs > 500


SWEEPS = [_sweep_conv1x1, _sweep_conv_ws3, _sweep_conv_small_and_small32, _sweep_conv_mid, _sweep_pool16_and_first_layer, _sweep_conv_igemm]


@pytest.fixture(scope="module")
def sweep_hits():
    """every sweep on one trace: each asserts its launcher's invariants on the way and records the clause sides it took"""
    tr = lg.Trace()
    for sweep in SWEEPS:
        sweep(tr)
    return tr


@pytest.mark.parametrize("sweep", SWEEPS, ids=lambda f: f.__name__[7:])
def test_sweep_invariants(sweep, sweep_hits):
    """(the fixture has run every sweep and would have raised; this names them one by one and reruns none)"""
    assert any(l.split(".")[0] for l in sweep_hits.hits)


def test_dead_clauses_stay_dead_and_the_sweep_reaches_what_the_table_cannot(sweep_hits):
    hits = sweep_hits.hits
    assert len(hits) > 100
    table = _table_trace().hits
    # (s32.odd_map / p16.odd_map: dead because the C ABI refuses a stride-2 pool on an odd map; the sweeps feed those two launchers even maps
    # only and are no evidence for them)
    for label, (side, why) in lg.DEAD.items():
        assert side not in hits.get(label, set()) and side not in table.get(label, set()), f"{label} is not dead: {why}"
    for label, (side, why) in lg.OVER_CAP.items():
        assert side in hits.get(label, set()), f"the sweep does not reach {label} either"
