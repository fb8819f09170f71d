"""The general conv kernel's restated launcher and K layout (tests/kxk_geometry.py) on the CPU: its reference against the oracle, the case
table's coverage of every labelled clause and its cost caps, the launcher's invariants over a seeded sweep with strides up to 16, the packed A
fragments unpacked with the layout the restatement states, and what the older hand-picked grid of test_gpu_conv_kxk.py reaches."""
import copy

import numpy as np
import pytest

import kxk_geometry as kg
import launch_geometry as lg
import oracle
from yolo_quantization_amd import binding

MB = 1 << 20


# ------------------------------------------------------------------------------------------------------------ the reference
REF_SHAPES = [
    # (B, c, n, H, W, k, stride, pad)
    (3, 3, 16, 5, 7, 3, 1, 1), (2, 5, 9, 6, 4, 2, 1, 0), (2, 16, 7, 7, 9, 5, 2, 4), (2, 1, 4, 9, 9, 11, 4, 5), (1, 24, 30, 3, 5, 1, 1, 0),
    (2, 9, 17, 8, 6, 4, 3, 3), (3, 3, 8, 1, 1, 3, 1, 2), (2, 20, 12, 4, 4, 3, 1, 5), (2, 8, 16, 13, 10, 7, 5, 0), (1, 33, 5, 6, 9, 6, 2, 3),
    (2, 4, 16, 9, 11, 3, 2, 1), (2, 12, 32, 6, 10, 2, 3, 2),
]


@pytest.mark.parametrize("shape", REF_SHAPES, ids=lambda s: "B%d_c%d_n%d_%dx%d_k%d_s%d_p%d" % s)
def test_reference_equals_oracle_image_by_image(shape):
    B, c, n, H, W, k, stride, pad = shape
    rng = np.random.default_rng(sum(shape))
    x = rng.integers(0, 256, (B, c, H, W), dtype=np.uint8)
    wq, zp_w, bias, mv, sv = lg.rand_layer(rng, n, c, k)
    zp_per_image = rng.integers(0, 256, B).astype(np.uint8)
    for zp in (int(rng.integers(0, 256)), zp_per_image):
        for store in (oracle.STORE_WRAP, oracle.STORE_SATURATE):
            acc, got = kg.conv_ref(x, wq, zp_w, k, stride, pad, zp, bias, mv, sv, 23, oracle.ACT["leaky"], store)
            for b in range(B):
                z = int(np.broadcast_to(np.asarray(zp), (B,))[b])
                a = oracle.conv_acc(x[b], wq, zp_w, k, stride, pad, z)
                assert np.array_equal(acc[b], a), (b, "int32")
                want = oracle.requant(a, bias, mv, sv, 23, oracle.ACT["leaky"], store).reshape(got[b].shape)
                assert np.array_equal(got[b], want), (b, store)
    if k == 3 and pad == 1:  # where launch_geometry's reference applies the two agree
        assert np.array_equal(kg.conv_acc_ref(x, wq, zp_w, k, stride, pad, zp_per_image)[0], lg.conv_acc_ref(x, wq, zp_w, k, stride, zp_per_image)[0])


def test_reference_wraps_accumulators_as_the_oracle_does():
    """1024 channels of a 7 x 7 window at stride 2, padding 5: 50 176 products of 255 x 255 pass 2^31 where the window lies in the image and its
    zero-point fill (255) alike; the mirror-image filter goes below -2^31.  The reference must wrap them to int32 exactly as oracle.conv_acc does"""
    c, k = 1024, 7
    x = np.full((2, c, 5, 6), 255, np.uint8)
    x[1] = np.random.default_rng(5).integers(200, 256, (c, 5, 6), dtype=np.uint8)
    wq = np.stack([np.full(c * k * k, 255, np.uint8), np.zeros(c * k * k, np.uint8)])
    zp_w = np.array([0, 255], np.uint8)
    got, OH, OW = kg.conv_acc_ref(x, wq, zp_w, k, 2, 5, 255)
    exact = c * k * k * 255 * 255
    assert exact > 2 ** 31 and got[0, 0] == exact - 2 ** 32 and got[1, 0] == 2 ** 32 - exact, "a window of image 0, wrapped"
    for b in range(2):
        want = oracle.conv_acc(x[b], wq, zp_w, k, 2, 5, 255)
        assert np.array_equal(got[:, b * OH * OW:(b + 1) * OH * OW], want)


# ------------------------------------------------------------------------------------------------------------ the case table
def _traces(cs):
    """the case's trace, and its ref-f32 twin's where it runs one"""
    out = [kg.trace_case(cs)]
    if cs.twin:
        c2 = copy.copy(cs)
        c2.accum = "ref_f32"
        out.append(kg.trace_case(c2))
    return out


def _table_trace():
    tot = kg.Trace()
    for cs in kg.CASES:
        for tr, _ in _traces(cs):
            tot.merge(tr)
    return tot


def _launches():
    return [(cs, g) for cs in kg.CASES for g in [kg.trace_case(cs)[1]] if g != "specialised" and g["kernel"] == 9]


def test_case_names_are_unique():
    names = [cs.name for cs in kg.CASES]
    assert len(set(names)) == len(names)


def test_every_clause_is_reached_on_both_sides():
    hits = _table_trace().hits
    excused = {**{l: True for l in kg.SIZE_GUARDS}, **{l: side for l, (side, _) in kg.DEAD.items()}}
    assert set(excused) <= set(kg.ALL_LABELS)
    missing = [(label, side) for label in kg.ALL_LABELS for side in (True, False)
               if side not in hits.get(label, set()) and excused.get(label) is not side]
    assert not missing, f"no case reaches {missing}"
    for label, side in excused.items():
        assert side not in hits.get(label, set()), f"{label} is declared unreached on its {side} side, but a case reaches it"
        assert (not side) in hits.get(label, set()), f"{label}: not even the other side is reached"
    for d in (kg.SIZE_GUARDS, kg.DEAD):
        for label, why in d.items():
            assert (why if isinstance(why, str) else why[1]).strip(), label
    assert set(kg.DEAD) >= {"l.slots>128", "l.tw>npx", "l.in_cs4_needs_unit4"} and set(kg.SIZE_GUARDS) == {"l.grid_2^31"}


@pytest.mark.parametrize("cs", kg.CASES, ids=repr)
def test_case_cost_caps(cs):
    for name, nbytes in kg.device_tensors(cs).items():
        assert nbytes <= 64 * MB, (name, nbytes)
    assert kg.macs(cs) <= 6e9


def test_accepted_cases_keep_the_kernel_invariants():
    for cs, g in _launches():
        kg.check_launch(g, cs.B, cs.H, cs.W, cs.c, cs.n, cs.k, cs.stride, cs.pad, cs.in_cs())


# what the arithmetic allows: with 16-byte units no stride leaves room for 8 columns x 32 rows where 16 x 16 does not fit and the second
# configuration is not needed ((15 s + k)^2 > 10 208 cells >= (31 s + k)(7 s + k) has no solution with k <= 11); with 4- and 8-byte units the
# first configuration's fall-back to 16 is never taken (it needs s < k, and then 16 x 16 fits: (15 * 10 + 11)^2 = 25 921 cells of 8 bytes and
# more are over the limit only from s = 11); the second configuration's fall-back to 8 is never taken by any unit (an 8-wide patch of 8 rows
# is the larger one whenever s < k, and for s > k the preferred width is 8 itself or fits).  The sweep below checks each of these.
LDS_OUTCOMES = {
    (16, 0, "pref"), (16, 0, "fall16"), (16, 1, "pref"), (16, 1, "fall16"), (16, None, "refused"),
    (8, 0, "pref"), (8, 0, "fall8"), (8, 1, "pref"), (8, 1, "fall16"), (8, None, "refused"),
    (4, 0, "pref"), (4, 0, "fall8"), (4, 1, "pref"), (4, 1, "fall16"), (4, None, "refused"),
}
INSTANTIATIONS = {(U, ms, wm) for U in (4, 8, 16) for ms, wm in ((1, 1), (2, 1), (1, 4))}


def _outcome(cs, g):
    return (kg.kxk_unit(cs.c), g.get("cfg"), g["choice"])


def test_table_reaches_every_lds_outcome_instantiation_and_width():
    got = {_outcome(cs, g) for cs in kg.CASES for g in [kg.trace_case(cs)[1]] if g != "specialised" and "choice" in g}
    assert got == LDS_OUTCOMES
    L = _launches()
    assert {g["inst"] for _, g in L} == INSTANTIATIONS
    # every instantiation at every tile width it can have, with dynamic LDS on each side of 64 KiB, and a small launch BEHIND the large one
    # (the large one raises the kernel's dynamic-LDS limit; the next launch must still be right)
    for inst in INSTANTIATIONS:
        mine = [g for _, g in L if g["inst"] == inst]
        assert {g["tw"] for g in mine} == {8, 16, 32}, inst
        big = [i for i, g in enumerate(mine) if g["lds"] > 64 * kg.KB]
        assert big and any(g["lds"] <= 64 * kg.KB for g in mine[big[0] + 1:]), inst
    # the second configuration: filter groups at n = 128 | 129, and tiles along x, along y, filter groups and B = 3 together, per unit
    wm4 = [(cs, g) for cs, g in L if g["inst"][2] == 4]
    assert {128, 129} <= {cs.n for cs, _ in wm4}
    for U in (4, 8, 16):
        for wm in (1, 4):
            assert any(g["tiles_x"] > 1 and g["tiles_y"] > 1 and g["mgroups"] > 1 and cs.B == 3 for cs, g in L if g["inst"][0] == U and g["inst"][2] == wm), (U, wm)
    # partial tiles on both axes at once; tile rows at OH = th | th + 1 for every width of the first configuration
    assert any(g["OW"] % g["tw"] and g["OH"] % g["th"] and g["tiles_x"] > 1 and g["tiles_y"] > 1 for _, g in L)
    for tw in (8, 16, 32):
        assert {g["OH"] - g["th"] for _, g in L if g["tw"] == tw and g["cfg"] == 0} >= {0, 1}, tw
    assert {8, 9, 16, 17, 32, 33} <= {g["OW"] for _, g in L}


def test_table_reaches_the_k_layout_edges():
    L = _launches()
    cs_of = {kg.kxk_unit(cs.c): set() for cs, _ in L}
    for cs, _ in L:
        cs_of[kg.kxk_unit(cs.c)].add((cs.c, cs.k))
    assert {1, 2, 3, 4} <= {c for c, _ in cs_of[4]} and {5, 7, 8} <= {c for c, _ in cs_of[8]}
    assert {1, 3, 4, 5, 12, 13, 15, 0} <= {c % 16 for c, _ in cs_of[16] if c > 16}, "the last chunk's mask on, under and over each dword edge"
    assert {9, 12, 13, 15, 16, 17} <= {c for c, _ in cs_of[16]}
    assert {1, 4, 11} <= {k for _, k in cs_of[4]} and {2, 3} <= {k for _, k in cs_of[8]}
    assert {k % 2 for _, k in cs_of[16]} == {0, 1}
    # the cells: c <= 4 from plain 4-byte cells and from 16-byte biased cells, 3 filters to plain cells, a y window off the dword grid
    assert {cs.in_cs() for cs, _ in L if cs.c <= 4} == {4, 16} and any(cs.out_cs() == 4 for cs, _ in L)
    assert any(cs.ywin and cs.ywin[1] % 4 for cs, _ in L)
    assert {1, 7, 33, 37, 32, 64, 65} <= {cs.n for cs, _ in L}
    # paddings 0, k / 2, k - 1 and beyond k; strides whose last window ends short of the map's edge
    pads = {("0" if cs.pad == 0 else "k/2" if cs.pad == cs.k // 2 else "k-1" if cs.pad == cs.k - 1 else ">k" if cs.pad > cs.k else "") for cs, _ in L}
    assert {"0", "k/2", "k-1", ">k"} <= pads
    assert any((cs.H + 2 * cs.pad - cs.k) % cs.stride and (cs.W + 2 * cs.pad - cs.k) % cs.stride for cs, _ in L)
    # every ref-f32 twin, one per unit at least
    assert {kg.kxk_unit(cs.c) for cs, _ in L if cs.twin} == {4, 8, 16}


def test_operands_exercise_both_store_modes():
    """every case's random layer gives bytes that differ between wrap and saturate: the device's two store modes are told apart"""
    for cs in kg.CASES:
        ops = kg.Operands(cs)
        if ops.want is not None:
            assert ops.stores_differ(), cs.name


# ------------------------------------------------------------------------------------------------------------ the sweep
@pytest.fixture(scope="module")
def sweep():
    """a few thousand random (c, n, k, s, pad, H, W, B) with strides up to 16: the invariants of every accepted launch, and of every refusal"""
    rng = np.random.default_rng(9)
    tr = kg.Trace()
    seen, outcomes = set(), set()
    for _ in range(3000):
        c = int(rng.choice([1, 2, 3, 4, 5, 7, 8, 9, 12, 16, 17, 24, 33, 40, 66]))
        n = int(rng.choice([1, 3, 7, 17, 32, 33, 64, 65, 128, 129, 200, 255]))
        k, s = int(rng.integers(1, 12)), int(rng.integers(1, 17))
        if rng.random() < 0.15:
            s = int(rng.integers(17, 33))  # (beyond the sweep's range: where the narrow units refuse)
        pad = int(rng.choice([0, k // 2, k - 1, k + 1]))
        OH, OW = int(rng.integers(1, 40)), int(rng.integers(1, 40))
        H, W = (OH - 1) * s + k - 2 * pad + int(rng.integers(0, s)), (OW - 1) * s + k - 2 * pad + int(rng.integers(0, s))
        B = int(rng.choice([1, 2, 3, 5]))
        if H < 1 or W < 1 or (k == 1 and (s != 1 or pad)):
            continue
        g = kg.conv_kxk_launch(tr, B, H, W, c, n, k, s, pad)
        U = kg.kxk_unit(c)
        outcomes.add((U, g.get("cfg"), g["choice"]))
        if g["refused"]:
            assert kg.nothing_fits(U, k, s, kg.out_size(H, W, k, s, pad)[1]), "refused although a configuration of the list fits"
            continue
        assert not kg.nothing_fits(U, k, s, g["OW"])
        kg.check_launch(g, B, H, W, c, n, k, s, pad)
        seen.add((g["inst"], g["tw"]))
    # every (unit, size, stride up to 32) at each preferred width, on maps of three tile rows at most: the LDS arithmetic exhaustively
    for c in (3, 8, 16):
        for k in range(2, 12):
            for s in range(1, 33):
                for OW in (5, 12, 20):
                    H, W = 2 * s + k, (OW - 1) * s + k
                    g = kg.conv_kxk_launch(tr, 1, H, W, c, 40, k, s, 0)
                    outcomes.add((kg.kxk_unit(c), g.get("cfg"), g["choice"]))
                    if g["refused"]:
                        assert kg.nothing_fits(kg.kxk_unit(c), k, s, OW)
                    else:
                        kg.check_launch(g, 1, H, W, c, 40, k, s, 0)
                        seen.add((g["inst"], g["tw"]))
    return tr, seen, outcomes


def test_sweep_invariants_and_reach(sweep):
    tr, seen, outcomes = sweep
    assert {inst for inst, _ in seen} == INSTANTIATIONS and {tw for _, tw in seen} == {8, 16, 32}
    assert outcomes == LDS_OUTCOMES, "the outcomes the arithmetic allows, no other (see LDS_OUTCOMES)"
    assert tr.hits["l.fall8_fits"] == {True, False} and tr.hits["l.fall16_fits"] == {True, False}


def test_dead_clauses_stay_dead(sweep):
    hits, table = sweep[0].hits, _table_trace().hits
    for label, (side, why) in kg.DEAD.items():
        assert side not in hits.get(label, set()) and side not in table.get(label, set()), f"{label} is not dead: {why}"
    for label in kg.SIZE_GUARDS:
        assert True not in hits.get(label, set()) and True not in table.get(label, set())
    # the slot count behind l.slots>128, for every unit and size
    for c in (1, 8, 16):
        for k in range(1, 12):
            g = kg.kxk_geom(16, c, k)
            assert k * k <= g["spc"] * 2 * g["tpl"] <= kg.MAX_SLOTS
    assert kg.kxk_geom(16, 3, 11)["spc"] * 8 == kg.MAX_SLOTS


# ------------------------------------------------------------------------------------------------------------ the packing
HDR = np.dtype([("magic", "<u4"), ("n", "<i4"), ("c", "<i4"), ("ksize", "<i4"), ("mpad", "<i4"), ("cb", "<i4"),
                ("nchunks", "<i4"), ("upc", "<i4"), ("spc", "<i4"), ("ksteps", "<i4"), ("ktrue", "<i4"), ("first", "<i4"),
                ("off_wp", "<u8"), ("off_cw", "<u8"), ("off_dzp", "<u8"), ("off_bias", "<u8"), ("off_mval", "<u8"),
                ("off_sval", "<u8"), ("total", "<u8"), ("off_shift", "<u8"), ("pow2", "<i4"), ("generic", "<i4"),
                ("off_mprime", "<u8"), ("off_cwb", "<u8"), ("off_ws", "<u8"), ("off_ept", "<u8"), ("off_gen", "<u8")])

# one shape per unit and tail kind: U = 16 even | odd k, one | two chunks with a partial last one; U = 8 exact | masked; U = 4 seven masked slots |
# exact | the table full; a specialised 3x3 blob's and a 3-filter 1x1 blob's general section; filters over one 128-row tile
PACK_SHAPES = [(12, 24, 6), (12, 24, 7), (8, 16, 2), (40, 9, 3), (12, 6, 2), (12, 7, 3), (12, 3, 1), (12, 3, 4), (12, 2, 11), (130, 5, 3), (16, 16, 3),
               (3, 32, 1), (33, 37, 5)]


@pytest.mark.parametrize("n,c,k", PACK_SHAPES, ids=lambda v: str(v))
def test_general_section_unpacks_to_the_weights(n, c, k):
    """the general section of mi355_conv_pack's blob, unpacked with the layout the restatement states (lane, half, tap slot, channel), gives
    the weights minus 128 back; padding channels, padding slots and padding filters are zero"""
    rng = np.random.default_rng(n * 1000 + c * 10 + k)
    wq, zp_w, bias, mv, sv = lg.rand_layer(rng, n, c, k)
    wq[wq == 128] = 129  # no weight packs to zero: a zero byte is padding
    blob = binding.conv_pack(wq, zp_w, c, k, bias, mv, sv)
    h = {key: int(v) for key, v in zip(HDR.names, np.frombuffer(blob[:HDR.itemsize].tobytes(), HDR)[0])}
    g = kg.kxk_geom(n, c, k)
    assert h["off_gen"] and h["generic"] == (0 if kg.specialised_shape(c, k) else 1)
    if h["generic"]:
        assert (h["cb"], h["nchunks"], h["spc"], h["ksteps"], h["mpad"]) == (g["unit"], g["nchunks"], g["spc"], g["ksteps"], g["mpad"])
    nbytes = g["mpad"] // 32 * g["ksteps"] * 1024
    assert h["off_gen"] + nbytes <= h["total"]
    frag = blob[h["off_gen"]:h["off_gen"] + nbytes].view(np.int8).reshape(g["mpad"] // 32, g["ksteps"], 64, 16)
    tap, chan = kg.frag_index(g, k)
    real = (tap >= 0) & (chan < c)                                                   # [ksteps, 64, 16]
    row = 32 * np.arange(g["mpad"] // 32)[:, None, None, None] + (np.arange(64) % 32)[None, None, :, None] + 0 * tap[None]
    real4 = real[None] & (row < n)
    assert not frag[~real4].any(), "padding channels, padding tap slots and padding filters carry weight 0"
    assert frag[real4].all(), "(and every real weight is there: none of them is 128)"
    # unpack: weight (filter, channel, tap) from its one place in the fragments
    got = np.zeros((n, c, k * k), np.int16)
    cnt = np.zeros((n, c, k * k), np.int32)
    idx = np.nonzero(real4)
    np.add.at(got, (row[idx], np.broadcast_to(chan[None], real4.shape)[idx], np.broadcast_to(tap[None], real4.shape)[idx]), frag[idx])
    np.add.at(cnt, (row[idx], np.broadcast_to(chan[None], real4.shape)[idx], np.broadcast_to(tap[None], real4.shape)[idx]), 1)
    assert (cnt == 1).all(), "every weight is packed exactly once"
    assert np.array_equal(got, wq.astype(np.int16).reshape(n, c, k * k) - 128)


# ------------------------------------------------------------------------------------------------------------ the older grid
def test_what_the_hand_picked_grid_reaches():
    """the 22 shapes of test_gpu_conv_kxk.py through the restatement: six of the nine instantiations, every one at its preferred width.  The
    second configuration, both fall-backs, U = 8 with 64-filter waves and every stand-alone case of more than one tile along x are this
    table's"""
    import test_gpu_conv_kxk as old
    assert len(old.GRID) == 22
    reach, multi_x = set(), 0
    for B, c, n, H, W, k, s, pad, act in old.GRID:
        g = kg.conv_kxk_launch(kg.Trace(), B, H, W, c, n, k, s, pad)
        reach.add((g["inst"], g["tw"], g["choice"]))
        multi_x += g["tiles_x"] > 1
    assert reach == {((4, 1, 1), 8, "pref"), ((4, 1, 1), 16, "pref"), ((4, 2, 1), 8, "pref"), ((4, 2, 1), 16, "pref"), ((4, 2, 1), 32, "pref"),
                     ((8, 1, 1), 16, "pref"), ((16, 1, 1), 8, "pref"), ((16, 1, 1), 16, "pref"),
                     ((16, 2, 1), 8, "pref"), ((16, 2, 1), 16, "pref"), ((16, 2, 1), 32, "pref")}
    assert multi_x == 0
    g = kg.conv_kxk_launch(kg.Trace(), 1, 60, 60, 32, 40, 11, 6, 5)
    assert (g["inst"], g["tw"], kg.LDS_MAX - g["lds"]) == ((16, 2, 1), 16, 112), "the 11 x 11 stride-6 case: the first configuration, under the limit by 112 bytes"
