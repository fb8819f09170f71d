"""The conv launchers' tile geometry, restated clause by clause, and the case table built from it (no GPU needed).

Every specialised convolution kernel sits behind a host launcher that derives its geometry from (B, H, W, c, n, plan): tile size,
rounds of 256 workgroups, one tile per workgroup or a persistent walk, half or whole workgroups, flat runs or 2-D patches, the LDS
row cap, single or double image buffers, the row-image slot width, a grid widened past its cap, or a refusal that hands the shape
to the next kernel.  The functions below say in plain Python what each launcher decides.  Every decision goes through a Trace
under a label, so that tests/test_launch_geometry_cpu.py can demand that the case table reaches both sides of every labelled
clause, and tests/test_gpu_launch_geometry.py can demand that a launch on the device took the family and the (grid, threads, lds)
the restatement names before it compares bytes.

Restated: conv1x1_ws_launch (conv1x1.hip), conv_ws3_launch (conv_ws3.hip), conv_small_pool_launch (conv_small.hip: the 16 / 32
channel form and the 64-channel form), conv_small32_launch (conv_small32.hip), conv_pool16_launch (conv_pool16.hip),
conv_first_mfma_pool_launch / conv_first_mfma_launch with per_image_grid (conv_aux.hip), conv_igemm_launch with conv_rows_launch,
conv_rows16_launch and launch_cfg (conv_igemm.hip, conv_rows.hip, conv_rows16.hip), and the order in which conv_forward_impl
(shim.hip) offers a layer to them.

Three kinds of labels are not reached on both sides by the table, each listed by name with its reason:
  SIZE_GUARDS   need tensors of 2 GiB and more;
  DEAD          cannot be true given the clauses in front of them (the reason gives the arithmetic; the CPU sweep checks it);
  OVER_CAP      reachable only with a device tensor above the table's 64 MB cap (reached by the CPU sweep instead).

Also here: a vectorised exact reference (zero-point-padded windows, one float64 matrix product -- exact, |acc| < 2^53 -- wrapped to
int32 as oracle.conv_acc does, one oracle.requant call on [n, B * OH * OW]) and the two max-pools in numpy: a per-image Python loop
over 65 537 images would take longer than a test may."""
import numpy as np

KB = 1024
LDS_MAX = 160 * KB


def cdiv(a, b):
    return -(-a // b)


def in_cells(B, H, W):
    """cells of a padded PHWC tensor (mi355_tensor_describe: lead 2, one pad row and column per image, tail W + 3)"""
    return 2 + B * (H + 1) * (W + 1) + W + 3


def cell_bytes(C):
    return 4 if C == 3 else cdiv(C, 16) * 16


def tensor_bytes(B, H, W, C):
    return in_cells(B, H, W) * cell_bytes(C)


# ------------------------------------------------------------------------------------------------------------ labels
LABELS = {
    "conv1x1": ("c1.in_bytes_2^32", "c1.gmax32", "c1.gmax16", "c1.mtiles>1", "c1.mtiles4", "c1.rounds>1", "c1.tp<16", "c1.plan1_round32",
                "c1.plan1_grow", "c1.grow_loop_ran", "c1.n_ragged", "c1.sets>1", "c1.lds_limit_160", "c1.lds_refused"),
    "conv_ws3": ("w3.plan_one_round", "w3.pool_cells_24bit", "w3.s2_odd_map", "w3.kp2", "w3.mtiles>1", "w3.pm1", "w3.pm1_hw<64",
                 "w3.pm1_hw>256", "w3.pm1_B*mtiles<128", "w3.pm1_plan_fits", "w3.units<64", "w3.tp1<=256", "w3.tp1_plan_fits",
                 "w3.pool_not_one_tile", "w3.row_image_better", "w3.db_tried", "w3.in_bytes_2^32", "w3.db_even_ok", "w3.db_rows_ok",
                 "w3.sb_even_ok", "w3.sb_rows_ok", "w3.alias", "w3.persistent"),
    "conv_small": ("sm.odd_map", "sm.in_bytes_2^32", "sm.total_p_2^31", "sm.wide", "sm.odd_OW", "sm.cells<64", "sm.cells>kmax",
                   "sm.lds>160K", "sm.per_cu2", "sm.per_cu3", "sm.persistent"),
    "conv_mid": ("m64.odd_map", "m64.in_bytes_2^32", "m64.total_p_2^31", "m64.wide", "m64.odd_OW", "m64.rounds>1", "m64.tp<32", "m64.plan1",
                 "m64.plan1_tp>128", "m64.want_half", "m64.half_lds_fits", "m64.half_cells>=64", "m64.cells<64", "m64.lds>160K"),
    "conv_small32": ("s32.odd_map", "s32.in_bytes_2^32", "s32.total_p_2^31", "s32.wide", "s32.odd_OW", "s32.cells<64", "s32.cells>kdma",
                     "s32.2lds>160K", "s32.persistent"),
    "conv_pool16": ("p16.odd_map", "p16.in_bytes_2^31", "p16.pool_bytes_2^32", "p16.tx_ty_10bit", "p16.ntiles_2^31", "p16.ntiles<cap",
                    "p16.need_widens", "p16.ragged_tx", "p16.ragged_ty"),
    "conv_first": ("l0.pool", "l0.odd_map", "l0.in_cells_2^31", "l0.pool_bytes_2^32", "l0.ntiles_2^31", "l0.tx_ty_10bit", "l0.ntiles<cap",
                   "l0.need_widens", "l0.per_image", "l0.pi_raise_64", "l0.pi_clamp_tpi", "l0.grid_2^31"),
    "conv_igemm": ("ig.rows_path", "ig.thr_128_only", "ig.best384", "ig.best256", "ig.best128", "ig.nt>nt0", "ig.sub0_reset", "ig.retry128",
                   "ig.rows_refused", "ig.patch", "ig.tiles<200", "ig.cb64_or_s2", "ig.staging_fallback",
                   "rows.k1", "rows16.need<=16", "rows16.bm32", "rows16.narrow384", "rows.need<=16", "rows.need<=32", "rows.need<=64",
                   "rows.ntiles_raised", "rows.too_narrow", "rows.in_bytes_2^32", "rows.epi_lds_larger", "rows.lds>160K",
                   "cfg.bpt_budget", "cfg.epi_lds_larger", "cfg.lds>160K"),
}
ALL_LABELS = {l: k for k, ls in LABELS.items() for l in ls}

# labels whose TRUE side needs tensors of 2 GiB and more: the only ones the table may leave unreached for their size
SIZE_GUARDS = {
    "c1.in_bytes_2^32": "in_cells * in_cs >= 2^32: a 4 GiB input",
    "w3.in_bytes_2^32": "in_cells * in_cs >= 2^32: a 4 GiB input",
    "sm.in_bytes_2^32": "in_cells * in_cs >= 2^32: a 4 GiB input",
    "m64.in_bytes_2^32": "in_cells * in_cs >= 2^32: a 4 GiB input",
    "s32.in_bytes_2^32": "in_cells * in_cs >= 2^32: a 4 GiB input",
    "rows.in_bytes_2^32": "in_cells * in_cs >= 2^32: a 4 GiB input",
    "p16.in_bytes_2^31": "in_cells * in_cs >= 2^31: a 2 GiB input",
    "l0.in_cells_2^31": "in_cells + 64 (W + 1) >= 2^31: an 8 GiB input (or a 2 GiB row)",
    "w3.pool_cells_24bit": "the 24-bit pooled-cell guard: 2^24 pooled cells of 64 bytes and more are 1 GiB, of an input four times that",
    "p16.pool_bytes_2^32": "the pooled tensor's 32-bit byte offsets: a 4 GiB pooled tensor (the pooled-cell guard of this kernel)",
    "l0.pool_bytes_2^32": "the pooled tensor's 32-bit byte offsets: a 4 GiB pooled tensor (the pooled-cell guard of this kernel)",
    "sm.total_p_2^31": "total_p + 256 >= 2^31: 2^31 pooled pixels of 16 channels are 128 GiB",
    "m64.total_p_2^31": "total_p + 256 >= 2^31",
    "s32.total_p_2^31": "total_p + 256 >= 2^31",
    "p16.ntiles_2^31": "grid > 2^31: 2^31 tiles of at least 2 x 2 x 16 bytes",
    "l0.ntiles_2^31": "grid > 2^31: 2^31 tiles",
    "l0.grid_2^31": "grid > 2^31: 2^31 workgroups",
}
# label -> (the side that cannot happen, why).  test_launch_geometry_cpu.py checks that neither the table nor the sweep reaches it.
DEAD = {
    "sm.cells<64": (True, "flat: rows_cap >= 2 * ((126 + OW) / OW + 1) + 3 and pitch >= 2 OW + 2; a pitch <= 9 needs OW <= 3, then rows_cap >= 87"),
    "sm.lds>160K": (True, "after cells <= 4 * SM_KMAX * 64 = 1536: lds <= (2 * 2 * 16 + 4) * 1536 + 2048 = 106 496"),
    "m64.cells<64": (True, "rows_cap >= 2 * ((30 + OW) / OW + 1) + 3 and pitch >= 2 OW + 2: OW <= 3 gives rows_cap >= 27, wide maps 18 * 40"),
    "m64.half_cells>=64": (False, "as m64.cells<64: the cell count never falls below 64"),
    "s32.cells<64": (True, "as sm.cells<64 (the same flat geometry)"),
    "s32.odd_map": (True, "mi355_conv_pool_forward refuses a 2x2 / stride-2 pool on an odd map before any launcher; this kernel has no form without a pool"),
    "p16.odd_map": (True, "as s32.odd_map (for both the reason is the C ABI's own check, which these tests do not probe: the sweeps feed even maps only)"),
    "rows.epi_lds_larger": (True, "the epilogue tile is bn * (bm + 8) bytes; the K-loop buffers hold ra * bm * 64 + rb * rows_cap * rowb with rows_cap >= (bn - 2) / 62 + 2 rows of "
                                  "at least 1 KiB: more for every (bm, bn) the launchers pick"),
    "cfg.epi_lds_larger": (True, "3 * bm * 64 + 2 KiB per staged chunk against bn * (bm + 8): a patch or a flat run of bn pixels stages more than bn cells"),
}
# label -> (side the table cannot reach under its 64 MB cap, why).  The CPU sweep reaches it.
OVER_CAP = {
    "w3.pm1_plan_fits": (False, "the stride-1 pool's whole-image tile misses LDS only with 256 input channels, hw >= 161 and B * n >= 128 * 128: 6.08e9 "
                                "multiply-adds, over the table's 6e9"),
    "l0.pi_raise_64": (True, "per-image grid below ceil(tpi / 64): the pooled form widens its shared grid to ntiles / 64 first, so there "
                             "ceil(g / B) >= ceil(tpi / 64) always; the form without a pool needs B * tpi > 65 536 with tpi >= 65, and its "
                             "16-byte output cells alone are then 100 MB (B = 1024, 2 x 2050 maps)"),
}


class Trace:
    """records which side of which labelled clause a restatement took"""

    def __init__(self):
        self.hits = {}

    def __call__(self, label, cond):
        assert label in ALL_LABELS, label
        cond = bool(cond)
        self.hits.setdefault(label, set()).add(cond)
        return cond

    def merge(self, other):
        for k, v in other.hits.items():
            self.hits.setdefault(k, set()).update(v)


def _refuse(family, why, **kw):
    return dict(kernel=None, family=family, refused=why, grid=None, threads=None, lds=None, **kw)


def _ok(family, kernel, grid, threads, lds, **kw):
    return dict(kernel=kernel, family=family, refused=None, grid=int(grid), threads=int(threads), lds=int(lds), **kw)


# ------------------------------------------------------------------------------------------------------------ conv1x1.hip
def conv1x1_eligible(n, c, k):
    return k == 1 and c in (64, 128, 256, 512, 1024) and n >= 1 and (n <= 256 or (n <= 1024 and n % 256 == 0))


def conv1x1(tr, B, H, W, c, n, plan, single_tile_only=False):
    """conv1x1_ws_launch.  single_tile_only: a head or a fused upsample (one filter tile only)"""
    assert conv1x1_eligible(n, c, 1)
    if tr("c1.in_bytes_2^32", in_cells(B, H, W) * c >= 2 ** 32):
        return _refuse("conv1x1", "in_bytes")
    total = B * H * W
    gmax = 32 if tr("c1.gmax32", c <= 64) else (16 if tr("c1.gmax16", c == 128) else 8)
    n32 = (n + 31) & ~31
    mtiles = cdiv(n32, 256) if tr("c1.mtiles>1", n32 > 256) else 1
    tr("c1.mtiles4", mtiles == 4)
    want = 256 // mtiles
    rounds = cdiv(total, want * gmax * 32)
    tr("c1.rounds>1", rounds > 1)
    tp = cdiv(total, want * rounds)
    if tr("c1.tp<16", tp < 16):
        tp = 16
    if tr("c1.plan1_round32", plan == 1):
        tp = (tp + 31) & ~31
    if tr("c1.plan1_grow", plan == 1 and rounds == 1):
        abytes = min(n32, 256) * c
        tp0 = tp
        while abytes > 2 * tp * c and (c // 64) * 2 * ((tp + 32) // 32) * 1024 <= 128 * KB:
            tp += 32
        tr("c1.grow_loop_ran", tp > tp0)
    ntiles = cdiv(total, tp)
    G = cdiv(tp, 32)
    ncell = 2 * G
    lds = (c // 64) * ncell * 1024
    nfw = min(n32, 256)
    lds += nfw * 16 + 1024 + ncell * 16 * 16
    one = tr("c1.lds_limit_160", rounds == 1 and ntiles * mtiles <= 256)
    if tr("c1.lds_refused", lds > (160 if one else 96) * KB):
        return _refuse("conv1x1", "lds", tp=tp, rounds=rounds, mtiles=mtiles)
    assert not (mtiles > 1 and single_tile_only)
    tr("c1.n_ragged", n % 32 != 0)
    nq = nfw // 32  # 1..8, so 8 / nq >= 1 always (the launcher's `> 0 ? : 1` never takes its second arm)
    sets = 8 // nq
    tr("c1.sets>1", sets > 1)
    return _ok("conv1x1", 3, ntiles * mtiles, sets * nq * 64, lds, tp=tp, rounds=rounds, mtiles=mtiles, ntiles=ntiles, gmax=gmax)


# ------------------------------------------------------------------------------------------------------------ conv_ws3.hip
WS3_GMAX = 8


def ws3_quads(n, c):
    return min(n // 32, 8 // (c // 128))


def ws3_eligible(n, c, k):
    if k != 3 or c not in (128, 256) or n % 32:
        return False
    nq = ws3_quads(n, c)
    return nq & (nq - 1) == 0 and (n // 32) % nq == 0


def row_slots(W):
    return 16 if W + 2 <= 16 else (32 if W + 2 <= 32 else 64)


def default_bm(n):
    return 128 if n >= 128 else (64 if n > 32 else 32)


def mpad_of(n):
    bm = default_bm(n)
    return cdiv(n, bm) * bm


def plan_one_round(plan, n, total_n, W):
    return plan == 1 and cdiv(mpad_of(n), 128) * cdiv(total_n, 384) <= 256 and 10 * (W + 2) >= 7 * row_slots(W)


def conv_ws3(tr, B, H, W, c, n, stride, pm, plan, flags=0):
    """conv_ws3_launch.  pm: 0 no pool, 1 the fused 2x2 / stride-1 pool, 2 the fused 2x2 / stride-2 pool"""
    assert ws3_eligible(n, c, 3) and stride in (1, 2) and (not pm or stride == 1)
    S = stride
    OH, OW = (H + 2 - 3) // S + 1, (W + 2 - 3) // S + 1
    total_n = B * OH * OW
    if tr("w3.plan_one_round", plan_one_round(plan, n, total_n, W) and not flags & (1 << 27)):
        return _refuse("conv_ws3", "plan_one_round")
    if pm:
        assert pm == 1 or not ((OH | OW) & 1)  # (the C ABI refuses a stride-2 pool on an odd map before any launcher)
        d = 2 if pm == 2 else 1
        pcells = 2 + B * (OH // d + 1) * (OW // d + 1)
        pool_cs = cell_bytes(n)
        if tr("w3.pool_cells_24bit", pcells >= 1 << 24 or pool_cs >= 1 << 24 or pcells * pool_cs >= 1 << 32):
            return _refuse("conv_ws3", "pool_cells")
    if tr("w3.s2_odd_map", S == 2 and ((H & 1) or (W & 1))):
        return _refuse("conv_ws3", "s2_odd_map")
    kp = 2 if tr("w3.kp2", c == 256) else 1
    nq, pieces = ws3_quads(n, c), 8 * kp
    mtiles, nset = n // (32 * nq), 8 // (nq * kp)
    tr("w3.mtiles>1", mtiles > 1)
    hw = OH * OW
    OWp, ohwp = OW // 2, (OH // 2) * (OW // 2)
    total = B * ohwp if pm == 2 else total_n
    upx = 4 if pm == 2 else 1
    want = max(256 // mtiles, 1)

    def plan_tiles(tp, db=False):
        ntiles = cdiv(total, tp)
        G = cdiv(tp * upx, 32)
        t = np.arange(ntiles, dtype=np.int64)
        p0 = t * tp
        p1 = np.minimum(p0 + tp, total) - 1
        if pm == 2:
            b0 = p0 // ohwp; r0 = 2 * ((p0 - b0 * ohwp) // OWp)
            b1 = p1 // ohwp; r1 = 2 * ((p1 - b1 * ohwp) // OWp) + 1
        else:
            b0 = p0 // hw; r0 = (p0 - b0 * hw) // OW
            b1 = p1 // hw; r1 = (p1 - b1 * hw) // OW
        rows_cap = int((b1 * (H + 1) + S * r1 - b0 * (H + 1) - S * r0 + 3).max())
        alias = S == 1 and pm != 2 and tp == hw and total % hw == 0 and rows_cap == H + 2
        if alias:
            rows_cap = H + 1
        cells = rows_cap * (W + 2)
        lds = cells * (pieces + 1) * 16
        if db:
            lds = 2 * ((lds + 1023) & ~1023)
        lds += ((cells + 3) & ~3) * 4 + G * 32 * 12 + (G * 8 * 4 if pm == 2 else 0)
        lds = (lds + 15) & ~15
        lds += 32 * nq * 16
        if kp == 2:
            lds += nq * nset * cdiv(G, nset) * 4096
        if pm and kp == 1:
            lds += nq * nset * cdiv(G, nset) * (32 * 36 + 128)
        if lds > LDS_MAX:
            return None
        return dict(tp=tp, ntiles=ntiles, rows_cap=rows_cap, alias=alias, db=db, lds=lds)

    tp1 = cdiv(total, want)
    if tr("w3.pm1", pm == 1):
        if tr("w3.pm1_hw<64", hw < 64):
            return _refuse("conv_ws3", "pm1_hw<64")
        if tr("w3.pm1_hw>256", hw > WS3_GMAX * 32):
            return _refuse("conv_ws3", "pm1_hw>256")
        if tr("w3.pm1_B*mtiles<128", B * mtiles < 128):
            return _refuse("conv_ws3", "pm1_B*mtiles<128")
        p = plan_tiles(hw)
        if not tr("w3.pm1_plan_fits", p is not None):
            return _refuse("conv_ws3", "pm1_lds")
        nwg = min(p["ntiles"], want)
    elif tr("w3.units<64", tp1 * upx < 64):
        return _refuse("conv_ws3", "units<64")
    else:
        p = None
        if tr("w3.tp1<=256", tp1 * upx <= WS3_GMAX * 32):
            p = plan_tiles(tp1)
            tr("w3.tp1_plan_fits", p is not None)
        if p is not None:
            nwg = p["ntiles"]
        elif tr("w3.pool_not_one_tile", pm):
            return _refuse("conv_ws3", "pool_not_one_tile")
        else:
            if tr("w3.row_image_better", S == 1 and W <= 62 and (W + 2) >= 0.7 * row_slots(W)):
                return _refuse("conv_ws3", "row_image_better")
            if tr("w3.db_tried", kp == 1 and not flags & (1 << 29)) and not tr("w3.in_bytes_2^32", in_cells(B, H, W) * c >= 2 ** 32):
                for tpm in range(WS3_GMAX * 32, 95, -32):
                    per = cdiv(total, want * tpm)
                    tp = cdiv(total, per * want)
                    if tp >= 64 and per >= 2:
                        p = plan_tiles(tp, True)
                    if p:
                        break
                if not tr("w3.db_even_ok", p is not None):
                    for k in range((WS3_GMAX * 32) // OW, 0, -1):
                        if OH % k == 0 and k * OW >= 64 and B * (OH // k) >= 2 * want:
                            p = plan_tiles(k * OW, True)
                        if p:
                            break
                    tr("w3.db_rows_ok", p is not None)
            if p is None:
                for tpm in range(WS3_GMAX * 32, 63, -32):
                    per = cdiv(total, want * tpm)
                    tp = cdiv(total, per * want)
                    if tp >= 48:
                        p = plan_tiles(tp)
                    if p:
                        break
                if not tr("w3.sb_even_ok", p is not None):
                    for k in range((WS3_GMAX * 32) // OW, 0, -1):
                        if OH % k == 0 and k * OW >= 32:
                            p = plan_tiles(k * OW)
                        if p:
                            break
                    if not tr("w3.sb_rows_ok", p is not None):
                        return _refuse("conv_ws3", "no_plan_fits")
            nwg = min(p["ntiles"], want)
    tr("w3.alias", p["alias"])
    tr("w3.persistent", p["ntiles"] > nwg)
    return _ok("conv_ws3", 4, mtiles * nwg, 512, p["lds"], mtiles=mtiles, nwg=nwg, total=total, upx=upx, pm=pm, S=S, **{k: v for k, v in p.items() if k != "lds"})


# ------------------------------------------------------------------------------------------------------------ conv_small.hip
SM_PPB, SM_GMAX, SM_KMAX = 128, 8, 6


def conv_small_eligible(n, c, k):
    if k != 3:
        return False
    if c == 64:
        return n % 32 == 0 and 64 <= n <= 128
    return c in (16, 32) and n in (32, 64)


def _flat_rows_cap(tp, OH, OW):
    """rows of a run of tp pooled pixels: pooled rows it can touch, two image rows each, one pad row per image boundary crossed, one halo row
    above and below"""
    return 2 * ((tp - 2 + OW) // OW + 1) + (tp - 2 + OH * OW) // (OH * OW) + 2


def _flat_pitch(W, OW, odd):
    lcell = W + 2
    return lcell + (0 if odd else (OW // 2 - lcell) % 8)


def conv_small(tr, B, H, W, c, n, plan, flags=0):
    """conv_small_pool_launch, 16 / 32 input channels: persistent four-wave workgroups over 128-pooled-pixel tiles.  The same geometry serves
    the pooled, the stride-1 and the stride-2 form (OH, OW: the 2 x 2 blocks of the input map).  `grid` is what LDS allows; the launch may
    clamp it further to 256 x (workgroups per CU the kernel's registers allow), which only the code object knows: per_cu says how far."""
    assert conv_small_eligible(n, c, 3) and c in (16, 32)
    if tr("sm.odd_map", (H & 1) or (W & 1)):
        return _refuse("conv_small", "odd_map")
    if tr("sm.in_bytes_2^32", in_cells(B, H, W) * c >= 2 ** 32):
        return _refuse("conv_small", "in_bytes")
    OH, OW = H // 2, W // 2
    total_p = B * OH * OW
    if tr("sm.total_p_2^31", total_p + 256 >= 1 << 31):
        return _refuse("conv_small", "total_p")
    if tr("sm.wide", OW >= 64):
        tx, ty = cdiv(OW, 16), cdiv(OH, 8)
        ncell, rows_cap, ntiles = 40, 18, B * tx * ty
    else:
        tx = ty = 0
        ncell = _flat_pitch(W, OW, tr("sm.odd_OW", OW & 1))
        rows_cap = _flat_rows_cap(SM_PPB, OH, OW)
        ntiles = cdiv(total_p, SM_PPB)
    cells = rows_cap * ncell
    if tr("sm.cells<64", cells < 64) or tr("sm.cells>kmax", cells > 4 * SM_KMAX * 64):
        return _refuse("conv_small", "cells", rows_cap=rows_cap, ncell=ncell)
    lds = 2 * (c // 16) * cells * 16 + cells * 4
    lds = (lds + 15) & ~15
    lds += n * 32
    if tr("sm.lds>160K", lds > LDS_MAX):
        return _refuse("conv_small", "lds")
    per_cu = 2 if tr("sm.per_cu2", 2 * lds <= LDS_MAX) else 1
    if tr("sm.per_cu3", c == 16 and n == 32 and 3 * lds <= LDS_MAX):
        per_cu = 3
    grid = min(ntiles, 256 * per_cu)
    tr("sm.persistent", ntiles > grid)
    return _ok("conv_small", 2, grid, 256, lds, per_cu=per_cu, ntiles=ntiles, rows_cap=rows_cap, ncell=ncell, tp=SM_PPB, tiles_x=tx, tiles_y=ty,
               OH=OH, OW=OW, total=total_p)


def conv_mid(tr, B, H, W, n, plan, flags=0):
    """conv_small_pool_launch, 64 input channels: one single-buffered tile per workgroup, n / 32 waves x (half: 1, whole: 2) sets"""
    assert conv_small_eligible(n, 64, 3)
    if tr("m64.odd_map", (H & 1) or (W & 1)):
        return _refuse("conv_mid", "odd_map")
    if tr("m64.in_bytes_2^32", in_cells(B, H, W) * 64 >= 2 ** 32):
        return _refuse("conv_mid", "in_bytes")
    OH, OW = H // 2, W // 2
    total_p = B * OH * OW
    if tr("m64.total_p_2^31", total_p + 256 >= 1 << 31):
        return _refuse("conv_mid", "total_p")
    rounds = 1
    if tr("m64.wide", OW >= 64):
        tx, ty = cdiv(OW, 16), cdiv(OH, 8)
        lcell, ncell, rows_cap, ntiles, tp = 34, 40, 18, B * tx * ty, SM_PPB
    else:
        tx = ty = 0
        lcell = W + 2
        ncell = _flat_pitch(W, OW, tr("m64.odd_OW", OW & 1))
        rounds = cdiv(total_p, 256 * SM_GMAX * 32)
        tr("m64.rounds>1", rounds > 1)
        tp = cdiv(total_p, 256 * rounds)
        if tr("m64.tp<32", tp < 32):
            tp = 32
        if tr("m64.plan1", plan == 1):
            if tr("m64.plan1_tp>128", tp > 128):
                tp = 128
            else:
                tp = (tp // 32) * 32
        rows_cap = _flat_rows_cap(tp, OH, OW)
        ntiles = cdiv(total_p, tp)
    gt = cdiv(tp, 32)

    def lds_need(ncell):
        l = 4 * rows_cap * ncell * 16 + ((rows_cap * ncell + 1) & ~1) * 4 + gt * 128 * 8 + gt * 32 * 8
        return ((l + 15) & ~15) + n * 32

    half = False
    if tr("m64.want_half", plan == 1 or ntiles > 256):
        nc = lcell if tx == 0 else ncell  # flat tiles: the unpadded pitch
        half = tr("m64.half_lds_fits", 2 * lds_need(nc) <= LDS_MAX) and tr("m64.half_cells>=64", rows_cap * nc >= 64)
        if half:
            ncell = nc
    if tr("m64.cells<64", rows_cap * ncell < 64):
        return _refuse("conv_mid", "cells")
    lds = lds_need(ncell)
    if tr("m64.lds>160K", lds > LDS_MAX):
        return _refuse("conv_mid", "lds", tp=tp, rows_cap=rows_cap, ncell=ncell)
    return _ok("conv_mid", 2, ntiles, (1 if half else 2) * (n // 32) * 64, lds, tp=tp, half=half, ntiles=ntiles, rounds=rounds, rows_cap=rows_cap,
               ncell=ncell, tiles_x=tx, tiles_y=ty, OH=OH, OW=OW, total=total_p)


# ------------------------------------------------------------------------------------------------------------ conv_small32.hip
S32_PPB, S32_KDMA = 128, 3


def conv_small32(tr, B, H, W, flags=0):
    """conv_small32_launch: 32 -> 64 + maxpool on eight-wave workgroups, two per CU (debug bit 4096 selects it)"""
    c, n = 32, 64
    if tr("s32.odd_map", (H & 1) or (W & 1)):
        return _refuse("conv_small32", "odd_map")
    if tr("s32.in_bytes_2^32", in_cells(B, H, W) * c >= 2 ** 32):
        return _refuse("conv_small32", "in_bytes")
    OH, OW = H // 2, W // 2
    total_p = B * OH * OW
    if tr("s32.total_p_2^31", total_p + 256 >= 1 << 31):
        return _refuse("conv_small32", "total_p")
    if tr("s32.wide", OW >= 64):
        tx, ty = cdiv(OW, 16), cdiv(OH, 8)
        ncell, rows_cap, ntiles = 40, 18, B * tx * ty
    else:
        tx = ty = 0
        ncell = _flat_pitch(W, OW, tr("s32.odd_OW", OW & 1))
        rows_cap = _flat_rows_cap(S32_PPB, OH, OW)
        ntiles = cdiv(total_p, S32_PPB)
    cells = rows_cap * ncell
    if tr("s32.cells<64", cells < 64) or tr("s32.cells>kdma", cells > 8 * S32_KDMA * 64):
        return _refuse("conv_small32", "cells")
    lds = 2 * (c // 16) * cells * 16 + cells * 4
    lds = ((lds + 15) & ~15) + n * 32
    if tr("s32.2lds>160K", 2 * lds > LDS_MAX):
        return _refuse("conv_small32", "lds")
    grid = min(ntiles, 512)
    tr("s32.persistent", ntiles > grid)
    return _ok("conv_small32", 8, grid, 512, lds, ntiles=ntiles, rows_cap=rows_cap, ncell=ncell, tp=S32_PPB, tiles_x=tx, tiles_y=ty, OH=OH, OW=OW,
               total=total_p)


# ------------------------------------------------------------------------------------------------------------ conv_pool16.hip
def _widened(ntiles, cap):
    """persistent grid: the cap, never more workgroups than tiles, never more than 64 tiles per workgroup whichever eighth of the tiles an XCD
    takes ((grid / 8) * 64 >= ceil(ntiles / 8))"""
    return min(ntiles, cap), cdiv(cdiv(ntiles, 8), 64) * 8


def conv_pool16(tr, B, H, W, flags=0):
    """conv_pool16_launch: 16 -> 32 + maxpool on 8 x 16 pooled patches (needs the blob's epilogue table)"""
    c, n = 16, 32
    if tr("p16.odd_map", (H & 1) or (W & 1)):
        return _refuse("conv_pool16", "odd_map")
    if tr("p16.in_bytes_2^31", in_cells(B, H, W) * c >= 1 << 31):
        return _refuse("conv_pool16", "in_bytes")
    OH, OW = H // 2, W // 2
    if tr("p16.pool_bytes_2^32", (2 + B * (OH + 1) * (OW + 1) + OW + 2) * cell_bytes(n) >= 1 << 32):
        return _refuse("conv_pool16", "pool_bytes")
    tx, ty = cdiv(OW, 16), cdiv(OH, 8)
    if tr("p16.tx_ty_10bit", tx > 1023 or ty > 1023):
        return _refuse("conv_pool16", "tx_ty")
    ntiles = B * tx * ty
    if tr("p16.ntiles_2^31", ntiles >= 1 << 31):
        return _refuse("conv_pool16", "ntiles")
    tr("p16.ragged_tx", OW % 16 != 0)
    tr("p16.ragged_ty", OH % 8 != 0)
    tr("p16.ntiles<cap", ntiles < 768)
    g, need = _widened(ntiles, 768)
    if tr("p16.need_widens", g < need):
        g = need
    return _ok("conv_pool16", 7, g, 256, 0, ntiles=ntiles, tiles_x=tx, tiles_y=ty, OH=OH, OW=OW)


# ------------------------------------------------------------------------------------------------------------ conv_aux.hip (first layer)
def conv_first(tr, B, H, W, n, pool, per_image=False, planar=False):
    """conv_first_mfma_pool_launch (pool) / conv_first_mfma_launch: 3 -> 16 | 32 on the matrix pipe, 8 x 16 patches of 2 x 2 blocks"""
    assert n in (16, 32)
    tr("l0.pool", pool)
    if tr("l0.odd_map", (H & 1) or (W & 1)):
        return _refuse("conv_first", "odd_map")
    assert not planar or W % 4 == 0
    if tr("l0.in_cells_2^31", (0 if planar else in_cells(B, H, W)) + 64 * (W + 1) >= 1 << 31):
        return _refuse("conv_first", "in_cells")
    OH, OW = H // 2, W // 2
    tx, ty = cdiv(OW, 16), cdiv(OH, 8)
    if pool:
        if tr("l0.pool_bytes_2^32", (2 + B * (OH + 1) * (OW + 1) + OW + 2) * cell_bytes(n) >= 1 << 32):
            return _refuse("conv_first", "pool_bytes")
        assert not planar or B * 3 * H * W < 1 << 31
    ntiles = B * tx * ty
    if tr("l0.ntiles_2^31", ntiles >= 1 << 31):
        return _refuse("conv_first", "ntiles")
    if pool and tr("l0.tx_ty_10bit", tx > 1023 or ty > 1023):
        return _refuse("conv_first", "tx_ty")
    tr("l0.ntiles<cap", ntiles < 1024)
    g = min(ntiles, 1024)
    if pool:
        need = _widened(ntiles, 1024)[1]
        if tr("l0.need_widens", g < need):
            g = need
    wpi = 0
    if tr("l0.per_image", per_image):
        tpi = ntiles // B
        wpi = cdiv(g, B)
        if tr("l0.pi_raise_64", wpi < cdiv(tpi, 64)):
            wpi = cdiv(tpi, 64)
        if tr("l0.pi_clamp_tpi", wpi > tpi):
            wpi = tpi
        g = wpi * B
    if tr("l0.grid_2^31", g >= 1 << 31):
        return _refuse("conv_first", "grid")
    return _ok("conv_first", 1, g, 256, 0, ntiles=ntiles, tiles_x=tx, tiles_y=ty, wpi=wpi, pool=pool, OH=OH, OW=OW, B=B)


# ------------------------------------------------------------------------------------------------------------ conv_igemm.hip / conv_rows*.hip
ROWS_WAVES = {(128, 384): 8, (128, 256): 8, (128, 192): 4, (128, 128): 4, (64, 256): 4, (64, 128): 4, (32, 256): 4, (32, 128): 4}


def _nb_slots(BN, RS, DW, KS):
    wmin, halo = RS * 3 // 4, 1 if KS == 3 else 0
    rows = (BN - 2 + wmin) // wmin + 1 + (BN - 2 + wmin * wmin) // (wmin * wmin) + 2 * halo
    return cdiv(rows * (RS // 16), DW)


def _ra_stages(KS, BN):
    return (4 if BN <= 192 else 6) if KS == 3 else (4 if BN <= 128 else 3)


def _rows_cfg(tr, B, H, W, c, n, k, bm, bn, RS, ntiles_n, exact_rows, nbx=0):
    """rows_launch_cfg (conv_rows.hip: the row cap of ANY bn pixels) / rows16_launch_cfg (conv_rows16.hip: the most a tile of this plan spans)"""
    NW = ROWS_WAVES[(bm, bn)]
    DW = 4 if NW == 8 and k == 3 else NW
    halo = 1 if k == 3 else 0
    total_n = B * H * W
    if tr("rows.ntiles_raised", ntiles_n < cdiv(total_n, bn)):
        ntiles_n = cdiv(total_n, bn)
    q, r = divmod(total_n, ntiles_n)
    if exact_rows:
        hw = H * W
        t = np.arange(ntiles_n, dtype=np.int64)
        n0 = t * q + np.minimum(t, r)
        n1 = n0 + q + (t < r) - 1
        ok = n1 >= n0

        def grow(p):
            b = p // hw
            return b * (H + 1) + (p - b * hw) // W + 1
        rows_cap = int((grow(n1[ok]) - grow(n0[ok]) + 1).max()) + 2 * halo
    else:
        rows_cap = (bn - 2 + W) // W + 1 + (bn - 2 + H * W) // (H * W) + 2 * halo
    if tr("rows.too_narrow", cdiv(rows_cap * (RS // 16), DW) > _nb_slots(bn, RS, DW, k) + nbx):
        return _refuse("conv_rows", "too_narrow", bn=bn)
    if tr("rows.in_bytes_2^32", in_cells(B, H, W) * c >= 2 ** 32):
        return _refuse("conv_rows", "in_bytes")
    rowb = RS * 64 + 16 * (W & 15)
    ra = _ra_stages(k, bn)
    rb = 2 if k == 3 else ra
    lds = ra * bm * 64 + rb * rows_cap * rowb + rows_cap * RS * 4
    lds_epi = bn * (bm + 4) + bn * 4
    if tr("rows.epi_lds_larger", lds_epi > lds):
        lds = lds_epi
    lds = ((lds + 15) & ~15) + bm * 32
    if tr("rows.lds>160K", lds > LDS_MAX):
        return _refuse("conv_rows", "lds", bn=bn)
    mtiles = mpad_of(n) // bm
    return _ok("conv_rows", 5, ntiles_n * mtiles, 64 * NW, lds, bm=bm, bn=bn, RS=RS, ntiles=ntiles_n, rows_cap=rows_cap, tile_q=q, tile_r=r,
               mtiles=mtiles, rows16=exact_rows, total=total_n, halo=halo)


def _conv_rows(tr, B, H, W, c, n, k, bm, bn, ntiles_n):
    """conv_rows_launch: the 16 x 16 x 64 kernel where it is the measured choice, else the 32 x 32 x 32 one on 16 / 32 / 64-slot rows"""
    need = W + 2
    if not tr("rows.k1", k == 1):
        g = None
        if tr("rows16.need<=16", need <= 16):
            if not tr("rows16.bm32", bm == 32):
                g = _rows_cfg(tr, B, H, W, c, n, k, bm, bn, 16, ntiles_n, True)
        elif tr("rows16.narrow384", need < 24 and bm == 128 and bn == 384):
            g = _rows_cfg(tr, B, H, W, c, n, k, bm, bn, 32, ntiles_n, True, nbx=4)
        if g is not None and not g["refused"]:
            return g
    if tr("rows.need<=16", need <= 16):
        return _rows_cfg(tr, B, H, W, c, n, k, bm, bn, 16, ntiles_n, False)
    if tr("rows.need<=32", need <= 32):
        return _rows_cfg(tr, B, H, W, c, n, k, bm, bn, 32, ntiles_n, False)
    if tr("rows.need<=64", need <= 64):
        return _rows_cfg(tr, B, H, W, c, n, k, bm, bn, 64, ntiles_n, False)
    return _refuse("conv_rows", "W>62")


def _launch_cfg(tr, B, H, W, OH, OW, c, n, k, stride, bm, bn, patch):
    """launch_cfg (conv_igemm.hip): the implicit-GEMM kernel on 2-D patches or flat runs"""
    cb = 64 if c % 64 == 0 else (32 if c % 32 == 0 else 16)
    NW = 8 if (bm, bn) == (128, 256) else 4
    cpc = 1024 // cb
    if patch:
        TH, TW = bn // 16, 16
        ntiles = B * cdiv(OW, TW) * cdiv(OH, TH)
        ncell = ((TH - 1) * stride + 3) * ((TW - 1) * stride + 3)
    else:
        assert stride == 1
        ntiles = cdiv(B * OH * OW, bn)
        halo = W + 2 if k == 3 else 0
        ncell = bn + (bn + W - 1) // W + 1 + ((bn + H * W - 1) // (H * W) + 1) * (W + 1) + 2 * halo
    bchunks = cdiv(ncell, cpc)
    bpt = cdiv(bchunks, NW)
    if tr("cfg.bpt_budget", bpt > 12 or cdiv(bm // 16, NW) + bpt > 20):
        return _refuse("conv_igemm", "bpt")
    lds = 3 * bm * 64 + 2 * (bchunks << 10)
    lds_epi = bn * (bm + 4) + bn * 4
    if tr("cfg.epi_lds_larger", lds_epi > lds):
        lds = lds_epi
    if tr("cfg.lds>160K", lds > LDS_MAX):
        return _refuse("conv_igemm", "lds")
    return _ok("conv_igemm", 5, ntiles * (mpad_of(n) // bm), 64 * NW, lds, bm=bm, bn=bn, patch=patch, ntiles=ntiles)


def conv_igemm(tr, B, H, W, c, n, k, stride, pool, plan):
    """conv_igemm_launch: the row-image kernel under its cost model where it applies, else the implicit-GEMM kernel"""
    cb = 64 if c % 64 == 0 else (32 if c % 32 == 0 else 16)
    ksteps = (c // cb) * cdiv(k * k * (cb // 16), 4)
    bm = default_bm(n)
    pad = k // 2
    OH, OW = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    total_n = B * OH * OW
    if tr("ig.rows_path", cb == 64 and not pool and stride == 1):
        mt = cdiv(mpad_of(n), bm)
        thr = tr("ig.thr_128_only", plan_one_round(plan, n, total_n, W) and k == 3)
        best, pick = 1e30, None
        for cbn in ((128,) if thr else (384, 256, 128)):
            if cbn == 384 and bm != 128:
                continue
            nt0 = cdiv(total_n, cbn)
            blocks0 = mt * nt0
            slots = 512 if cbn == 128 and blocks0 > 256 else 256
            rounds = cdiv(blocks0, slots)
            nt = max((rounds * slots) // mt, nt0)
            waves_n = 2 if cbn == 128 and bm == 128 else 4
            px = cdiv(total_n, nt)
            sub = cdiv(cdiv(px, 32), waves_n)
            px0 = cdiv(total_n, nt0)
            sub0 = cdiv(cdiv(px0, 32), waves_n)
            reset = sub0 == sub and slots == 512
            if reset:
                nt, px = nt0, px0
            ms = 2 if bm >= 64 else 1
            step = 0.2 + 0.04 * (2.0 * ms * sub)
            shape = (1.15 if k == 3 else 0.85) if cbn == 128 else 1.0
            rs = row_slots(W)
            narrow_ok = bm == 128 and cbn == 384 and rs == 32
            rowpen = 1.5 if (cbn != 128 and k == 3 and (W + 2) < 0.7 * rs and not narrow_ok) else 1.0
            nrounds = (mt * nt) / slots if slots == 512 else float(rounds)
            cost = (1.0 if nrounds < 1.0 else nrounds) * (10.0 + ksteps * step) * shape * rowpen + 0.005 * cbn
            if cost < best:
                best, pick = cost, (cbn, nt, nt > nt0, reset)
        best_bn, best_nt, more, reset = pick
        tr("ig.best384", best_bn == 384)
        tr("ig.best256", best_bn == 256)
        tr("ig.best128", best_bn == 128)
        tr("ig.nt>nt0", more)
        tr("ig.sub0_reset", reset)
        g = _conv_rows(tr, B, H, W, c, n, k, bm, best_bn, best_nt)
        if tr("ig.retry128", g["refused"] is not None):
            g = _conv_rows(tr, B, H, W, c, n, k, bm, 128, 0)
        if not tr("ig.rows_refused", g["refused"] is not None):
            return g
    patch = tr("ig.patch", k == 3 and W >= 24 and H >= 8)
    if pool:
        patch = True
    tiles = B * cdiv(OW, 16) * cdiv(OH, 16) if patch else cdiv(total_n, 256)
    tiles *= cdiv(n, bm)
    bn = 128 if tr("ig.tiles<200", tiles < 200) else 256
    if tr("ig.cb64_or_s2", cb == 64 or stride != 1):
        bn = 128
    if k == 1:
        patch = False
    if stride != 1:
        patch = True
    g = _launch_cfg(tr, B, H, W, OH, OW, c, n, k, stride, bm, bn, patch)
    if tr("ig.staging_fallback", g["refused"] is not None):
        g = _launch_cfg(tr, B, H, W, OH, OW, c, n, k, stride, bm, 128, True if (pool or stride != 1) else (not patch if k == 3 else False))
    return g


# ------------------------------------------------------------------------------------------------------------ the dispatch (shim.hip)
F_SMALL, F_C1X1, F_WS3, F_S32, F_P16 = 1024, 8192, 16384, 4096, 1 << 30  # mi355_debug_flags: families switched off (4096: small32 ON)


class NotFusable(Exception):
    """conv_pool_forward answers MI355_EINVAL: the host runs the two layers apart"""


def route(tr, cs):
    """what conv_forward_impl offers the layer to, in order, under cs.flags; returns (the accepting launcher's geometry, [refusals before it])"""
    B, H, W, c, n, k, S, plan, fl = cs.B, cs.H, cs.W, cs.c, cs.n, cs.k, cs.stride, cs.plan, cs.flags
    pool = cs.fuse in ("pool2", "pool1")
    refusals = []
    assert cs.fuse != "pool2" or not ((H | W) & 1), "the C ABI refuses a stride-2 pool on an odd map"
    if c == 3:
        assert k == 3 and S == 1 and cs.fuse in (None, "pool2")
        if not fl & F_SMALL:
            g = conv_first(tr, B, H, W, n, pool, cs.per_image, cs.planar)
            if not g["refused"]:
                return g, refusals
            refusals.append(g)
        # the VALU kernels (conv_first_pool_launch / conv_first_launch): one thread per pooled / output pixel, the weights in LDS
        assert not cs.planar, "the planar layout is served by the MFMA kernels only"
        if pool:
            return _ok("conv_first_valu", 1, cdiv(B * (H // 2) * (W // 2), 256), 256, n * 11 * 4), refusals
        return _ok("conv_first_valu", 1, cdiv(B * H * W, 256), 256, n * 9 * 4), refusals
    ws = conv1x1_eligible(n, c, k) or ws3_eligible(n, c, k) or conv_small_eligible(n, c, k)
    g = None

    def offer(x):
        nonlocal g
        g = x
        if g["refused"]:
            refusals.append(g)
        return not g["refused"]

    if pool and (cs.fuse == "pool1" or c in (128, 256)):
        if ws and ws3_eligible(n, c, k) and not fl & (F_WS3 | 1 << 21) and offer(conv_ws3(tr, B, H, W, c, n, S, 1 if cs.fuse == "pool1" else 2, plan, fl)):
            return g, refusals
        raise NotFusable(refusals)
    if cs.fuse == "pool2" and cs.epilogue and conv_small_eligible(n, c, k) and (c, n) == (16, 32) and not fl & (F_SMALL | F_P16):
        if offer(conv_pool16(tr, B, H, W, fl)):
            return g, refusals
    if cs.fuse == "pool2" and ws and (c, n, k) == (32, 64, 3) and (fl & (F_SMALL | F_S32)) == F_S32:
        if offer(conv_small32(tr, B, H, W, fl)):
            return g, refusals
    if k == 3 and conv_small_eligible(n, c, k) and not fl & F_SMALL:
        if offer(conv_mid(tr, B, H, W, n, plan, fl) if c == 64 else conv_small(tr, B, H, W, c, n, plan, fl)):
            return g, refusals
    if not pool and conv1x1_eligible(n, c, k) and not fl & F_C1X1:
        if offer(conv1x1(tr, B, H, W, c, n, plan)):
            return g, refusals
    if not pool and ws3_eligible(n, c, k) and not fl & F_WS3:
        if offer(conv_ws3(tr, B, H, W, c, n, S, 0, plan, fl)):
            return g, refusals
    if offer(conv_igemm(tr, B, H, W, c, n, k, S, pool, plan)):
        return g, refusals
    raise NotFusable(refusals)


# ------------------------------------------------------------------------------------------------------------ invariants (CPU)
def xcd_walk_tiles(grid, ntiles):
    """tiles each workgroup of a persistent launch walks (conv_pool16 / first layer: every XCD takes ceil(ntiles / 8) contiguous tiles when the
    grid is a multiple of 8, else workgroup w walks w, w + grid, ...) -> (max tiles per workgroup, every tile exactly once?)"""
    seen = np.zeros(ntiles, np.int32)
    most = 0
    xw = grid % 8 == 0
    per_x = cdiv(ntiles, 8) if xw else ntiles
    stride = grid // 8 if xw else grid
    for w in range(grid):
        base = (w & 7) * per_x if xw else 0
        end = min(base + per_x, ntiles)
        t0 = base + (w >> 3 if xw else w)
        idx = np.arange(t0, end, stride)
        seen[idx] += 1
        most = max(most, len(idx))
    return most, bool((seen == 1).all())


def per_image_walk_tiles(B, tpi, wpi):
    """per-image first layer: image b's workgroup k walks b * tpi + k, + wpi, ... -> (max tiles per workgroup, every tile exactly once?)"""
    seen = np.zeros(tpi, np.int32)
    most = 0
    for kk in range(wpi):
        idx = np.arange(kk, tpi, wpi)
        seen[idx] += 1
        most = max(most, len(idx))
    return most, bool((seen == 1).all())


def flat_span_pooled(p0, p1, OH, OW):
    """LDS rows a run of pooled pixels p0..p1 spans in the padded input (H + 1 rows an image, two image rows a pooled row, a halo row above
    and below)"""
    H = 2 * OH
    b0, b1 = p0 // (OH * OW), p1 // (OH * OW)
    r0, r1 = (p0 - b0 * OH * OW) // OW, (p1 - b1 * OH * OW) // OW
    return b1 * (H + 1) + 2 * r1 + 1 - b0 * (H + 1) - 2 * r0 + 1 + 2


def worst_flat_span(tp, total, OH, OW):
    t = np.arange(cdiv(total, tp), dtype=np.int64)
    p0 = t * tp
    p1 = np.minimum(p0 + tp, total) - 1
    return int(flat_span_pooled(p0, p1, OH, OW).max())


def worst_rows_span(g, H, W):
    """the row-image kernels: rows tile t of the plan spans (tiles split the pixel range evenly: tile_q, the first tile_r one longer)"""
    t = np.arange(g["ntiles"], dtype=np.int64)
    n0 = t * g["tile_q"] + np.minimum(t, g["tile_r"])
    n1 = n0 + g["tile_q"] + (t < g["tile_r"]) - 1
    ok = n1 >= n0
    hw = H * W

    def grow(p):
        b = p // hw
        return b * (H + 1) + (p - b * hw) // W
    return int((grow(n1[ok]) - grow(n0[ok]) + 1).max()) + 2 * g["halo"]


def tile_stats(cs, g):
    """(fill, crossings) of the worst tile of a flat launch: the fullest tile's pixels over the tile's capacity, and the most image boundaries a
    tile crosses.  None for 2-D patches and per-image tiles (a patch lies in one image)."""
    fam = g["family"]
    if fam == "conv_rows":
        t = np.arange(g["ntiles"], dtype=np.int64)
        n0 = t * g["tile_q"] + np.minimum(t, g["tile_r"])
        n1 = n0 + g["tile_q"] + (t < g["tile_r"]) - 1
        ok = n1 >= n0
        return (g["tile_q"] + (1 if g["tile_r"] else 0)) / g["bn"], int((n1[ok] // (cs.H * cs.W) - n0[ok] // (cs.H * cs.W)).max())
    if fam == "conv_igemm":
        if g["patch"]:
            return None
        tp, total, per, cap = g["bn"], cs.B * cs.H * cs.W, cs.H * cs.W, g["bn"]
    elif fam in ("conv_small", "conv_mid", "conv_small32"):
        if g["tiles_x"]:
            return None
        tp, total, per, cap = g["tp"], g["total"], g["OH"] * g["OW"], g["tp"]
    elif fam == "conv_ws3":
        OH, OW = (cs.H - 1) // g["S"] + 1, (cs.W - 1) // g["S"] + 1
        tp, total, per, cap = g["tp"], g["total"], (OH // 2) * (OW // 2) if g["pm"] == 2 else OH * OW, WS3_GMAX * 32 // g["upx"]
    elif fam == "conv1x1":
        tp, total, per, cap = g["tp"], cs.B * cs.H * cs.W, cs.H * cs.W, g["tp"]
    else:
        return None
    t = np.arange(cdiv(total, tp), dtype=np.int64)
    p0, p1 = t * tp, np.minimum(t * tp + tp, total) - 1
    return min(tp, total) / cap, int((p1 // per - p0 // per).max())


# ------------------------------------------------------------------------------------------------------------ reference
def conv_windows(x, k, stride, zp_in):
    """x [B, c, H, W] u8 -> float64 [c * k * k, B * OH * OW], the zero-point-padded windows in im2col order (channel, ky, kx)"""
    B, c, H, W = x.shape
    pad = k // 2
    OH, OW = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    if k == 1:
        return x.transpose(1, 0, 2, 3).reshape(c, B * H * W).astype(np.float64), OH, OW
    zp = np.broadcast_to(np.asarray(zp_in, np.uint8).reshape(-1, 1, 1, 1), (B, 1, 1, 1))
    xp = np.empty((B, c, H + 2 * pad, W + 2 * pad), np.uint8)
    xp[:] = zp
    xp[:, :, pad:pad + H, pad:pad + W] = x
    col = np.empty((c, k, k, B, OH, OW), np.float64)
    for ky in range(k):
        for kx in range(k):
            col[:, ky, kx] = xp[:, :, ky:ky + stride * (OH - 1) + 1:stride, kx:kx + stride * (OW - 1) + 1:stride].transpose(1, 0, 2, 3)
    return col.reshape(c * k * k, B * OH * OW), OH, OW


def conv_acc_ref(x, wq, zp_w, k, stride, zp_in, chunk_elems=1 << 24):
    """exact accumulators [n, B * OH * OW] int32 (wrapped as oracle.conv_acc wraps them).  zp_in: a scalar, or one per image"""
    B = x.shape[0]
    wd = wq.astype(np.float64) - zp_w.astype(np.float64)[:, None]
    K = wd.shape[1]
    zp_in = np.broadcast_to(np.asarray(zp_in, np.uint8), (B,))
    pad = k // 2
    P = ((x.shape[2] + 2 * pad - k) // stride + 1) * ((x.shape[3] + 2 * pad - k) // stride + 1)
    step = max(1, chunk_elems // (K * P))
    out = np.empty((wd.shape[0], B * P), np.int32)
    for b0 in range(0, B, step):
        b1 = min(B, b0 + step)
        col, OH, OW = conv_windows(x[b0:b1], k, stride, zp_in[b0:b1])
        acc = wd @ col
        assert np.abs(acc).max() < 2.0 ** 53
        out[:, b0 * P:b1 * P] = acc.astype(np.int64).astype(np.int32)  # (int64 -> int32: the low 32 bits, as the C cast)
    return out, OH, OW


def conv_ref(x, wq, zp_w, k, stride, zp_in, bias, mv, sv, zp_act, act, store):
    """-> u8 [B, n, OH, OW]: conv_acc_ref + ONE oracle.requant call on [n, B * OH * OW]"""
    import oracle
    acc, OH, OW = conv_acc_ref(x, wq, zp_w, k, stride, zp_in)
    u8 = oracle.requant(acc, bias, mv, sv, zp_act, act, store)
    return np.ascontiguousarray(u8.reshape(wq.shape[0], x.shape[0], OH, OW).transpose(1, 0, 2, 3))


def maxpool2(u8):
    """2 x 2 / stride 2 on [..., H, W] (even H, W)"""
    *lead, H, W = u8.shape
    return u8.reshape(*lead, H // 2, 2, W // 2, 2).max(axis=(-3, -1))


def maxpool1(u8):
    """2 x 2 / stride 1, the reference's pad = 1: windows y..y+1, x..x+1 clipped at the border"""
    o = u8.copy()
    o[..., :-1, :] = np.maximum(o[..., :-1, :], u8[..., 1:, :])
    r = o.copy()
    r[..., :, :-1] = np.maximum(r[..., :, :-1], o[..., :, 1:])
    return r


def macs(cs):
    pad = cs.k // 2
    OH, OW = (cs.H + 2 * pad - cs.k) // cs.stride + 1, (cs.W + 2 * pad - cs.k) // cs.stride + 1
    return cs.B * OH * OW * cs.n * cs.c * cs.k * cs.k


def device_tensors(cs):
    """bytes of every device tensor the case's call touches"""
    pad = cs.k // 2
    OH, OW = (cs.H + 2 * pad - cs.k) // cs.stride + 1, (cs.W + 2 * pad - cs.k) // cs.stride + 1
    out = {"x": cs.B * 3 * cs.H * cs.W if cs.planar else tensor_bytes(cs.B, cs.H, cs.W, cs.c), "x_nchw": cs.B * cs.c * cs.H * cs.W}
    if cs.fuse == "pool2":
        out["ypool"] = tensor_bytes(cs.B, OH // 2, OW // 2, cs.n)
        out["y_nchw"] = cs.B * cs.n * (OH // 2) * (OW // 2)
    else:
        out["y"] = tensor_bytes(cs.B, OH, OW, cs.n)
        out["y_nchw"] = cs.B * cs.n * OH * OW
    return out


# ------------------------------------------------------------------------------------------------------------ the case table
class Case:
    """one layer call.  fuse: None | 'pool2' | 'pool1'.  flags: mi355_debug_flags of the call.  alt: debug flags of a second route whose bytes
    are compared as well (None: none).  store: the store mode that runs first and on the second route ('wrap' | 'sat'); the other runs after it."""

    def __init__(self, name, c, n, H, W, B, k=3, stride=1, fuse=None, plan=0, flags=0, epilogue=False, planar=False, per_image=False,
                 act="leaky", alt=None, store="wrap"):
        self.name, self.c, self.n, self.H, self.W, self.B, self.k, self.stride = name, c, n, H, W, B, k, stride
        self.fuse, self.plan, self.flags, self.epilogue, self.planar, self.per_image = fuse, plan, flags, epilogue, planar, per_image
        self.act, self.alt, self.store = act, alt, store

    def __repr__(self):
        return self.name


def trace_case(cs):
    """-> (Trace, geometry | None when the fused call is refused outright, refusals)"""
    tr = Trace()
    try:
        g, refusals = route(tr, cs)
    except NotFusable as e:
        g, refusals = None, e.args[0]
    return tr, g, refusals


def _c(*a, **kw):
    return Case(*a, **kw)


CASES = []  # filled below, family by family


def _add(*cases):
    CASES.extend(cases)


GEN = F_SMALL | F_C1X1 | F_WS3  # the generic route: the row-image / implicit-GEMM kernels (first layer: its VALU kernels)

# ---- conv1x1.hip: gmax 32 / 16 / 8 on each side of one round | two; filter tiles 1 / 2 / 4; the tp clamp; plan-1 rounding and growth;
# ragged n; the LDS limit on each side (160 KB for one round of the chip, 96 KB beyond)
_add(
    _c("c1_64_32_4x4_B16384_1round", 64, 32, 4, 4, 16384, k=1, alt=F_C1X1),
    _c("c1_64_32_4x4_B16385_2rounds", 64, 32, 4, 4, 16385, k=1, store="sat"),
    _c("c1_128_32_4x4_B8192_1round", 128, 32, 4, 4, 8192, k=1, store="sat"),
    _c("c1_128_32_4x4_B8193_2rounds", 128, 32, 4, 4, 8193, k=1, alt=F_C1X1),
    _c("c1_256_32_62_B17_1round", 256, 32, 62, 62, 17, k=1),
    _c("c1_256_32_62_B18_2rounds", 256, 32, 62, 62, 18, k=1, store="sat", alt=F_C1X1),
    _c("c1_1024_32_16_B128_lds_fits", 1024, 32, 16, 16, 128, k=1),
    _c("c1_1024_32_16_B129_lds_refused", 1024, 32, 16, 16, 129, k=1, store="sat"),
    _c("c1_512_30_3x3_B1_tp16_ragged", 512, 30, 3, 3, 1, k=1),
    _c("c1_64_255_5x7_B3_ragged", 64, 255, 5, 7, 3, k=1, store="sat", alt=F_C1X1),
    _c("c1_256_512_5x5_B70_mtiles2", 256, 512, 5, 5, 70, k=1),
    _c("c1_128_1024_3x3_B40_mtiles4", 128, 1024, 3, 3, 40, k=1, store="sat", alt=F_C1X1),
    _c("c1_256_128_13_B7_plan1_round32", 256, 128, 13, 13, 7, k=1, plan=1),
    _c("c1_256_32_13_B7_plan1_no_growth", 256, 32, 13, 13, 7, k=1, plan=1, store="sat"),
    _c("c1_1024_256_2x2_B300_plan1_grow", 1024, 256, 2, 2, 300, k=1, plan=1, store="sat", alt=F_C1X1),
    _c("c1_256_64_62_B18_plan1_2rounds", 256, 64, 62, 62, 18, k=1, plan=1),
    _c("c1_512_32_16_B322_96K_refused", 512, 32, 16, 16, 322, k=1, store="sat"),
)

# ---- conv_pool16.hip (16 -> 32 + maxpool, epilogue table): tile counts below, at and above the 768 cap; the `need` widening at its
# lower end (a grid of 8 for fewer tiles) and above 768 x 64 tiles; ragged and whole patches; the ten-bit tile words' refusal
_add(
    _c("p16_2x2_B1_need8", 16, 32, 2, 2, 1, fuse="pool2", epilogue=True, alt=F_P16),
    _c("p16_2x2_B8", 16, 32, 2, 2, 8, fuse="pool2", epilogue=True, store="sat"),
    _c("p16_2x2_B767", 16, 32, 2, 2, 767, fuse="pool2", epilogue=True),
    _c("p16_2x2_B768", 16, 32, 2, 2, 768, fuse="pool2", epilogue=True, store="sat"),
    _c("p16_2x2_B769", 16, 32, 2, 2, 769, fuse="pool2", epilogue=True, alt=F_SMALL),
    _c("p16_2x2_B49152_at_768x64", 16, 32, 2, 2, 49152, fuse="pool2", epilogue=True, store="sat"),
    _c("p16_2x2_B49153_widened_776", 16, 32, 2, 2, 49153, fuse="pool2", epilogue=True, alt=F_P16),
    _c("p16_16x32_B100_whole_patches", 16, 32, 16, 32, 100, fuse="pool2", epilogue=True, store="sat", alt=F_P16),
    _c("p16_18x34_B50_ragged_patches", 16, 32, 18, 34, 50, fuse="pool2", epilogue=True, plan=1),
    _c("p16_2x32752_B1_tx1024_refused", 16, 32, 2, 32752, 1, fuse="pool2", epilogue=True),
    _c("p16_2x32736_B1_tx1023", 16, 32, 2, 32736, 1, fuse="pool2", epilogue=True, store="sat"),
)

# ---- first layer (conv_aux.hip): the cap of 1024 on each side, the widening (a grid of 8 below 8 tiles, 1032 above 65 536 tiles),
# the form without a pool (no widening), per-image grids (raised / clamped / neither), planar input, the refusal
_add(
    _c("l0p_2x2_B1_need8", 3, 16, 2, 2, 1, fuse="pool2", epilogue=True, alt=F_SMALL),
    _c("l0p_2x2_B1023", 3, 16, 2, 2, 1023, fuse="pool2", epilogue=True, store="sat"),
    _c("l0p_2x2_B1024", 3, 32, 2, 2, 1024, fuse="pool2", epilogue=True),
    _c("l0p_2x2_B1025", 3, 16, 2, 2, 1025, fuse="pool2", epilogue=True, store="sat", alt=F_SMALL),
    _c("l0p_2x2_B65536_at_1024x64", 3, 16, 2, 2, 65536, fuse="pool2", epilogue=True),
    _c("l0p_2x2_B65537_widened_1032", 3, 16, 2, 2, 65537, fuse="pool2", epilogue=True, store="sat", alt=F_SMALL),
    _c("l0p_4x4_B65537_planar_widened", 3, 32, 4, 4, 65537, fuse="pool2", epilogue=True, planar=True),
    _c("l0p_34x66_B40_ragged", 3, 32, 34, 66, 40, fuse="pool2", epilogue=True, store="sat"),
    _c("l0p_2x32752_B1_tx1024_refused", 3, 16, 2, 32752, 1, fuse="pool2", epilogue=True),
    _c("l0_2x2_B1023", 3, 16, 2, 2, 1023, store="sat", alt=F_SMALL),
    _c("l0_2x2_B1025", 3, 32, 2, 2, 1025),
    _c("l0_2x2_B65537_no_widening", 3, 16, 2, 2, 65537, store="sat"),
    _c("l0_3x5_B9_odd_refused", 3, 16, 3, 5, 9),
    _c("l0p_pi_2x2_B1500_one_each", 3, 16, 2, 2, 1500, fuse="pool2", epilogue=True, per_image=True),
    _c("l0p_pi_2x2_B5_clamped", 3, 32, 2, 2, 5, fuse="pool2", epilogue=True, per_image=True, store="sat"),
    _c("l0p_pi_32x64_B5_wpi", 3, 16, 32, 64, 5, fuse="pool2", epilogue=True, per_image=True, store="sat"),
    _c("l0p_pi_2x2080_B300_65_tiles", 3, 16, 2, 2080, 300, fuse="pool2", epilogue=True, per_image=True),
    _c("l0_pi_2x2_B1500_one_each", 3, 32, 2, 2, 1500, per_image=True, store="sat"),
    _c("l0_pi_48x64_B7_wpi", 3, 16, 48, 64, 7, per_image=True),
)

# ---- conv_small.hip, 16 / 32 channels: flat runs over many images (4 x 4 maps: 32 images a tile), the 2 x 2 refusal, pitch padding for
# even and odd OW, wide maps at OW 63 | 64, per_cu 1 / 2 / 3, persistent grids below the tile count
_add(
    _c("sm_16_32_4x4_B70_flat_32_images", 16, 32, 4, 4, 70, fuse="pool2", alt=F_SMALL),
    _c("sm_16_64_4x4_B64_flat", 16, 64, 4, 4, 64, fuse="pool2", store="sat"),
    _c("sm_32_64_4x4_B200_flat", 32, 64, 4, 4, 200, fuse="pool2", plan=1),
    _c("sm_16_32_2x2_B300_refused", 16, 32, 2, 2, 300, fuse="pool2"),
    _c("sm_32_32_4x2_B500_odd_OW", 32, 32, 4, 2, 500, fuse="pool2", store="sat", alt=F_SMALL),
    _c("sm_16_32_6x10_B40_odd_OW_s1", 16, 32, 6, 10, 40),
    _c("sm_32_64_10x12_B30_s2", 32, 64, 10, 12, 30, stride=2, store="sat", alt=F_SMALL),
    _c("sm_16_32_2x126_B20_OW63", 16, 32, 2, 126, 20, fuse="pool2"),
    _c("sm_16_32_2x128_B20_OW64_wide", 16, 32, 2, 128, 20, fuse="pool2", store="sat", alt=F_SMALL),
    _c("sm_32_64_18x130_B3_wide_ragged", 32, 64, 18, 130, 3, fuse="pool2"),
    _c("sm_16_32_4x4_B25000_persistent3", 16, 32, 4, 4, 25000, fuse="pool2", store="sat"),
    _c("sm_32_64_4x4_B8300_persistent", 32, 64, 4, 4, 8300, fuse="pool2", alt=F_SMALL),
    _c("sm_16_64_2x128_B300_wide_persistent", 16, 64, 2, 128, 300, plan=1, store="sat"),
    _c("sm_16_32_5x6_B4_odd_map_refused", 16, 32, 5, 6, 4),
)

# ---- conv_small32.hip (debug bit 4096): the same clauses; its two refusals hand the layer to conv_small.hip / the generic kernel
_add(
    _c("s32_2x6_B400_flat", 32, 64, 2, 6, 400, fuse="pool2", flags=F_S32, alt=0),
    _c("s32_4x4_B300_lds_refused", 32, 64, 4, 4, 300, fuse="pool2", flags=F_S32, store="sat"),
    _c("s32_2x2_B300_cells_refused", 32, 64, 2, 2, 300, fuse="pool2", flags=F_S32),
    _c("s32_12x10_B60_odd_OW", 32, 64, 12, 10, 60, fuse="pool2", flags=F_S32, store="sat", alt=0),
    _c("s32_2x126_B20_OW63", 32, 64, 2, 126, 20, fuse="pool2", flags=F_S32),
    _c("s32_2x128_B20_OW64_wide", 32, 64, 2, 128, 20, fuse="pool2", flags=F_S32, store="sat", alt=0),
    _c("s32_8x8_B4200_persistent", 32, 64, 8, 8, 4200, fuse="pool2", flags=F_S32, alt=0),
)

# ---- conv_small.hip, 64 channels: rounds 1 | 2, the tp clamp, plan-1 rounding (down to 32s, capped at 128), half | whole workgroups, the
# LDS test that vetoes half, wide maps, the LDS refusal on tiny maps
_add(
    _c("m64_64_4x4_B10_tp32", 64, 64, 4, 4, 10, fuse="pool2", alt=F_SMALL),
    _c("m64_128_8x8_B700_whole", 64, 128, 8, 8, 700, store="sat"),
    _c("m64_96_8x8_B700_plan1_half", 64, 96, 8, 8, 700, fuse="pool2", plan=1),
    _c("m64_64_8x8_B2500_plan1_tp128", 64, 64, 8, 8, 2500, stride=2, plan=1, store="sat", alt=F_SMALL),
    _c("m64_64_8x8_B4096_s2_1round", 64, 64, 8, 8, 4096, stride=2),
    _c("m64_64_8x8_B4097_s2_2rounds_half", 64, 64, 8, 8, 4097, stride=2, store="sat"),
    _c("m64_128_10x6_B300_odd_OW", 64, 128, 10, 6, 300, fuse="pool2", alt=F_SMALL),
    _c("m64_64_126x126_B8_plan1_half_vetoed", 64, 64, 126, 126, 8, plan=1, store="sat"),
    _c("m64_64_2x128_B40_wide", 64, 64, 2, 128, 40, fuse="pool2"),
    _c("m64_128_18x130_B3_wide_plan1", 64, 128, 18, 130, 3, plan=1, store="sat", alt=F_SMALL),
    _c("m64_64_2x2_B53300_s2_lds_refused", 64, 64, 2, 2, 53300, stride=2),
    _c("m64_64_5x4_B6_odd_map_refused", 64, 64, 5, 4, 6, store="sat"),
)

# ---- conv_ws3.hip: kp 1 | 2, stride 1 | 2, the three pool modes; below 64 units; one tile per workgroup; the whole-image alias; the
# double- and single-buffered persistent loops; the row-image refusal; the stride-1 pool's bounds; plan_one_round
_add(
    _c("w3_128_64_8x8_B256_alias", 128, 64, 8, 8, 256, alt=F_WS3),
    _c("w3_128_64_8x8_B3_units_refused", 128, 64, 8, 8, 3, store="sat"),
    _c("w3_256_256_6x6_B250_kp2_mtiles2", 256, 256, 6, 6, 250, store="sat", alt=F_WS3),
    _c("w3_128_32_32x32_B16_one_tile", 128, 32, 32, 32, 16),
    _c("w3_128_32_16x16_B257_db_even", 128, 32, 16, 16, 257, store="sat", alt=F_WS3),
    _c("w3_128_32_4x128_B129_db_rows", 128, 32, 4, 128, 129),
    _c("w3_256_32_66x66_B8_sb_even", 256, 32, 66, 66, 8, store="sat"),
    _c("w3_128_32_2x300_B129_s2_sb_rows", 128, 32, 2, 300, 129, stride=2, alt=F_WS3),
    _c("w3_128_32_2x300_B31_no_plan", 128, 32, 2, 300, 31, store="sat"),
    _c("w3_128_32_26x26_B100_row_image_better", 128, 32, 26, 26, 100),
    _c("w3_128_64_7x7_B40_s2_odd_refused", 128, 64, 7, 7, 40, stride=2, store="sat"),
    _c("w3_128_64_8x8_B1024_s2", 128, 64, 8, 8, 1024, stride=2, alt=F_WS3),
    _c("w3_128_64_10x10_B30_plan1_refused", 128, 64, 10, 10, 30, plan=1, store="sat"),
    _c("w3_128_32_19x19_B64_plan1_w19_kept", 128, 32, 19, 19, 64, plan=1),
    _c("w3_128_32_8x8_B128_pool1", 128, 32, 8, 8, 128, fuse="pool1", store="sat"),
    _c("w3_128_32_8x8_B257_pool1_persistent", 128, 32, 8, 8, 257, fuse="pool1"),
    _c("w3_128_32_8x8_B127_pool1_refused", 128, 32, 8, 8, 127, fuse="pool1", store="sat"),
    _c("w3_128_32_7x9_B200_pool1_hw63_refused", 128, 32, 7, 9, 200, fuse="pool1"),
    _c("w3_128_32_16x17_B200_pool1_hw272_refused", 128, 32, 16, 17, 200, fuse="pool1", store="sat"),
    _c("w3_256_128_12x12_B128_pool1_kp2", 256, 128, 12, 12, 128, fuse="pool1"),
    _c("w3_128_64_8x8_B256_pool2", 128, 64, 8, 8, 256, fuse="pool2", store="sat"),
    _c("w3_256_64_12x12_B120_pool2_kp2", 256, 64, 12, 12, 120, fuse="pool2"),
    _c("w3_128_32_2x300_B31_pool2_refused", 128, 32, 2, 300, 31, fuse="pool2", store="sat"),
)

# ---- conv_igemm.hip -> conv_rows.hip / conv_rows16.hip / launch_cfg, reached with the specialised kernels switched off (GEN) or on
# shapes none of them takes: the candidate the cost model picks, more and narrower tiles, the sub-tile reset, the row-slot widths at
# W + 2 = 16 | 17, 32 | 33, 64 | 65, the narrow-map 384 variant, "map too narrow" -> 128 -> implicit GEMM, patch | flat, bn 256 | 128,
# the staging-budget fallback
_add(
    _c("ig_192_128_15x15_B40_narrow384", 192, 128, 15, 15, 40),
    _c("ig_64_16_10x10_B50_best256_too_narrow_to_flat", 64, 16, 10, 10, 50, flags=GEN, store="sat"),
    _c("ig_64_16_23x24_B64_k1_reset", 64, 16, 23, 24, 64, k=1, flags=GEN),
    _c("ig_64_16_64x64_B8_k1_W64_refused_to_flat", 64, 16, 64, 64, 8, k=1, flags=GEN, store="sat"),
    _c("ig_64_48_14x14_B30_rows16", 64, 48, 14, 14, 30, flags=GEN),
    _c("ig_64_48_15x15_B30_rs32_too_narrow_to_flat", 64, 48, 15, 15, 30, flags=GEN, store="sat"),
    _c("ig_64_16_14x14_B30_rows16_bm32", 64, 16, 14, 14, 30, flags=GEN),
    _c("ig_192_64_30x30_B10_rs32", 192, 64, 30, 30, 10, store="sat"),
    _c("ig_192_64_31x31_B10_rs64_too_narrow_to_patch", 192, 64, 31, 31, 10),
    _c("ig_192_64_62x62_B3_rs64", 192, 64, 62, 62, 3, store="sat"),
    _c("ig_192_64_63x63_B3_patch", 192, 64, 63, 63, 3),
    _c("ig_64_16_1x1_B700_k1_too_narrow", 64, 16, 1, 1, 700, k=1, flags=GEN, store="sat"),
    _c("ig_64_16_4x30_B9_k1", 64, 16, 4, 30, 9, k=1, flags=GEN),
    _c("ig_128_64_10x10_B3_plan1_thr", 128, 64, 10, 10, 3, plan=1, store="sat"),
    _c("ig_16_16_23x24_B9_s2_patch", 16, 16, 23, 24, 9, stride=2, flags=GEN),
    _c("ig_48_16_7x30_B9_flat", 48, 16, 7, 30, 9, store="sat"),
    _c("ig_16_16_2x2_B255_pool_bn256", 16, 16, 2, 2, 255, fuse="pool2"),
    _c("ig_16_32_6x6_B30_pool_bn128", 16, 32, 6, 6, 30, fuse="pool2", flags=GEN, store="sat"),
    _c("ig_16_16_2x1000_B3_staging_fallback", 16, 16, 2, 1000, 3),
    _c("ig_16_128_2x1200_B22_lds_fallback", 16, 128, 2, 1200, 22, store="sat"),
    _c("ig_32_200_13x13_B5_k1_ragged", 32, 200, 13, 13, 5, k=1),
    _c("ig_64_256_40x11_B100_k1_lds_retry128", 64, 256, 40, 11, 100, k=1, flags=GEN, store="sat"),
)

# ---- the row-image kernels with FULL tiles that cross image boundaries (the cases above fill one round of 256 workgroups with a handful of
# pixels each): 128, 256 and 384 columns on 16-, 32- and 64-slot rows (conv_rows.hip, both kernel sizes) and on conv_rows16.hip's exact
# rows, each on the lowest maps its DMA-slot test admits (W >= 3/4 of the slots; many tiny images beyond that are refused as "too narrow").
# A full 384-column 3x3 tile in every workgroup of a round costs 256 x 384 x 128 x 576 = 7.2e9 multiply-adds: those stay at 73-80 %.
_add(
    _c("rows_k1_128_rs16_2x14_B1500", 64, 16, 2, 14, 1500, k=1, flags=GEN),
    _c("rows_k1_128_rs32_3x30_B450", 64, 16, 3, 30, 450, k=1, flags=GEN, store="sat"),
    _c("rows_k1_128_rs64_3x48_B300", 64, 16, 3, 48, 300, k=1, flags=GEN),
    _c("rows_k1_384_rs16_14x14_B500", 64, 128, 14, 14, 500, k=1, flags=GEN, store="sat"),
    _c("rows_k1_384_rs32_6x24_B2000", 64, 128, 6, 24, 2000, k=1, flags=GEN),
    _c("rows_k1_384_rs64_4x62_B1500", 64, 128, 4, 62, 1500, k=1, flags=GEN, store="sat"),
    _c("rows_k3_128_rs16_4x14_B700_plan1", 64, 16, 4, 14, 700, plan=1, flags=GEN),
    _c("rows_k3_128_rs32_3x30_B450_plan1", 64, 16, 3, 30, 450, plan=1, flags=GEN, store="sat"),
    _c("rows_k3_128_rs64_3x48_B100", 64, 16, 3, 48, 100, flags=GEN),
    _c("rows_k3_256_rs16_4x14_B8000", 64, 16, 4, 14, 8000, flags=GEN, store="sat"),
    _c("rows_k3_256_rs32_3x30_B5000", 64, 16, 3, 30, 5000, flags=GEN),
    _c("rows_k3_256_rs64_6x62_B700", 64, 16, 6, 62, 700, flags=GEN, store="sat"),
    _c("rows_k3_384_rs32_4x30_B300", 64, 256, 4, 30, 300, flags=GEN),
    _c("rows_k3_384_rs64_4x62_B300", 64, 128, 4, 62, 300, flags=GEN, store="sat"),
    _c("rows16_128_3x14_B1000", 64, 48, 3, 14, 1000, flags=GEN),
    _c("rows16_256_3x14_B1500", 64, 128, 3, 14, 1500, flags=GEN, store="sat"),
    _c("rows16_384_2x12_B3000_12_images", 64, 128, 2, 12, 3000, flags=GEN),
    _c("rows16_narrow384_1x15_B2000_8_images", 64, 128, 1, 15, 2000, flags=GEN, store="sat"),
    _c("rows16_narrow384_4x19_B1000", 64, 128, 4, 19, 1000, flags=GEN),
)
# ---- flat 3x3 implicit-GEMM tiles and a conv_ws3 tile over 2 x 2 maps: 128 / 256 pixels span 32 / 64 images
_add(
    _c("ig_48_16_2x2_B4000_flat128_32_images", 48, 16, 2, 2, 4000, store="sat"),
    _c("ig_48_16_2x2_B13000_flat256_64_images", 48, 16, 2, 2, 13000),
    _c("ig_48_16_3x3_B6000_flat256", 48, 16, 3, 3, 6000, store="sat"),
    _c("w3_128_32_2x2_B16384_64_images", 128, 32, 2, 2, 16384, alt=F_WS3),
)


# ------------------------------------------------------------------------------------------------------------ for the other tests
def geom_conv1x1(c, n, B, H, W, plan):
    """conv1x1.hip's launch for test_gpu_plan_slots.py: grid, threads, lds, tp, mtiles, rounds"""
    return conv1x1(Trace(), B, H, W, c, n, plan)


def geom_small64(n, B, H, W, plan):
    """conv_small.hip, 64 channels, flat tiles (pooled / 2x2-block width < 64), for test_gpu_plan_slots.py: grid, threads, tp, half, ntiles"""
    g = conv_mid(Trace(), B, H, W, n, plan)
    assert g["tiles_x"] == 0
    return g


def rand_layer(rng, n, c, k, gain="some-wrap"):
    """weights in the suite's wrap regimes (test_gpu_parity.py), the multiplier range scaled with K from the 144 of a 16-channel 3x3; zero points
    0 and 255 among them (128 - zp_w leaves the int8 range there: the correction terms of the few-channel kernels)"""
    K = c * k * k
    wq = rng.integers(0, 256, (n, K), dtype=np.uint8)
    zp_w = rng.integers(90, 166, n, dtype=np.uint8)
    zp_w[0], zp_w[1 % n] = 0, 255
    bias = rng.integers(-20000, 20000, n).astype(np.int32)
    lo, hi = {"some-wrap": (2.0 ** -14, 2.0 ** -12), "much-wrap": (2.0 ** -11, 2.0 ** -7)}[gain]
    f = 144.0 / K
    M = rng.uniform(lo * f, hi * f, n)
    shift = np.floor(-np.log2(M)).astype(int)
    M0 = np.round(M * 2.0 ** shift * 2 ** 31)
    if gain == "some-wrap":
        bias = (bias // 16).astype(np.int32)
    return wq, zp_w, bias, M0 * 2.0 ** -31, 2.0 ** -shift.astype(np.float64)
