"""GPU: every conv kernel's requantise epilogue AT its switch points (`-m gpu`).  tests/epilogue_points.py builds layers whose accumulators
sit one step inside, on and one step outside every point where csrc/common.h changes form -- the branch-free LEAKY's q >= -40000 and its
wave-wide fallback, the 24-bit multiply's |q| + 5 < 65536, the ties of round(q / 10), the byte's wrap at both ends, SAT's clamp of q, the
pooled kernels' wrap-safe range [lo, hi] (true, the packed table's own, the clamps at +-2^30), the integer form's accept / reject edge, shifts
that are not powers of two -- and tests/test_epilogue_points_cpu.py proves that aim on the CPU.  Here the same launches run through the C-ABI
and every byte is compared with oracle.requant (then oracle.maxpool_u8 for the pooled calls): exact, no tolerance.  After each call
mi355_last_conv_kernel() must name the family meant.  Nothing here reads the reference tree."""
import ctypes as C

import numpy as np
import pytest

import epilogue_points as ep
import oracle
from yolo_quantization_amd import binding

pytestmark = pytest.mark.gpu

ACT_ZP = [(a, z) for a in (ep.LEAKY, ep.RELU6, ep.LINEAR) for z in ep.ZP_ACTS[a]]
STORES = [binding.STORE_WRAP, binding.STORE_SATURATE]


@pytest.fixture(scope="module", autouse=True)
def device():
    binding.init(0)


def _want(L, store):
    """oracle.requant of the launch's accumulators: [B, n, OH, OW]"""
    acc = L.acc_of()
    v = L.value_of()
    B, n, P = acc.shape   # (one call for the whole batch: the images side by side)
    u8 = oracle.requant(acc.transpose(1, 0, 2).reshape(n, B * P), L.bias, L.M, L.S, L.zp, oracle.ACT[L.act], store)
    return np.ascontiguousarray(u8.reshape(n, B, P).transpose(1, 0, 2)).reshape(v.shape)


def _explain(L, got, want, what):
    """the first differing values with every intermediate of the restatement"""
    bad = np.argwhere(got != want)
    lines = ["%s: %s: %d of %d bytes differ" % (L.name, what, len(bad), got.size)]
    v = L.value_of()
    for b, o, y, x in bad[:6]:
        if v.shape == got.shape:
            a = int(v[b, o, y, x])
            lines.append("  image %d channel %d (%d, %d): acc + bias = %d = target %+d, q = %d, got %d want %d"
                         % (b, o, y, x, a, a - int(L.T[o]), int(ep.q_of(a, L.M[o], L.S[o])), got[b, o, y, x], want[b, o, y, x]))
        else:
            win = v[b, o, 2 * y:2 * y + 2, 2 * x:2 * x + 2].ravel()
            lines.append("  image %d channel %d pooled (%d, %d): window acc + bias - target = %s (target %d), q = %s, got %d want %d"
                         % (b, o, y, x, (win - int(L.T[o])).tolist(), int(L.T[o]), ep.q_of(win, L.M[o], L.S[o]).tolist(), got[b, o, y, x], want[b, o, y, x]))
    return "\n".join(lines)


@pytest.mark.parametrize("store", STORES, ids=["wrap", "saturate"])
@pytest.mark.parametrize("act,zp", ACT_ZP, ids=lambda v: str(v))
@pytest.mark.parametrize("fname", ep.PER_PIXEL)
def test_per_pixel_switch_points(fname, act, zp, store):
    """The kernels that requantise every pixel (first layer without pool, conv1x1.hip, conv_ws3.hip, the row-image kernels, the implicit GEMM,
    conv_kxk.hip, conv_small.hip without pool) on the whole per-pixel catalogue: the boundaries of q, the fallback launches, exact products,
    |acc + bias| = 2^30, shifts that are no powers of two."""
    fam = ep.FAMILIES[fname]
    failures = []
    binding.shim().mi355_debug_flags(fam.get("flags", 0))
    try:
        for L in ep.per_pixel_launches(fname, act, zp):
            xt = binding.DevTensor.from_nchw(L.x, ep.ZP_IN)
            got = binding.conv_forward(xt, L.wq, L.zp_w, fam["k"], L.bias, L.M, L.S, ep.ZP_IN, zp, 1.0, binding.ACT[act], store,
                                       binding.ACC_EXACT, want_acc=False, stride=fam.get("stride", 1))["u8"]
            assert binding.shim().mi355_last_conv_kernel() == fam["id"], "%s: the call should be served by kernel family %d" % (L.name, fam["id"])
            want = _want(L, store)
            if not np.array_equal(got, want):
                failures.append(_explain(L, got, want, fname))
    finally:
        binding.shim().mi355_debug_flags(0)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("store", STORES, ids=["wrap", "saturate"])
@pytest.mark.parametrize("act,zp", ACT_ZP, ids=lambda v: str(v))
@pytest.mark.parametrize("fname", ep.POOLED)
def test_pooled_switch_points(fname, act, zp, store):
    """The conv + maxpool kernels (first-layer MFMA kernels, conv_small.hip, conv_pool16.hip, conv_small32.hip) in every launch-wide state --
    all channels integer-capable, exactly one not, random multipliers, both ends of the range clamped, shifts that are no powers of two -- with
    the packed table, a table packed for another zero point, and none; windows on the range's end, one value one step beyond it, in both
    directions; under both plans where the plan changes the launch."""
    fam = ep.FAMILIES[fname]
    n, c, H, W = fam["n"], fam["c"], fam["H"], fam["W"]
    failures = []

    def pack(L, zp_t=None, table=True):
        return binding.conv_pack(L.wq, L.zp_w, c, 3, L.bias, L.M, L.S, *((binding.ACT[act], L.zp if zp_t is None else zp_t) if table else ()))

    modes = ("match", "mismatch", "none") if store == binding.STORE_WRAP else ("none",)   # (a saturating launch ignores the table)
    binding.shim().mi355_debug_flags(fam.get("flags", 0))
    try:
        for state in ep.STATES:
            Ls, _ = ep.pooled_set(fname, act, zp, state, pack)
            for L in Ls:
                B = L.x.shape[0]
                xt = binding.DevTensor.from_nchw(L.x, ep.ZP_IN)
                u8 = _want(L, store)
                want = np.stack([oracle.maxpool_u8(u8[b], 2, 2, 1) for b in range(B)])
                for mode in modes:
                    blob = binding.DevBuf.from_numpy(pack(L, (zp + 1) % 256 if mode == "mismatch" else None, mode != "none"))
                    for plan in fam.get("plans", (0,)):
                        yp = binding.DevTensor(B, H // 2, W // 2, n, zp)
                        d = binding.ConvDesc(n, c, 3, 1, 1, binding.ACT[act], store, binding.ACC_EXACT, ep.ZP_IN, zp, 1.0)
                        d.plan = plan
                        d.epilogue_packed = fam.get("hint", 0)
                        binding.check(binding.shim().mi355_conv_pool_forward(C.byref(d), xt.ref(), blob.ptr, None, yp.ref(), None), "conv_pool")
                        assert binding.shim().mi355_last_conv_kernel() == fam["id"], "%s: the call should be served by kernel family %d" % (L.name, fam["id"])
                        got = yp.to_nchw()
                        if not np.array_equal(got, want):
                            failures.append(_explain(L, got, want, "%s table %s plan %d" % (fname, mode, plan)))
    finally:
        binding.shim().mi355_debug_flags(0)
    assert not failures, "\n".join(failures[:8]) + "\n(%d failing launches)" % len(failures)
