"""CPU proof of tests/epilogue_points.py's aim (no GPU): every launch that tests/test_gpu_epilogue_points.py runs is built here and checked
against the oracle and the packed epilogue table BEFORE any kernel sees it -- the convolution gives the intended accumulators, the numpy
restatement gives the oracle's bytes, every probe straddles its point, and a table launch is in the launch-wide state it is named after."""
import numpy as np
import pytest

import epilogue_points as ep
import oracle
from yolo_quantization_amd import binding

ACT_ZP = [(a, z) for a in (ep.LEAKY, ep.RELU6, ep.LINEAR) for z in ep.ZP_ACTS[a]]


def _conv_checked(fname, act, zp):
    """Which launches go through oracle.conv_acc.  The weights and images of a launch depend on the family, the direction and the catalogue
    entry; activation and zero point only move the bias, which the convolution never sees.  So: every launch where the convolution is
    cheap (c <= 16), one zero point per activation elsewhere, and `rows32` (the layers of `rows` under another debug switch) not at all."""
    if ep.FAMILIES[fname]["c"] <= 16:
        return True
    return fname != "rows32" and zp == (128 if act == ep.LINEAR else 23)


def _check_bytes(L):
    """oracle.requant of the intended accumulators == the numpy restatement, both stores; returns (wrap, sat) [B, n, P]"""
    acc = L.acc_of()
    val = L.value_of().reshape(acc.shape)
    res = []
    for store in (oracle.STORE_WRAP, oracle.STORE_SATURATE):
        B, n, P = acc.shape   # (one call for the whole batch: the images side by side)
        got = oracle.requant(acc.transpose(1, 0, 2).reshape(n, B * P), L.bias, L.M, L.S, L.zp, oracle.ACT[L.act], store).reshape(n, B, P).transpose(1, 0, 2)
        want = ep.byte_of(val, L.M[None, :, None], L.S[None, :, None], L.zp, L.act, store == oracle.STORE_SATURATE)
        assert np.array_equal(got, want), (L.name, "restatement != oracle.requant")
        res.append(got)
    return res


def _check_acc(L):
    f = L.fam
    acc = L.acc_of()
    for b in range(min(acc.shape[0], 3) if acc.shape[0] > 16 else acc.shape[0]):   # (a family that needs a large batch to reach its kernel repeats its images' pattern)
        got = oracle.conv_acc(L.x[b], L.wq, L.zp_w, f["k"], f.get("stride", 1), f["k"] // 2, ep.ZP_IN)
        assert np.array_equal(got, acc[b]), (L.name, b, "oracle.conv_acc != sigma * x")


@pytest.mark.parametrize("fname", ep.PER_PIXEL)
def test_per_pixel_launches_are_aimed(fname):
    ep.DROPPED.clear()
    launches = probes = 0
    for act, zp in ACT_ZP:
        for L in ep.per_pixel_launches(fname, act, zp):
            if _conv_checked(fname, act, zp):
                _check_acc(L)
            wrap, sat = _check_bytes(L)
            if L.kind == "q":
                ch = L.live & (L.out != 0)
                assert (ep.q_of(L.T, L.M, L.S)[ch] != ep.q_of(L.T + L.out, L.M, L.S)[ch]).all(), (L.name, "the pair does not straddle")
                assert L.aimed_mask().reshape(wrap.shape)[:, ch].any(), (L.name, "no aimed value reaches the output")
            launches += 1
            probes += L.probes()
    dropped = sorted(set(ep.DROPPED))
    print("\n%s: %d launches, %d probes within one step of a target; dropped: %s" % (fname, launches, probes, dropped or "none"))
    # every drop is a boundary beyond +-2^30 (none is expected at the multipliers the builder picks) or the fallback channel's forced sign
    assert all(r in ("target beyond +-2^30", "sign forced by zp_w") for *_, r in dropped)
    assert not dropped


def _pack(L):
    return binding.conv_pack(L.wq, L.zp_w, L.fam["c"], 3, L.bias, L.M, L.S, binding.ACT[L.act], L.zp)


@pytest.mark.parametrize("fname", ep.POOLED)
def test_pooled_launches_are_aimed(fname):
    ep.DROPPED.clear()
    launches = probes = narrower = 0
    n = ep.FAMILIES[fname]["n"]
    for act, zp in ACT_ZP:
        for state in ep.STATES:
            Ls, t = ep.pooled_set(fname, act, zp, state, _pack)
            # the launch-wide state, as the table shows it
            assert not (t["flags"] & 1), "EPT_NEVER: see epilogue_points.UNREACHABLE"
            assert bool(t["flags"] & 4) == (state != "notpow2")
            lo_t, hi_t = ep.true_range(Ls[0].M, Ls[0].S, zp, act)
            if state != "notpow2":   # the table's range lies inside the true one (a folded multiplier is meaningless otherwise)
                assert (t["lb"][:n] >= np.maximum(lo_t, -ep.LIM)).all() and (t["lb"][:n] + t["rg"][:n] <= np.minimum(hi_t, ep.LIM - 1)).all()
            if act != ep.LINEAR:
                if state == "int":
                    assert not (t["flags"] & 2) and (t["m0"][:n] == Ls[0].m0).all(), (fname, act, zp, "every channel integer-capable")
                if state == "one-noint":
                    assert (t["flags"] & 2) and np.array_equal(np.flatnonzero(t["m0"][:n] == 0), [Ls[0].odd]), (fname, act, zp, "exactly one channel not")
                if state == "notpow2":
                    assert (t["flags"] & 2) and not t["m0"][:n].any()
            if state == "clamp":
                assert (t["lb"][:n] == -ep.LIM).all() and (t["lb"][:n] + t["rg"][:n] == ep.LIM - 1).all()
            for L in Ls:
                narrower += "-table" in L.name
                if _conv_checked(fname, act, zp):
                    _check_acc(L)
                wrap, sat = _check_bytes(L)
                diff = (wrap != sat)
                aimed = L.aimed_mask().reshape(diff.shape)
                if L.name.endswith("/on"):
                    assert not diff.any(), (L.name, "a launch without outside values wraps")
                else:
                    edge_ch = L.true_edge
                    assert np.array_equal(diff[:, edge_ch], aimed[:, edge_ch]), (L.name, "wrap != saturate is not exactly the aimed set")
                    assert not diff[:, ~edge_ch].any(), (L.name, "a value beside a clamp / a table's end wraps")
                launches += 1
                probes += L.probes()
        if act == ep.LEAKY and zp in (1, 23, 254):
            assert not ep.DROPPED, "no probe may be dropped for the pooled LEAKY families at these zero points"
    dropped = sorted(set(ep.DROPPED))
    print("\n%s: %d launches (%d aimed at a narrower table range), %d probes within one step of a target; dropped: %s"
          % (fname, launches, narrower, probes, dropped or "none"))
    assert not dropped


def test_every_output_channel_is_aimed_on_both_sides():
    """over the `out` launches of a state every output channel has a value one step beyond its upper AND one beyond its lower end"""
    for fname in ep.POOLED:
        n = ep.FAMILIES[fname]["n"]
        up, down = np.zeros(n, bool), np.zeros(n, bool)
        for L in ep.pooled_launches(fname, ep.LEAKY, 23, "int"):
            hit = L.aimed_mask().any(axis=(0, 2, 3))
            up |= hit & (L.out > 0)
            down |= hit & (L.out < 0)
        assert up.all() and down.all(), fname


def test_unreachable_probes_are_listed_with_reasons():
    assert all(len(reason) > 40 for _, reason in ep.UNREACHABLE)
    print("\nunreachable for every family: %s" % [name for name, _ in ep.UNREACHABLE])
