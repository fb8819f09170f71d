"""GPU suite (`-m gpu`): whole networks through the plain-C host in the configurations users and the benchmark run, against OracleNet.

Every net of tests/netgen.py's sweep (seeded random topologies + AIMED, one hand-written net per planner clause) runs at batch 3 with three
distinct images in eight modes (RUNS).  Compared per image, tensor by tensor: int32 accumulators (dump modes), every STORED u8 tensor and
every quant_stop float exactly, yolo floats to atol 2e-7.  `Net.plan` (dnq_layer_plan) is read before and after the forward passes: a fuse
flag that was set before and is clear after was refused by a launcher and re-run unfused.  AIMED_EXPECT asserts, per aimed net, the outcome
its comment names; test_dynamic_coverage asserts that the sweep reached every planner outcome on the device.  Nothing here reads the
reference's sources.

Mutation check (made on the MI355X on scratch copies of the host, not committed).  Mutant 1, view_producer_ok ignoring `zp_differs`: 18 tests
red, every production mode of view_zp_differs (layer 2 u8), shared_route_zp_differs (layer 4 u8) and glue_own_zp.  Mutant 2, the fall-back
of layers.c not clearing fuse_next_upsample: refused_upsample_5x5 red in the default, graph, throughput, replica and nohead modes (layer 2
u8: the executor skipped the upsample the launcher had refused to fuse)."""
import numpy as np
import pytest

import netgen
import oracle
from yolo_quantization_amd import binding, synth

pytestmark = pytest.mark.gpu

NETS = netgen.sweep()
B = 3
# mode -> what it pins
RUNS = {
    "dump": "dump_int32: own buffers, nothing fused; int32 accumulators of every conv, every u8 tensor, every float tail",
    "default": "latency plan: fusions and views on",
    "graph": "the same captured into a graph and replayed twice: refusal / fall-back during capture",
    "throughput": "network_set_plan re-plans the fusions for the throughput plan",
    "nofuse": "fuse_maxpool = 0: views without fusion",
    "replica": "a replica in flight beside its parent on other images: shared packed weights, flags cleared in one executor",
    "ref_f32": "the f32 twin (MI355_ACC_REF_F32) through the host",
    "nohead": "the library's own default keep_head_float = 0: a head fused with its yolo layer does not store its own float tensor",
}
CASES = [(name, mode) for name in NETS for mode in RUNS if not (mode == "ref_f32" and name in netgen.AIMED_BIG)]
FUSE_KEYS = ("fuse_next_pool", "fuse_next_upsample", "fuse_next_shortcut", "fuse_next_yolo")

OBS = {}     # (name, mode) -> observation of the device run (plans, kernels); filled by _device_run
_WANT = {}   # (name, image set, accum) -> oracle outputs per image; a few entries (the cases are ordered by net)


@pytest.fixture(scope="module", autouse=True)
def device():
    binding.init(0)


def _files(tmp_path, name):
    spec = NETS[name]
    cfg = str(tmp_path / f"{name}.cfg")
    with open(cfg, "w") as f:
        f.write(spec["cfg"])
    wts = str(tmp_path / f"{name}.weights")
    synth.synth_weights(cfg, wts, seed=spec["wseed"], act_gain=spec["act_gain"], glue_own_zp=spec["glue_own_zp"])
    return cfg, wts


def _images(name, cfg, which):
    net, _ = synth.layer_shapes(synth.read_cfg(cfg))
    return synth.synth_image_u8(3, int(net["height"]), int(net["width"]), seed=NETS[name]["wseed"] * 2 + which, batch=B)


def _want(name, cfg, wts, which, accum):
    key = (name, which, accum)
    if key not in _WANT:
        while len(_WANT) >= 4:
            _WANT.pop(next(iter(_WANT)))
        onet = oracle.OracleNet(cfg, wts)
        onet.prepare(np.float32(1.0 / 255.0), 0)
        x = _images(name, cfg, which)
        _WANT[key] = [onet.forward(x[b], accum=accum) for b in range(B)]
    return _WANT[key]


def _plans(net):
    return [net.plan(i) for i in range(net.n)]


def _compare(net, want, tag, int32):
    """every stored tensor of `net` against the oracle's per-image outputs"""
    for i, inf in enumerate(net.info):
        got = net.pull(i)
        per = inf["outputs"]
        stored = not (inf["type"] == binding.T_CONV and net.is_fused(i))  # a fused conv's own tensor is not stored
        for b in range(B):
            sl = slice(b * per, (b + 1) * per)
            w = want[b][i]
            if int32 and inf["type"] == binding.T_CONV:
                assert np.array_equal(got["int32"][sl], w["int32"].ravel()), f"{tag}: image {b} layer {i} int32"
            if inf["type"] != binding.T_YOLO and stored:
                assert np.array_equal(got["u8"][sl], w["u8"].ravel()), f"{tag}: image {b} layer {i} u8"
            if inf["type"] == binding.T_YOLO:
                np.testing.assert_allclose(got["f32"][sl], w["f32"].ravel(), rtol=0, atol=2e-7, err_msg=f"{tag}: image {b} layer {i} yolo")
            elif inf["quant_stop"] and "f32" in got:  # (keep_head_float = 0: a head fused with its yolo layer stores no float tensor)
                assert np.array_equal(got["f32"][sl], w["f32"].ravel()), f"{tag}: image {b} layer {i} f32"


def _observe(name, mode, net, before):
    after = _plans(net)
    OBS[(name, mode)] = dict(before=before, after=after, kern=[net.conv_kernel(i) for i in range(net.n)],
                             fuses=[net.fuses_next(i) for i in range(net.n)], info=net.info)
    return OBS[(name, mode)]


def _device_run(name, mode, tmp_path, compare=True):
    cfg, wts = _files(tmp_path, name)
    dump = mode in ("dump", "ref_f32")
    net = binding.Net(cfg, wts, batch=B, accum=binding.ACC_REF_F32 if mode == "ref_f32" else binding.ACC_EXACT, dump_int32=dump,
                      use_graph=mode == "graph", fuse_maxpool=mode != "nofuse", keep_head_float=mode != "nohead")
    net.prepare_fixed(1.0 / 255.0, 0)
    if mode == "throughput":
        net.set("plan", 1)
    x = _images(name, cfg, 0)
    oacc = oracle.ACC_REF_F32 if mode == "ref_f32" else oracle.ACC_EXACT
    try:
        if mode == "replica":
            rep = net.replica()
            try:
                before = _plans(rep)
                x2 = _images(name, cfg, 1)
                rep.push_input(x2); net.push_input(x)
                rep.sync(); net.sync()
                for _ in range(2):
                    rep.forward(); net.forward()
                rep.sync(); net.sync()
                obs = _observe(name, mode, rep, before)
                # the parent was re-planned for the throughput plan when the replica was made and ran the same passes: each executor
                # clears the flags its own launches refused, so both end with the same ones
                parent_after = _plans(net)
                for i, (pa, ra) in enumerate(zip(parent_after, obs["after"])):
                    assert {k: pa[k] for k in FUSE_KEYS} == {k: ra[k] for k in FUSE_KEYS}, f"{name}: layer {i} parent / replica flags"
                if compare:
                    _compare(net, _want(name, cfg, wts, 0, oacc), f"{name} parent", False)
                    _compare(rep, _want(name, cfg, wts, 1, oacc), f"{name} replica", False)
            finally:
                rep.close()  # a parent is freed after its replicas
            return obs
        before = _plans(net)
        net.push_input(x)
        net.forward()
        if mode == "graph":  # the first call warmed up, captured and launched once: two more replays
            net.forward(); net.forward()
        net.sync()
        obs = _observe(name, mode, net, before)
        if compare:
            _compare(net, _want(name, cfg, wts, 0, oacc), f"{name} {mode}", dump)
        return obs
    finally:
        net.close()


def _refused(obs, key):
    """layers whose `key` flag was a candidate before the forward passes and was cleared by the launcher's refusal"""
    return [i for i, (b, a) in enumerate(zip(obs["before"], obs["after"])) if b[key] and not a[key]]


def _taken(obs, key):
    return [i for i, a in enumerate(obs["after"]) if a[key] and obs["fuses"][i]]


def _routes(obs, elided):
    return [i for i, (inf, a) in enumerate(zip(obs["info"], obs["after"]))
            if inf["type"] == binding.T_ROUTE and inf["n"] >= 2 and bool(a["route_elided"]) == elided]


# ------------------------------------------------------------------------------- what each aimed net must show
def _x_view_same_zp(o):
    assert o["after"][3]["route_elided"] == 1 and o["after"][1]["out_view"] and o["after"][2]["out_view"]
    assert (o["after"][2]["view_offset"], o["after"][1]["view_offset"]) == (0, 16)


def _x_view_zp_differs(o):
    assert o["after"][3]["route_elided"] == 0 and not o["after"][1]["out_view"] and not o["after"][2]["out_view"]


def _x_shared_same(o):
    assert o["after"][3]["route_elided"] == 1 and o["after"][3]["out_view"] == 1 and o["after"][5]["route_elided"] == 1
    assert o["after"][3]["view_offset"] == o["after"][1]["view_offset"] == 32 + 16


def _x_shared_differs(o):
    assert o["after"][3]["route_elided"] == 1 and o["after"][3]["out_view"] == 1  # the one-input route still shares layer 1's own tensor
    assert o["after"][5]["route_elided"] == 0 and not o["after"][1]["out_view"]


def _x_view_pool_up(o):
    assert o["after"][5]["route_elided"] == 1 and o["after"][2]["out_view"] and o["after"][4]["out_view"]
    assert (o["after"][4]["view_offset"], o["after"][2]["view_offset"]) == (0, 32)


def _x_glue_own_zp(o):
    assert o["after"][5]["route_elided"] == 0 and not o["after"][2]["out_view"]  # maxpool 2's zero point differs from route 5's, conv 3 is 3x3


def _x_fused_up_window(o):
    assert o["after"][5]["route_elided"] == 1 and o["after"][4]["out_view"] == 1 and o["after"][4]["view_offset"] == 0
    assert o["after"][3]["fuse_next_upsample"] == 1 and o["fuses"][3], "conv 3 stores into the upsample's window"


def _x_pool_keep(o):
    assert o["after"][5]["route_elided"] == 1 and o["after"][1]["out_view"] == 1 and o["after"][4]["view_offset"] == 32
    a = o["after"][1]
    assert (a["fuse_next_pool"], a["fuse_pool_keep"]) == (1, 1) and o["kern"][1] == 4


def _x_pool_keep_throughput(o):
    assert _refused(o, "fuse_next_pool") == [1] and o["after"][5]["route_elided"] == 1


def _x_fused_shortcut(o):
    assert o["after"][5]["route_elided"] == 1 and o["after"][0]["out_view"] == 1 and o["after"][0]["view_offset"] == 16
    assert o["after"][2]["fuse_next_shortcut"] == 1 and o["fuses"][2] and o["kern"][2] == 4


def _x_fused_shortcut_throughput(o):
    assert _refused(o, "fuse_next_shortcut") == [2]


def _x_two_routes(o):
    assert o["after"][3]["route_elided"] == 1 and o["after"][1]["out_view"] == 1 and o["after"][5]["route_elided"] == 0
    assert not o["after"][4]["out_view"]


def _x_same_twice(o):
    assert o["after"][2]["route_elided"] == 0 and not o["after"][1]["out_view"]


def _x_byte_copy(o):
    assert o["after"][3]["route_elided"] == 0


def _x_shortcut_neighbours(o):
    assert o["before"][2]["fuse_next_shortcut"] == 1 and o["before"][4]["fuse_next_shortcut"] == 0
    assert _refused(o, "fuse_next_shortcut") == [2]


def _x_refused(key, layer=1):
    def check(o):
        assert o["before"][layer][key] == 1 and _refused(o, key) == [layer] and o["kern"][layer] == 9 and not o["fuses"][layer]
    return check


def _x_pool_64(o):
    assert o["after"][1]["fuse_next_pool"] == 1 and o["fuses"][1] and o["kern"][1] == 2


def _x_pool_16(o):
    assert o["after"][1]["fuse_next_pool"] == 1 and o["fuses"][1] and o["kern"][1] == 7


def _x_non_candidates(o):
    assert all(not o["before"][i]["fuse_next_pool"] for i in (1, 3))


def _x_kxk_window(o):
    assert o["after"][4]["route_elided"] == 1 and o["after"][2]["out_view"] == 1 and o["after"][2]["view_offset"] == 16
    assert o["kern"][3] == 9 and o["after"][6]["route_elided"] == 0


def _x_cell4(o):
    assert o["kern"][1] == 9 and o["kern"][3] == 9  # the 3-filter layers (a 1x1 and a 3x3 on c = 16 / 32) store plain 4-byte cells: general kernel
    assert o["kern"][2] == 1 and o["kern"][4] == 9  # their readers: the 3-channel 3x3 on the first-layer kernel, the 5x5 on the general one


def _x_up_quant_stop(o):
    assert o["after"][1]["fuse_next_upsample"] == 0 and not o["fuses"][1]


def _x_stride7(o):
    import kxk_geometry
    assert o["kern"][1] == 9 and o["info"][1]["stride"] == 7 and o["info"][1]["c"] == 16
    g = kxk_geometry.conv_kxk_launch(kxk_geometry.Trace(), B, 58, 58, 16, 40, 3, 7, 1)
    assert g["inst"] == (16, 1, 4), "the restated launcher: 128 filters x 64 pixels, four waves along M"


AIMED_EXPECT = {  # name -> {mode: check}; "default" checks also hold under graph capture
    "view_same_zp": {"default": _x_view_same_zp, "nofuse": _x_view_same_zp},
    "view_zp_differs": {"default": _x_view_zp_differs, "nofuse": _x_view_zp_differs},
    "shared_route_same_zp": {"default": _x_shared_same},
    "shared_route_zp_differs": {"default": _x_shared_differs},
    "view_maxpool_upsample": {"default": _x_view_pool_up, "nofuse": _x_view_pool_up},
    "glue_own_zp": {"default": _x_glue_own_zp},
    "fused_upsample_window_s3": {"default": _x_fused_up_window},
    "fused_upsample_window_s4": {"default": _x_fused_up_window},
    "pool_keep_view": {"default": _x_pool_keep, "throughput": _x_pool_keep_throughput, "replica": _x_pool_keep_throughput},
    "fused_shortcut_from_view": {"default": _x_fused_shortcut, "throughput": _x_fused_shortcut_throughput, "replica": _x_fused_shortcut_throughput},
    "producer_in_two_routes": {"default": _x_two_routes},
    "route_same_layer_twice": {"default": _x_same_twice},
    "route_byte_copy": {"default": _x_byte_copy},
    "shortcut_neighbours": {"default": _x_shortcut_neighbours, "replica": _x_shortcut_neighbours},
    "refused_upsample_5x5": {m: _x_refused("fuse_next_upsample") for m in ("default", "throughput", "replica")},
    "refused_shortcut_5x5": {m: _x_refused("fuse_next_shortcut") for m in ("default", "throughput", "replica")},
    "refused_yolo_5x5": {m: _x_refused("fuse_next_yolo") for m in ("default", "throughput", "replica")},
    "refused_pool_padding0": {m: _x_refused("fuse_next_pool") for m in ("default", "throughput", "replica")},
    "pool_64_to_96": {"default": _x_pool_64},
    "pool_16_to_32": {"default": _x_pool_16},
    "pool_non_candidates": {"default": _x_non_candidates},
    "kxk_reads_window": {"default": _x_kxk_window},
    "cell4_conv_feeds_conv": {"default": _x_cell4},
    "fused_upsample_quant_stop": {"default": _x_up_quant_stop},
    "kxk_stride7_wide_m_tile": {m: _x_stride7 for m in ("dump", "default", "throughput", "replica")},
}


def test_every_aimed_net_has_an_expectation():
    assert set(AIMED_EXPECT) == set(netgen.AIMED)


@pytest.mark.parametrize("name,mode", CASES, ids=[f"{n}-{m}" for n, m in CASES])
def test_net_vs_oracle(tmp_path, name, mode):
    """One net of the sweep in one run mode equals OracleNet on every stored tensor of every image; an aimed net also shows the planner
    outcome its comment names."""
    obs = _device_run(name, mode, tmp_path)
    if mode in ("dump", "ref_f32"):  # parity dumps: no view, no fused launch
        assert not any(a["route_elided"] or a["out_view"] for a in obs["after"]) and not any(obs["fuses"])
    if mode == "nofuse":
        assert not any(obs["fuses"])
    if mode == "nohead":  # every head the launcher fused dropped its float tensor, every other quant_stop tensor was compared
        heads = [i for i, inf in enumerate(obs["info"]) if inf["type"] == binding.T_CONV and inf["quant_stop"] and obs["fuses"][i]]
        assert all(obs["after"][i]["fuse_next_yolo"] for i in heads)
    check = AIMED_EXPECT.get(name, {}).get("default" if mode in ("graph", "nohead") else mode)
    if check:
        check(obs)


def test_dynamic_coverage(tmp_path):
    """Over the production runs of the whole sweep the device reached every planner outcome (read through dnq_layer_plan and the kernel
    ids; which copy kernel a refused route takes and whose tensor a general-kernel conv reads are inferred from the cfg's shapes: the
    byte copy when an input other than the last has c % 16 != 0, layer i - 1 as conv i's input): elided, refused (byte and 16-byte copy) and
    shared routes, each fusion taken and each refused by the launcher and re-run unfused, fuse_pool_keep, a fused write into a window, a
    general-kernel conv reading a window, and the kernel families 1, 2, 3, 4, 5, 7 and 9."""
    prod = [(n, m) for n, m in CASES if m in ("default", "graph", "throughput", "replica", "nohead")]
    for n, m in prod:  # runs of this session are reused; a run that was deselected is made up for (without the comparison)
        if (n, m) not in OBS:
            _device_run(n, m, tmp_path, compare=False)
    seen = set()
    for n, m in prod:
        o = OBS[(n, m)]
        info, after = o["info"], o["after"]
        if _routes(o, True):
            seen.add("route_elided")
        for r in _routes(o, False):
            srcs = [int(x) if int(x) >= 0 else r + int(x) for x in netgen.parse(NETS[n]["cfg"])[r][1]["layers"].split(",")]
            seen.add("route_byte_copy" if any(info[s]["out_c"] % 16 for s in srcs[:-1]) else "route_16_byte_copy")
        if any(inf["type"] == binding.T_ROUTE and inf["n"] == 1 and a["route_elided"] for inf, a in zip(info, after)):
            seen.add("route_shared")
        for key in FUSE_KEYS:
            if _taken(o, key):
                seen.add(key + "_taken")
            if _refused(o, key):
                seen.add(key + "_refused")
        for i, a in enumerate(after):
            if info[i]["type"] != binding.T_CONV:
                continue
            seen.add(f"kernel{o['kern'][i]}")
            if a["fuse_next_pool"] and a["fuse_pool_keep"] and o["fuses"][i]:
                seen.add("fuse_pool_keep")
                if a["out_view"]:
                    seen.add("fused_write_into_window")
            if o["fuses"][i] and (a["fuse_next_upsample"] or a["fuse_next_shortcut"] or a["fuse_next_pool"]) and after[i + 1]["out_view"]:
                seen.add("fused_write_into_window")
            if o["kern"][i] == 9 and i > 0 and after[i - 1]["out_view"] and after[i - 1]["view_offset"] > 0:
                seen.add("kxk_reads_window")
    need = {"route_elided", "route_byte_copy", "route_16_byte_copy", "route_shared", "fuse_pool_keep", "fused_write_into_window",
            "kxk_reads_window"} | {k + s for k in FUSE_KEYS for s in ("_taken", "_refused")} | {f"kernel{k}" for k in (1, 2, 3, 4, 5, 7, 9)}
    assert not need - seen, sorted(need - seen)
