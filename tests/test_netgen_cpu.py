"""CPU suite for the network generator of the whole-network sweep (tests/netgen.py): determinism, acceptance by the shape inference and by
the host parser, an oracle run of every net, liveness of the oracle's data and static coverage of the sweep; and the host planner's fusion
candidates (plan_fusion), which the host-only prep leaves readable.  No device.

Mutation check of the planner tests (scratch copies of host/network.c):
  * plan_fusion sets the upsample kind where it should set pool: test_planner_invariants and test_fusion_candidates_are_the_recorded_ones
    are red for every net with a pool candidate (pool_keep_view, refused_pool_padding0, pool_64_to_96, pool_16_to_32 in both, rand135 in
    the first, yolov3-tiny in the second).
  * plan_fusion's shortcut case without `index != i`: nothing goes red, and nothing can.  output_read_elsewhere already answers 1 for a
    conv that is the `from` of any shortcut, the one after it included, so the condition is implied by the one beside it and the plans of
    all nets are the same without it.  With that reader not counted either, conv 4 of shortcut_neighbours becomes a candidate and
    test_fusion_candidates_are_the_recorded_ones[shortcut_neighbours] is red."""
import hashlib
import os

import numpy as np
import pytest

import netgen
import oracle
from yolo_quantization_amd import binding, synth

NETS = netgen.sweep()


def _files(tmp_path, name):
    spec = NETS[name]
    cfg = str(tmp_path / f"{name}.cfg")
    with open(cfg, "w") as f:
        f.write(spec["cfg"])
    wts = str(tmp_path / f"{name}.weights")
    info = synth.synth_weights(cfg, wts, seed=spec["wseed"], act_gain=spec["act_gain"], glue_own_zp=spec["glue_own_zp"])
    return cfg, wts, info


def test_generator_is_deterministic(tmp_path):
    """The same seed gives the same cfg text and the same weights sha256; different seeds give different nets."""
    texts = [netgen.random_net(seed) for seed, _, _ in netgen.SEEDS]
    assert texts == [netgen.random_net(seed) for seed, _, _ in netgen.SEEDS]
    assert len(set(texts)) == len(texts)
    assert [n["cfg"] for n in netgen.sweep().values()] == [n["cfg"] for n in NETS.values()]
    name = f"rand{netgen.SEEDS[1][0]}"
    (tmp_path / "a").mkdir(); (tmp_path / "b").mkdir()
    a, b = _files(tmp_path / "a", name)[2], _files(tmp_path / "b", name)[2]
    assert a["sha256"] == b["sha256"]
    assert hashlib.sha256(open(str(tmp_path / "a" / f"{name}.weights"), "rb").read()).hexdigest() == a["sha256"]


def test_glue_own_zp_is_opt_in(cfg_dir, tmp_path):
    """synth_weights writes the bytes it always wrote unless glue_own_zp is asked for; with it, every glue record keeps its input's scale
    and carries another zero point."""
    cfg = os.path.join(cfg_dir, "yolov3-tiny_quant.cfg")
    a = synth.synth_weights(cfg, str(tmp_path / "a.weights"), seed=5)
    b = synth.synth_weights(cfg, str(tmp_path / "b.weights"), seed=5, glue_own_zp=False)
    c = synth.synth_weights(cfg, str(tmp_path / "c.weights"), seed=5, glue_own_zp=True)
    assert a["sha256"] == b["sha256"] != c["sha256"] and a["bytes"] == c["bytes"]
    _, shapes = synth.layer_shapes(synth.read_cfg(cfg))
    wa, wc = oracle.read_weights(str(tmp_path / "a.weights"), shapes), oracle.read_weights(str(tmp_path / "c.weights"), shapes)
    glue = [i for i, L in enumerate(shapes) if L.type != "conv" and "s_act" in wa[i]]
    assert len(glue) >= 8
    for i in glue:
        assert wc[i]["s_act"] == wa[i]["s_act"] and wc[i]["zp_act"] != wa[i]["zp_act"], i


@pytest.mark.parametrize("name", list(NETS))
def test_net_is_accepted_runs_and_is_alive(tmp_path, name):
    """Every net of the sweep: synth.layer_shapes and the host parser accept it and agree on every shape, the host prep (per-channel
    integers, packing: every conv shape is admitted) runs without a device, OracleNet runs one image, and no conv layer of the oracle's
    run is dead: its most frequent output byte covers at most 75 % of the elements."""
    cfg, wts, _ = _files(tmp_path, name)
    _, shapes = synth.layer_shapes(synth.read_cfg(cfg))
    net = binding.Net(cfg, wts)
    net.prepare_host_only(1.0 / 255.0, 0)
    assert net.n == len(shapes)
    onet = oracle.OracleNet(cfg, wts)
    onet.prepare(np.float32(1.0 / 255.0), 0)
    for i, (L, inf) in enumerate(zip(shapes, net.info)):
        assert (inf["out_c"], inf["out_h"], inf["out_w"]) == (L.out_c, L.out_h, L.out_w), i
        if L.type == "conv":
            assert np.array_equal(net.prep(i)["biases_int32"], onet.p[i]["biases_int32"]), i
            assert net.prep(i)["zp_in"] == onet.p[i]["zp_in"], i
    net.close()
    x = synth.synth_image_u8(3, int(onet.netopt["height"]), int(onet.netopt["width"]), seed=5)
    outs = onet.forward(x)
    for i, (L, o) in enumerate(zip(shapes, outs)):
        if L.type == "conv":
            u = o["u8"].ravel()
            top = np.bincount(u, minlength=256).max() / u.size
            assert top <= 0.75, f"layer {i}: byte {np.bincount(u).argmax()} covers {top:.2f} of the tensor"


def test_wrapping_stores_occur_for_every_activation(tmp_path):
    """For each activation some net of the sweep has a conv layer whose wrapped store differs from the saturated one, so the device's
    STORE_WRAP epilogues are compared on bytes that wrapped."""
    wraps = set()
    for name, spec in NETS.items():
        if spec["act_gain"] == 1.0 or name in netgen.AIMED_BIG:
            continue
        cfg, wts, _ = _files(tmp_path, name)
        onet = oracle.OracleNet(cfg, wts)
        onet.prepare(np.float32(1.0 / 255.0), 0)
        x = synth.synth_image_u8(3, int(onet.netopt["height"]), int(onet.netopt["width"]), seed=5)
        for i, (L, o) in enumerate(zip(onet.layers, onet.forward(x))):
            if L.type == "conv" and L.activation not in wraps:
                p = onet.p[i]
                sat = oracle.requant(o["int32"], p["biases_int32"], p["M_value"], p["shift_value"], onet.w[i]["zp_act"],
                                     oracle.ACT[L.activation], oracle.STORE_SATURATE)
                if not np.array_equal(sat.ravel(), o["u8"].ravel()):
                    wraps.add(L.activation)
    assert wraps == set(netgen.ACTS)


def test_static_coverage_of_the_sweep(tmp_path):
    """Counted from the cfg texts alone: every conv size, stride, padding form, filter count, activation, pool geometry, upsample stride,
    route arity / index form / sharing, shortcut source, quant_stop tail and head count of the specification occurs in the sweep."""
    have = set()
    sums = []
    for name, spec in NETS.items():
        have |= netgen.features(spec["cfg"])
        cfg = str(tmp_path / f"{name}.cfg")
        with open(cfg, "w") as f:
            f.write(spec["cfg"])
        _, shapes = synth.layer_shapes(synth.read_cfg(cfg))
        sums += [L.out_c for L in shapes if L.type == "route" and len(L.inputs) > 1]
        assert not any(sec == "shortcut" and int(o.get("first_time", 0)) for sec, o in netgen.parse(spec["cfg"]))
    rand = set().union(*(netgen.features(netgen.random_net(seed)) for seed, _, _ in netgen.SEEDS))
    assert {"upsample4", "quant_stop_upsample", "pool_64_to_64_128", "maxpool_on_odd_map", "maxpool_on_even_map"} <= rand  # not left to AIMED alone
    missing = [f for f in netgen.REQUIRED_FEATURES if f not in have]
    assert not missing, missing
    assert any(s % 16 == 0 for s in sums) and any(s % 16 for s in sums)  # concatenations that are and are not multiples of 16
    assert len(netgen.AIMED) >= 12 and all(a["clause"] for a in netgen.AIMED.values())


KINDS = {"fuse_next_pool": "pool", "fuse_next_upsample": "upsample", "fuse_next_shortcut": "shortcut", "fuse_next_yolo": "yolo"}
NEXT_TYPE = {"pool": binding.T_MAXPOOL, "upsample": binding.T_UPSAMPLE, "shortcut": binding.T_SHORTCUT, "yolo": binding.T_YOLO}


def _candidates(cfg, wts):
    """(layer index -> kind, "pool+keep" for a pool with fuse_pool_keep) as Net.plan shows it after the host-only prep, with the
    invariants every plan keeps checked on the way."""
    net = binding.Net(cfg, wts)
    net.prepare_host_only(1.0 / 255.0, 0)
    got = {}
    for i in range(net.n):
        p = net.plan(i)
        kinds = [kind for key, kind in KINDS.items() if p[key]]
        assert len(kinds) <= 1, (i, p)
        assert not p["fuse_pool_keep"] or p["fuse_next_pool"], (i, p)
        if kinds:
            assert net.info[i]["type"] == binding.T_CONV and i + 1 < net.n and net.info[i + 1]["type"] == NEXT_TYPE[kinds[0]], (i, p)
            got[i] = kinds[0] + ("+keep" if p["fuse_pool_keep"] else "")
    net.close()
    return got


@pytest.mark.parametrize("name", list(NETS))
def test_planner_invariants(tmp_path, name):
    """Every net of the sweep after the host-only prep: a layer carries at most one fusion kind, a kind sits on a conv whose successor has
    the matching type, and fuse_pool_keep comes only with the pool kind."""
    cfg, wts, _ = _files(tmp_path, name)
    _candidates(cfg, wts)


# The planner's candidates as the commit before the single fuse_next field gave them (recorded from a build of that commit, with only
# plan_fusion's call moved into the host prep): layer index -> kind.
CANDIDATES = {
    "view_same_zp": {5: "yolo"},
    "view_zp_differs": {5: "yolo"},
    "shared_route_same_zp": {7: "yolo"},
    "shared_route_zp_differs": {7: "yolo"},
    "view_maxpool_upsample": {7: "yolo"},
    "glue_own_zp": {9: "yolo"},
    "fused_upsample_window_s3": {3: "upsample", 7: "yolo"},
    "fused_upsample_window_s4": {3: "upsample", 7: "yolo"},
    "pool_keep_view": {1: "pool+keep", 7: "yolo"},
    "fused_shortcut_from_view": {2: "shortcut", 6: "yolo"},
    "producer_in_two_routes": {6: "yolo"},
    "route_same_layer_twice": {4: "yolo"},
    "route_byte_copy": {5: "yolo"},
    "shortcut_neighbours": {2: "shortcut", 6: "yolo"},
    "refused_upsample_5x5": {1: "upsample", 3: "yolo"},
    "refused_shortcut_5x5": {1: "shortcut", 3: "yolo"},
    "refused_yolo_5x5": {1: "yolo"},
    "refused_pool_padding0": {1: "pool", 3: "yolo"},
    "pool_64_to_96": {1: "pool", 3: "yolo"},
    "pool_16_to_32": {1: "pool", 3: "yolo"},
    "pool_non_candidates": {5: "yolo"},
    "kxk_reads_window": {},
    "cell4_conv_feeds_conv": {5: "yolo"},
    "fused_upsample_quant_stop": {3: "yolo"},
    "kxk_stride7_wide_m_tile": {},
    "cfg/yolov3-tiny_quant.cfg": {0: "pool", 2: "pool", 4: "pool", 6: "pool", 8: "pool+keep", 10: "pool", 15: "yolo", 18: "upsample", 22: "yolo"},
    "cfg/yolov3_quant.cfg": {**{i: "shortcut" for i in (3, 7, 10, 14, 17, 20, 23, 26, 29, 32, 35, 39, 42, 45, 48, 51, 54, 57, 60, 64, 67, 70, 73)},
                             81: "yolo", 84: "upsample", 93: "yolo", 96: "upsample", 105: "yolo"},
    "cfg/res_unit.cfg": {2: "shortcut", 6: "shortcut", 8: "upsample", 13: "yolo"},
}


def test_candidate_table_covers_every_aimed_net():
    assert set(netgen.AIMED) <= set(CANDIDATES)


@pytest.mark.parametrize("name", list(CANDIDATES))
def test_fusion_candidates_are_the_recorded_ones(cfg_dir, tmp_path, name):
    """plan_fusion marks exactly the recorded (layer, kind) pairs in every aimed net of the sweep and in the shipped yolov3-tiny, yolov3
    and residual-unit nets."""
    if name.startswith("cfg/"):
        cfg = os.path.join(cfg_dir, name[4:])
        wts = str(tmp_path / "shipped.weights")
        synth.synth_weights(cfg, wts, seed=1)
    else:
        cfg, wts, _ = _files(tmp_path, name)
    assert _candidates(cfg, wts) == CANDIDATES[name]
