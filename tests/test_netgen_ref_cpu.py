"""CPU suite for tests/golden/netgen_ref.json: the tensors of the whole-network sweep (tests/netgen.py) as the reference itself computed
them (tests/golden/make_golden_netgen.py).  No device.

The chain is reference -> file -> {oracle, device}.  Here: the file's inputs are reproducible; OracleNet in its bit-faithful mode
(ACC_REF_F32) reproduces every hash of every net, image and layer; the exact integers (ACC_EXACT), teacher-forced with the reference's
own layer inputs, reproduce the masked hashes and the low-range tensors; orc_yolo_detections reproduces the reference's records; the
product's host prep reproduces the reference's per-channel integers; the pool and upsample restatements reproduce the one-layer nets; and
where the reference is built, a live run of it reproduces the file byte for byte.  tests/test_gpu_netgen_ref.py is the device's half.

The reference runs the TWIN of a net (netgen.reference_twin): it has no integer [shortcut], so the features of
netgen.SHORTCUT_FEATURES are pinned by the oracle alone (tests/test_gpu_residual.py, tests/test_gpu_random_nets.py)."""
import os
import sys

import numpy as np
import pytest

import glue_edges
import netgen
import netgen_ref as nr
import oracle
import refdrv
from yolo_quantization_amd import binding, synth

G = nr.load()
NETS = netgen.ref_sweep()


# ------------------------------------------------------------------------------------------------ the twins
def test_twin_replaces_shortcuts_only():
    """A twin has a one-input route where the net has a shortcut, with its quantized / quant_stop lines, and every other line as it was:
    same section count, same shape of every layer."""
    some = 0
    for name, spec in netgen.sweep().items():
        twin = netgen.reference_twin(spec["cfg"])
        a, b = netgen.parse(spec["cfg"]), netgen.parse(twin)
        assert len(a) == len(b)
        for i, ((ta, oa), (tb, ob)) in enumerate(zip(a, b)):
            if ta == "shortcut":
                assert tb == "route" and ob == {"layers": "-1", "quantized": oa["quantized"], "quant_stop": oa["quant_stop"]}, (name, i)
                some += 1
            else:
                assert (ta, oa) == (tb, ob), (name, i)
        if "[shortcut]" not in spec["cfg"]:
            assert twin == spec["cfg"]
        assert netgen._map_sizes(twin, b) == netgen._map_sizes(spec["cfg"], a)
    assert some >= 19
    assert set(NETS) == (set(netgen.sweep()) - set(netgen.AIMED_BIG)) | set(netgen.REF_EXTRA) == set(G["nets"])


def test_twins_keep_every_feature_but_the_shortcuts():
    """features() over the twins reaches every entry of REQUIRED_FEATURES except the four that name shortcuts."""
    have = set().union(*(netgen.features(spec["cfg"]) for spec in NETS.values()))
    lost = [f for f in netgen.REQUIRED_FEATURES if f not in have]
    assert sorted(lost) == sorted(netgen.SHORTCUT_FEATURES), lost
    # won for the twin list by REF_EXTRA: a quant_stop route whose inputs carry different records (no net of the sweep has one, so a
    # route tail dequantised with one record for all inputs passed every test; found by mutating the host)
    assert "quant_stop_route_mixed_records" in have


# ------------------------------------------------------------------------------- floor against truncation
SHORT_POOLS = [(3, 3, 0, 1, 1), (5, 4, 1, 2, 3), (3, 3, 1, 1, 1), (5, 3, 2, 2, 3), (2, 2, 0, 1, 1), (5, 4, 0, 2, 3)]  # size, stride, padding, h, w


def test_pool_shorter_than_its_window_has_one_output_row(tmp_path):
    """h + padding < size: C's truncating division gives one output row (ref: src/maxpool_layer.c:31-32, host/layers.c), Python's floor
    gives none.  synth.layer_shapes, netgen's own shape tracking, the host parser, the oracle and the file (the shapes the reference's
    parser reported) agree on every such pool of the one-layer nets."""
    pools = netgen.pool_nets()
    short = {n: g for n, (_, g) in pools.items() if g[3] + g[2] < g[0] or g[4] + g[2] < g[0]}
    assert {g for g in short.values()} >= set(SHORT_POOLS) and len(short) >= 20
    for name, (size, stride, padding, h, w) in short.items():
        cfg, wts, _ = nr.write_model(tmp_path, name, pools[name][0], netgen.ONE_LAYER_WSEED)
        _, shapes = synth.layer_shapes(synth.read_cfg(cfg))
        want = (glue_edges.pool_out(h, size, stride, padding), glue_edges.pool_out(w, size, stride, padding))
        assert (h + padding - size) // stride + 1 < want[0] or (w + padding - size) // stride + 1 < want[1], "floor and truncation differ here"
        assert (shapes[1].out_h, shapes[1].out_w) == want
        assert netgen._map_sizes(pools[name][0], netgen.parse(pools[name][0]))[1] == want
        net = binding.Net(cfg, wts)
        assert (net.info[1]["out_h"], net.info[1]["out_w"]) == want
        net.close()
        assert G["one_layer"][name]["shapes"][1] == [17, want[0], want[1]], "the reference's parser"
        assert oracle.maxpool_u8(np.zeros((17, h, w), np.uint8), size, stride, padding).shape == (17,) + want


# ----------------------------------------------------------------------------------------- the file, net by net
@pytest.mark.parametrize("name", list(NETS))
def test_oracle_and_host_prep_reproduce_the_reference(tmp_path, name):
    """One net of the file: its cfg, weights and images are reproducible; OracleNet(ACC_REF_F32) has the reference's hash on every int32,
    uint8 and float tensor of both images; with the reference's own layer inputs the exact integers have the reference's masked hashes
    (the plain ones where the mask is whole) and its low-range tensors; orc_yolo_detections has its records; the product's host prep
    has its per-channel integers."""
    spec, g = NETS[name], G["nets"][name]
    assert nr.text_hash(spec["cfg"]) == g["cfg"]
    cfg, wts, wsha = nr.write_model(tmp_path, name, spec["cfg"], spec["wseed"], spec["act_gain"], spec["glue_own_zp"])
    assert wsha == g["weights"]
    sections = synth.read_cfg(cfg)
    netopt, layers = synth.layer_shapes(sections)
    H, W = int(netopt["height"]), int(netopt["width"])
    onet = oracle.OracleNet(cfg, wts)
    onet.prepare(np.float32(1.0 / 255.0), 0)
    hnet = binding.Net(cfg, wts)
    hnet.prepare_host_only(1.0 / 255.0, 0)
    convs = [i for i, L in enumerate(layers) if L.type == "conv"]
    assert sorted(g["prep"], key=int) == [str(i) for i in convs]
    for i in convs:
        assert nr.prep_hash(hnet.prep(i)) == g["prep"][str(i)], f"layer {i}: host prep"
        assert nr.prep_hash(onet.p[i]) == g["prep"][str(i)], f"layer {i}: oracle prep"
    hnet.close()
    inexact = set()
    for rec, seed in zip(g["images"], netgen.REF_IMAGE_SEEDS):
        x = synth.synth_image_u8(3, H, W, seed=seed)
        assert rec["seed"] == seed and nr.h128(x) == rec["input"]
        outs = onet.forward(x, accum=oracle.ACC_REF_F32)
        assert len(outs) == len(rec["layers"])
        for i, (L, o, e) in enumerate(zip(layers, outs, rec["layers"])):
            tag = f"image seed {seed} layer {i} ({L.type})"
            assert e["t"] == L.type
            assert ("i32" in e) == (L.type == "conv") and ("u8" in e) == (L.type != "yolo") and ("f32" in e) == bool(L.quant_stop or L.type == "yolo"), \
                f"{tag}: a tensor of this layer is pinned by nothing"
            if "i32" in e:
                assert nr.h128(o["int32"]) == e["i32"], f"{tag}: int32"
            if "u8" in e:
                assert nr.h128(o["u8"]) == e["u8"], f"{tag}: uint8"
            if "f32" in e:
                assert nr.h128(o["f32"]) == e["f32"], f"{tag}: float"
        # teacher forcing: the exact integers on the reference's own layer inputs (the oracle's, verified by hash just above)
        ins = nr.conv_inputs(layers, x, lambda i: outs[i]["u8"])
        for i in convs:
            L, p, d, e = layers[i], onet.p[i], onet.w[i], rec["layers"][i]
            ex, mask = nr.exact_mask(ins[i], d, L, p["zp_in"])
            u8 = oracle.requant(ex, p["biases_int32"], p["M_value"], p["shift_value"], d["zp_act"], oracle.ACT[L.activation])
            if mask.all():
                assert "mask" not in e and nr.h128(ex) == e["i32"] and nr.h128(u8) == e["u8"], f"image seed {seed} layer {i}: exact integers"
            else:
                inexact.add(i)
                assert nr.mask_fields(mask, ex, u8) == e["mask"], f"image seed {seed} layer {i}: exact integers inside the mask"
        for i, L in enumerate(layers):
            if L.type == "yolo":
                anchors, ymask, classes = nr.yolo_params(sections[i + 1])
                for (imw, imh, rel, th), want in zip(nr.DET_CALLS, rec["det"][str(i)]):
                    cnt, recs = oracle.yolo_detections(outs[i]["f32"].ravel(), L.n, classes, L.h, L.w, anchors, ymask, W, H, imw, imh, th, rel)
                    nr.assert_det_fields(cnt, recs, want, f"image seed {seed} yolo layer {i} call {(imw, imh, rel, th)}")
        assert sorted(rec["det"], key=int) == [str(i) for i, L in enumerate(layers) if L.type == "yolo"]
    assert g["all_exact"] == (not inexact) and sorted(g["lowrange"], key=int) == [str(i) for i in sorted(inexact)]
    for key, lr in g["lowrange"].items():
        i = int(key)
        L, p, d = layers[i], onet.p[i], onet.w[i]
        ex = oracle.conv_acc(nr.lowrange_input(L, lr), d["wq"], d["zp_w"], L.size, L.stride, L.pad, p["zp_in"], oracle.ACC_EXACT)
        u8 = oracle.requant(ex, p["biases_int32"], p["M_value"], p["shift_value"], d["zp_act"], oracle.ACT[L.activation])
        assert nr.h128(ex) == lr["i32"] and nr.h128(u8) == lr["u8"], f"layer {i}: low-range vector"


# ------------------------------------------------------------------------------------------ the one-layer nets
def test_pool_and_upsample_restatements_reproduce_the_one_layer_nets(tmp_path):
    """Every one-pool and one-upsample net of the file: OracleNet, oracle.maxpool_u8 / upsample_u8 and glue_edges.maxpool_ref /
    upsample_ref on the conv's tensor give one result, of the shape the reference's parser reported and with the reference's hash."""
    pools, ups = netgen.pool_nets(), netgen.upsample_nets()
    assert set(pools) | set(ups) == set(G["one_layer"])
    geoms = {g[:3] for _, g in pools.values()}
    assert geoms == {(k, s, p) for k in (1, 2, 3, 5) for s in (1, 2, 3, 4) for p in range(k + 2)}
    assert {g[0] for _, g in ups.values()} == {1, 2, 3, 4}
    for name, (text, geom) in {**pools, **ups}.items():
        g = G["one_layer"][name]
        cfg, wts, wsha = nr.write_model(tmp_path, "one", text, netgen.ONE_LAYER_WSEED)
        assert wsha == g["weights"] and list(geom) == g["geom"]
        netopt, layers = synth.layer_shapes(synth.read_cfg(cfg))
        assert [[L.out_c, L.out_h, L.out_w] for L in layers[:3]] == g["shapes"], name
        onet = oracle.OracleNet(cfg, wts)
        onet.prepare(np.float32(1.0 / 255.0), 0)
        for seed, want in zip(netgen.REF_IMAGE_SEEDS, g["u8"]):
            x = synth.synth_image_u8(3, int(netopt["height"]), int(netopt["width"]), seed=seed)
            outs = onet.forward(x, accum=oracle.ACC_REF_F32)
            assert nr.h128(np.concatenate([outs[i]["u8"].ravel() for i in range(2)])) == want, name
            c = outs[0]["u8"]
            if name in pools:
                size, stride, padding = geom[:3]
                a, b = oracle.maxpool_u8(c, size, stride, padding), glue_edges.maxpool_ref(c[None], size, stride, padding)[0]
            else:
                a, b = oracle.upsample_u8(c, geom[0]), glue_edges.upsample_ref(c[None], geom[0])[0]
            assert np.array_equal(a, outs[1]["u8"]) and np.array_equal(b, outs[1]["u8"]), name


# ------------------------------------------------------------------------------------------------- the live reference
@pytest.mark.skipif(not refdrv.available(), reason="oracle/_ref is not built")
def test_live_reference_reproduces_the_file():
    """The reference, run now (every net in a child process of its own: it aborts where it should refuse), writes the committed file
    byte for byte."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_golden_netgen
    with open(nr.PATH) as f:
        assert make_golden_netgen.dumps(make_golden_netgen.generate()) == f.read()


# ---------------------------------------------------------------------------------------------------------- coverage
def test_coverage_conditions():
    """Stated, not measured.  At least 9 in 10 conv layers of the twin sweep are wholly inside the fp32-exact mask on both images, so
    the reference's plain hashes pin the exact-integer kernels there.  Every other conv layer has a low-range vector on which the
    reference was exact on every element; its input is alive (not all zero) except where the pad taps alone pass 2^24, the layers of
    PADS_ALONE_OVERFLOW, which keep their masked hashes and the f32 twin.  The file is no larger than the largest fixture before it."""
    convs = whole = 0
    pads_alone = set()
    for name, g in G["nets"].items():
        idx = [i for i, e in enumerate(g["images"][0]["layers"]) if e["t"] == "conv"]
        for i in idx:
            convs += 1
            partial = any("mask" in rec["layers"][i] for rec in g["images"])
            whole += not partial
            assert partial == (str(i) in g["lowrange"]), f"{name} layer {i} is pinned by nothing on the exact path"
            if partial:
                lr = g["lowrange"][str(i)]
                assert 5 <= lr["shift"] <= 8 and (lr["in_mask"] or lr["shift"] == 8)
                if lr["shift"] == 8:
                    pads_alone.add((name, i))
        assert g["all_exact"] == (not g["lowrange"])
    assert convs >= 340 and whole * 10 >= convs * 9, (whole, convs)
    assert pads_alone == PADS_ALONE_OVERFLOW
    assert sum(g["all_exact"] for g in G["nets"].values()) >= 25
    assert os.path.getsize(nr.PATH) <= 352273


# conv layers with a zero point of 128 (or a glue layer's own) in front and a window that always reaches over the border of a small map:
# K * zp_in * 255 is past 2^24 whatever the input holds
PADS_ALONE_OVERFLOW = {("rand30", 9), ("rand30", 25), ("rand36", 7), ("rand36", 17), ("rand36", 20)}
