"""GPU suite (`-m gpu`): the whole-network sweep (tests/netgen.py) on the device against the tensors THE REFERENCE computed for it
(tests/golden/netgen_ref.json, written by tests/golden/make_golden_netgen.py running the reference; CPU half and the file's own
checks: tests/test_netgen_ref_cpu.py).  The chain is reference -> file -> device: what is asserted here is a hash of the reference's.

  * f32 twin: every net through the plain-C host with MI355_ACC_REF_F32 and dump_int32 at batch 3, the two images alternating over the
    slots: every int32, uint8 and quant_stop float tensor has the reference's hash; the device's box decode has the reference's records.
  * `all_exact` nets (every conv layer wholly inside the fp32-exact mask, so the reference's tensors ARE the exact integers): the
    production exact kernels in the sweep's run modes (RUNS), every stored tensor against the same hashes, and the box decode.
  * the other nets, teacher-forced layer by layer through binding.conv_forward: each conv on the reference's own input, masked (or,
    where the mask is whole, plain) int32 / uint8 hashes at batch 1 with dumps and at batch TEACHER_B without, under both plans; the
    low-range vectors on the whole tensor.  test_teacher_forced_layers_reach_the_sweeps_kernels asserts the kernel ids they reach.
  * the one-pool and one-upsample nets through the host.

Two things no hash of the file can pin on the device, and what stands in.  A yolo layer's floats: the device's logistic is within 2e-7 of
the reference's, not bit-equal (test_gpu_random_nets.py's rule), so they are compared, at that bound, with the reference's tensor as the
oracle rebuilds it -- verified against the file's hash before use, as is every teacher-forced layer input.  Integer [shortcut]s: the
reference has none, the file holds the twins (netgen.reference_twin), so netgen.SHORTCUT_FEATURES rest on the oracle alone.

Mutation check (made on the MI355X on a scratch copy of the host, not committed; profiles/netgen_ref_mutant_route_tail.log):
forward_route_layer_quant_gpu dequantising every input of a quant_stop route with the route's own record.  All 228 tests of the sweep's
own nets stayed green -- none has such a route with differing records -- which is why netgen.REF_EXTRA adds
route_quant_stop_mixed_records to the reference's list; its seven cases are red under the mutant.

Nothing here reads the reference's sources or needs oracle/_ref."""
import numpy as np
import pytest

import netgen
import netgen_ref as nr
import oracle
from yolo_quantization_amd import binding, synth

pytestmark = pytest.mark.gpu

G = nr.load()
NETS = netgen.ref_sweep()
B = 3                # host runs: slot b holds image b % 2
TEACHER_B = 32       # teacher-forced production runs: identical images, enough of them for the tile plans of a full batch
RUNS = {  # the sweep's run modes (test_gpu_random_nets.RUNS) on the all_exact nets
    "dump": "dump_int32: own buffers, nothing fused; the int32 accumulators too",
    "default": "latency plan: fusions and views on",
    "graph": "the same captured into a graph and replayed twice",
    "throughput": "network_set_plan re-plans the fusions for the throughput plan",
    "nofuse": "fuse_maxpool = 0: views without fusion",
    "nohead": "keep_head_float = 0: a head fused with its yolo layer does not store its own float tensor",
}
CASES = []
for _n, _g in G["nets"].items():
    CASES.append((_n, "ref_f32"))
    CASES += [(_n, m) for m in RUNS] if _g["all_exact"] else [(_n, "teacher")]

_MODEL, _REF = {}, {}
KERNELS = {}   # (net, layer) -> kernel ids that served it teacher-forced


@pytest.fixture(scope="module", autouse=True)
def device():
    binding.init(0)


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("netgen_ref")


def _model(workdir, name):
    if name not in _MODEL:
        spec, g = NETS[name], G["nets"][name]
        assert nr.text_hash(spec["cfg"]) == g["cfg"]
        cfg, wts, wsha = nr.write_model(workdir, name, spec["cfg"], spec["wseed"], spec["act_gain"], spec["glue_own_zp"])
        assert wsha == g["weights"]
        sections = synth.read_cfg(cfg)
        netopt, layers = synth.layer_shapes(sections)
        _MODEL[name] = (cfg, wts, sections, layers, int(netopt["height"]), int(netopt["width"]))
    return _MODEL[name]


def _images(name, H, W):
    xs = [synth.synth_image_u8(3, H, W, seed=s) for s in netgen.REF_IMAGE_SEEDS]
    for x, rec in zip(xs, G["nets"][name]["images"]):
        assert nr.h128(x) == rec["input"]
    return xs


def _reference_tensors(workdir, name):
    """per image the reference's tensors of every layer, rebuilt by the oracle's bit-faithful mode and verified, tensor by tensor,
    against the file's hashes (the cases are ordered by net: two entries are kept)"""
    if name not in _REF:
        while len(_REF) >= 2:
            _REF.pop(next(iter(_REF)))
        cfg, wts, _, layers, H, W = _model(workdir, name)
        onet = oracle.OracleNet(cfg, wts)
        onet.prepare(np.float32(1.0 / 255.0), 0)
        per = []
        for x, rec in zip(_images(name, H, W), G["nets"][name]["images"]):
            outs = onet.forward(x, accum=oracle.ACC_REF_F32)
            for i, (o, e) in enumerate(zip(outs, rec["layers"])):
                for key, field in (("int32", "i32"), ("u8", "u8"), ("f32", "f32")):
                    if field in e:
                        assert nr.h128(o[key]) == e[field], f"{name} layer {i}: the rebuilt {key} tensor is not the reference's"
            per.append(outs)
        _REF[name] = (onet, per)
    return _REF[name]


# ------------------------------------------------------------------------------------------- whole nets through the host
def _compare(net, name, want, tag, int32):
    """every stored tensor of `net`, slot by slot, against the file's hashes of image b % 2"""
    recs = G["nets"][name]["images"]
    for i, inf in enumerate(net.info):
        got = net.pull(i)
        per = inf["outputs"]
        stored = not (inf["type"] == binding.T_CONV and net.is_fused(i))  # a fused conv's own tensor is not stored
        for b in range(B):
            sl = slice(b * per, (b + 1) * per)
            e = recs[b % 2]["layers"][i]
            if int32 and inf["type"] == binding.T_CONV:
                assert nr.h128(got["int32"][sl]) == e["i32"], f"{tag}: slot {b} layer {i} int32"
            if inf["type"] != binding.T_YOLO and stored:
                assert nr.h128(got["u8"][sl]) == e["u8"], f"{tag}: slot {b} layer {i} u8"
            if inf["type"] == binding.T_YOLO:
                np.testing.assert_allclose(got["f32"][sl], want[b % 2][i]["f32"].ravel(), rtol=0, atol=2e-7, err_msg=f"{tag}: slot {b} layer {i} yolo")
            elif inf["quant_stop"] and "f32" in got:  # (keep_head_float = 0: a head fused with its yolo layer stores no float tensor)
                assert nr.h128(got["f32"][sl]) == e["f32"], f"{tag}: slot {b} layer {i} f32"


def _detections(net, name, sections, tag):
    """Net.detections_batch at DET_CALLS against the reference's get_yolo_detections records of every head; a net whose heads differ in
    class count is refused by the batched call (network_detections_batch_shape) and goes head by head through Net.detections"""
    heads = [i for i, inf in enumerate(net.info) if inf["type"] == binding.T_YOLO]
    classes = [nr.yolo_params(sections[i + 1])[2] for i in heads]
    recs_of = G["nets"][name]["images"]
    for k, (imw, imh, rel, th) in enumerate(nr.DET_CALLS):
        if len(set(classes)) == 1:
            counts, offsets, recs = net.detections_batch(imw, imh, th, rel)
            for b in range(B):
                at = int(offsets[b])
                for hk, i in enumerate(heads):
                    cnt = int(counts[b, hk])
                    nr.assert_det_fields(cnt, recs[at:at + cnt], recs_of[b % 2]["det"][str(i)][k], f"{tag}: slot {b} head {i} call {k}")
                    at += cnt
                assert at == offsets[b + 1]
        else:
            with pytest.raises(binding.MI355Error):
                net.detections_shape()
            for i, cl in zip(heads, classes):
                cand = net.info[i]["outputs"] // (cl + 5)
                counts, recs = net.detections(i, cl, imw, imh, th, rel, cand)
                for b in range(B):
                    cnt = int(counts[b])
                    nr.assert_det_fields(cnt, recs[b, :cnt], recs_of[b % 2]["det"][str(i)][k], f"{tag}: slot {b} head {i} call {k}")


def _host_run(workdir, name, mode):
    cfg, wts, sections, layers, H, W = _model(workdir, name)
    _, want = _reference_tensors(workdir, name)
    dump = mode in ("dump", "ref_f32")
    net = binding.Net(cfg, wts, batch=B, accum=binding.ACC_REF_F32 if mode == "ref_f32" else binding.ACC_EXACT, dump_int32=dump,
                      use_graph=mode == "graph", fuse_maxpool=mode != "nofuse", keep_head_float=mode != "nohead")
    try:
        net.prepare_fixed(1.0 / 255.0, 0)
        if mode == "throughput":
            net.set("plan", 1)
        xs = _images(name, H, W)
        net.push_input(np.stack([xs[b % 2] for b in range(B)]))
        net.forward()
        if mode == "graph":  # the first call warmed up, captured and launched once: two more replays
            net.forward(); net.forward()
        net.sync()
        assert [(inf["out_c"], inf["out_h"], inf["out_w"]) for inf in net.info] == [(L.out_c, L.out_h, L.out_w) for L in layers]
        _compare(net, name, want, f"{name} {mode}", dump)
        _detections(net, name, sections, f"{name} {mode}")
        if dump:
            assert not any(net.fuses_next(i) for i in range(net.n))
    finally:
        net.close()


# ------------------------------------------------------------------------------------ teacher-forced, layer by layer
def _run_conv(xin, L, d, p, batch, want_acc, plan=0):
    xb = np.broadcast_to(xin[None], (batch,) + xin.shape)
    xt = binding.DevTensor.from_nchw(xb, p["zp_in"])
    got = binding.conv_forward(xt, d["wq"], d["zp_w"], L.size, p["biases_int32"], p["M_value"], p["shift_value"], p["zp_in"], d["zp_act"],
                               d["s_act"], binding.ACT[L.activation], binding.STORE_WRAP, binding.ACC_EXACT, want_acc=want_acc, want_f32=False,
                               stride=L.stride, pad=L.pad, plan=plan, epilogue=not want_acc)
    return got, binding.last_conv_kernel()


def _pin_conv(xin, L, d, p, want, mask, tag, seen):
    """conv L on input xin: the dump path at batch 1 (int32 and bytes) and the production path at batch TEACHER_B under both plans
    (bytes) against `want` = (int32 hash, u8 hash) of the reference, masked where `mask` is given"""
    def hashes(acc, u8):
        if mask is None:
            return (nr.h128(acc) if acc is not None else None), nr.h128(u8)
        return (nr.h128(np.where(mask, acc.reshape(mask.shape), 0).astype(np.int32)) if acc is not None else None,
                nr.h128(np.where(mask, u8.reshape(mask.shape), 0).astype(np.uint8)))
    got, kern = _run_conv(xin, L, d, p, 1, want_acc=True)
    seen.add(kern)
    assert hashes(got["int32"], got["u8"]) == want, f"{tag}: dump path (kernel {kern}) vs the reference"
    for plan in (0, 1):
        fast, kern = _run_conv(xin, L, d, p, TEACHER_B, want_acc=False, plan=plan)
        seen.add(kern)
        fu = fast["u8"].reshape(TEACHER_B, -1)
        assert all(np.array_equal(fu[b], fu[0]) for b in range(1, TEACHER_B)), f"{tag}: identical images, different bytes (kernel {kern})"
        assert hashes(None, fu[0])[1] == want[1], f"{tag}: production path, plan {plan} (kernel {kern}) vs the reference"


def _teacher(workdir, name):
    cfg, wts, _, layers, H, W = _model(workdir, name)
    onet, per = _reference_tensors(workdir, name)
    g = G["nets"][name]
    hnet = binding.Net(cfg, wts)          # the product's own host prep supplies the per-channel integers
    hnet.prepare_host_only(1.0 / 255.0, 0)
    preps = {i: hnet.prep(i) for i, L in enumerate(layers) if L.type == "conv"}
    hnet.close()
    for i, p in preps.items():
        assert nr.prep_hash(p) == g["prep"][str(i)], f"{name} layer {i}: host prep vs the reference's"
    for x, outs, rec in zip(_images(name, H, W), per, g["images"]):
        ins = nr.conv_inputs(layers, x, lambda i: outs[i]["u8"])
        for i, p in preps.items():
            L, d, e = layers[i], onet.w[i], rec["layers"][i]
            seen = KERNELS.setdefault((name, i), set())
            tag = f"{name} image seed {rec['seed']} layer {i}"
            if "mask" in e:
                _, mask = nr.exact_mask(ins[i], d, L, p["zp_in"])
                assert int(mask.sum()) == e["mask"]["n"] and nr.h128(np.packbits(mask.ravel())) == e["mask"]["bits"], f"{tag}: mask"
                if e["mask"]["n"]:
                    _pin_conv(ins[i], L, d, p, (e["mask"]["i32"], e["mask"]["u8"]), mask, tag, seen)
            else:
                _pin_conv(ins[i], L, d, p, (e["i32"], e["u8"]), None, tag, seen)
    for key, lr in g["lowrange"].items():
        i = int(key)
        _pin_conv(nr.lowrange_input(layers[i], lr), layers[i], onet.w[i], preps[i], (lr["i32"], lr["u8"]), None, f"{name} layer {i} low-range",
                  KERNELS.setdefault((name, i), set()))


@pytest.mark.parametrize("name,mode", CASES, ids=[f"{n}-{m}" for n, m in CASES])
def test_net_vs_reference(workdir, name, mode):
    """One net of the file in one mode (the module's docstring): every tensor the device stores has the reference's hash."""
    if mode == "teacher":
        _teacher(workdir, name)
    else:
        _host_run(workdir, name, mode)


# Kernel ids (mi355_last_conv_kernel) the sweep reaches in test_gpu_random_nets.test_dynamic_coverage: 1, 2, 3, 4, 5, 7, 9.  Through
# binding.conv_forward, one unfused conv at a time, two of them cannot be reached by any layer:
UNREACHABLE = {7: "conv_pool16 exists only as the fused conv + 2x2 maxpool form; plan_fusion picks it, mi355_conv_forward never does "
                  "(pinned on all_exact nets by the production runs above: pool_16_to_32)"}
TEACHER_KERNELS = {1, 2, 3, 4, 5, 9}


def test_teacher_forced_layers_reach_the_sweeps_kernels(workdir):
    """The layers pinned teacher-forced were served by every kernel id of the sweep but UNREACHABLE's."""
    for name, mode in CASES:
        if mode == "teacher" and not any(k[0] == name for k in KERNELS):  # deselected: made up for
            _teacher(workdir, name)
    seen = set().union(*KERNELS.values())
    print("teacher-forced kernel ids:", {k: sum(k in v for v in KERNELS.values()) for k in sorted(seen)}, "layers each, of", len(KERNELS))
    assert not set(UNREACHABLE) & TEACHER_KERNELS
    assert not TEACHER_KERNELS - seen, sorted(TEACHER_KERNELS - seen)


# ------------------------------------------------------------------------------------------------- the one-layer nets
ONE = {**netgen.pool_nets(), **netgen.upsample_nets()}
GROUPS = {f"pool_k{k}": [n for n in ONE if n.startswith(f"pool_k{k}_")] for k in (1, 2, 3, 5)}
GROUPS["upsample"] = [n for n in ONE if n.startswith("up_")]


@pytest.mark.parametrize("group", list(GROUPS))
def test_one_layer_nets_vs_reference(workdir, group):
    """1x1 conv, one pool (sizes 1, 2, 3, 5, strides 1..4, padding 0..size + 1, pools shorter than their window included) or one
    upsample (strides 1..4), a head, through the host's production path at batch 3: the conv's and the glue layer's bytes of every slot
    have the reference's hash, the shapes are those its parser reported."""
    assert sum(len(v) for v in GROUPS.values()) == len(ONE) == len(G["one_layer"])
    for name in GROUPS[group]:
        g = G["one_layer"][name]
        cfg, wts, wsha = nr.write_model(workdir, "one", ONE[name][0], netgen.ONE_LAYER_WSEED)
        assert wsha == g["weights"] and list(ONE[name][1]) == g["geom"]
        h, w = ONE[name][1][-2:]
        xs = [synth.synth_image_u8(3, h, w, seed=s) for s in netgen.REF_IMAGE_SEEDS]
        net = binding.Net(cfg, wts, batch=B)
        try:
            net.prepare_fixed(1.0 / 255.0, 0)
            net.push_input(np.stack([xs[b % 2] for b in range(B)]))
            net.forward(); net.sync()
            assert [[inf["out_c"], inf["out_h"], inf["out_w"]] for inf in net.info[:3]] == g["shapes"], name
            assert not net.is_fused(0) and not net.fuses_next(0), name
            got = [net.pull(i)["u8"] for i in (0, 1)]
            for b in range(B):
                both = np.concatenate([t[b * inf["outputs"]:(b + 1) * inf["outputs"]] for t, inf in zip(got, net.info[:2])])
                assert nr.h128(both) == g["u8"][b % 2], f"{name}: slot {b}"
        finally:
            net.close()
