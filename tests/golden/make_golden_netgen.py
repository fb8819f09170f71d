#!/usr/bin/env python3
"""tests/golden/netgen_ref.json: the tensors of the whole-network sweep (tests/netgen.py) as THE REFERENCE ITSELF computes them
(oracle/_ref, built by oracle/build_ref.sh), with make_golden.py's recipe.

  python tests/golden/make_golden_netgen.py          # rewrites tests/golden/netgen_ref.json

The reference runs the TWIN of every net (netgen.reference_twin: it has no integer [shortcut]), on the sweep's own weights, on two seeded
images (netgen.REF_IMAGE_SEEDS; input scale 1/255, zero point 0).  Every net runs in a fresh child process: the reference aborts where it
should refuse, and a child that dies stops the generator, which names the net.

The file is data only, 128-bit prefixes of SHA-256 throughout.  Per net: hashes of the cfg text, the weights and the inputs; per layer
and image the hashes of output_int32, output_uint8_final and output (f32: quant_stop tails and yolo layers); per conv layer the hash of
the host prep arrays (biases_int32, M_value, shift_value) and, where the layer is not wholly inside it, the fp32-exact mask of
make_golden_kxk.py (pass-1 sum and zp_w * sum(x) both below 2^24 on the reference's own layer input: count, hash of the packed bits,
hashes of the masked int32 / uint8 tensors); `all_exact` for a net whose every conv layer is wholly inside the mask on both images; for
every other conv layer a low-range vector (the layer alone on seeded bytes >> shift through refdrv.forward_layer, full-tensor hashes,
the shift raised until the reference is exact on every element); the reference's get_yolo_detections of every head at make_golden's
DET_CALLS (count, hash of the exact fields, and the w / h floats of the first WH_KEEP records).  Written only after the exact integers
were found equal to the reference on every masked element and every low-range tensor.

Then the one-pool and one-upsample nets (netgen.pool_nets / upsample_nets: 1x1 conv, the layer, a head): shapes and one hash per image
over the uint8 tensors of the conv and the pool or upsample (the head conv runs fused with its yolo layer in production and need not
store its own)."""
import json
import os
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.normpath(os.path.join(HERE, "..", ".."))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
from yolo_quantization_amd import synth  # noqa: E402
import netgen  # noqa: E402
import oracle  # noqa: E402
import refdrv  # noqa: E402

from netgen_ref import DET_CALLS, PATH, WH_KEEP, conv_inputs, det_fields, exact_mask, h128, mask_fields, prep_hash, text_hash, write_model  # noqa: E402

LOWRANGE_SEED, LOWRANGE_SHIFT = 500, 5
ONE_LAYER_CHUNK = 24  # one-layer nets per child process


# ----------------------------------------------------------------------------------------------- in the child
def record_net(name, tmp):
    spec = netgen.ref_sweep()[name]
    cfg, wts, wsha = write_model(tmp, name, spec["cfg"], spec["wseed"], spec["act_gain"], spec["glue_own_zp"])
    sections = synth.read_cfg(cfg)
    netopt, layers = synth.layer_shapes(sections)
    wrec = oracle.read_weights(wts, layers)
    net = refdrv.RefNet(cfg, wts)
    H, W = int(netopt["height"]), int(netopt["width"])
    out = {"cfg": text_hash(spec["cfg"]), "weights": wsha, "has_shortcut": spec["has_shortcut"], "prep": {}, "images": [], "lowrange": {}}
    inexact = set()
    for k, seed in enumerate(netgen.REF_IMAGE_SEEDS):
        x = synth.synth_image_u8(3, H, W, seed=seed)
        if k == 0:
            xq = net.prepare(synth.image_u8_to_float(x))
            assert np.array_equal(xq, x.ravel()), "layer-0 quantiser is expected to be the identity on pinned images"
            for i, L in enumerate(layers):
                if L.type == "conv":
                    out["prep"][str(i)] = prep_hash(net.prep(i))
        else:
            net.set_input_u8(x)
        net.forward()
        ins = conv_inputs(layers, x, net.layer_u8)
        rec = {"seed": seed, "input": h128(x), "layers": [], "det": {}}
        for i, L in enumerate(layers):
            e = {"t": L.type}
            if L.type == "conv":
                a, u = net.layer_int32(i), net.layer_u8(i)
                e["i32"] = h128(a)
                ex, mask = exact_mask(ins[i], wrec[i], L, net.prep(i)["zp_in"])
                ref = a.reshape(ex.shape)
                assert not ((ex != ref) & mask).any(), f"{name} layer {i}: exact != reference inside the fp32-exact mask"
                if not mask.all():
                    inexact.add(i)
                    e["mask"] = mask_fields(mask, ref, u)
            if L.type != "yolo":
                e["u8"] = h128(net.layer_u8(i))
            if L.quant_stop or L.type == "yolo":
                e["f32"] = h128(net.layer_f32(i))
            if L.type == "yolo":
                classes = int(sections[i + 1].get("classes", 20))
                rec["det"][str(i)] = [det_fields(*net.yolo_detections(i, classes, imw, imh, th, rel, L.n * L.h * L.w))
                                      for imw, imh, rel, th in DET_CALLS]
            rec["layers"].append(e)
        out["images"].append(rec)
    out["all_exact"] = not inexact
    for i in sorted(inexact):  # after the whole-net hashes: a conv's forward only overwrites that layer's own outputs
        L, d, zp_in = layers[i], wrec[i], net.prep(i)["zp_in"]
        # The mask is a sufficient condition only; what a low-range vector needs is that the reference IS exact on every element.  A
        # layer whose pad taps alone pass 2^24 (a large window on a small map behind a zero point of 128) is never wholly inside the
        # mask: the shift goes up until the reference equals the exact integers, at 8 the input is all zero and only the pads count.
        for shift in range(LOWRANGE_SHIFT, 9):
            xl = (synth.synth_image_u8(L.c, L.h, L.w, seed=LOWRANGE_SEED + i) >> shift).astype(np.uint8)
            ex, mask = exact_mask(xl, d, L, zp_in)
            net.forward_layer(i, xl)
            a, u = net.layer_int32(i), net.layer_u8(i)
            if np.array_equal(ex.ravel(), a):
                break
        assert np.array_equal(ex.ravel(), a), f"{name} layer {i}: the reference is not exact on any low-range input"
        out["lowrange"][str(i)] = {"seed": LOWRANGE_SEED + i, "shift": shift, "in_mask": bool(mask.all()), "input": h128(xl),
                                   "i32": h128(a), "u8": h128(u)}
    return out


def record_one_layer(name, tmp):
    nets = dict(netgen.pool_nets()); nets.update(netgen.upsample_nets())
    cfg_text, geom = nets[name]
    cfg, wts, wsha = write_model(tmp, name, cfg_text, netgen.ONE_LAYER_WSEED)
    netopt, layers = synth.layer_shapes(synth.read_cfg(cfg))
    net = refdrv.RefNet(cfg, wts)
    out = {"geom": list(geom), "weights": wsha, "shapes": [[inf["out_c"], inf["out_h"], inf["out_w"]] for inf in net.info[:3]], "u8": []}
    for k, seed in enumerate(netgen.REF_IMAGE_SEEDS):
        x = synth.synth_image_u8(3, int(netopt["height"]), int(netopt["width"]), seed=seed)
        if k == 0:
            assert np.array_equal(net.prepare(synth.image_u8_to_float(x)), x.ravel())
        else:
            net.set_input_u8(x)
        net.forward()
        out["u8"].append(h128(np.concatenate([net.layer_u8(i) for i in range(2)])))
    return out


def child(kind, names, dest):
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name in names:
            res[name] = (record_net if kind == "net" else record_one_layer)(name, tmp)
    with open(dest, "w") as f:
        json.dump(res, f)


# ---------------------------------------------------------------------------------------------- in the parent
def _spawn(job):
    kind, names, tmp = job
    dest = os.path.join(tmp, f"{names[0]}.json")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", kind, ",".join(names), dest], stdout=subprocess.DEVNULL,
                       stderr=subprocess.PIPE, text=True)
    if r.returncode != 0 or not os.path.exists(dest):
        raise RuntimeError(f"the reference's child process for {names} ended with status {r.returncode}:\n{r.stderr[-2000:]}")
    with open(dest) as f:
        return json.load(f)


def generate(workers=None):
    """the file's content as a dict; every net in a child process of its own (the one-layer nets ONE_LAYER_CHUNK to a child)"""
    assert refdrv.available(), "run oracle/build_ref.sh first (it needs the reference's sources)"
    one = list(netgen.pool_nets()) + list(netgen.upsample_nets())
    with tempfile.TemporaryDirectory() as tmp:
        jobs = [("net", [name], tmp) for name in netgen.ref_sweep()]
        jobs += [("one", one[k:k + ONE_LAYER_CHUNK], tmp) for k in range(0, len(one), ONE_LAYER_CHUNK)]
        with ThreadPoolExecutor(workers or min(8, os.cpu_count() or 1)) as ex:
            parts = list(ex.map(_spawn, jobs))
    nets, one_layer = {}, {}
    for (kind, _, _), part in zip(jobs, parts):
        (nets if kind == "net" else one_layer).update(part)
    return {"reference": "default build (GPU=0 QUANTIZATION=1 -Ofast), the twin of every net of netgen.sweep() but AIMED_BIG",
            "hash": "first 128 bits of SHA-256", "image_seeds": list(netgen.REF_IMAGE_SEEDS), "det_calls": [list(c) for c in DET_CALLS],
            "wh_keep": WH_KEEP, "nets": nets, "one_layer": one_layer}


def dumps(doc):
    """one line per net: small, and a regenerated file differs only in the lines that changed"""
    def block(d):
        return "{\n" + ",\n".join(f' "{k}": ' + json.dumps(v, separators=(",", ":"), sort_keys=True) for k, v in d.items()) + "\n}"
    head = {k: v for k, v in doc.items() if k not in ("nets", "one_layer")}
    return ('{"head": ' + json.dumps(head, sort_keys=True) + ',\n"nets": ' + block(doc["nets"]) + ',\n"one_layer": ' + block(doc["one_layer"])
            + "}\n")


if __name__ == "__main__":
    if len(sys.argv) == 5 and sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3].split(","), sys.argv[4])
    else:
        text = dumps(generate())
        with open(PATH, "w") as f:
            f.write(text)
        print(f"netgen_ref.json: {len(text)} bytes")
