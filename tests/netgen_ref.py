"""What tests/golden/make_golden_netgen.py (the writer) and tests/test_netgen_ref_cpu.py / tests/test_gpu_netgen_ref.py (the readers) of
tests/golden/netgen_ref.json share: the hashes, the fp32-exact mask, the layer hand-off and the detection fields.

TEST INFRASTRUCTURE, CPU-only code.  Nothing here needs the reference: the file holds what it computed."""
import hashlib
import json
import os

import numpy as np

import oracle
from yolo_quantization_amd import synth

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "netgen_ref.json")
DET_CALLS = [(640, 480, 1, 0.5), (300, 500, 0, 0.3), (416, 416, 1, 0.6)]  # make_golden.DET_CALLS: (image w, h, relative, thresh)
WH_KEEP = 16          # w / h floats kept per head, call and image (the other fields of every record are in the hash)
BOUND = 2 ** 24


def h128(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:32]


def text_hash(s):
    return hashlib.sha256(s.encode()).hexdigest()[:32]


def prep_hash(p):
    return h128(np.concatenate([p["biases_int32"].view(np.uint8), p["M_value"].view(np.uint8), p["shift_value"].view(np.uint8)]))


def exact_mask(x, d, L, zp_in):
    """(exact int32 [n, oh*ow], mask) of conv L on input x: where the reference's fp32 accumulation (src/gemm.c:279-299) is provably
    exact, make_golden_kxk.py's condition: pass-1 sum and zp_w * (sum of the receptive field) both below 2^24"""
    ex, s1 = oracle.conv_acc(x, d["wq"], d["zp_w"], L.size, L.stride, L.pad, zp_in, oracle.ACC_EXACT, want_s1=True)
    ones = np.ones((1, x.shape[0] * L.size * L.size), np.uint8)
    sx = oracle.conv_acc(x, ones, np.zeros(1, np.uint8), L.size, L.stride, L.pad, zp_in, oracle.ACC_EXACT)
    return ex, (s1 < BOUND) & (d["zp_w"].astype(np.int64)[:, None] * sx.astype(np.int64) < BOUND)


def mask_fields(mask, i32, u8):
    """what the file keeps of a conv layer that is not wholly inside the mask"""
    return {"n": int(mask.sum()), "bits": h128(np.packbits(mask.ravel())),
            "i32": h128(np.where(mask, i32.reshape(mask.shape), 0).astype(np.int32)),
            "u8": h128(np.where(mask, u8.reshape(mask.shape), 0).astype(np.uint8))}


def det_fields(cnt, recs):
    """what the file keeps of one get_yolo_detections call: the count, the hash of the fields that are reproducible bit for bit (rank,
    centre, objectness, scores) and the w / h floats of the first WH_KEEP records"""
    exact = [0, 1, 2] + list(range(5, recs.shape[1]))
    return {"n": int(cnt), "x": h128(recs[:, exact]), "wh": np.ascontiguousarray(recs[:WH_KEEP, 3:5]).tobytes().hex()}


def assert_det_fields(cnt, recs, want, tag):
    """test_oracle_golden.assert_detections_match's rule on the kept fields: same count, same records in the same order, rank, centre,
    objectness and scores bit for bit, width / height to 4 ulp (the reference's -Ofast exp() is no correctly rounded libm call)"""
    got = det_fields(cnt, recs)
    assert got["n"] == want["n"], f"{tag}: {got['n']} detections, the reference has {want['n']}"
    assert got["x"] == want["x"], f"{tag}: rank / centre / objectness / scores differ from the reference's"
    wh = np.frombuffer(bytes.fromhex(want["wh"]), np.float32).reshape(-1, 2)
    np.testing.assert_allclose(recs[:WH_KEEP, 3:5], wh, rtol=5e-7, atol=0, err_msg=f"{tag}: box width / height")


def conv_inputs(layers, x, u8_of):
    """the uint8 input of every layer under forward_network's hand-off (src/network.c:229-261): the tensor of the layer before, a yolo
    layer handing on what it was given"""
    cur, ins = x, []
    for i, L in enumerate(layers):
        ins.append(cur)
        if L.type != "yolo":
            cur = u8_of(i).reshape(L.out_c, L.out_h, L.out_w)
    return ins


def write_model(tmp, name, cfg_text, wseed, act_gain=1.0, glue_own_zp=False):
    """cfg and weights files of a net under `tmp` -> (cfg path, weights path, 128-bit weights hash)"""
    cfg, wts = os.path.join(str(tmp), f"{name}.cfg"), os.path.join(str(tmp), f"{name}.weights")
    with open(cfg, "w") as f:
        f.write(cfg_text)
    meta = synth.synth_weights(cfg, wts, seed=wseed, act_gain=act_gain, glue_own_zp=glue_own_zp)
    return cfg, wts, meta["sha256"][:32]


def load(path=PATH):
    with open(path) as f:
        raw = json.load(f)
    return dict(raw["head"], nets=raw["nets"], one_layer=raw["one_layer"])


def lowrange_input(L, lr):
    x = (synth.synth_image_u8(L.c, L.h, L.w, seed=lr["seed"]) >> lr["shift"]).astype(np.uint8)
    assert h128(x) == lr["input"]
    return x


def yolo_params(section):
    """(anchors f32 [2 * num], mask i32, classes) of a [yolo] section as synth.read_cfg returns it"""
    anchors = np.array([float(v) for v in section["anchors"].split(",")], np.float32)
    mask = np.array([int(v) for v in section["mask"].split(",")], np.int32)
    return anchors, mask, int(section.get("classes", 20))
