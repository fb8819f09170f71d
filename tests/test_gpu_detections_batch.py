"""Detections out, one call per batch (detect.hip -> mi355_yolo_detections_batch -> network_yolo_detections_batch_gpu ->
Net.detections_batch / Net.detect): the ordered device decode of all yolo layers and all images against the oracle, against the
per-layer entry points it replaces (bit for bit), against the reference's fixtures, and its truncation / determinism / executor
contracts."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import oracle
from yolo_quantization_amd import binding, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = np.uint32(0x7FC0DEAD)  # a NaN no decode produces


@pytest.fixture(scope="module", autouse=True)
def device():
    binding.init(0)


# ------------------------------------------------------------------------------------------ the kernels through the C-ABI
NETW, NETH = 416, 320
ANCHORS = np.array([10, 14, 23, 27, 37, 58, 81, 82, 135, 169, 344, 319, 20, 31, 55, 44, 100, 77], np.float32)  # num = 9
HEADS = {"n3_1x1": (3, 1, 1, [0, 1, 2]), "n3_5x7": (3, 5, 7, [3, 4, 5]), "n1_13x13": (1, 13, 13, [6]), "n5_19x19": (5, 19, 19, [1, 3, 5, 7, 8])}
HEAD_SETS = [c for k in (1, 2, 3) for c in itertools.combinations(HEADS, k)]  # alone, and as sets of 2 and 3
PATTERNS = ["all", "none", "first", "last", "every64", "every65", "rand1", "rand50", "empty_mid"]
SIZES = [(640, 480), (300, 500), (416, 416), (1920, 1080), (77, 311)]  # a distinct (imw, imh) per slot


def _tensors(names, B, classes, pattern, seed):
    """yolo layer outputs [B][n][classes + 5][H][W] of every head with the objectness plane set by `pattern` over the image's candidates
    in reference order (heads in order, rank = cell * n + anchor) -> (tensors, thresh)"""
    rng = np.random.default_rng(seed)
    outs = []
    for nm in names:
        n, H, W, _ = HEADS[nm]
        t = rng.random((B, n, classes + 5, H * W), dtype=np.float32)
        t[:, :, 2:4] = t[:, :, 2:4] * np.float32(4) - np.float32(2)  # raw w / h entries: exp() of both signs
        outs.append(t)
    total = sum(HEADS[nm][0] * HEADS[nm][1] * HEADS[nm][2] for nm in names)
    g = np.arange(total)
    for b in range(B):
        if pattern == "all":
            above = np.ones(total, bool)
        elif pattern == "none":
            above = np.zeros(total, bool)
        elif pattern == "first":
            above = g == 0
        elif pattern == "last":
            above = g == total - 1
        elif pattern == "every64":
            above = g % 64 == 0
        elif pattern == "every65":
            above = g % 65 == 0
        elif pattern == "rand1":
            above = rng.random(total) < 0.01
        elif pattern == "rand50":
            above = rng.random(total) < 0.5
        else:  # an empty image between two full ones
            above = np.full(total, b != 1)
        obj = np.where(above, rng.random(total) * 0.4 + 0.55, rng.random(total) * 0.4 + 0.05).astype(np.float32)
        at = 0
        for nm, t in zip(names, outs):
            n, H, W, _ = HEADS[nm]
            t[b, :, 4, :] = obj[at:at + n * H * W].reshape(H * W, n).T  # candidate rank = cell * n + anchor
            at += n * H * W
    return outs, (-1.0 if pattern == "all" else 0.5)


def _abi_decode(names, outs, B, classes, imw, imh, thresh, relative, max_per_image, extra_heads=0):
    """mi355_yolo_detections_batch on uploaded tensors -> (rc, counts [B, nheads], offsets [B + 1], whole record buffer as uint32
    [capacity + guard records, 6 + classes], pre-filled with SENTINEL)"""
    S = binding.shim()
    nh = len(names) + extra_heads
    heads = (binding.YoloHead * max(nh, 1))()
    keep = []
    anchors = binding.DevBuf.from_numpy(ANCHORS)
    cand = 0
    for k in range(nh):
        nm = names[k % len(names)]
        n, H, W, mask = HEADS[nm]
        t, m = binding.DevBuf.from_numpy(outs[k % len(names)]), binding.DevBuf.from_numpy(np.asarray(mask, np.int32))
        keep += [t, m]
        heads[k] = binding.YoloHead(t.ptr, anchors.ptr, m.ptr, n, H, W, 0)
        cand += n * H * W
    rl = 6 + max(classes, 1)
    cap = B * min(max(max_per_image, 1), cand) + 3  # three guard records behind the capacity the header asks for
    recs = binding.DevBuf.from_numpy(np.full(cap * rl, SENTINEL, np.uint32))
    counts, offsets = binding.DevBuf(4 * B * nh), binding.DevBuf(4 * (B + 1))
    work_ints = max(int(S.mi355_yolo_detections_batch_work_ints(heads, nh, B)), 1)
    work = binding.DevBuf(4 * work_ints)
    sizes = binding.DevBuf.from_numpy(np.concatenate([np.asarray(imw, np.int32), np.asarray(imh, np.int32)]))
    rc = S.mi355_yolo_detections_batch(heads, nh, B, classes, NETW, NETH, sizes.ptr, sizes.ptr.value + 4 * B, C.c_float(thresh),
                                       int(relative), int(max_per_image), recs.ptr, counts.ptr, offsets.ptr, work.ptr, work_ints, None)
    if rc != 0:
        return rc, None, None, None
    binding.check(S.mi355_stream_sync(None), "sync")
    return (0, counts.to_numpy(np.int32, B * nh).reshape(B, nh), offsets.to_numpy(np.int32, B + 1),
            recs.to_numpy(np.uint32, cap * rl).reshape(cap, rl))


def _oracle_image(names, outs, b, classes, imw, imh, thresh, relative):
    """per head (count, records) of image b from the CPU restatement of get_yolo_detections + correct_yolo_boxes"""
    res = []
    for nm, t in zip(names, outs):
        n, H, W, mask = HEADS[nm]
        res.append(oracle.yolo_detections(t[b].ravel(), n, classes, H, W, ANCHORS, mask, NETW, NETH, imw, imh, thresh, relative))
    return res


def _assert_vs_oracle(got, want):
    """count, order, rank, centre, objectness and scores exact; w / h at rtol 3e-7 (device exp() against glibc's, the tolerance of
    test_yolo_detections_batch64_vs_oracle)"""
    assert got.shape == want.shape
    exact = [0, 1, 2] + list(range(5, got.shape[1]))
    assert np.array_equal(got[:, exact].view(np.uint32), want[:, exact].view(np.uint32))
    np.testing.assert_allclose(got[:, 3:5], want[:, 3:5], rtol=3e-7, atol=0)


@pytest.mark.parametrize("si", range(len(HEAD_SETS)), ids=["+".join(s) for s in HEAD_SETS])
def test_kernel_vs_oracle(si):
    """Every head set x every objectness pattern; classes (1, 5, 80), B (1, 3, 5) and relative (0, 1) rotate over the cases so that every
    pairing of them occurs.  The candidate counts (3, 105, 169, 1805 and their sums) are no multiples of 64 or 256."""
    names = HEAD_SETS[si]
    for pi, pattern in enumerate(PATTERNS):
        classes = (1, 5, 80)[(pi + si) % 3]
        B = 3 if pattern == "empty_mid" else (1, 3, 5)[(pi // 3 + si) % 3]
        relative = (pi + si) % 2
        imw, imh = [s[0] for s in SIZES[:B]], [s[1] for s in SIZES[:B]]
        outs, thresh = _tensors(names, B, classes, pattern, seed=100 * si + pi)
        cand = sum(HEADS[nm][0] * HEADS[nm][1] * HEADS[nm][2] for nm in names)
        rc, counts, offsets, buf = _abi_decode(names, outs, B, classes, imw, imh, thresh, relative, cand)
        assert rc == 0, binding.shim().mi355_last_error()
        recs = buf.view(np.float32)
        assert offsets[0] == 0
        for b in range(B):
            want = _oracle_image(names, outs, b, classes, imw[b], imh[b], thresh, relative)
            assert counts[b].tolist() == [c for c, _ in want], (pattern, b)
            assert offsets[b + 1] - offsets[b] == sum(c for c, _ in want), (pattern, b)
            at = offsets[b]
            for cnt, w in want:  # per head: the image's slice holds the heads one after the other
                _assert_vs_oracle(recs[at:at + cnt], w)
                at += cnt
        if pattern == "all":
            assert (counts.sum(axis=1) == cand).all()
        if pattern == "none":
            assert offsets[-1] == 0
        if pattern == "empty_mid":
            assert offsets[1] == offsets[2] and offsets[1] == cand and offsets[3] == 2 * cand
        assert (buf[offsets[-1]:] == SENTINEL).all(), f"{pattern}: a float at or beyond recs[offsets[B]] was written"


MANY = [(B, names, pattern, mpi) for B in (257, 600) for names in (("n3_1x1",), ("n3_5x7",), ("n3_1x1", "n3_5x7"))
        for pattern, mpi in (("all", None), ("rand50", None), ("empty_mid", None))]
MANY.append((600, ("n3_5x7",), "rand50", 52))  # about half of 105 candidates are found: 52 kept truncates some images and not others


@pytest.mark.parametrize("B,names,pattern,mpi", MANY, ids=[f"B{B}-{'+'.join(n)}-{p}" + (f"-max{m}" if m else "") for B, n, p, m in MANY])
def test_kernel_vs_oracle_many_images(B, names, pattern, mpi):
    """det_scan_kernel scans the images 256 at a time and carries the sum from one chunk to the next: batches of 257 (one image into the second
    chunk) and 600 (two full chunks and a partial third), with and without a max_per_image that cuts some images short"""
    classes, relative = 5, B % 2
    imw, imh = [SIZES[b % len(SIZES)][0] + b % 7 for b in range(B)], [SIZES[b % len(SIZES)][1] + b % 3 for b in range(B)]
    outs, thresh = _tensors(names, B, classes, pattern, seed=B + len(pattern))
    cand = sum(HEADS[nm][0] * HEADS[nm][1] * HEADS[nm][2] for nm in names)
    rc, counts, offsets, buf = _abi_decode(names, outs, B, classes, imw, imh, thresh, relative, mpi or cand)
    assert rc == 0, binding.shim().mi355_last_error()
    recs = buf.view(np.float32)
    found = np.zeros(B, np.int64)
    assert offsets[0] == 0
    for b in range(B):
        want = _oracle_image(names, outs, b, classes, imw[b], imh[b], thresh, relative)
        assert counts[b].tolist() == [c for c, _ in want], (pattern, b)
        found[b] = sum(c for c, _ in want)
        kept = min(found[b], mpi or cand)
        assert offsets[b + 1] - offsets[b] == kept, (pattern, b)
        allw = np.concatenate([w for _, w in want]) if found[b] else np.zeros((0, recs.shape[1]), np.float32)
        _assert_vs_oracle(recs[offsets[b]:offsets[b] + kept], allw[:kept])  # the heads one after the other, the first `kept` of them
    if pattern == "all":
        assert (found == cand).all()
    if pattern == "empty_mid":
        assert found[1] == 0 and offsets[1] == offsets[2] == cand and offsets[-1] == (B - 1) * cand
    if mpi:
        assert (found > mpi).any() and (found < mpi).any(), "the limit must cut some images short and leave others whole"
    assert (buf[offsets[-1]:] == SENTINEL).all(), f"{pattern}: a float at or beyond recs[offsets[B]] was written"


def test_truncation_keeps_the_first_records_and_writes_nothing_behind_them():
    names, B, classes = ("n3_5x7", "n5_19x19"), 3, 5
    imw, imh = [s[0] for s in SIZES[:B]], [s[1] for s in SIZES[:B]]
    outs, thresh = _tensors(names, B, classes, "rand50", seed=77)
    cand = 105 + 1805
    rc, fcounts, foff, fbuf = _abi_decode(names, outs, B, classes, imw, imh, thresh, 1, cand)
    assert rc == 0
    found = int(fcounts[0].sum())
    per_image = fcounts.sum(axis=1)
    assert len(set(per_image.tolist())) == B and found > 300  # the images differ, and found crosses several blocks
    for mpi in (1, 4, found - 1, found, found + 1):
        rc, counts, off, buf = _abi_decode(names, outs, B, classes, imw, imh, thresh, 1, mpi)
        assert rc == 0
        assert np.array_equal(counts, fcounts), "counts report what was found, not what was kept"
        kept = np.minimum(per_image, mpi)
        assert np.array_equal(off, np.concatenate([[0], np.cumsum(kept)])), "offsets are the prefix sums of the kept counts"
        for b in range(B):
            assert np.array_equal(buf[off[b]:off[b + 1]], fbuf[foff[b]:foff[b] + kept[b]]), (mpi, b)  # the first k of the full result
        assert (buf[off[-1]:] == SENTINEL).all(), mpi


def test_abi_refusals():
    names, B = ("n3_5x7",), 2
    outs, thresh = _tensors(names, B, 5, "rand50", seed=1)
    imw, imh = [640, 300], [480, 500]
    S = binding.shim()
    assert _abi_decode(names, outs, B, 5, imw, imh, thresh, 1, 8, extra_heads=8)[0] == -22 and b"heads" in S.mi355_last_error()  # nine
    assert _abi_decode(names, outs, B, 5, imw, imh, thresh, 1, 0)[0] == -22 and b"max_per_image" in S.mi355_last_error()
    assert _abi_decode(names, outs, B, 0, imw, imh, thresh, 1, 8)[0] == -22 and b"classes" in S.mi355_last_error()
    assert _abi_decode(names, outs, B, 5, imw, imh, thresh, 1, 8, extra_heads=7)[0] == 0  # eight are served


# ------------------------------------------------------------------------------------------------------- through the network
def _weights(tmp, cfg, seed, **kw):
    p = str(tmp / (os.path.basename(cfg) + f".{seed}.weights"))
    if not os.path.exists(p):
        synth.synth_weights(cfg, p, seed=seed, **kw)
    return p


def _heads_of(net):
    return [i for i, inf in enumerate(net.info) if inf["type"] == binding.T_YOLO]


def _old_image_records(net, imw, imh, thresh, relative, classes):
    """The per-layer entry point (Net.detections_sizes), layer after layer: per image the records concatenated in head order, and the
    counts [B, nheads]"""
    B = net.batch
    per, cnts = [[] for _ in range(B)], []
    for i in _heads_of(net):
        inf = net.info[i]
        cand = inf["outputs"] // (classes + 5)
        counts, recs = net.detections_sizes(i, classes, imw, imh, thresh, relative, cand)
        cnts.append(counts)
        for b in range(B):
            per[b].append(recs[b, :counts[b]])
    return [np.concatenate(p) for p in per], np.stack(cnts, axis=1)


@pytest.fixture(scope="module")
def nets(tmp_path_factory, golden_dir, cfg_dir):
    """the three networks of the new-against-old test, forwarded once: name -> (net, classes)"""
    tmp = tmp_path_factory.mktemp("detb")
    made = {}
    for name in ("tiny_unit", "s2_unit"):
        g = np.load(os.path.join(golden_dir, f"{name}_seed1.npz"))
        cfg = os.path.join(cfg_dir, f"{name}.cfg")
        net = binding.Net(cfg, _weights(tmp, cfg, 1, act_gain=float(g["act_gain"])), batch=3)
        net.prepare_fixed(1.0 / 255.0, 0)
        net.push_input(np.repeat(g["input_u8"][None], 3, axis=0))
        net.forward(); net.sync()
        made[name] = net
    cfg = os.path.join(cfg_dir, "yolov3-tiny_quant.cfg")
    xb = np.repeat(synth.synth_image_u8(3, 416, 416, seed=7)[None], 8, axis=0)
    xb[1::2] = synth.synth_image_u8(3, 416, 416, seed=8)
    net = binding.Net(cfg, _weights(tmp, cfg, 1234), batch=8)
    net.prepare_fixed(1.0 / 255.0, 0)
    net.push_input(xb)
    net.forward(); net.sync()
    made["yolov3-tiny"] = net
    yield made
    for net in made.values():
        net.close()


@pytest.mark.parametrize("name", ["tiny_unit", "s2_unit", "yolov3-tiny"])
def test_new_call_equals_the_per_layer_calls_bitwise(nets, name):
    from test_oracle_golden import DET_CALLS
    net = nets[name]
    B = net.batch
    nh, classes, cand = net.detections_shape()
    assert nh == len(_heads_of(net)) and classes == 5
    distinct = ([SIZES[b % 5][0] + b for b in range(B)], [SIZES[b % 5][1] - b for b in range(B)], 1, 0.4)
    some = 0
    for imw, imh, rel, th in list(DET_CALLS) + [distinct]:
        w = np.broadcast_to(np.asarray(imw, np.int32), (B,)); h = np.broadcast_to(np.asarray(imh, np.int32), (B,))
        want, want_counts = _old_image_records(net, w, h, th, rel, classes)
        counts, offsets, recs = net.detections_batch(imw, imh, th, rel)
        assert np.array_equal(counts, want_counts)
        assert np.array_equal(offsets, np.concatenate([[0], np.cumsum(want_counts.sum(axis=1))]))
        assert recs.shape == (offsets[-1], 6 + classes)
        for b in range(B):  # every field, w and h included
            assert np.array_equal(recs[offsets[b]:offsets[b + 1]].view(np.uint32), want[b].view(np.uint32)), (imw, imh, b)
        some += int(offsets[-1])
    assert some > 0 or name == "s2_unit"  # (the reference finds nothing on that fixture either)


@pytest.mark.parametrize("name", ["tiny_unit", "s2_unit"])
def test_against_the_reference_fixtures(nets, golden_dir, name):
    from test_oracle_golden import DET_CALLS, assert_detections_match
    g = np.load(os.path.join(golden_dir, f"{name}_seed1.npz"))
    net = nets[name]
    for k, (imw, imh, rel, th) in enumerate(DET_CALLS):
        counts, offsets, recs = net.detections_batch(imw, imh, th, rel)
        for b in range(net.batch):
            at = offsets[b]
            for hk, i in enumerate(_heads_of(net)):
                cnt = int(counts[b, hk])
                assert_detections_match(cnt, recs[at:at + cnt], int(g[f"L{i}_det{k}_count"]), g[f"L{i}_det{k}_recs"])
                at += cnt
            assert at == offsets[b + 1]


def test_network_truncation_and_determinism(nets):
    net = nets["yolov3-tiny"]
    B = net.batch
    counts, offsets, recs = net.detections_batch(640, 424, 0.5, 1)
    c2, o2, r2 = net.detections_batch(640, 424, 0.5, 1)
    assert counts.tobytes() == c2.tobytes() and offsets.tobytes() == o2.tobytes() and recs.tobytes() == r2.tobytes()
    per_image = counts.sum(axis=1)
    found = int(per_image[0])
    assert found > 4 and per_image[1] != per_image[0]
    for mpi in (1, 4, found - 1, found, found + 1):
        ck, ok, rk = net.detections_batch(640, 424, 0.5, 1, max_per_image=mpi)
        kept = np.minimum(per_image, mpi)
        assert np.array_equal(ck, counts) and np.array_equal(ok, np.concatenate([[0], np.cumsum(kept)]))
        for b in range(B):
            assert np.array_equal(rk[ok[b]:ok[b + 1]].view(np.uint32), recs[offsets[b]:offsets[b] + kept[b]].view(np.uint32)), (mpi, b)


def test_replica_and_graph_replay_give_the_eager_parents_result(nets, tmp_path, cfg_dir):
    parent = nets["yolov3-tiny"]
    want = parent.detections_batch([640 + b for b in range(8)], 424, 0.5, 1)
    assert want[1][-1] > 0
    x = np.repeat(synth.synth_image_u8(3, 416, 416, seed=7)[None], 8, axis=0)
    x[1::2] = synth.synth_image_u8(3, 416, 416, seed=8)
    rep = parent.replica()
    rep.push_input(x)
    rep.forward(); parent.forward()  # side by side on their streams
    rep.sync(); parent.sync()
    got_rep = rep.detections_batch([640 + b for b in range(8)], 424, 0.5, 1)
    got_par = parent.detections_batch([640 + b for b in range(8)], 424, 0.5, 1)
    rep.close()
    cfg = os.path.join(cfg_dir, "yolov3-tiny_quant.cfg")
    graph = binding.Net(cfg, _weights(tmp_path, cfg, 1234), batch=8, use_graph=True)
    graph.prepare_fixed(1.0 / 255.0, 0)
    graph.push_input(x)
    graph.forward(); graph.sync()  # captures
    graph.forward(); graph.sync()  # replays
    assert graph.graph_handle()
    got_graph = graph.detections_batch([640 + b for b in range(8)], 424, 0.5, 1)
    graph.close()
    for got in (got_rep, got_par, got_graph):
        for a, b in zip(got, want):
            assert a.tobytes() == b.tobytes()


def test_per_image_input_mode_slot_equals_batch1(tmp_path, cfg_dir):
    cfg = os.path.join(cfg_dir, "tiny_unit.cfg")
    wts = _weights(tmp_path, cfg, 9)
    rng = np.random.default_rng(3)
    ims = [rng.random((3, 37, 53), dtype=np.float32) * np.float32(0.4),
           rng.random((3, 20, 12), dtype=np.float32) * np.float32(0.9) + np.float32(0.05),
           rng.random((3, 12, 12), dtype=np.float32) * np.float32(0.2) + np.float32(0.3)]
    net = binding.Net(cfg, wts, batch=3)
    net.set_input_per_image(True)
    net.prepare_from_images_gpu(ims)
    net.forward(); net.sync()
    imw, imh = [im.shape[2] for im in ims], [im.shape[1] for im in ims]
    counts, offsets, recs = net.detections_batch(imw, imh, 0.3, 1)
    n1 = binding.Net(cfg, wts, batch=1)
    total = 0
    for b, im in enumerate(ims):
        n1.prepare_from_images_gpu([im])
        n1.forward(); n1.sync()
        c1, o1, r1 = n1.detections_batch(imw[b], imh[b], 0.3, 1)
        assert np.array_equal(c1[0], counts[b]) and o1.tolist() == [0, offsets[b + 1] - offsets[b]]
        assert r1.tobytes() == recs[offsets[b]:offsets[b + 1]].tobytes(), b
        total += int(o1[-1])
    assert total > 0
    n1.close()
    net.close()


def test_detect_equals_old_records_through_nms(nets):
    """Net.detect (network_detections_batch + the host's NMS) against the per-layer records passed through do_nms_sort_arrays: the
    surviving scores and their order"""
    H = binding.host()
    for name, th in (("yolov3-tiny", 0.25), ("tiny_unit", 0.3)):
        net = nets[name]
        B = net.batch
        classes = net.detections_shape()[1]
        imw, imh = [SIZES[b % 5][0] for b in range(B)], [SIZES[b % 5][1] for b in range(B)]
        want, want_counts = _old_image_records(net, np.asarray(imw, np.int32), np.asarray(imh, np.int32), th, 1, classes)
        res = net.detect(imw, imh, thresh=th, nms=0.45)
        assert len(res) == B
        suppressed = 0
        for b in range(B):
            r = want[b]
            boxes, obj, probs = np.ascontiguousarray(r[:, 1:5]), np.ascontiguousarray(r[:, 5]), np.ascontiguousarray(r[:, 6:])
            before = probs.copy()
            H.do_nms_sort_arrays(boxes.ctypes.data, probs.ctypes.data, obj.ctypes.data, len(obj), classes, C.c_float(0.45))
            suppressed += int((probs != before).sum())
            d = res[b]
            assert d["found"] == int(want_counts[b].sum()) and d["kept"] == len(obj)
            assert np.array_equal(d["boxes"].view(np.uint32), boxes.view(np.uint32))
            assert np.array_equal(d["objectness"].view(np.uint32), obj.view(np.uint32))
            assert np.array_equal(d["probs"].view(np.uint32), probs.view(np.uint32))
        assert suppressed > 0 or name != "yolov3-tiny"
        capped = net.detect(imw, imh, thresh=th, nms=0, max_per_image=2)
        for b in range(B):
            k = min(2, len(want[b]))
            assert capped[b]["kept"] == k and capped[b]["found"] == len(want[b])
            assert np.array_equal(capped[b]["probs"].view(np.uint32), want[b][:k, 6:].view(np.uint32))


def test_host_refusals(nets, tmp_path, cfg_dir):
    net = nets["tiny_unit"]
    with pytest.raises(binding.MI355Error):
        net.detections_batch([640, 0, 640], 480, 0.5, 1)  # a non-positive size
    with pytest.raises(binding.MI355Error):
        net.detect(640, [480, 480, -1])
    # two yolo layers with different `classes`: refused as a whole (each can still be decoded on its own)
    base = open(os.path.join(cfg_dir, "tiny_unit.cfg")).read()
    second = ("\n[route]\nlayers = -3\nquantized=1\nquant_stop=0\n\n[convolutional]\nfilters=21\nsize=1\nstride=1\npad=1\nactivation=linear\n"
              "quantized=1\nquant_stop=1\n\n[yolo]\nmask = 3,4,5\nanchors = 10,14,  23,27,  37,58,  81,82,  135,169,  344,319\nclasses=2\n"
              "num=6\njitter=.3\nignore_thresh = .7\ntruth_thresh = 1\nrandom=1\n")
    cfg = str(tmp_path / "two_classes.cfg")
    open(cfg, "w").write(base + second)
    wts = str(tmp_path / "two_classes.weights")
    synth.synth_weights(cfg, wts, seed=1)
    mixed = binding.Net(cfg, wts, batch=2)
    with pytest.raises(binding.MI355Error):
        mixed.detections_shape()
    B = 2
    w, h = np.full(B, 640, np.int32), np.full(B, 480, np.int32)
    recs, counts, offsets = np.zeros(1024, np.float32), np.zeros(2 * B, np.int32), np.zeros(B + 1, np.int32)
    assert mixed.H.network_yolo_detections_batch_gpu(mixed.h, w.ctypes.data, h.ctypes.data, C.c_float(0.5), 1, 4, recs.ctypes.data,
                                                      counts.ctypes.data, offsets.ctypes.data) == -22
    mixed.close()
