"""CPU suite: the device-free half of the batched detection output (host/detect.c detections_from_records: packed records ->
`detection` arrays -> do_nms_sort) against do_nms_sort_arrays on the same boxes, and the new symbols of both libraries.  No GPU."""
import ctypes as C
import os

import numpy as np
import pytest

from yolo_quantization_amd import binding


def _pack(images, classes):
    """images: list of (boxes [k, 4], objectness [k], probs [k, classes], ranks [k]) -> (recs [total, 6 + classes], offsets [B + 1])"""
    rows, offsets = [], [0]
    for boxes, obj, probs, ranks in images:
        k = len(obj)
        r = np.zeros((k, 6 + classes), np.float32)
        r[:, 0], r[:, 1:5], r[:, 5], r[:, 6:] = ranks, boxes, obj, probs
        rows.append(r)
        offsets.append(offsets[-1] + k)
    return np.ascontiguousarray(np.concatenate(rows)), np.asarray(offsets, np.int32)


def _two_heads(k, split):
    """ranks of k records of an image: `split` from the first head, the rest from the second (each ascending from its own 0)"""
    return np.concatenate([np.arange(split) * 2, np.arange(k - split) * 3]).astype(np.float32)


def _from_records(recs, offsets, classes, nms):
    """detections_from_records -> per image (boxes, objectness, probs) in the order of the detection array it returns"""
    H = binding.host()
    B = len(offsets) - 1
    dets, num = (C.c_void_p * B)(), (C.c_int * B)()
    H.detections_from_records(recs.ctypes.data, offsets.ctypes.data, B, classes, C.c_float(nms), dets, num)
    out = []
    for b in range(B):
        k = num[b]
        assert dets[b] is not None, "an image without records still gets an array (get_network_boxes_batch returns one)"
        boxes, obj, probs = np.zeros((k, 4), np.float32), np.zeros(k, np.float32), np.zeros((k, classes), np.float32)
        H.detections_to_arrays(dets[b], k, classes, boxes.ctypes.data, obj.ctypes.data, probs.ctypes.data)
        out.append((boxes, obj, probs))
    H.free_detections_batch(dets, num, B)
    assert all(dets[b] is None and num[b] == 0 for b in range(B))
    return out


def _nms_arrays(boxes, obj, probs, nms):
    H = binding.host()
    p = np.ascontiguousarray(probs.copy())
    b = np.ascontiguousarray(boxes)
    o = np.ascontiguousarray(obj)
    H.do_nms_sort_arrays(b.ctypes.data, p.ctypes.data, o.ctypes.data, len(o), p.shape[1], C.c_float(nms))
    return p


def _rows(boxes, obj, probs):
    """the records as a sorted multiset of rows: do_nms_sort permutes the array, do_nms_sort_arrays keeps every row in its place"""
    m = np.concatenate([boxes, obj[:, None], probs], axis=1).view(np.uint32)
    return m[np.lexsort(m.T[::-1])]


def _fabricated(k, classes, seed):
    """k records with a few distinct score values only (a dequantised uint8 head: ties are the normal case), heavily overlapping boxes,
    every fifth objectness 0 and two identical records"""
    rng = np.random.default_rng(seed)
    boxes = np.concatenate([rng.integers(3, 6, (k, 2)) / 8.0, rng.integers(2, 5, (k, 2)) / 8.0], axis=1).astype(np.float32)
    levels = np.array([0.0, 0.25, 0.5, 0.75], np.float32)
    probs = levels[rng.integers(0, 4, (k, classes))]
    obj = levels[rng.integers(1, 4, k)]
    obj[::5] = 0.0
    boxes[7], probs[7], obj[7] = boxes[3], probs[3], obj[3]
    return boxes, obj, probs


@pytest.mark.parametrize("name", ["a", "b"])
@pytest.mark.parametrize("nms", [0.0, 0.45, "golden"])
def test_detections_from_records_equals_nms_arrays(golden_dir, name, nms):
    """3 images, 2 heads: the reference's own NMS vectors (tests/golden/nms.npz) as image 0, an image without records, and fabricated
    records with equal scores, identical boxes and objectness == 0 as image 2."""
    g = np.load(os.path.join(golden_dir, "nms.npz"))
    gb, go, gp = g[f"{name}_boxes"], g[f"{name}_obj"], g[f"{name}_probs"]
    classes = gp.shape[1]
    golden = nms == "golden"  # the threshold the reference's vector was made with: its own result is then known too
    if golden:
        nms = float(g[f"{name}_thresh"])
    fb, fo, fp = _fabricated(41, classes, seed=5)
    assert (fo == 0).sum() >= 8 and len(np.unique(fp)) <= 4
    empty = (np.zeros((0, 4), np.float32), np.zeros(0, np.float32), np.zeros((0, classes), np.float32))
    images = [(gb, go, gp), empty, (fb, fo, fp)]
    recs, offsets = _pack([im + (_two_heads(len(im[1]), len(im[1]) // 3),) for im in images], classes)
    assert offsets.tolist() == [0, len(go), len(go), len(go) + 41]
    got = _from_records(recs, offsets, classes, nms)
    assert len(got) == 3 and len(got[1][1]) == 0
    for (boxes, obj, probs), (gbx, gob, gpr) in zip(images, got):
        assert gbx.shape == boxes.shape and gpr.shape == probs.shape
        if nms == 0:  # no NMS: the array get_network_boxes_batch builds, record by record
            assert np.array_equal(gbx.view(np.uint32), boxes.view(np.uint32))
            assert np.array_equal(gob.view(np.uint32), obj.view(np.uint32))
            assert np.array_equal(gpr.view(np.uint32), probs.view(np.uint32))
            continue
        want = _nms_arrays(boxes, obj, probs, nms)
        assert np.array_equal(_rows(gbx, gob, gpr), _rows(boxes, obj, want))
        nz = np.flatnonzero(gob == 0)  # do_nms_sort moves the objectness == 0 entries behind the others (ref: src/box.c:60-69)
        assert len(nz) == (obj == 0).sum() and (len(nz) == 0 or nz[0] == len(gob) - len(nz))
    if golden:  # image 0 is the reference's vector: its own do_nms_sort kept / suppressed exactly these scores
        assert np.array_equal(_rows(*got[0]), _rows(gb, go, g[f"{name}_out"]))
    if nms:
        assert (_nms_arrays(fb, fo, fp, nms) != fp).any(), "the fabricated image must contain suppressed scores"


def test_new_symbols_are_exported():
    S, H = binding.shim(), binding.host()
    for sym in ("mi355_yolo_detections_batch", "mi355_yolo_detections_batch_work_ints"):
        assert hasattr(S, sym), sym
    for sym in ("network_yolo_detections_batch_gpu", "network_detections_batch", "free_detections_batch", "detections_from_records",
                "detections_to_arrays", "network_detections_batch_shape"):
        assert hasattr(H, sym), sym
    # the existing entry points stay
    for sym in ("network_yolo_detections_gpu", "network_yolo_detections_gpu_sizes", "get_network_boxes_batch", "do_nms_sort_arrays"):
        assert hasattr(H, sym), sym
    assert C.sizeof(binding.YoloHead) == 40


def test_batch_entry_refuses_before_touching_the_device():
    """The C-ABI's refusals come before any launch, so they can be seen without a device: more than 8 heads, n * H * W >= 2^24,
    classes < 1, max_per_image < 1."""
    S = binding.shim()
    heads = (binding.YoloHead * 9)()
    for k in range(9):
        heads[k] = binding.YoloHead(8, 8, 8, 3, 5, 7, 0)  # never dereferenced: refused first

    def call(nheads=2, B=2, classes=5, mpi=4, work_ints=1 << 20):
        return S.mi355_yolo_detections_batch(heads, nheads, B, classes, 416, 416, 8, 8, C.c_float(0.5), 1, mpi, 8, 8, 8, 8, work_ints, None)

    assert call(nheads=9) == -22 and b"heads" in S.mi355_last_error()
    assert call(nheads=0) == -22
    assert call(classes=0) == -22 and b"classes" in S.mi355_last_error()
    assert call(mpi=0) == -22 and b"max_per_image" in S.mi355_last_error()
    assert call(work_ints=1) == -22 and b"work" in S.mi355_last_error()
    heads[1] = binding.YoloHead(8, 8, 8, 4, 2048, 2048, 0)  # 4 * 2^22 = 2^24 candidates: rank would not fit a float
    assert call() == -22 and b"2^24" in S.mi355_last_error()
    assert S.mi355_yolo_detections_batch_work_ints(heads, 2, 2) == 0
    heads[1] = binding.YoloHead(8, 8, 8, 3, 13, 13, 0)
    assert S.mi355_yolo_detections_batch_work_ints(heads, 2, 3) == 3 * 2 and S.mi355_yolo_detections_batch_work_ints(heads, 9, 3) == 0
