"""One Net fed every kind of frames in turn: a network keeps one frame table and one staging arena for all of them, so a table that
held 32-byte entries is reused for 64-byte ones, the arena serves one, two and three planes per frame, and a re-batch frees and
re-allocates both.

Every comparison is exact.  After each feed the prepared input, scales and zero points must be what a second Net, which is only ever
fed through prepare_from_frames_u8, gives for the RGB frames that the numpy conversion (frames_util.yuv_to_rgb, the specification)
makes of the planes."""
import numpy as np
import pytest

from frames_util import CFG, SHIFTS, _assert_same_run, _bits, _layers_and_dets, _wts, plane_shapes, yuv_to_rgb
from yolo_quantization_amd import binding

pytestmark = pytest.mark.gpu

SIZES = [(53, 37), (12, 20), (12, 12)]  # w x h: wide, tall, network size (the host-level tests' frames)
MATRICES = ["bt601", "bt601f", "bt709", "bt709f"]


@pytest.fixture(scope="module", autouse=True)
def _dev():
    binding.init(0)


def _planar(fmt, w, h, rng):
    return tuple(rng.integers(0, 256, s, dtype=np.uint8) for s in plane_shapes(fmt, w, h))


def _planar_rgb(planes, fmt, matrix):
    """interleaved RGB of a planar frame: pixel (x, y) takes Y[y][x] and the chroma samples at [y >> sy][x >> sx]"""
    if fmt == "rgb":
        return np.ascontiguousarray(np.stack(planes, axis=-1))
    y, u, v = planes
    sx, sy = SHIFTS[fmt]
    rows, cols = (np.arange(y.shape[0]) >> sy)[:, None], (np.arange(y.shape[1]) >> sx)[None, :]
    return np.ascontiguousarray(yuv_to_rgb(y, u[rows, cols], v[rows, cols], MATRICES.index(matrix)))


def _feed(net, kind, matrix, sizes, rng):
    """feeds a random batch of `kind` to net; returns (what the entry point returned, the RGB frames it stands for)"""
    if kind == "u8":
        rgb = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for w, h in sizes]
        return net.prepare_from_frames_u8(rgb), rgb
    if kind in ("nv12", "nv21"):
        frames = [(rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, ((h + 1) // 2, (w + 1) // 2, 2), dtype=np.uint8))
                  for w, h in sizes]
        rgb = []
        for y, uv in frames:
            c = uv[(np.arange(y.shape[0]) // 2)[:, None], (np.arange(y.shape[1]) // 2)[None, :]]
            u, v = (c[..., 0], c[..., 1]) if kind == "nv12" else (c[..., 1], c[..., 0])
            rgb.append(np.ascontiguousarray(yuv_to_rgb(y, u, v, MATRICES.index(matrix))))
        return net.prepare_from_frames_nv12(frames, layout=kind, matrix=matrix), rgb
    frames = [_planar(kind, w, h, rng) for w, h in sizes]
    got = net.prepare_from_frames_planar(frames, format=kind, matrix="bt601" if kind == "rgb" else matrix)
    return got, [_planar_rgb(f, kind, matrix) for f in frames]


def _same_prepared(got, want, what):
    got, want = (got, want) if isinstance(got, tuple) else ((got,), (want,))
    assert len(got) == len(want)
    for a, b in zip(got, want):
        a, b = (_bits(a), _bits(b)) if a.dtype == np.float32 else (a, b)
        assert np.array_equal(a, b), what


@pytest.mark.parametrize("per_image", [False, True], ids=["shared_scale", "per_image"])
def test_one_net_fed_every_kind_in_turn_equals_the_u8_path(tmp_path, per_image):
    wts = _wts(tmp_path, seed=4)
    net, ref = binding.Net(CFG, wts, batch=3, dump_int32=True), binding.Net(CFG, wts, batch=3, dump_int32=True)
    net.set_input_per_image(per_image)
    ref.set_input_per_image(per_image)
    rng = np.random.default_rng(1234)
    feeds = [(3, "u8", "bt601"), (3, "i420", "bt709"), (3, "nv12", "bt601f"), (3, "rgb", "bt601"), (3, "nv21", "bt709f"), (3, "u8", "bt601"),
             (2, "i444", "bt601"), (2, "u8", "bt601")]
    for n, (batch, kind, matrix) in enumerate(feeds):
        what = f"feed {n} ({kind}, batch {batch})"
        if batch != net.batch:
            for x in (net, ref):
                x.H.set_batch_network(x.h, batch)
                x.batch = batch
        got, rgb = _feed(net, kind, matrix, SIZES[:batch], rng)
        _same_prepared(got, ref.prepare_from_frames_u8(rgb), what)
        sa, sb = net.input_quantization(), ref.input_quantization()
        assert np.array_equal(_bits(sa[0]), _bits(sb[0])) and np.array_equal(sa[1], sb[1]), what
        if n in (0, len(feeds) - 1):
            _assert_same_run(_layers_and_dets(net, rgb), _layers_and_dets(ref, rgb), what)
    net.close(); ref.close()
