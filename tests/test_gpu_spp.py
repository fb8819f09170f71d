"""GPU suite (`-m gpu`) for the fused SPP pools (spp.hip, mi355_spp_forward): the kernel against a numpy max over in-image taps with
its outputs as channel windows of one concat buffer, the C-ABI's refusals, and the host's fused group against its own parity dump."""
import os

import numpy as np
import pytest

from yolo_quantization_amd import binding, synth

pytestmark = pytest.mark.gpu
B = 3


@pytest.fixture(scope="module", autouse=True)
def device():
    binding.init(0)


def _pool(x, k):
    """the max over the in-image taps of the k x k window centred on each cell, from uint8 0; x: [B, C, H, W] uint8"""
    r, (H, W) = k // 2, x.shape[2:]
    p = np.zeros(x.shape[:2] + (H + 2 * r, W + 2 * r), np.uint8)
    p[:, :, r:r + H, r:r + W] = x
    return np.max([p[:, :, dy:dy + H, dx:dx + W] for dy in range(k) for dx in range(k)], axis=0)


def _cell_bytes(t, off, u8):
    """(flat byte indices, biased bytes) of a [B, C, H, W] array at channel offset `off` of tensor t's cells"""
    b, ch, y, x = np.meshgrid(*[np.arange(n) for n in u8.shape], indexing="ij")
    return ((t.lead + (b * (t.H + 1) + y + 1) * (t.W + 1) + x) * t.cs + off + ch).ravel(), (u8 ^ 0x80).ravel()


def _window(cat, off, Cn):
    t = binding.Tensor.from_buffer_copy(cat.t)
    t.data, t.C = cat.buf.ptr.value + off, Cn
    return t


# Tiles are the fewest equal ones of at most 20 a side (never below 8), channel chunks 32 bytes.  (C, H, W, sizes, data)
SIZES = [(5, 9, 13), (3, 5, 9), (3, 7), (5, 13), (13,), (3,)]
CASES = [
    (16, 1, 1, (5, 9, 13), "rand"), (17, 2, 3, (3, 5, 9), "rand"), (64, 6, 7, (3, 7), "rand"),   # maps smaller than the halo
    (80, 13, 13, (5, 9, 13), "rand"), (16, 19, 19, (5, 13), "rand"),                             # the block's real maps
    (17, 20, 9, (13,), "rand"), (16, 21, 8, (3,), "rand"),                                       # either side of the tile's height
    (16, 9, 20, (5, 9, 13), "rand"), (16, 8, 21, (3, 5, 9), "rand"),                             # ... and of its width
    (80, 23, 45, (5, 9, 13), "rand"),                                                            # 2 x 3 tiles, three chunks
] + [(16, 23, 25, s, "impulse") for s in SIZES]                                                  # 2 x 2 tiles of 12 x 13


@pytest.mark.parametrize("case", range(len(CASES)), ids=lambda i: "C%d_%dx%d_%s_%s" % CASES[i])
def test_kernel_vs_numpy(case):
    Cn, H, W, sizes, data = CASES[case]
    Cp, n = (Cn + 15) // 16 * 16, len(sizes)  # the kernels read and store whole 16-byte groups: the spare bytes are pooled like channels
    rng = np.random.default_rng(2000 + case)
    if data == "rand":
        x = rng.integers(0, 256, (B, Cp, H, W), dtype=np.uint8)
    else:  # one 255 per map: a corner, an edge, the first cell behind the tile seam, the interior
        x = np.zeros((B, Cp, H, W), np.uint8)
        spots = [(0, 0), (H - 1, W // 3), (12, 13), (H // 2 + 2, W // 2 - 1)]
        for b in range(B):
            for c in range(Cp):
                x[(b, c) + spots[(b + c) % 4]] = 255
    want = [_pool(x, k) for k in sizes]  # (an impulse: 255 exactly on the k x k window around it, 0 elsewhere)
    # the block's concat: (largest pool, ..., smallest pool, x), every window Cp bytes of the cell
    cat = binding.DevTensor(B, H, W, (n + 1) * Cp, 0)
    buf = np.full(cat.buf.nbytes, 0x5A, np.uint8)  # a sentinel everywhere
    idx, val = _cell_bytes(cat.t, n * Cp, x)
    buf[idx] = val
    binding.check(binding.shim().mi355_h2d(cat.buf.ptr, buf.ctypes.data, buf.nbytes, None), "h2d")
    xt = _window(cat, n * Cp, Cn)
    ys = [_window(cat, (n - 1 - i) * Cp, Cn) for i in range(n)]
    for i in range(n):
        idx, val = _cell_bytes(cat.t, (n - 1 - i) * Cp, want[i])
        buf[idx] = val
    assert binding.spp_forward(xt, sizes, ys) == 0
    assert np.array_equal(cat.buf.to_numpy(np.uint8, buf.size), buf), "concat buffer: x, pad cells and every window included"
    # the same call into separate tensors stores what the plain kernel stores
    sep = [binding.DevTensor(B, H, W, Cn, 77) for _ in sizes]
    assert binding.spp_forward(xt, sizes, sep) == 0
    for k, y in zip(sizes, sep):
        plain = binding.DevTensor(B, H, W, Cn, 77)
        binding.check(binding.shim().mi355_maxpool_forward(xt, plain.ref(), k, 1, k - 1, None), "maxpool")
        assert np.array_equal(y.buf.to_numpy(np.uint8, y.buf.nbytes), plain.buf.to_numpy(np.uint8, y.buf.nbytes)), k


REFUSALS = {
    "even size": dict(sizes=(4, 9, 13)), "equal sizes": dict(sizes=(5, 5, 13)), "decreasing sizes": dict(sizes=(9, 5, 13)),
    "15": dict(sizes=(5, 9, 15)), "n = 0": dict(sizes=()), "n = 4": dict(sizes=(3, 5, 7, 9)), "cs of 4": dict(cs=4),
    "another map size": dict(other=True), "null": dict(null=True),
}


@pytest.mark.parametrize("what", list(REFUSALS))
def test_refusals_write_nothing(what):
    r = REFUSALS[what]
    sizes = r.get("sizes", (5, 9, 13))
    x = binding.DevTensor(1, 6, 6, 16, 0)
    ys = [binding.DevTensor(1, 6, 7 if r.get("other") and i == 1 else 6, 16, 33) for i in range(max(len(sizes), 1))]
    before = [y.buf.to_numpy(np.uint8, y.buf.nbytes) for y in ys]
    xt = binding.Tensor.from_buffer_copy(x.t)
    xt.cs = r.get("cs", xt.cs)
    args = ys[:len(sizes)]
    if r.get("null"):
        args = args[:-1] + [None]
    assert binding.spp_forward(xt, sizes, args) == -22
    assert "spp:" in binding.shim().mi355_last_error().decode()
    for y, b in zip(ys, before):
        assert np.array_equal(y.buf.to_numpy(np.uint8, y.buf.nbytes), b)


def test_host_group_equals_its_parity_dump(cfg_dir, tmp_path):
    """spp_unit: the parity dump runs the plain pools; the latency plan, graph replay, the throughput plan with a replica beside its
    parent and a packed import run the fused group and give the same tensors.  A leader of size 4 forms no group: the planner refuses
    all the launcher refuses on tensors the host allocates, so the executor's fallback behind MI355_EINVAL is not reachable from here."""
    cfg, wts, cfg4 = os.path.join(cfg_dir, "spp_unit.cfg"), str(tmp_path / "spp.weights"), str(tmp_path / "size4.cfg")
    synth.synth_weights(cfg, wts, seed=6)
    with open(cfg4, "w") as f:
        f.write(open(cfg).read().replace("size=5", "size=4", 1))
    x, x2 = (synth.synth_image_u8(3, 26, 26, seed=s, batch=B) for s in (31, 32))
    pull = lambda net: (net.sync(), [net.pull(i) for i in range(net.n)])[1]

    def run(c, xin, group, keep=False, **kw):
        net = binding.Net(c, wts, batch=B, **kw)
        net.prepare_fixed(1.0 / 255.0, 0)
        net.push_input(xin)
        for _ in range(3 if kw.get("use_graph") else 1):
            net.forward()
        assert [net.spp(i) for i in (2, 4, 6)] == group
        got = pull(net)
        return (net, got) if keep else (net.close(), got)[1]

    def same(got, want, what):
        for i, (g, w) in enumerate(zip(got, want)):
            for key in (g.keys() & w.keys()) - {"int32"}:
                assert np.array_equal(g[key], w[key]), (what, i, key)

    want, want2, want4 = (run(c, xin, [0, 0, 0], dump_int32=True) for c, xin in ((cfg, x), (cfg, x2), (cfg4, x)))
    same(run(cfg, x, [1, 2, 2], use_graph=True), want, "graph replay")
    same(run(cfg4, x, [0, 0, 0]), want4, "a leader of size 4")
    parent, got = run(cfg, x, [1, 2, 2], keep=True)
    same(got, want, "latency plan")
    packed = parent.export_packed()
    rep = parent.replica()  # switches the parent to the throughput plan
    rep.push_input(x2); parent.push_input(x); rep.sync(); parent.sync()
    for _ in range(3):
        rep.forward(); parent.forward()
    same(pull(parent), want, "throughput plan, parent")
    same(pull(rep), want2, "replica")
    assert [rep.spp(i) for i in (2, 4, 6)] == [1, 2, 2]
    rep.close(); parent.close()
    imp = binding.Net(cfg, None, batch=B)
    imp.import_packed(packed); imp.push_input(x); imp.forward()
    same(pull(imp), want, "packed import")
    assert [imp.spp(i) for i in (2, 4, 6)] == [1, 2, 2]
    imp.close()
