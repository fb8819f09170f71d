"""Input quantisation on the device (set_input_quantization_on_device): mi355_input_pairs and mi355_l0_derive through the C-ABI, the
host's device input paths with the mode on, Net.set_input_on_device and `detector test -input_device`.

Every comparison is exact: bytes and float bits.  What is expected never comes from the code under test: bank entries from the host
prep (network_layer0_entry), pairs from the oracle's quantiser, whole runs from the synchronous path of a second network on the same
data and from OracleNet prepared with each image's pair."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import input_on_device_cases as cases
import oracle
from frames_util import _bits, _blocks, _write_ppm
from yolo_quantization_amd import binding, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE = 12


@pytest.fixture(scope="module", autouse=True)
def _dev():
    binding.init(0)


def _wts(tmp_path, cfg, seed=3):
    p = str(tmp_path / (os.path.basename(cfg) + f".{seed}.weights"))
    synth.synth_weights(cfg, p, seed=seed)
    return p


# ------------------------------------------------------------------------------------------------ 1. the derive kernel
def _derive(net, pairs, shared=False):
    """mi355_l0_derive on a bank of len(pairs) slots (one with shared) initialised with the network's prepared blob and fed `pairs`
    directly -> (slots [E][entry_bytes], scale, zp, kept scale, kept zp, status, the prepared blob)"""
    B = len(pairs)
    E = 1 if shared else B
    size = binding.shim().mi355_conv_pack_size(net.info[0]["n"], 3, 3)
    eb = (size + 255) & ~255
    blob = np.zeros(eb, np.uint8)
    blob[:size] = net.layer0_entry(1.0 / 255.0, 0)
    consts = net.layer0_consts()
    bufs = dict(consts=consts, bank=np.tile(blob, E), scale=np.array([p[0] for p in pairs], np.float32),
                zp=np.array([p[1] for p in pairs], np.uint8), kscale=np.full(B, np.float32(1.0 / 255.0), np.float32),
                kzp=np.zeros(B, np.uint8), status=np.zeros(B, np.uint32))
    dev = {k: binding.DevBuf.from_numpy(v) for k, v in bufs.items()}
    binding.check(binding.shim().mi355_l0_derive(dev["consts"].ptr, consts.ctypes.data, dev["bank"].ptr, eb, B, int(shared), dev["scale"].ptr,
                                                 dev["zp"].ptr, dev["kscale"].ptr, dev["kzp"].ptr, dev["status"].ptr, None), "mi355_l0_derive")
    out = (dev["bank"].to_numpy(np.uint8, E * eb).reshape(E, eb), dev["scale"].to_numpy(np.float32, B), dev["zp"].to_numpy(np.uint8, B),
           dev["kscale"].to_numpy(np.float32, B), dev["kzp"].to_numpy(np.uint8, B), dev["status"].to_numpy(np.uint32, B), blob)
    for d in dev.values():
        d.free()
    return out


SWEEP = [(f, a, False) for f in cases.FILTERS for a in cases.ACTS] + [(f, a, True) for f, a in cases.STATE_MODELS]


@pytest.mark.parametrize("filters,act,crafted", SWEEP)
def test_derived_entries_equal_the_host_prep(tmp_path, filters, act, crafted):
    """the table of test_input_on_device_cpu.py: every first layer and pair, the crafted model with its tiny scales (pow2 = 0, EPT_D2)"""
    net = binding.Net(*cases.make_model(tmp_path, filters, act, crafted))
    net.prepare_host_only(1.0 / 255.0, 0)
    table = dict(cases.pairs_table(), **(cases.TINY if crafted else {}))
    names = list(table) + ["M too large"]
    pairs = [table[k] for k in table] + [cases.M_TOO_LARGE]
    slots, s, z, ks, kz, status, blob = _derive(net, pairs)
    size = len(net.layer0_entry(1.0 / 255.0, 0))
    for e, name in enumerate(names[:-1]):
        want = net.layer0_entry(pairs[e][0], pairs[e][1])
        assert status[e] == 0, name
        assert np.array_equal(slots[e][:size], want), f"{name}: entry bytes differ at {np.flatnonzero(slots[e][:size] != want)[:8]}"
        assert not slots[e][size:].any(), name
        assert _bits(ks[e]) == _bits(pairs[e][0]) == _bits(s[e]) and kz[e] == pairs[e][1] == z[e], name
    if crafted:
        flags = {int(np.frombuffer(slots[e].tobytes(), "<u4", 1, cases.blob_header(slots[e].tobytes())["off_ept"] + 4)[0]) for e in range(len(table))}
        assert all(f & cases.EPT_D2 for f in flags) and {bool(f & cases.EPT_POW2) for f in flags} == {True, False}
    # M >= 1 in every channel: the bit, the slot untouched, the pair back at the one the slot stands for
    hdr, ch = cases.consts_of(net)
    assert (cases.M_TOO_LARGE[0] * ch["w_scale"] / hdr["s_act"] >= 1).all()
    assert status[-1] == cases.M_RANGE
    assert np.array_equal(slots[-1], blob)
    assert _bits(s[-1]) == _bits(np.float32(1.0 / 255.0)) == _bits(ks[-1]) and z[-1] == 0 == kz[-1]
    net.close()


def test_derive_shared_writes_entry_0_and_every_images_pair(tmp_path):
    cfg = cases.write_l0_cfg(tmp_path / "l0.cfg", 16, "leaky")
    net = binding.Net(cfg, _wts(tmp_path, cfg))
    net.prepare_host_only(1.0 / 255.0, 0)
    pair = cases.pair_of(1.4, -0.7)
    slots, s, z, ks, kz, status, blob = _derive(net, [pair] * 3, shared=True)
    want = net.layer0_entry(*pair)
    assert np.array_equal(slots[0][:len(want)], want) and not status.any()
    assert (_bits(ks) == _bits(pair[0])).all() and (kz == pair[1]).all()
    slots, s, z, ks, kz, status, blob = _derive(net, [cases.M_TOO_LARGE] * 3, shared=True)
    assert np.array_equal(slots[0], blob) and (status == cases.M_RANGE).all()
    assert (_bits(s) == _bits(np.float32(1.0 / 255.0))).all() and not z.any()
    net.close()


# -------------------------------------------------------------------------------------------------- 2. the pair kernel
MINMAX = [(1.0, 0.0), (1.0, -0.5), (0.7, -0.0), (0.0, -1.0), (1e-3, -3.0), (0.0, -1e-30), (254.0 / 255.0, 0.0), (3.0, -0.1), (0.5, -0.5),
          (1.0, -1e-3), (0.0, 0.0)]  # (max, min); the last one is the all-zero image


def _pairs(mm, shared, prev=(0.25, 9)):
    B = len(mm)
    dev = dict(mm=np.array(mm, np.float32).ravel(), entry=np.full(B, -1, np.int32), scale=np.full(B, prev[0], np.float32),
               zp=np.full(B, prev[1], np.uint8), status=np.full(B, 0xFFFF, np.uint32))
    dev = {k: binding.DevBuf.from_numpy(v) for k, v in dev.items()}
    binding.check(binding.shim().mi355_input_pairs(dev["mm"].ptr, B, int(shared), dev["entry"].ptr, dev["scale"].ptr, dev["zp"].ptr,
                                                   dev["status"].ptr, None), "mi355_input_pairs")
    out = (dev["entry"].to_numpy(np.int32, B), dev["scale"].to_numpy(np.float32, B), dev["zp"].to_numpy(np.uint8, B),
           dev["status"].to_numpy(np.uint32, B))
    for d in dev.values():
        d.free()
    return out


def test_pairs_equal_the_oracles_quantiser():
    entry, s, z, status = _pairs(MINMAX, shared=False)
    assert np.array_equal(entry, np.arange(len(MINMAX)))
    zps = set()
    for b, (mx, mn) in enumerate(MINMAX[:-1]):
        _, ws, wz = oracle.quantize_image(np.array([mx, mn], np.float32))
        assert status[b] == 0 and _bits(s[b]) == _bits(ws) and z[b] == wz, (mx, mn)
        assert (_bits(ws), wz) == (_bits(cases.pair_of(mx, mn)[0]), cases.pair_of(mx, mn)[1])  # the shared helper states the same
        zps.add(int(wz))
    assert {0, 255} <= zps and len(zps) > 4  # both clamps and values between them
    assert status[-1] == cases.ALL_ZERO and _bits(s[-1]) == _bits(np.float32(0.25)) and z[-1] == 9  # kept what it held
    # shared: slot 0's pair everywhere; an all-zero image 0 flags every slot and keeps every pair
    entry, s, z, status = _pairs(MINMAX[1:4], shared=True)
    _, ws, wz = oracle.quantize_image(np.array(MINMAX[1], np.float32))
    assert not entry.any() and not status.any() and (_bits(s) == _bits(ws)).all() and (z == wz).all()
    entry, s, z, status = _pairs([MINMAX[-1], MINMAX[1]], shared=True)
    assert (status == cases.ALL_ZERO).all() and (_bits(s) == _bits(np.float32(0.25))).all() and (z == 9).all()


# ------------------------------------------------------------------------------------------------------ 3. end to end
def _float_images(B, seed):
    """the ranges of test_gpu_per_image._synth_images: zero points > 0, a near-constant image, images 0 and 1 sharing a pair"""
    rng = np.random.default_rng(seed)
    out = []
    for b in range(B):
        u = rng.random((3, SIZE, SIZE), dtype=np.float32)
        kind = b % 5
        if b == 1:
            x = out[0][::-1].copy()
        elif kind == 0:
            x = u * np.float32(0.8 + 0.05 * b + 0.01 * (seed % 7))
        elif kind == 1:
            x = (u - np.float32(0.35)) * np.float32(2.0 + 0.1 * b)
        elif kind == 2:
            x = np.float32(0.5) + u * np.float32(1e-3)
        elif kind == 3:
            x = -u * np.float32(0.2 + 0.01 * b)
        else:
            x = u * np.float32(3.0) - np.float32(0.1 * (b % 7))
        out.append(np.ascontiguousarray(x, np.float32))
    return out


def _u8_frames(B, seed):
    rng = np.random.default_rng(seed)
    sizes = [(53, 37), (12, 20), (12, 12), (30, 17), (13, 15)]
    return [rng.integers(10 * (b % 3), 256 - 40 * ((b + seed) % 4), (sizes[b % 5][1], sizes[b % 5][0], 3), dtype=np.uint8) for b in range(B)]


def _nv12_frames(B, seed):
    rng = np.random.default_rng(seed)
    out = []
    for b in range(B):
        w, h = [(53, 37), (12, 20), (12, 12), (30, 17), (13, 15)][b % 5]
        lo, hi = 20 * (b % 3), 236 - 30 * ((b + seed // 10) % 5)  # near-neutral chroma: no channel saturates, the maximum follows hi
        out.append((rng.integers(lo, hi, (h, w), dtype=np.uint8), rng.integers(118, 138, ((h + 1) // 2, (w + 1) // 2, 2), dtype=np.uint8)))
    return out


class _Source:
    """one kind of input for both networks: feed(net, batch index) -> the uint8 input the device holds"""

    def __init__(self, kind, B):
        self.kind, self.B, self.bufs = kind, B, []

    def feed(self, net, k):
        seed = 100 + 50 * k
        if self.kind == "float":
            net.prepare_from_float_gpu(np.stack(_float_images(self.B, seed)))
        elif self.kind == "float_host":  # the host quantiser: its pairs go up, layer 0 is derived from them on the device all the same
            net.prepare_from_float(np.stack(_float_images(self.B, seed)))
        elif self.kind == "u8":
            net.prepare_from_frames_u8(_u8_frames(self.B, seed))
        elif self.kind == "packed":
            net.prepare_from_frames_packed([np.concatenate([f, np.full(f.shape[:2] + (1,), 0xEE, np.uint8)], axis=2) for f in _u8_frames(self.B, seed)],
                                           format="rgba")
        else:  # NV12 planes that already lie in device memory
            dev = []
            for y, uv in _nv12_frames(self.B, seed):
                h, w = y.shape
                by, buv = binding.DevBuf.from_numpy(y), binding.DevBuf.from_numpy(uv)
                self.bufs += [by, buv]
                dev.append((by.ptr.value, buv.ptr.value, w, h, w, 2 * ((w + 1) // 2)))
            got = net.prepare_from_frames_nv12(dev, on_device=True)
            assert (got is None) == bool(getattr(net, "input_on_device", False))
        return net._pull_input()

    def free(self):
        for b in self.bufs:
            b.free()


def _run(net):
    net.forward()
    net.sync()
    outs = [net.pull(i) for i in range(net.n)]
    dets = net.detect([SIZE] * net.batch, [SIZE] * net.batch, thresh=0.005)
    return outs, dets


def _assert_same(got, want, what):
    (oa, da), (ob, db) = got, want
    for i, (a, b) in enumerate(zip(oa, ob)):
        assert a.keys() == b.keys()
        for k in a:
            assert np.array_equal(a[k], b[k]), f"{what}: layer {i} {k}"
    assert len(da) == len(db)
    for x, y in zip(da, db):
        assert x.keys() == y.keys()
        for k in x:
            assert np.array_equal(np.asarray(x[k]), np.asarray(y[k])), f"{what}: detections {k}"


@pytest.mark.parametrize("source", ["float", "float_host", "u8", "nv12dev", "packed"])
@pytest.mark.parametrize("accum", [binding.ACC_EXACT, binding.ACC_REF_F32])
@pytest.mark.parametrize("per_image", [True, False])
def test_on_device_run_equals_the_synchronous_run_and_the_oracle(tmp_path, per_image, accum, source):
    cfg = cases.write_net_cfg(tmp_path / "net.cfg", SIZE)
    wts = _wts(tmp_path, cfg)
    B = 5
    onet = oracle.OracleNet(cfg, wts)
    for dump in (True, False):  # dump_int32 off: layer 0 reads the planes in place, the fused forms run
        dev = binding.Net(cfg, wts, batch=B, accum=accum, dump_int32=dump)
        ref = binding.Net(cfg, wts, batch=B, accum=accum, dump_int32=dump)
        for n in (dev, ref):
            n.set_input_per_image(per_image)
        dev.set_input_on_device(True)
        src = _Source(source, B)
        seen = []
        for k in range(2):  # the second batch brings other pairs to the same network: a stale slot would show
            what = f"dump {dump} batch {k}"
            xd, xr = src.feed(dev, k), src.feed(ref, k)
            assert np.array_equal(xd, xr), f"{what}: input bytes"
            (sd, zd), (sr, zr) = dev.input_quantization(), ref.input_quantization()
            assert np.array_equal(_bits(sd), _bits(sr)) and np.array_equal(zd, zr), f"{what}: pairs"
            assert not dev.input_status().any()
            size = len(dev.layer0_entry(sd[0], zd[0]))
            for b in range(B):
                e = dev.input_bank_entry(b)
                assert np.array_equal(e[:size], dev.layer0_entry(sd[b], zd[b])) and not e[size:].any(), f"{what}: bank entry {b}"
            got = _run(dev)
            _assert_same(got, _run(ref), what)
            if dump:
                for b in range(B):
                    onet.prepare(sd[b], int(zd[b]))
                    want = onet.forward(xd[b * dev.inputs:(b + 1) * dev.inputs].reshape(3, SIZE, SIZE), accum=accum)
                    for i, inf in enumerate(dev.info):
                        if inf["type"] == binding.T_YOLO:
                            continue
                        per = inf["outputs"]
                        assert np.array_equal(got[0][i]["u8"][b * per:(b + 1) * per], want[i]["u8"].ravel()), f"{what}: oracle slot {b} layer {i}"
            seen.append((sd.tobytes(), zd.tobytes()))
        assert seen[0] != seen[1]
        assert per_image == (len(set(sd.tolist())) > 1)
        src.free()
        dev.close(); ref.close()


# ----------------------------------------------------------------------------------------------------- 4. no host wait
def _device_nv12(B, seed, keep):
    dev = []
    for y, uv in _nv12_frames(B, seed):
        h, w = y.shape
        by, buv = binding.DevBuf.from_numpy(y), binding.DevBuf.from_numpy(uv)
        keep += [by, buv]
        dev.append((by.ptr.value, buv.ptr.value, w, h, w, 2 * ((w + 1) // 2)))
    return dev


@pytest.mark.parametrize("per_image", [True, False])
def test_no_host_wait_between_frames_and_detections(tmp_path, per_image):
    cfg = cases.write_net_cfg(tmp_path / "net.cfg", SIZE)
    wts = _wts(tmp_path, cfg)
    B, keep = 5, []
    batches = [_device_nv12(B, 10 + k, keep) for k in range(4)]
    rose = {}
    for on in (True, False):
        net = binding.Net(cfg, wts, batch=B)
        net.set_input_per_image(per_image)
        net.set_input_on_device(on)
        net.prepare_from_frames_nv12(batches[0], on_device=True)  # warm-up: preparation, allocations
        net.forward()
        net.sync()
        before = net.host_waits()
        for k in (1, 2, 3):
            assert (net.prepare_from_frames_nv12(batches[k], on_device=True) is None) == on
            net.forward()
        rose[on] = net.host_waits() - before
        net.sync()
        assert not net.input_status().any()
        net.close()
    assert rose[True] == 0
    assert rose[False] >= 3
    for b in keep:
        b.free()


# ----------------------------------------------------------------------------------------------------- 5. graph replay
def test_graph_replay_shared_scale_follows_new_pairs(tmp_path):
    cfg = cases.write_net_cfg(tmp_path / "net.cfg", SIZE)
    wts = _wts(tmp_path, cfg)
    B = 5
    eager, graph = binding.Net(cfg, wts, batch=B), binding.Net(cfg, wts, batch=B, use_graph=True)
    for n in (eager, graph):
        n.set_input_on_device(True)
    handle, pairs = None, set()
    for k in range(3):
        x = np.stack(_float_images(B, 7 + 3 * k)[::-1] if k == 1 else _float_images(B, 7 + 3 * k))
        res = []
        for n in (eager, graph):
            n.prepare_from_float_gpu(x)
            res.append(_run(n))
        _assert_same(res[1], res[0], f"batch {k}")
        if handle is None:
            handle = graph.graph_handle()
            assert handle
        assert graph.graph_handle() == handle  # one captured graph, whatever the pair
        s, z = graph.input_quantization()
        pairs.add((s[0].tobytes(), int(z[0])))
    assert len(pairs) == 3 and len({p[1] for p in pairs}) > 1  # the zero point changed too
    eager.close(); graph.close()


# ---------------------------------------------------------------------------------------------------------- 6. replicas
def test_parent_and_replicas_back_to_back(tmp_path):
    cfg = cases.write_net_cfg(tmp_path / "net.cfg", SIZE)
    wts = _wts(tmp_path, cfg)
    B, keep = 5, []
    parent = binding.Net(cfg, wts, batch=B)
    parent.set_input_per_image(True)
    parent.set_input_on_device(True)
    parent.prepare_from_frames_nv12(_device_nv12(B, 1, keep), on_device=True)
    nets = [parent, parent.replica(), parent.replica()]
    batches = [_device_nv12(B, 20 + k, keep) for k in range(3)]
    for net, fr in zip(nets, batches):  # fed back to back, nothing waited for in between
        assert net.prepare_from_frames_nv12(fr, on_device=True) is None
        net.forward()
    ref = binding.Net(cfg, wts, batch=B)
    ref.set_input_per_image(True)
    for k, (net, fr) in enumerate(zip(nets, batches)):
        xw, sw, zw = ref.prepare_from_frames_nv12(fr, on_device=True)
        assert np.array_equal(net._pull_input(), xw)
        s, z = net.input_quantization()
        assert np.array_equal(_bits(s), _bits(sw)) and np.array_equal(z, zw)
        ref.forward()
        ref.sync()
        for i in range(net.n):
            got, want = net.pull(i), ref.pull(i)
            for key in want:
                if key in got:
                    assert np.array_equal(got[key], want[key]), f"executor {k} layer {i} {key}"
    for n in nets[:0:-1]:
        n.close()
    ref.close(); parent.close()
    for b in keep:
        b.free()


# -------------------------------------------------------------------------------------------------------- 7. black frame
def test_black_frame_keeps_its_slot_and_is_flagged(tmp_path):
    cfg = cases.write_net_cfg(tmp_path / "net.cfg", SIZE)
    wts = _wts(tmp_path, cfg)
    B = 5
    first, second = _u8_frames(B, 3), _u8_frames(B, 4)
    second[2] = np.zeros((24, 24, 3), np.uint8)  # the net's aspect ratio: no grey bars, every letterboxed sample is 0
    net = binding.Net(cfg, wts, batch=B, dump_int32=True)
    ref = binding.Net(cfg, wts, batch=B, dump_int32=True)
    for n in (net, ref):
        n.set_input_per_image(True)
    net.set_input_on_device(True)
    net.prepare_from_frames_u8(first)
    kept_s, kept_z = (a[2] for a in net.input_quantization())
    x = net.prepare_from_frames_u8(second)[0]
    assert np.array_equal(net.input_status(), np.array([0, 0, cases.ALL_ZERO, 0, 0], np.uint32))
    s, z = net.input_quantization()
    assert _bits(s[2]) == _bits(kept_s) and z[2] == kept_z
    assert (x[2 * net.inputs:3 * net.inputs] == kept_z).all()
    got = _run(net)
    healthy = list(second)
    healthy[2] = first[2]
    xr = ref.prepare_from_frames_u8(healthy)[0]
    want = _run(ref)
    for b in (0, 1, 3, 4):
        assert np.array_equal(x[b * net.inputs:(b + 1) * net.inputs], xr[b * net.inputs:(b + 1) * net.inputs])
        for i, inf in enumerate(net.info):
            per = inf["outputs"]
            for key in want[0][i]:
                assert np.array_equal(got[0][i][key][b * per:(b + 1) * per], want[0][i][key][b * per:(b + 1) * per]), f"slot {b} layer {i} {key}"
    net.close(); ref.close()


# ------------------------------------------------------------------------------------------------------------------ 8. CLI
def test_cli_input_device_prints_what_it_prints_without(tmp_path):
    exe = os.path.join(ROOT, "yolo_quantization_amd", "bin", "darknet")
    cfg = cases.write_net_cfg(tmp_path / "net.cfg", SIZE)
    wts = _wts(tmp_path, cfg, seed=1)
    names = str(tmp_path / "x.names")
    open(names, "w").write("\n".join(["ant", "bee", "cat", "dog", "eel"]) + "\n")
    data = str(tmp_path / "x.data")
    open(data, "w").write(f"classes= 5\nnames = {names}\n")
    ppms = []
    for k, f in enumerate(_u8_frames(4, 9)):
        ppms.append(str(tmp_path / f"im{k}.ppm"))
        _write_ppm(ppms[-1], f)
    lst = str(tmp_path / "list.txt")
    open(lst, "w").write("\n".join(ppms) + "\n")

    def run(extra):
        r = subprocess.run([exe, "detector", "test", data, cfg, wts] + extra + ["-thresh", "0.3", "-boxes"], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        return _blocks(r.stdout)

    one = run([ppms[0], "-frames", "u8"])
    assert any(line.startswith("box:") for line in one[0])
    assert run([ppms[0], "-frames", "u8", "-input_device"]) == one
    many = run(["-list", lst, "-batch", "3", "-frames", "u8"])
    assert len(many) == 4
    assert run(["-list", lst, "-batch", "3", "-frames", "u8", "-input_device"]) == many
