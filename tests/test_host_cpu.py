"""CPU suite for the product's host side: the C-ABI library loads and exports every declared symbol, the packer and the
plain-C darknet host (cfg parser, .weights reader, integer prep) agree with the oracle / golden fixtures.
No compute kernels are launched here (no GPU in this container)."""
import ctypes as C
import hashlib
import json
import os
import re
import sys

import numpy as np
import pytest

import oracle
from epilogue_points import read_ept
from yolo_quantization_amd import binding, synth

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def _declared(header, prefix_re):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(" + prefix_re + r")\s*\(", txt)))


def test_shim_exports_every_declared_symbol():
    names = _declared("mi355_yolo_int8.h", r"mi355_\w+")
    assert len(names) >= 30
    L = binding.shim()
    missing = [n for n in names if not hasattr(L, n)]
    assert not missing, missing


def test_host_exports_every_declared_symbol():
    names = _declared("darknet_q.h", r"[a-z_]+\w*")
    names = [n for n in names if n not in ("defined", "sizeof", "void") and not n.startswith("mi355")]
    L = binding.host()
    missing = [n for n in names if not hasattr(L, n)]
    assert not missing, missing
    assert "forward_network_gpu" in names and "quantization_weights_and_activations" in names


def test_ctypes_structs_match_the_c_header(tmp_path):
    """The Python mirror of the C-ABI's structs (binding.ConvDesc / Tensor) has the header's layout: a field added to one side only (round 5:
    mi355_conv_desc.epilogue_packed) would shift every call's arguments silently."""
    import subprocess
    fields = {"mi355_conv_desc": [f[0] for f in binding.ConvDesc._fields_], "mi355_tensor": [f[0] for f in binding.Tensor._fields_]}
    src = "#include <stddef.h>\n#include <stdio.h>\n#include \"mi355_yolo_int8.h\"\nint main(void) {\n"
    for st, names in fields.items():
        src += f'    printf("{st} %zu", sizeof({st}));\n'
        for n in names:
            src += f'    printf(" %zu", offsetof({st}, {n}));\n'
        src += '    printf("\\n");\n'
    src += "    return 0;\n}\n"
    c = tmp_path / "layout.c"
    c.write_text(src)
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    for line, (st, cls) in zip(out, [("mi355_conv_desc", binding.ConvDesc), ("mi355_tensor", binding.Tensor)]):
        vals = [int(v) for v in line.split()[1:]]
        assert vals[0] == C.sizeof(cls), st
        assert vals[1:] == [getattr(cls, f[0]).offset for f in cls._fields_], st


def test_no_device_fails_loudly():
    """On a box without a gfx950 the product must refuse, not fall back."""
    L = binding.shim()
    if L.mi355_device_count() > 0:
        pytest.skip("a GPU is present")
    assert L.mi355_init(0) < 0
    assert b"no HIP device" in L.mi355_last_error() or b"gfx950" in L.mi355_last_error()


def test_quant_multiplier_matches_golden(golden_dir):
    f = np.load(os.path.join(golden_dir, "funcs.npz"))
    H = binding.host()
    for m, m0, sh in zip(f["qm_M"], f["qm_M0"], f["qm_shift"]):
        a = C.c_int32(); b = C.c_int()
        H.quant_multi_smaller_than_one_to_scale_and_shift(float(m), C.byref(a), C.byref(b))
        assert (a.value, b.value) == (int(m0), int(sh))


@pytest.mark.parametrize("name", ["signed", "unit"])
def test_image_quantiser_matches_golden(golden_dir, name):
    f = np.load(os.path.join(golden_dir, "funcs.npz"))
    x = np.ascontiguousarray(f[f"qimg_{name}_x"])
    out = np.zeros(x.size, np.uint8); s = C.c_float(); z = C.c_uint8()
    binding.host().quant_image_with_min_max(x.size, x.ctypes.data, out.ctypes.data, C.byref(s), C.byref(z))
    assert np.float32(s.value) == f[f"qimg_{name}_scale"] and z.value == f[f"qimg_{name}_zp"]
    assert np.array_equal(out, f[f"qimg_{name}_u8"])


@pytest.mark.parametrize("tag", ["leaky", "relu6"])
def test_host_prep_matches_reference_hashes(golden_dir, cfg_dir, tmp_path, tag):
    """cfg parser + .weights reader + integer prep of the plain-C host == the reference's prep (golden SHA-256)."""
    g = json.load(open(os.path.join(golden_dir, f"yolov3_tiny_{tag}.json")))
    cfg = os.path.join(cfg_dir, g["cfg"])
    wts = str(tmp_path / "w.weights")
    synth.synth_weights(cfg, wts, seed=g["weight_seed"])
    net = binding.Net(cfg, wts)
    net.prepare_host_only(1.0 / 255.0, 0)
    _, shapes = synth.layer_shapes(synth.read_cfg(cfg))
    assert net.n == len(shapes)
    for i, (L, e) in enumerate(zip(shapes, g["layers"])):
        inf = net.info[i]
        assert (inf["out_c"], inf["out_h"], inf["out_w"]) == (L.out_c, L.out_h, L.out_w), i
        if "prep_sha256" in e:
            p = net.prep(i)
            h = hashlib.sha256(np.concatenate([p["biases_int32"].view(np.uint8), p["M_value"].view(np.uint8),
                                               p["shift_value"].view(np.uint8)]).tobytes()).hexdigest()
            assert h == e["prep_sha256"], f"layer {i}"
    net.close()


def _unpack_check(blob, wq, zp_w, c, ksize):
    """Decode the packed blob with an independent numpy reading of the documented layout and rebuild the GEMM
    operands; returns (W' [n,Kp] int8 in unit order, cw, dzp)."""
    hdr = np.frombuffer(blob, dtype=np.int32, count=11, offset=4)
    n, cc, ks, mpad, cb, nchunks, upc, spc, ksteps, ktrue, first = [int(v) for v in hdr[:11]]
    offs = np.frombuffer(blob, dtype=np.uint64, count=7, offset=48)  # magic + 11 ints = 48 bytes
    return dict(n=n, c=cc, ksize=ks, mpad=mpad, cb=cb, nchunks=nchunks, upc=upc, spc=spc, ksteps=ksteps, ktrue=ktrue,
                first=first, offs=[int(o) for o in offs])


@pytest.mark.parametrize("n,c,k", [(32, 16, 3), (30, 256, 1), (128, 64, 3), (256, 384, 3), (20, 48, 3), (16, 3, 3)])
def test_pack_blob_reconstructs_exact_accumulators(n, c, k):
    """Algebra check of the offset decomposition on the packed operands, CPU only:
    sum w'x' + d*sum x' + cw  ==  sum (w_u8 - zp_w) x_u8  for random data, via the blob's own contents."""
    rng = np.random.default_rng(n * 1000 + c + k)
    K = c * k * k
    wq = rng.integers(0, 256, (n, K), dtype=np.uint8)
    zp_w = rng.integers(0, 256, n, dtype=np.uint8)
    blob = binding.conv_pack(wq, zp_w, c, k, np.arange(n, dtype=np.int32), np.full(n, 0.5), np.full(n, 2.0 ** -9))
    h = _unpack_check(blob.tobytes(), wq, zp_w, c, k)
    assert (h["n"], h["c"], h["ksize"], h["ktrue"]) == (n, c, k, K)
    off_wp, off_cw, off_dzp, off_bias, off_mval, off_sval, total = h["offs"]
    assert total == blob.size
    cw = np.frombuffer(blob, np.int32, h["mpad"], off_cw)
    dzp = np.frombuffer(blob, np.int32, h["mpad"], off_dzp)
    assert np.array_equal(np.frombuffer(blob, np.int32, n, off_bias), np.arange(n))
    x = rng.integers(0, 256, K, dtype=np.uint8)  # one im2col column in the reference's (ci,ky,kx) order
    want = (wq.astype(np.int64) - zp_w[:, None].astype(np.int64)) @ x.astype(np.int64)
    if h["first"]:
        wp = np.frombuffer(blob, np.uint32, n * 9, off_wp).reshape(n, 9)
        xs = x.reshape(c, 9).astype(np.int64)
        got = np.zeros(n, np.int64)
        for t in range(9):
            for ci in range(3):
                got += ((wp[:, t] >> (8 * ci)) & 0xFF).astype(np.int64) * xs[ci, t]
        got -= (128 - dzp[:n].astype(np.int64)) * x.astype(np.int64).sum()
        assert np.array_equal(got, want)
        return
    cb, bpc = h["cb"], h["cb"] // 16
    wp = np.frombuffer(blob, np.int8, h["mpad"] * h["ksteps"] * 64, off_wp).reshape(h["mpad"] // 16, h["ksteps"], 4, 16, 16)
    xs = x.reshape(c, k * k).astype(np.int64) - 128  # x' per (ci, tap)
    mf = np.zeros(n, np.int64); sx = 0
    for chunk in range(h["nchunks"]):
        for s in range(h["spc"]):
            g = chunk * h["spc"] + s
            for kg in range(4):
                u = 4 * s + kg
                if u >= h["upc"]:
                    assert not wp[:, g, kg].any()
                    continue
                tap, blk = u // bpc, u % bpc
                ci0 = chunk * cb + blk * 16
                xv = xs[ci0:ci0 + 16, tap]
                wv = wp[:, g, kg].reshape(h["mpad"], 16)[:n].astype(np.int64)
                mf += wv @ xv
                sx += xv.sum()
    got = mf + dzp[:n].astype(np.int64) * sx + cw[:n].astype(np.int64)
    assert np.array_equal(got, want)
    assert np.abs(got).max() < 2 ** 31


# ------------------------------------------------------------------------------------------ round 2 additions
def test_saturate_mode_equals_mkl_epilogue_for_every_requantised_value(golden_dir):
    """`saturate` is builder-defined: the default path's formulas with the clamp moved before the uint8 store.  The MKL
    flavour (src/convolutional_layer.c:572-596) cannot be built here, but its epilogue is plain C and restated in
    orc_requant_mkl; its LEAKY multiplier (M0_lut0, shift) is pinned from the default build of the reference.  Exhaustive
    over all 2^31 + 1 non-positive int32 q: default-LEAKY + clamp and MKL-LEAKY + clamp store the same byte for every zero
    point, so `saturate` == the MKL epilogue for LEAKY (LINEAR / RELU6 are the same expressions; RELU differs: :591)."""
    g = json.load(open(os.path.join(golden_dir, "yolov3_tiny_leaky.json")))
    luts = {(e["M0_lut0"], e["M0_right_shift_lut0"]) for e in g["layers"] if e["type"] == "conv" and e["M0_lut0"]}
    assert luts == {(1717986944, 3)}          # == (float)0.1 exactly: 1717986944 * 2^-31 * 2^-3
    assert 1717986944 * 2.0 ** -34 == float(np.float32(0.1))
    L = oracle.lib()
    assert L.orc_mkl_leaky_mismatches(-2 ** 31, 0, 1717986944, 3) == 0
    assert L.orc_mkl_leaky_mismatches(1, 2 ** 20, 1717986944, 3) == 0
    # and through the two epilogue functions on random accumulators, every activation
    rng = np.random.default_rng(5)
    acc = rng.integers(-3_000_000, 3_000_000, (8, 4096)).astype(np.int32)
    acc[0, :64] = np.arange(-32, 32)
    bias = rng.integers(-1000, 1000, 8).astype(np.int32)
    mv = rng.uniform(0.5, 1.0, 8); sv = 2.0 ** -rng.integers(6, 14, 8).astype(np.float64)
    for act in (oracle.LEAKY, oracle.LINEAR, oracle.RELU6):
        a = oracle.requant(acc, bias, mv, sv, 23, act, oracle.STORE_SATURATE)
        b = oracle.requant_mkl(acc, bias, mv, sv, 23, act, 1717986944, 3)
        assert np.array_equal(a, b), act
    a = oracle.requant(acc, bias, mv, sv, 23, oracle.RELU, oracle.STORE_SATURATE)
    b = oracle.requant_mkl(acc, bias, mv, sv, 23, oracle.RELU, 1717986944, 3)
    assert not np.array_equal(a, b)           # documented difference: the MKL flavour adds no zero point for RELU


def test_shortcut_spec_properties():
    """The builder-specified quantized residual add (oracle.c:orc_shortcut_u8 is the normative statement): agrees with the
    real-valued sum to half an output step, saturates, is symmetric in its operands, and K follows the float ratio."""
    rng = np.random.default_rng(9)
    sa, sb, so = np.float32(6.6 / 255), np.float32(6.0 / 255), np.float32(9.5 / 255)
    za, zb, zo = 23, 0, 10
    Ka, Kb = oracle.shortcut_multiplier(sa, so), oracle.shortcut_multiplier(sb, so)
    assert Ka == int(np.floor(np.float64(np.float32(sa / so)) * 65536 + 0.5))
    a = rng.integers(0, 256, 100_000, dtype=np.uint8); b = rng.integers(0, 256, 100_000, dtype=np.uint8)
    y = oracle.shortcut_u8(a, b, Ka, Kb, za, zb, zo)
    real = (np.float64(sa) * (a.astype(np.int64) - za) + np.float64(sb) * (b.astype(np.int64) - zb)) / np.float64(so) + zo
    ideal = np.clip(np.floor(real + 0.5), 0, 255)
    assert np.abs(y.astype(np.int64) - ideal).max() <= 1 and (y != ideal).mean() < 0.02   # 16.16 multipliers: rare off-by-one at ties
    assert (y == 255).any() and (y == 0).any()
    assert np.array_equal(y, oracle.shortcut_u8(b, a, Kb, Ka, zb, za, zo))
    # exact integer restatement in numpy
    t = Ka * (a.astype(np.int64) - za) + Kb * (b.astype(np.int64) - zb) + 32768
    assert np.array_equal(y, np.clip(zo + (t >> 16), 0, 255).astype(np.uint8))
    K = C.c_int32()
    S = binding.shim()
    S.mi355_shortcut_multiplier.argtypes = [C.c_float, C.c_float, C.c_void_p]
    for s_in, s_out in ((sa, so), (sb, so), (so, sa), (np.float32(1.0), np.float32(0.05))):
        assert S.mi355_shortcut_multiplier(float(s_in), float(s_out), C.byref(K)) == 0
        assert K.value == oracle.shortcut_multiplier(s_in, s_out)
    assert S.mi355_shortcut_multiplier(1.0, 0.01, C.byref(K)) < 0       # ratio >= 32
    assert S.mi355_shortcut_multiplier(0.0, 0.01, C.byref(K)) < 0


@pytest.mark.parametrize("name,nconv,nshort", [("yolov3_quant", 75, 23), ("res_unit", 8, 2)])
def test_host_parses_residual_nets(cfg_dir, tmp_path, name, nconv, nshort):
    """cfg parser + weights reader + host prep of the nets with `[shortcut] quantized=1` (BASELINE config[4] is the real
    107-layer YOLOv3 topology): shapes equal the independent shape inference of synth.py, the shortcut multipliers equal
    the oracle's, a packed export / import round-trips (blobs + layer-0 record + shortcut records)."""
    cfg = os.path.join(cfg_dir, f"{name}.cfg")
    wts = str(tmp_path / "w.weights")
    synth.synth_weights(cfg, wts, seed=3)
    _, shapes = synth.layer_shapes(synth.read_cfg(cfg))
    net = binding.Net(cfg, wts)
    net.prepare_host_only(1.0 / 255.0, 0)
    assert net.n == len(shapes)
    assert sum(i["type"] == binding.T_CONV for i in net.info) == nconv
    assert sum(i["type"] == binding.T_SHORTCUT for i in net.info) == nshort
    onet = oracle.OracleNet(cfg, wts)
    onet.prepare(np.float32(1.0 / 255.0), 0)
    for i, (L, inf) in enumerate(zip(shapes, net.info)):
        assert (inf["out_c"], inf["out_h"], inf["out_w"]) == (L.out_c, L.out_h, L.out_w), i
        if L.type == "shortcut":
            ka, kb = net.shortcut_multipliers(i)
            assert ka == oracle.shortcut_multiplier(onet.act[i - 1][0], onet.act[i][0])
            assert kb == oracle.shortcut_multiplier(onet.act[L.inputs[1]][0], onet.act[i][0])
        if L.type == "conv":
            assert np.array_equal(net.prep(i)["biases_int32"], onet.p[i]["biases_int32"]), i
    packed = net.export_packed()
    f = str(tmp_path / "net.packed")
    net.save_packed(f)
    assert open(f, "rb").read() == packed.tobytes()
    net2 = binding.Net(cfg, None)
    net2.import_packed_host(packed)
    assert np.array_equal(net2.export_packed(), packed)
    for i, L in enumerate(shapes):
        if L.type == "shortcut":
            assert net2.shortcut_multipliers(i) == net.shortcut_multipliers(i)
    net.close(); net2.close()


def test_oracle_restatement_is_clean_under_asan_ubsan(tmp_path, cfg_dir):
    """SURVEY.md 5 (race detection / sanitizers row): the reference RELIES on undefined behaviour (out-of-range
    double -> uint8 conversions, src/convolutional_layer.c:737, src/maxpool_layer.c:143); the restatement must not.
    oracle.c is compiled with -fsanitize=address,undefined (-fno-sanitize-recover) together with a small driver that runs
    every entry point on wrap-on-store data, and must finish without a sanitizer report."""
    import shutil
    import subprocess
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    drv = os.path.join(ROOT, "tests", "sanitize_driver.c")
    exe = str(tmp_path / "orc_san")
    cmd = ["gcc", "-O1", "-g", "-std=c11", "-fno-fast-math", "-ffp-contract=off", "-fopenmp", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "oracle"), os.path.join(ROOT, "oracle", "oracle.c"), drv,
           "-o", exe, "-lm"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr.lower() or "cannot find" in r.stderr.lower()):
        pytest.skip("sanitizer runtime not installed: " + r.stderr[-200:])
    assert r.returncode == 0, r.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1", OMP_NUM_THREADS="2")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "sanitize_driver: OK" in r.stdout


@pytest.mark.parametrize("name", ["a", "b", "c", "empty"])
def test_host_nms_matches_reference(golden_dir, name):
    """do_nms_sort of the plain-C host (host/detect.c, ref: src/box.c:58-89) against scores the reference's own
    do_nms_sort kept / suppressed (tests/golden/nms.npz)."""
    g = np.load(os.path.join(golden_dir, "nms.npz"))
    boxes, obj, probs, want = g[f"{name}_boxes"], g[f"{name}_obj"], g[f"{name}_probs"].copy(), g[f"{name}_out"]
    n, classes = probs.shape
    H = binding.host()
    H.do_nms_sort_arrays.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float]
    H.do_nms_sort_arrays(boxes.ctypes.data, probs.ctypes.data, obj.ctypes.data, n, classes, float(g[f"{name}_thresh"]))
    assert np.array_equal(probs, want)
    if n > 10:
        assert (want == 0).sum() > (g[f"{name}_probs"] == 0).sum(), "fixture must contain suppressed scores"


def test_reference_side_binding_compiles_against_the_real_header(tmp_path):
    """INTEGRATION.md section B is code, not a sketch: integration/mi355_glue.c compiles against the reference's own
    include/darknet.h, integration/reference_mi355.patch applies to the reference's examples/detector.c and Makefile and
    the patched detector.c compiles with -DMI355.  (Build container only: needs /root/reference.)"""
    import shutil
    import subprocess
    ref = "/root/reference"
    if not os.path.isdir(os.path.join(ref, "src")):
        pytest.skip("reference sources are not on this box")
    inc = ["-DQUANTIZATION", "-DMI355", "-w", "-idirafter", f"{ref}/include", f"-I{ref}/src", f"-I{ROOT}/include", f"-I{ROOT}/integration"]
    r = subprocess.run(["gcc", "-fsyntax-only", "-Wall", "-Werror=implicit-function-declaration", "-Werror=incompatible-pointer-types"] + inc +
                       [os.path.join(ROOT, "integration", "mi355_glue.c")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    work = tmp_path / "ref"
    os.makedirs(work / "examples")
    shutil.copy(f"{ref}/Makefile", work / "Makefile")
    shutil.copy(f"{ref}/examples/detector.c", work / "examples" / "detector.c")
    r = subprocess.run(["patch", "-p1", "--binary", "-i", os.path.join(ROOT, "integration", "reference_mi355.patch")], cwd=work,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run(["gcc", "-fsyntax-only", "-Werror=implicit-function-declaration"] + inc + [str(work / "examples" / "detector.c")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert b"mi355_bind_network" in open(work / "examples" / "detector.c", "rb").read()
    assert b"MI355_ROOT" in open(work / "Makefile", "rb").read()
    # and the linked form the GPU tests run exists: the unmodified reference objects + the glue + libmi355yolo.so
    import refdrv
    if refdrv.available("mi355"):
        L = refdrv.lib("mi355")
        assert hasattr(L, "refdrv_mi355_bind") and hasattr(L, "mi355_bind_network") and hasattr(L, "forward_network_mi355")


def test_host_parser_swallows_the_reference_s_shipped_cfg(tmp_path, cfg_dir, golden_dir):
    """the repo's cfgs are regenerated (tools/make_cfg.py, training keys stripped); host/parser.c must also take
    the reference's OWN file (ref cfg/yolov3_tiny_quant_channelwise.cfg through ref src/parser.c:579-674's key set: `# Training`
    comments, `start_quantization_step`, spaced `saturation = 1.5`, blank lines), and the same file with CRLF line ends.  Checked:
    the 24 layer shapes of SURVEY.md section 8 and equality with the parse of the regenerated relu6 cfg.  The file is stored
    byte for byte as the fixture tests/golden/yolov3_tiny_quant_channelwise.cfg."""
    from yolo_quantization_amd import binding
    ref_cfg = os.path.join(golden_dir, "yolov3_tiny_quant_channelwise.cfg")
    crlf = tmp_path / "crlf.cfg"
    crlf.write_bytes(open(ref_cfg, "rb").read().replace(b"\r\n", b"\n").replace(b"\n", b"\r\n"))
    keys = ("type", "c", "h", "w", "n", "size", "stride", "pad", "out_c", "out_h", "out_w", "activation", "batch_normalize", "quantized", "quant_stop", "outputs")
    parses = []
    for p in (ref_cfg, str(crlf), os.path.join(cfg_dir, "yolov3-tiny_quant_relu6.cfg")):
        net = binding.Net(p, None)
        parses.append([tuple(inf[k] for k in keys) for inf in net.info])
        net.close()
    assert parses[0] == parses[1] == parses[2]
    # (type, Cin, Cout, out H) of the 24 layers; conv = 0, maxpool = 3, route = 8, yolo = 23, upsample = 26
    want = [(0, 3, 16, 416), (3, 16, 16, 208), (0, 16, 32, 208), (3, 32, 32, 104), (0, 32, 64, 104), (3, 64, 64, 52), (0, 64, 128, 52),
            (3, 128, 128, 26), (0, 128, 256, 26), (3, 256, 256, 13), (0, 256, 512, 13), (3, 512, 512, 13), (0, 512, 1024, 13),
            (0, 1024, 256, 13), (0, 256, 512, 13), (0, 512, 30, 13), (23, 30, 30, 13), (8, 0, 256, 13), (0, 256, 128, 13),
            (26, 128, 128, 26), (8, 0, 384, 26), (0, 384, 256, 26), (0, 256, 30, 26), (23, 30, 30, 26)]
    got = [(t[0], t[1], t[8], t[9]) for t in parses[0]]
    assert got == want


def test_error_dies_with_this_library_s_message_inside_python(tmp_path, cfg_dir):
    """The reference's error convention (ref src/utils.c:232-237: message, exit) must hold when libdarknet_q.so is loaded into a
    process whose executable already binds `error` to glibc's error(int, int, fmt, ...) -- python does: without -Bsymbolic-functions
    the host's own error("...") calls landed there, printed "python: " and crashed (round 4 finding)."""
    import subprocess
    code = f"""
import sys; sys.path.insert(0, {ROOT!r})
from yolo_quantization_amd import binding, synth
cfg = {os.path.join(cfg_dir, 'tiny_unit.cfg')!r}
synth.synth_weights(cfg, {str(tmp_path / 'w.weights')!r}, seed=1)
net = binding.Net(cfg, {str(tmp_path / 'w.weights')!r}, batch=2)
net.replica()   # not prepared: error()
"""
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 255, (r.returncode, r.stderr[-500:])
    assert "darknet_q: network_replica: the parent network is not prepared" in r.stderr


@pytest.mark.parametrize("n,c,act", [(16, 3, "leaky"), (32, 16, "leaky"), (64, 32, "relu6"), (128, 64, "linear"), (32, 3, "relu6"), (64, 16, "relu")])
def test_pack_epilogue_table(n, c, act):
    """mi355_conv_pack_epilogue (host side of the C-ABI, no GPU): per channel the table's range [lb, lb + rg] must be wrap-safe under the
    oracle's requantisation (ref src/convolutional_layer.c:726-751), and wherever it offers the integer form (m0 != 0) that form must equal the
    FP64 one over the whole range -- checked at both ends, around zero and on random accumulators, over multipliers / shifts that straddle
    intrq_make's accept / reject conditions (large shifts, few and many trailing zero bits of M0, tiny M)."""
    rng = np.random.default_rng(n + c)
    K = c * 9
    wq = rng.integers(0, 256, (n, K), dtype=np.uint8)
    zp_w = rng.integers(0, 256, n, dtype=np.uint8)
    bias = rng.integers(-5000, 5000, n).astype(np.int32)
    # M_value = M0 * 2^-31 with M0 in [2^30, 2^31): as the reference builds it from a float (>= 7 trailing zeros), plus odd M0s
    m0s = rng.integers(1 << 30, (1 << 31) - 1, n, dtype=np.int64)
    m0s[::2] &= ~np.int64(0x7F)
    m0s[1::4] = (m0s[1::4] >> 20) << 20
    mv = m0s.astype(np.float64) * 2.0 ** -31
    s = rng.integers(1, 20, n)
    s[:4] = [1, 2, 30, 31]
    sv = 2.0 ** -s.astype(np.float64)
    zp_act = 23 if act != "linear" else 128
    blob = binding.conv_pack(wq, zp_w, c, 3, bias, mv, sv, binding.ACT[act], zp_act)
    t = read_ept(blob)   # (tests/epilogue_points.py: the reader shared with the epilogue-point tests)
    off_ept, total, mpad, key, flags, ent = t["off"], t["total"], t["mpad"], t["key"], t["flags"], t["ent"]
    assert off_ept and total == blob.size
    kact = binding.ACT["linear"] if act == "relu" else binding.ACT[act]
    assert key == (0x45500000 | (kact << 8) | zp_act)
    oact = oracle.ACT[act]
    accepted = 0
    for ch in range(n):
        lb = int(ent[ch, 0]); rg = int(np.uint32(ent[ch, 1])); m0 = int(ent[ch, 2]); sh = int(ent[ch, 3])
        qc = int(np.frombuffer(ent[ch, 4:6].tobytes(), np.int64)[0]); cbl = int(ent[ch, 6])
        assert qc == lb * m0
        hi = lb + rg
        assert -(1 << 30) <= lb and hi < (1 << 30)
        cand = np.unique(np.clip(np.concatenate([[lb, lb + 1, hi - 1, hi, -1, 0, 1], rng.integers(lb, hi + 1, 400)]), lb, hi)).astype(np.int64)
        # accumulators as the kernel sees them: cw + bias + sum; the oracle adds `bias` itself, so feed acc = a - bias
        acc = (cand - int(bias[ch])).astype(np.int64)
        ok = np.abs(acc) < (1 << 31)
        cand, acc = cand[ok], acc[ok].astype(np.int32).reshape(1, -1)
        one = lambda arr: np.ascontiguousarray(arr[ch:ch + 1])
        wrap = oracle.requant(acc, one(bias), one(mv), one(sv), zp_act, oact, oracle.STORE_WRAP)
        sat = oracle.requant(acc, one(bias), one(mv), one(sv), zp_act, oact, oracle.STORE_SATURATE)
        if not (flags & 1):
            assert np.array_equal(wrap, sat), f"channel {ch}: a byte inside the table's range wraps"
        if m0:
            accepted += 1
            assert m0 == int(m0s[ch]) and sh == int(s[ch]) - 1
            # the integer form: f = floor(a * M0 / 2^(32 + sh)); q = trunc(fl(a * M_value) * 2^-s) in FP64
            for a in cand.tolist():
                if act == "relu6" and a < 0:
                    assert (a * m0) >> (32 + sh) < 0  # only the sign matters below zero (neg_any)
                    continue
                f = (a * m0) >> (32 + sh)
                q = int(np.trunc(np.float64(a) * mv[ch] * sv[ch]))
                assert q == (f + 1 if (a < 0 and (a * m0) % (1 << (32 + sh))) else f), (ch, a)
    assert bool(flags & 2) == (accepted < n)
    if c == 3 and act == "leaky":  # the first layer's byte table: entry i <-> f (all channels integer) or q = i - 3072
        lut = np.frombuffer(blob, np.uint8, 4096, t["lut_off"])
        for i in (0, 1, 3000, 3071, 3072, 3073, 3300, 4095):
            v = i - 3072
            q = v + 1 if (v < 0 and not (flags & 2)) else v
            want = (zp_act + (q if q >= 0 else -((-q + 5) // 10))) & 0xFF
            assert lut[i] == want ^ 0x80
    # a blob packed without the second step carries no key
    plain = binding.conv_pack(wq, zp_w, c, 3, bias, mv, sv)
    assert int(np.frombuffer(plain, np.uint32, 1, off_ept)[0]) == 0


def test_first_layer_tile_loop_has_no_memory_wait_inside_its_mfma_chains():
    """tools/check_l0_waits.py on the sources as they are (cross-compiles conv_aux.hip for gfx950, ~40 s): the 16-filter first-layer kernels must not
    carry an `s_waitcnt vmcnt` between a tile's B-fragment reads and the last MFMA of the chain -- a register-allocation accident that costs a
    memory round trip per tile and that no parity test can see."""
    import subprocess
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_l0_waits.py")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]


def test_no_register_of_a_hand_written_load_is_touched_before_its_wait(tmp_path):
    """tools/check_asm_loads.py: a load issued from inline asm is invisible to the compiler's wait-count model, so the register
    allocator may spill or copy its destination before the hand-written wait -- silently wrong bytes, and only in the instantiations that
    happen to spill.  The checker walks every kernel's control-flow graph with the hardware's vmcnt semantics.  (1) it finds the hazard in a
    unit written to have it; (2) every kernel of conv_aux.hip -- the one unit that ever carried such loads -- is clean."""
    import subprocess
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    tool = os.path.join(ROOT, "tools", "check_asm_loads.py")
    bad = tmp_path / "bad.hip"
    bad.write_text('#include <hip/hip_runtime.h>\n'
                   '__global__ void k(const unsigned *p, unsigned *o) {\n'
                   '    unsigned v = 7, off = threadIdx.x * 4;\n'
                   '    asm volatile("global_load_dword %0, %1, %2" : "+v"(v) : "v"(off), "s"(p) : "memory");\n'
                   '    o[threadIdx.x] = v;                       // read with the load in flight, as far as the compiler knows a plain register\n'
                   '    asm volatile("s_waitcnt vmcnt(0)" : "+v"(v)::"memory");\n'
                   '    o[threadIdx.x + 64] = v;\n'
                   '}\n')
    r = subprocess.run([sys.executable, tool, "--src", str(bad)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "still in flight" in r.stdout, r.stdout + r.stderr
    r = subprocess.run([sys.executable, tool], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]


def test_no_hand_written_register_loads_outside_the_ab_switch():
    """The product build issues no vector-memory load with a REGISTER destination from inline asm (the compiler cannot order such a load's
    register against its wait: test above).  The one historical site lives behind -DMI355_L0_ASM_PREFETCH (A/B builds of conv_aux.hip only);
    LDS-DMA instructions (`global_load_lds_*`: no destination register) are fine and everywhere."""
    import re
    src_dir = os.path.join(ROOT, "yolo_quantization_amd", "csrc")
    pat = re.compile(r'asm\s+volatile\s*\(\s*"[^"]*\b(global|buffer|flat|scratch)_load_(?!lds)', re.S)
    for fn in sorted(os.listdir(src_dir)):
        if not fn.endswith((".hip", ".h")):
            continue
        text = open(os.path.join(src_dir, fn)).read()
        # drop the A/B-only block
        text = re.sub(r"#ifdef MI355_L0_ASM_PREFETCH.*?#(else|endif)", "", text, flags=re.S)
        assert not pat.search(text), f"{fn}: inline-asm load with a register destination outside the A/B switch"
