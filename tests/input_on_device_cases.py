"""What the tests of the on-device input quantisation share (test_input_on_device_cpu.py, test_gpu_input_on_device.py): the cfgs they write,
the table of first layers and (scale, zero point) pairs the layer-0 derivation is swept over, and a plain numpy / Python restatement of
the two kernels' arithmetic (input_dev.hip).  Importing it touches no device."""
import ctypes as C
import struct

import numpy as np

from yolo_quantization_amd import binding, synth

FILTERS = [4, 16, 20, 32, 64]  # 4: below one 16-row block; 20: the second block partly filled
ACTS = ["leaky", "relu6", "linear", "relu"]
ACT_ID = {"relu": 1, "linear": 3, "relu6": 8, "leaky": 9}  # MI355_ACT_* = the reference's ACTIVATION values

# status bits (mi355_yolo_int8.h MI355_INPUT_*)
ALL_ZERO, ZERO_SCALE, M_RANGE, NEG_SHIFT, PACK_RANGE, BIAS_RANGE, BAD_SLOT = 1, 2, 4, 8, 16, 32, 64
# epilogue-table flags (common.h EPT_*)
EPT_NEVER, EPT_NOINT, EPT_POW2, EPT_D2 = 1, 2, 4, 8

_L0 = """[net]
batch=1
subdivisions=1
width={size}
height={size}
channels=3

[convolutional]
batch_normalize=1
filters={filters}
size=3
stride=1
pad=1
activation={act}
quantized=1
quant_stop=0
"""
_HEAD = """
[convolutional]
filters=30
size=1
stride=1
pad=1
activation=linear
quantized=1
quant_stop=1

[yolo]
mask = 0,1,2
anchors = 10,14,  23,27,  37,58,  81,82,  135,169,  344,319
classes=5
num=6
jitter=.3
ignore_thresh = .7
truth_thresh = 1
random=1
"""
_BODY = """
[maxpool]
size=2
stride=2
quantized=1
quant_stop=0

[convolutional]
batch_normalize=1
filters=32
size=3
stride=1
pad=1
activation=leaky
quantized=1
quant_stop=0

[maxpool]
size=2
stride=1
quantized=1
quant_stop=0

[convolutional]
batch_normalize=1
filters=16
size=1
stride=1
pad=1
activation=leaky
quantized=1
quant_stop=0

[upsample]
stride=2
quantized=1
quant_stop=0

[route]
layers = -1, 0
quantized=1
quant_stop=0

[convolutional]
batch_normalize=1
filters=32
size=3
stride=1
pad=1
activation=relu6
quantized=1
quant_stop=0
"""


def write_l0_cfg(path, filters, act, size=12):
    """first layer 3 -> filters, 3x3, `act`, then a 1x1 head and a yolo layer: what the layer-0 derivation needs, nothing more"""
    open(path, "w").write(_L0.format(size=size, filters=filters, act=act) + _HEAD)
    return str(path)


def write_net_cfg(path, size=12, filters=16, act="leaky"):
    """cfg/tiny_unit.cfg's layers (conv + pool, conv + stride-1 pool, 1x1, upsample, route, conv, head, yolo) on a size x size input"""
    open(path, "w").write(_L0.format(size=size, filters=filters, act=act) + _BODY + _HEAD)
    return str(path)


def f32(x):
    return np.float32(x)


def pair_of(mx, mn):
    """(scale, zero point) of an image with that max / min: image_scale_zero_point (network.c) in numpy's IEEE float32 / float64"""
    mx, mn = f32(mx), f32(mn) + f32(0)
    s = f32(f32(mx - mn) * f32(f32(1.0) / f32(255.0)))
    izp = np.float64(f32(f32(0) - f32(mn / s)))
    z = 0 if izp < 0 else (255 if izp > 255 else int(np.floor(izp + 0.5)))  # round(): half away from zero, izp >= 0 here
    return s, z


def pairs_table():
    """the (scale, zero point) pairs the derivation is swept over, by name"""
    t = {}
    for m in (1, 254, 255):  # a frame's bytes / 255 with that maximum, minimum 0
        t[f"frame max {m}"] = pair_of(f32(m) / f32(255), 0)
    t["float -0.7 .. 1.4"] = pair_of(1.4, -0.7)
    t["float -0.2 .. 0"] = pair_of(0.0, -0.2)
    t["float -3 .. 0.01"] = pair_of(0.01, -3.0)
    p2 = f32(2.0 ** -8)
    t["just below 2^-8"] = (np.nextafter(p2, f32(0)), 0)  # the multipliers' shift steps between these two
    t["2^-8"] = (p2, 0)
    for z in (0, 1, 128, 255):
        t[f"zero point {z}"] = (f32(0.011) + f32(z) * f32(1e-5), z)
    return t


M_TOO_LARGE = (f32(4096.0), 7)  # s_in * s_w / s_act >= 1 for every channel of the synthetic models


# scales so small that some multiplier falls below 2^-32 (shift > 31: the header's pow2 is 0); the crafted model only
TINY = {"tiny 2^-40": (f32(2.0 ** -40), 0), "tiny 3e-13, zero point 200": (f32(3e-13), 200)}
STATE_MODELS = [(16, "leaky"), (20, "relu6"), (4, "linear")]  # the first layers the crafted model is swept with


def make_model(tmp_path, filters, act, crafted=False):
    """(cfg, weights) of a first layer 3 -> filters with `act`: synth.synth_weights as it is, or crafted (craft_weights: zero folded
    bias, filter 0's weight zero point 0)"""
    cfg = write_l0_cfg(tmp_path / "l0.cfg", filters, act)
    wts = str(tmp_path / "l0.weights")
    synth.synth_weights(cfg, wts, seed=filters)
    if crafted:
        craft_weights(wts, filters, zero_bias=True, zp_w0=0)
    return cfg, wts


def consts_of(net):
    """(header dict, channels structured array) of Net.layer0_consts()"""
    raw = net.layer0_consts()
    n, K, zp_act, act, s_act = struct.unpack_from("<iiiif", raw, 0)
    ch = np.frombuffer(raw, dtype=[("bias", "<f4"), ("w_scale", "<f4"), ("w_zp", "<i4"), ("wsum", "<i4")], count=n, offset=32)
    return dict(n=n, K=K, zp_act=zp_act, activation=act, s_act=f32(s_act)), ch


def craft_weights(path, n, zero_bias=False, zp_w0=None):
    """Edit layer 0's record of a synth.synth_weights file in place (src/parser.c:1124-1159: biases, scales, mean, variance, the two
    activation records, weight scales, weight zero points, ...).  zero_bias: biases and rolling means 0, so the folded bias is 0 and the
    integer bias stays inside int32 at any input scale; zp_w0: the zero point of filter 0's weights (0: a filter whose real weights are
    all >= 0, which is what gives the first layer's zero-point correction its value 128)."""
    buf = bytearray(open(path, "rb").read())
    off = 20  # major, minor, revision, seen
    if zero_bias:
        buf[off:off + 4 * n] = bytes(4 * n)                    # biases
        buf[off + 8 * n:off + 12 * n] = bytes(4 * n)           # rolling_mean (after biases, scales)
    if zp_w0 is not None:
        buf[off + 16 * n + 10 + 4 * n] = zp_w0                 # after the four float arrays, the 10-byte records, the weight scales
    open(path, "wb").write(bytes(buf))


# ---------------------------------------------------------------------------------------------------------------------------------
# The kernels' arithmetic restated (input_dev.hip; common.h's small_safe_range, biased_safe_range, intrq_make, leaky_byte_biased;
# shim.hip's ept_fill).  float32 steps are numpy float32 scalars, double steps Python floats, integers Python ints wrapped by hand.
# ---------------------------------------------------------------------------------------------------------------------------------
def _i32(v):
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v & 0x80000000 else v


def _trunc_q(accb, mp):
    return int(float(accb) * mp)  # requant_q_exact: (int32)((double)accb * Mp), |product| < 2^31 as 0 < Mp < 1


def _v_of(act, accb, mp, zp):
    q = _trunc_q(accb, mp)
    if act == "leaky":
        return zp + q if q >= 0 else zp - ((-q + 5) & 0xFFFFFFFF) // 10
    if act == "relu6":
        return zp + max(q, 0)
    return zp + q


def small_safe_range(act, mp, zp):
    IMIN, IMAX = -(1 << 31), (1 << 31) - 1
    gh = float(256 - zp) / mp
    h = IMAX if gh >= 2147483000.0 else int(gh)
    it = 0
    while it < 64 and h > -IMAX and _v_of(act, h, mp, zp) > 255:
        h -= 1 if it < 8 else 4096
        it += 1
    if _v_of(act, h, mp, zp) > 255:
        h = IMIN
    if act == "relu6":
        lo = IMIN
    else:
        qlo = -(10.0 * zp + 5.0) if act == "leaky" else -float(zp + 1)
        gl = qlo / mp
        lo = IMIN if gl <= -2147483000.0 else int(gl)
        it = 0
        while it < 64 and lo < IMAX and _v_of(act, lo, mp, zp) < 0:
            lo += 1 if it < 8 else 4096
            it += 1
        if _v_of(act, lo, mp, zp) < 0:
            lo = IMAX
    return lo, h


def biased_safe_range(lo, hi):
    L, H = max(lo, -(1 << 30)), min(hi, (1 << 30) - 1)
    return H >= L, L, (H - L if H >= L else 0)


def intrq_make(mval, s, lo, hi, neg_any):
    if not (0.0 < mval < 1.0) or s < 1 or s > 31:
        return False, 0, 0
    t = mval * 2147483648.0
    m = int(t)
    if float(m) != t or m <= 0:
        return False, 0, 0
    if neg_any and lo < 0:
        lo = 0
    if hi < lo:
        hi = lo
    amax = max(-lo, hi)
    tz = (m & -m).bit_length() - 1
    if amax < 0 or amax >= (1 << 31) or amax * (m >> tz) >= (1 << 53):
        return False, 0, 0
    e = 31 + s - tz
    if e < 40 and lo < 0 and -lo >= (1 << e):
        return False, 0, 0
    return True, m, s - 1


def leaky_byte_biased(q, zp):
    v = zp - ((-q + 5) & 0xFFFFFFFF) // 10 if q < 0 else q + zp
    return (v & 0xFF) ^ 0x80


def l0_channel(hdr, ch, s_in, zp_in):
    """one channel of the host prep -> (status bit, shift, biases_int32, M_value, shift_value)"""
    s_in = f32(s_in)
    mult = (hdr["K"] * zp_in * int(ch["w_zp"])) & 0xFFFFFFFF
    wsi = _i32(mult - ((int(ch["wsum"]) * zp_in) & 0xFFFFFFFF))
    with np.errstate(all="ignore"):
        M = f32(f32(s_in * ch["w_scale"]) / hdr["s_act"])
        if not (M > 0) or not (M < 1):
            return M_RANGE, 0, 0, 0.0, 0.0
        s = 0
        while M < f32(0.5):
            M = f32(M * f32(2))
            s += 1
        q = int(np.floor(np.float64(f32(M * f32(2.0 ** 31))) + 0.5))
        if q == 1 << 31:
            q //= 2
            s -= 1
        if s < 0:
            return NEG_SHIFT, 0, 0, 0.0, 0.0
        sval, mval = 2.0 ** -s, 2.0 ** -31 * q
        if not (0.0 < mval < 1.0) or not (0.0 < sval <= 1.0):
            return PACK_RANGE, 0, 0, 0.0, 0.0
        t = f32(f32(ch["bias"] / f32(s_in * ch["w_scale"])) + f32(wsi))
    if not (t >= f32(-2147483648.0) and t < f32(2147483648.0)):
        return BIAS_RANGE, 0, 0, 0.0, 0.0
    return 0, s, int(t), mval, sval


_HDR = struct.Struct("<I11i6QQQii5Q")  # common.h ConvBlobHeader
_HDR_KEYS = ["magic", "n", "c", "ksize", "mpad", "cb", "nchunks", "upc", "spc", "ksteps", "ktrue", "first", "off_wp", "off_cw", "off_dzp",
             "off_bias", "off_mval", "off_sval", "total", "off_shift", "pow2", "generic", "off_mprime", "off_cwb", "off_ws", "off_ept", "off_gen"]


def blob_header(blob):
    return dict(zip(_HDR_KEYS, _HDR.unpack_from(blob, 0)))


def derive_entry(slot, hdr, chans, act, s_in, zp_in):
    """mi355_l0_derive for one entry: `slot` (a packed layer-0 blob for any pair) -> (status, the slot's new bytes, EPT flags, pow2).  With a
    non-zero status the bytes are the slot's own."""
    kact = {"relu": "linear"}.get(act, act)  # the LINEAR table serves RELU
    h = blob_header(slot)
    n = hdr["n"]
    assert h["magic"] == 0x4D493335 and h["n"] == n and h["first"] == 1 and h["off_ept"]
    per = [l0_channel(hdr, chans[oc], s_in, zp_in) for oc in range(n)]
    status = 0
    for p in per:
        status |= p[0]
    if status:
        return status, slot.copy(), None, None
    pow2 = all(p[1] <= 31 for p in per)
    out = slot.copy()
    view = lambda key, dt, cnt=None: np.frombuffer(out.data, dtype=dt, count=cnt if cnt is not None else h["mpad"], offset=h[key])
    cw, dzp = view("off_cw", "<i4").copy(), view("off_dzp", "<i4").copy()
    bias, mval, sval = view("off_bias", "<i4"), view("off_mval", "<f8"), view("off_sval", "<f8")
    shift, mprime, cwb = view("off_shift", "<i4"), view("off_mprime", "<f8"), view("off_cwb", "<i4")
    ent_dt = np.dtype([("lb", "<i4"), ("rg", "<u4"), ("m0", "<i4"), ("sh", "<i4"), ("qc", "<i8"), ("cbl", "<i4"), ("pad", "<i4")])
    ent = np.frombuffer(out.data, dtype=ent_dt, count=h["mpad"], offset=h["off_ept"] + 16)
    flags = EPT_POW2 if pow2 else EPT_NOINT
    for oc, (_, s, b32, mv, sv) in enumerate(per):
        bias[oc], mval[oc], sval[oc] = b32, mv, sv
        shift[oc] = s if pow2 else 0
        cwb[oc] = _i32(int(cw[oc]) + b32)
        mp = mv * sv
        mprime[oc] = mp
        lo, hi = small_safe_range(kact, mp, hdr["zp_act"])
        ok, lb, rg = biased_safe_range(lo, hi)
        if not ok:
            flags |= EPT_NEVER
        okq, m0, sh = intrq_make(mv, s, lb, _i32(lb + rg), kact == "relu6") if pow2 else (False, 0, 0)
        if not okq:
            flags |= EPT_NOINT
            m0 = sh = 0
        ent[oc] = (lb, rg, m0, sh, lb * m0, _i32(int(cwb[oc]) - lb), 0)
        if dzp[oc] > 127:
            flags |= EPT_D2
    lut = np.frombuffer(out.data, dtype=np.uint8, count=4096, offset=h["off_ept"] + 16 + 32 * h["mpad"])
    by_floor = not (flags & EPT_NOINT)
    for i in range(4096):
        f = i - 3072
        lut[i] = leaky_byte_biased(f + 1 if by_floor and f < 0 else f, hdr["zp_act"]) if kact == "leaky" else 0
    lane_dt = np.dtype([("w", "<i4", (24,)), ("cb", "<i4", (4,)), ("lo", "<i4", (4,)), ("hi", "<i4", (4,)), ("qm0", "<i4", (4,)),
                        ("qsh", "<i4", (4,)), ("qc", "<i8", (4,)), ("mp", "<f8", (4,)), ("pad", "<i4", (4,))])
    assert lane_dt.itemsize == 256
    ntile = (n + 15) // 16
    lanes = np.frombuffer(out.data, dtype=lane_dt, count=64 * ntile, offset=h["off_ept"] + 16 + 32 * h["mpad"] + 4096)
    for idx in range(64 * ntile):
        mt, g = idx >> 6, (idx & 63) >> 4
        for r in range(4):
            c2 = 16 * mt + 4 * g + r
            if c2 >= n:
                continue
            e = ent[c2]
            lanes[idx]["cb"][r], lanes[idx]["lo"][r], lanes[idx]["hi"][r] = e["cbl"], e["lb"], _i32(int(e["rg"]))
            lanes[idx]["qm0"][r], lanes[idx]["qsh"][r], lanes[idx]["qc"][r], lanes[idx]["mp"][r] = e["m0"], e["sh"], e["qc"], mprime[c2]
    struct.pack_into("<i", out, 112, 1 if pow2 else 0)
    act_id = ACT_ID[kact]
    struct.pack_into("<IIII", out, h["off_ept"], 0x45500000 | ((act_id & 0xFF) << 8) | (hdr["zp_act"] & 0xFF), flags, 0, 0)
    return 0, out, flags, pow2
