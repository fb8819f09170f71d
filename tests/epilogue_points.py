"""Builder of conv layers whose accumulators sit ON the switch points of the requantise epilogue (csrc/common.h).

TEST INFRASTRUCTURE (numpy only): imported by tests/test_epilogue_points_cpu.py, tests/test_gpu_epilogue_points.py and
tests/test_host_cpu.py (the reader of a packed blob's epilogue table).

The construction.  The reference's pre-requant accumulator is sum((w - zp_w) * x_byte) (the input zero point is only the pad value), and the
requantised value is taken from acc + bias.  Every weight of channel o equals zp_w[o] except the centre tap of input channel k(o) = o % c,
which holds zp_w[o] + sigma[o].  Then acc_o(p) = sigma[o] * x[k(o)][p] exactly, and the bias alone places the channel:
acc + bias = T[o] + sigma[o] * (x - x0).  An image set has a direction `dirn`: calm pixels are x0 - dirn * {0..3}, an aimed pixel is
x0 + dirn, so channel o moves OUTWARD from its target by sigma[o] * dirn -- two launches (dirn = +1, -1) probe both sides of every target
whatever sign a weight zero point of 0 or 255 forces on sigma.

What a launch carries: the layer (wq, zp_w, bias, M, S), the images x, and everything needed to state the expected accumulators without
running a convolution (`acc_of`)."""
import numpy as np

LEAKY, RELU6, LINEAR = "leaky", "relu6", "linear"
LIM = 1 << 30          # the pooled kernels clamp their wrap-safe range to [-LIM, LIM - 1] (common.h biased_safe_range)
X0 = 131               # the input byte at which a channel sits on its target
ZP_IN = 9              # pad value of the input tensor: multiplied by zero everywhere (border taps hold w == zp_w)
ZP_ACTS = {LEAKY: (0, 1, 23, 128, 254, 255), RELU6: (0, 1, 23, 128, 254, 255), LINEAR: (128, 255)}


# ------------------------------------------------------------------------------------ the numpy restatement
def q_of(a, M, S):
    """ref src/convolutional_layer.c:732-733: t = trunc(float64(a) * M); q = trunc(t * S)."""
    t = np.trunc(np.asarray(a, np.int64).astype(np.float64) * M)
    return np.trunc(t * S).astype(np.int64)


def v_of(a, M, S, zp, act):
    """activation + zero point, unwrapped"""
    q = q_of(a, M, S)
    if act == LEAKY:
        return np.where(q >= 0, zp + q, zp - (np.abs(q) + 5) // 10)
    if act == RELU6:
        return zp + np.maximum(q, 0)
    return zp + q


def byte_of(a, M, S, zp, act, saturate):
    v = v_of(a, M, S, zp, act)
    if saturate:
        v = np.clip(v, 0, 255)
    return (v & 255).astype(np.uint8)


def edge(pred, lo, hi):
    """Bisection on a predicate that is true up to some point of [lo, hi] and false beyond: the largest a with pred(a), elementwise
    (lo, hi and pred's argument are int64 arrays of one shape).  pred(lo) must hold."""
    lo = np.array(lo, np.int64)
    hi = np.broadcast_to(np.array(hi, np.int64), lo.shape).copy()
    assert pred(lo).all(), "edge: the predicate must hold at the lower end"
    while (lo < hi).any():
        m = lo + (hi - lo + 1) // 2
        ok = pred(m)
        lo, hi = np.where(ok, m, lo), np.where(ok, hi, m - 1)
    return lo


def q_first(M, S, R, lim=LIM + 8):
    """Per channel the smallest accumulator T with q_of(T) >= R, so q_of(T - 1) < R <= q_of(T) -- with M * S < 1 that is the pair
    R - 1 | R.  exists[o] is false where the boundary lies beyond +-lim."""
    n = len(M)
    R = np.broadcast_to(np.asarray(R, np.int64), (n,))
    lo, hi = np.full(n, -lim, np.int64), np.full(n, lim, np.int64)
    exists = (q_of(lo, M, S) < R) & (q_of(hi, M, S) >= R)
    T = edge(lambda a: (q_of(a, M, S) < R) | ~exists, lo, hi) + 1
    return np.where(exists, T, 0), exists


def true_range(M, S, zp, act):
    """[lo, hi]: the accumulators whose stored byte does not wrap, by bisection on the restatement (lo = -2^31 for RELU6)."""
    n = len(M)
    z = np.zeros(n, np.int64)
    hi = edge(lambda a: v_of(a, M, S, zp, act) <= 255, z, np.full(n, (1 << 31) - 1, np.int64))
    lo = -edge(lambda a: v_of(-a, M, S, zp, act) >= 0, z, np.full(n, 1 << 31, np.int64))
    return lo, hi


def intrq_accepts(m0, s, lo, hi, neg_any):
    """common.h intrq_make's conditions, restated on python ints (one channel)."""
    m0, s, lo, hi = int(m0), int(s), int(lo), int(hi)
    if s < 1 or s > 31:
        return False
    if neg_any and lo < 0:
        lo = 0
    hi = max(hi, lo)
    amax = max(-lo, hi)
    tz = (m0 & -m0).bit_length() - 1
    if amax >= 1 << 31 or amax * (m0 >> tz) >= 1 << 53:
        return False
    e = 31 + s - tz
    return not (e < 40 and lo < 0 and -lo >= 1 << e)


# ------------------------------------------------------------------------------------------- layer and images
def layer(n, c, k, sigma, targets, x0, zp_w=None):
    """wq [n, c*k*k], zp_w [n], bias [n] with acc_o + bias_o = targets[o] + sigma[o] * (x[o % c] - x0) at the window's centre.
    zp_w is varied as the suite does (0, 255, 1 on the first three channels); sigma[o] must be reachable from zp_w[o]."""
    rng = np.random.default_rng(n * 131 + c)
    if zp_w is None:
        zp_w = rng.integers(90, 166, n).astype(np.int64)
        zp_w[:3] = [0, 255, 1][:min(n, 3)]
    zp_w = np.asarray(zp_w, np.int64)
    sigma = np.asarray(sigma, np.int64)
    w = zp_w + sigma
    assert ((w >= 0) & (w <= 255)).all(), "sigma not reachable from zp_w"
    wq = np.repeat(zp_w[:, None], c * k * k, 1)
    o = np.arange(n)
    wq[o, (o % c) * k * k + (k * k) // 2] = w
    bias = np.asarray(targets, np.int64) - sigma * x0
    assert (np.abs(bias) < (1 << 31) - 1).all()
    return wq.astype(np.uint8), zp_w.astype(np.uint8), bias.astype(np.int32)


def default_sigma(n):
    """+1 everywhere except where the weight zero point 255 forces -1 (channel 1; zp_w 0 on channel 0 forces +1)."""
    s = np.ones(n, np.int64)
    if n > 1:
        s[1] = -1
    return s


def images(B, c, H, W, x0, calm, aimed, seed=0):
    """x [B, c, H, W] u8: every pixel x0 + a calm offset; image b then takes its aimed pixels aimed[b] = (kb, [(y, x, d), ...]) in input
    channel kb only -- its other input channels stay calm."""
    rng = np.random.default_rng(seed + 7 * B + c + H * W)
    x = x0 + rng.choice(np.asarray(calm, np.int64), (B, c, H, W))
    for b, (kb, pts) in enumerate(aimed):
        for (y, xx, d) in pts:
            x[b, kb, y, xx] = x0 + d
    assert ((x >= 0) & (x <= 255)).all()
    return x.astype(np.uint8)


def positions(H, W, stride=1):
    """(0, 0), the last pixel and one interior pixel (on the output grid of a strided conv)"""
    p = [(0, 0), (H - 1, W - 1), (H // 2, W // 2 - 1)]
    return [((y // stride) * stride, (x // stride) * stride) for y, x in p]


class Launch:
    """One conv call.  T: per-channel target of acc + bias; out: outward direction sigma * dirn (0: channel not aimed); live: channels whose
    probe exists; kind: 'q' (a boundary of q: q differs across T | T + out), 'range' (an end of the wrap-safe range: where true_edge[o] the byte at
    T + out wraps, elsewhere T is a clamp or a table's narrower end and nothing wraps across it), 'plain' (no straddle claim)."""

    def __init__(self, name, fam, act, zp, M, S, T, sigma, dirn, x, aimed, kind, live=None, zp_w=None, x0=X0, state=None):
        n, c, k = fam["n"], fam["c"], fam["k"]
        self.name, self.fam, self.act, self.zp, self.M, self.S = name, fam, act, int(zp), np.asarray(M, np.float64), np.asarray(S, np.float64)
        self.T, self.sigma, self.dirn, self.x, self.aimed, self.kind, self.x0 = np.asarray(T, np.int64), np.asarray(sigma, np.int64), dirn, x, aimed, kind, x0
        self.out = self.sigma * dirn
        self.live = np.ones(n, bool) if live is None else np.asarray(live, bool)
        self.state = state
        self.wq, self.zp_w, self.bias = layer(n, c, k, self.sigma, self.T, x0, zp_w)

    def value_of(self):
        """acc + bias per output pixel: [B, n, OH, OW] int64"""
        f = self.fam
        st = f.get("stride", 1)
        xs = self.x[:, np.arange(f["n"]) % f["c"]].astype(np.int64)[:, :, ::st, ::st]
        return self.T[None, :, None, None] + self.sigma[None, :, None, None] * (xs - self.x0)

    def acc_of(self):
        """the pre-requant accumulators the construction intends: [B, n, OH*OW] int32"""
        v = self.value_of() - self.bias.astype(np.int64)[None, :, None, None]
        return v.reshape(v.shape[0], v.shape[1], -1).astype(np.int32)

    def aimed_mask(self):
        """[B, n, OH, OW] bool: output values that sit one step outside their target"""
        v = self.value_of()
        return (v == (self.T + self.out)[None, :, None, None]) & (self.out != 0)[None, :, None, None] & self.live[None, :, None, None]

    def probes(self):
        """number of (channel, pixel) values within one step of a live target: inside, on the point, outside"""
        v = self.value_of() - self.T[None, :, None, None]
        return int(((np.abs(v) <= 1) & self.live[None, :, None, None]).sum())


# ------------------------------------------------------------------------------------------------ families
# kernel: what mi355_last_conv_kernel() must report.  pooled: through mi355_conv_pool_forward.
FAMILIES = {
    "first16": dict(id=1, c=3, n=16, k=3, H=8, W=8), "first16_pool": dict(id=1, c=3, n=16, k=3, H=8, W=8, pooled=True),
    "first32_pool": dict(id=1, c=3, n=32, k=3, H=8, W=8, pooled=True),
    "small16_pool": dict(id=2, c=16, n=32, k=3, H=8, W=8, pooled=True), "small32_pool": dict(id=2, c=32, n=64, k=3, H=8, W=8, pooled=True),
    "small64_pool": dict(id=2, c=64, n=128, k=3, H=8, W=8, pooled=True, plans=(0, 1)),
    "small16_wide_pool": dict(id=2, c=16, n=32, k=3, H=4, W=128, pooled=True),
    "small64": dict(id=2, c=64, n=64, k=3, H=8, W=8),
    "pool16": dict(id=7, c=16, n=32, k=3, H=8, W=8, pooled=True, hint=1), "small32x": dict(id=8, c=32, n=64, k=3, H=8, W=8, pooled=True, flags=4096),
    "conv1x1": dict(id=3, c=64, n=32, k=1, H=13, W=13),
    # (conv_ws3.hip leaves batches of fewer than 64 pixels per workgroup to the row-image kernel: 96 images of 13 x 13 reach it)
    "ws3": dict(id=4, c=128, n=64, k=3, H=13, W=13, B=96),
    "rows": dict(id=5, c=256, n=64, k=3, H=13, W=13, flags=16384), "rows32": dict(id=5, c=256, n=64, k=3, H=13, W=13, flags=16384 | (1 << 20)),
    "igemm": dict(id=5, c=48, n=40, k=3, H=9, W=11),
    "kxk3": dict(id=9, c=5, n=7, k=3, H=8, W=8), "kxk5s2": dict(id=9, c=5, n=7, k=5, H=8, W=8, stride=2),
}
PER_PIXEL = [f for f, d in FAMILIES.items() if not d.get("pooled")]
POOLED = [f for f, d in FAMILIES.items() if d.get("pooled")]

# Probes that cannot exist: (family, act, zp_act, launch, channel or None, reason).  Filled by the builders, never silently.
DROPPED = []
# ... and the ones that cannot exist for ANY family, with the reason
UNREACHABLE = [
    ("pooled state `never` through a channel without a safe range",
     "small_safe_range starts within one step of the true end (its guess is the exact quotient, good to 1 ulp of a number below 2^31) and may move "
     "229 384 steps inwards; biased_safe_range only fails when the clamped range is empty, and every range contains 0.  With 0 < M < 1 and "
     "0 < S <= 1, which mi355_conv_pack enforces, EPT_NEVER is therefore never set: the CPU test asserts the flag clear on every packed launch.  "
     "The launch-wide `never` is reached through shifts that are not powers of two instead (state 'notpow2')."),
]


def _drop(fam, act, zp, launch, ch, reason):
    DROPPED.append((fam, act, zp, launch, ch, reason))


def _rand_m(rng, n, s_lo, s_hi):
    m0 = (rng.integers(1 << 30, 1 << 31, n) >> 7) << 7   # as the reference builds it from a float: >= 7 trailing zeros
    s = rng.integers(s_lo, s_hi + 1, n)
    return m0.astype(np.float64) * 2.0 ** -31, 2.0 ** -s.astype(np.float64), m0, s


def q_bounds(act, zp):
    """R of every boundary R - 1 | R of the per-pixel catalogue that needs no fallback"""
    if act == LEAKY:   # -6 | -5 | -4 (ties of round(q / 10)), -1 | 0 | 1, the byte's wrap at both ends, SAT's clamp of q, p << 19 leaving int32
        return [-5, -4, 0, 1, 256 - zp, -(10 * zp + 4), 2048, 4096]
    if act == LINEAR:
        return [0, 1, 256 - zp, -zp, 2048, 4096]
    return [0, 1, 256 - zp, 2048, 4096]


def _pp_images(fam, dirn, seed):
    c, H, W = fam["c"], fam["H"], fam["W"]
    pos = positions(H, W, fam.get("stride", 1))
    ka = min(c, fam["n"])
    B = fam.get("B", 3)
    aimed = [((b * 5 + 1) % ka, [(pos[b % 3][0], pos[b % 3][1], dirn)]) for b in range(B)]
    return images(B, c, H, W, X0, [-dirn * i for i in range(4)], aimed, seed), aimed


def per_pixel_launches(fname, act, zp):
    """Every per-pixel catalogue entry for one family, activation and zero point."""
    fam = FAMILIES[fname]
    n = fam["n"]
    rng = np.random.default_rng(n + zp + len(act))
    sig = default_sigma(n)
    out = []

    def add(name, M, S, first, exists, kind="q", both=True):
        # outward +: calm on the q < R side (T = first - 1); outward -: calm on the q >= R side (T = first)
        for dirn in ((1, -1) if both else (1,)):
            o = sig * dirn
            T = np.where(o > 0, first - 1, first) if kind == "q" else first
            for ch in np.flatnonzero(~exists):
                _drop(fname, act, zp, name, int(ch), "target beyond +-2^30")
            x, aimed = _pp_images(fam, dirn, len(out))
            out.append(Launch("%s/dir%+d" % (name, dirn), fam, act, zp, M, S, np.where(exists, T, 0), sig, dirn, x, aimed, kind, exists))

    # q boundaries, one per channel, rotated until every boundary was on some channel
    Rs = q_bounds(act, zp)
    M, S, _, _ = _rand_m(rng, n, 3, 9)
    for rot in range(-(-len(Rs) // n)):
        R = np.array([Rs[(o + rot * n) % len(Rs)] for o in range(n)], np.int64)
        add("q-bounds%d" % rot, M, S, *q_first(M, S, R))
    if act == LEAKY:
        # the branch-free form's limit q >= -40000 (wave-wide fallback below) and the 24-bit multiply's |q| + 5 < 65536
        Md, Sd, _, _ = _rand_m(rng, n, 1, 5)
        R = np.where(np.arange(n) % 2 == 0, -40000, -65530)
        add("deep", Md, Sd, *q_first(Md, Sd, R))
        out.extend(_fallback_launches(fname, fam, act, zp))
    # exact products: M0 = 2^30, s = 8 -> q = a / 512 exactly at a = -512 k, and (|q| + 5) % 10 == 0 for k = 5, 15
    Me, Se = np.full(n, 0.5), np.full(n, 2.0 ** -8)
    Te = np.where(np.arange(n) % 2 == 0, -512 * 5, -512 * 15).astype(np.int64)
    add("exact-products", Me, Se, Te, np.ones(n, bool), kind="plain")
    # |acc + bias| at 2^30 with M close to 1
    Mb, Sb = np.full(n, ((1 << 31) - 128) * 2.0 ** -31), np.full(n, 0.5)
    for dirn in (1, -1):
        o = sig * dirn
        x, aimed = _pp_images(fam, dirn, 50)
        out.append(Launch("two-to-30/dir%+d" % dirn, fam, act, zp, Mb, Sb, np.where(o > 0, LIM - 1, -LIM), sig, dirn, x, aimed, "plain"))
    # shifts times 0.75: accumulators where the two truncations differ from one
    Mn, Sn, Tn = _notpow2_points(n)
    add("notpow2", Mn, Sn, Tn, np.ones(n, bool), kind="plain")
    return out


_NOTPOW2 = {}


def _notpow2_points(n):
    """(M, S, T) with shifts 0.75 * 2^-s and per channel an accumulator T where trunc(trunc(a M) S) != trunc(a M S), found by search
    (alternating signs; a different hit per channel).  The same for every activation and zero point, so built once per channel count."""
    if n not in _NOTPOW2:
        Mn, Sn, _, _ = _rand_m(np.random.default_rng(n), n, 3, 7)
        Sn = Sn * 0.75
        a = np.arange(1, 400000, dtype=np.int64)
        Tn = np.zeros(n, np.int64)
        for ch in range(n):
            two = q_of(a, Mn[ch], Sn[ch])
            one = np.trunc(a.astype(np.float64) * Mn[ch] * Sn[ch]).astype(np.int64)
            hit = np.flatnonzero(two != one)
            assert hit.size, "no accumulator separates the two-step form from the folded one"
            Tn[ch] = a[hit[min(ch, hit.size - 1)]] * (1 if ch % 2 == 0 else -1)
        _NOTPOW2[n] = (Mn, Sn, Tn)
    return _NOTPOW2[n]


def _fallback_launches(fname, fam, act, zp):
    """One launch where a single pixel of a single channel has q = -40001 and nothing else is below -100, and one where that pixel has
    q = -40000, the launch's minimum: no lane falls back.  The aimed channel's only non-zero tap is -200 (w = 0 at zp_w = 200) and the aimed
    pixel lies 200 input steps away from the calm ones: 40 000 accumulator steps at M * S ~ 1."""
    n, c, H, W = fam["n"], fam["c"], fam["H"], fam["W"]
    M, S = np.full(n, ((1 << 31) - 128) * 2.0 ** -31), np.ones(n)
    o_star = n - 1
    kb = o_star % c
    sig = default_sigma(n)
    sig[np.arange(n) % c == kb] = 0          # channels that share the aimed input channel: constant (the aimed byte would move them by 200)
    sig[o_star] = -200
    zp_w = np.random.default_rng(n).integers(90, 166, n)
    zp_w[:3] = [0, 255, 1][:min(n, 3)]
    zp_w[o_star] = 200
    live = np.zeros(n, bool)
    live[o_star] = True
    if o_star < 3:
        _drop(fname, act, zp, "fallback", o_star, "sign forced by zp_w")
        return []
    first, ex = q_first(M, S, np.full(n, -40000))
    assert ex.all()
    res = []
    x0, D = 20, 200
    pos = positions(H, W, fam.get("stride", 1))[2]
    for name, t_aim in (("one-fallback-pixel", first[o_star] - 1), ("no-fallback", first[o_star])):
        T = np.zeros(n, np.int64)
        T[o_star] = t_aim + 200 * D          # calm value of the aimed channel: q about -1
        aimed = [(kb, [(pos[0], pos[1], D)])]
        x = images(fam.get("B", 1), c, H, W, x0, [0, 1, 2, 3], aimed, 3)   # (only image 0 is aimed)
        x[:, kb] = x0
        x[0, kb, pos[0], pos[1]] = x0 + D
        L = Launch(name, fam, act, zp, M, S, T, sig, 1, x, aimed, "plain", live, zp_w=zp_w, x0=x0)
        q = q_of(L.value_of(), M[None, :, None, None], S[None, :, None, None])
        want = -40001 if name == "one-fallback-pixel" else -40000
        assert q.min() == want and (q < -100).sum() == 1, "the fallback launch is not what it claims"
        res.append(L)
    return res


# ------------------------------------------------------------------------------------------------- pooled
STATES = ("int", "one-noint", "random", "clamp", "notpow2")


def pooled_multipliers(n, act, zp, state):
    """(M, S, m0, s, odd) of one launch-wide state; odd = the channel that differs in 'one-noint' (else None)."""
    rng = np.random.default_rng(n * 7 + zp + len(act) + len(state))
    odd = None
    if state in ("int", "one-noint"):
        # M0 = 2^30 + 2^tz, s = 8: the largest tz whose integer form intrq_make accepts over the channel's range -- the clause "no negative
        # exact multiple of 2^(31 + s - tz) inside the range" is then the deciding one, and tz + 1 fails it
        s = np.full(n, 8)
        tz = 29
        while tz > 0:
            m0 = (1 << 30) + (1 << tz)
            lo, hi = true_range(np.array([m0 * 2.0 ** -31]), np.array([2.0 ** -8]), zp, act)
            if intrq_accepts(m0, 8, max(int(lo[0]), -LIM), min(int(hi[0]), LIM - 1), act == RELU6):
                break
            tz -= 1
        m0 = np.full(n, (1 << 30) + (1 << tz), np.int64)
        if state == "one-noint":
            odd = n // 2 + 1
            if act == RELU6:   # below zero only the sign matters there: fail the 53-bit product at the upper end instead
                m0[odd], s[odd] = (1 << 30) + 1, 24
            else:
                m0[odd] = (1 << 30) + (1 << (tz + 1))
    elif state == "clamp":     # ranges wider than +-2^30: both ends clamped
        _, _, m0, s = _rand_m(rng, n, 31, 31)
        if act == RELU6 and zp <= 128:   # (some channels keep the integer form there; a zero point near 255 needs the larger shift to reach 2^30)
            s[:] = 24
    else:
        _, _, m0, s = _rand_m(rng, n, 5, 9)
    M, S = m0.astype(np.float64) * 2.0 ** -31, 2.0 ** -s.astype(np.float64)
    if state == "notpow2":
        S = S * 0.75
    return M, S, m0, s, odd


def pooled_launches(fname, act, zp, state, table=None):
    """The pooled catalogue of one state.  table = (lb, hi) per channel: aim at the kernel's own range instead of the true one.
    Per direction: one launch 'on' (nothing outside: windows with all four values on the target) and the launches 'out' (image b has one value
    one step outside in input channel b: three on the target + one outside / the last pixel / a lone pixel among calm ones)."""
    fam = FAMILIES[fname]
    n, c, H, W = fam["n"], fam["c"], fam["H"], fam["W"]
    M, S, m0, s, odd = pooled_multipliers(n, act, zp, state)
    lo_t, hi_t = true_range(M, S, zp, act)
    lo, hi = (lo_t, hi_t) if table is None else (np.asarray(table[0], np.int64), np.asarray(table[1], np.int64))
    lo_c, hi_c = np.maximum(lo, -LIM), np.minimum(hi, LIM - 1)
    sig = default_sigma(n)
    pos = positions(H, W)
    ka = min(c, n)
    res = []
    for dirn in (1, -1):
        o = sig * dirn
        T = np.where(o > 0, hi_c, lo_c)
        true_edge = T == np.where(o > 0, hi_t, lo_t)   # per channel: T is the true end (else a clamp or the table's narrower end)
        tag = "%s%s/dir%+d" % (state, "" if table is None else "-table", dirn)
        calm = [-dirn * i for i in range(4)]
        # on: image b has a whole window of input channel b on the target
        aimed = []
        for b in range(3):
            wy, wx = pos[b][0] & ~1, pos[b][1] & ~1
            aimed.append(((b * 5) % ka, [(wy + j // 2, wx + j % 2, 0) for j in range(4)]))
        res.append(Launch(tag + "/on", fam, act, zp, M, S, T, sig, dirn, images(3, c, H, W, X0, calm, aimed, 1), aimed, "plain", state=state))
        # out: every input channel that some output channel reads is aimed once
        for base in range(0, ka, 16):
            aimed = []
            for kb in range(base, min(base + 16, ka)):
                y, xx = pos[kb % 3]
                pts = [(y, xx, dirn)]
                if kb % 3 != 2:   # the rest of the window on the target: three on the point, one outside
                    wy, wx = y & ~1, xx & ~1
                    pts += [(wy + j // 2, wx + j % 2, 0) for j in range(4) if (wy + j // 2, wx + j % 2) != (y, xx)]
                aimed.append((kb, pts))
            x = images(len(aimed), c, H, W, X0, calm, aimed, 2 + base)
            res.append(Launch("%s/out%d" % (tag, base // 16), fam, act, zp, M, S, T, sig, dirn, x, aimed, "range", state=state))
            res[-1].true_edge = true_edge
    for L in res:
        L.m0, L.s, L.odd, L.lo_c, L.hi_c = m0, s, odd, lo_c, hi_c
    return res


def pooled_set(fname, act, zp, state, pack):
    """The launches of one state: aimed at the true range and, where the packed table's own range [lb, lb + rg] is narrower on some channel,
    at that as well.  pack(launch) -> the blob of mi355_conv_pack + mi355_conv_pack_epilogue for the launch's activation and zero point.
    Returns (launches, table of the first)."""
    Ls = pooled_launches(fname, act, zp, state)
    t = read_ept(pack(Ls[0]))
    n = Ls[0].fam["n"]
    lb, hi = t["lb"][:n], t["lb"][:n] + t["rg"][:n]
    if not (np.array_equal(lb, Ls[0].lo_c) and np.array_equal(hi, Ls[0].hi_c)):
        Ls += pooled_launches(fname, act, zp, state, table=(lb, hi))
    return Ls, t


# --------------------------------------------------------------------------------- a packed blob's epilogue table
def read_ept(blob):
    """The epilogue table of a mi355_conv_pack / mi355_conv_pack_epilogue blob (common.h EptHeader, EptEntry): dict(off, total, mpad, key,
    flags, lb, rg, m0, sh, qc, cbl per channel row, lut_off)."""
    off = int(np.frombuffer(blob, np.uint64, 1, 144)[0])
    total = int(np.frombuffer(blob, np.uint64, 1, 96)[0])
    mpad = int(np.frombuffer(blob, np.int32, 1, 16)[0])
    key, flags = [int(v) for v in np.frombuffer(blob, np.uint32, 2, off)]
    ent = np.frombuffer(blob, np.int32, mpad * 8, off + 16).reshape(mpad, 8)
    return dict(off=off, total=total, mpad=mpad, key=key, flags=flags, ent=ent,
                lb=ent[:, 0].astype(np.int64), rg=ent[:, 1].view(np.uint32).astype(np.int64), m0=ent[:, 2].astype(np.int64),
                sh=ent[:, 3].astype(np.int64), qc=np.ascontiguousarray(ent[:, 4:6]).view(np.int64).ravel(), cbl=ent[:, 6].astype(np.int64),
                lut_off=off + 16 + 32 * mpad)
