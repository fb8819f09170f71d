"""Network generator for the whole-network differential tests (tests/test_netgen_cpu.py, tests/test_gpu_random_nets.py).

TEST INFRASTRUCTURE, CPU-only code: `random_net(seed)` writes a seeded random topology inside the documented supported domain
(README "Supported [convolutional] shapes", INTEGRATION.md "Which convolutions the drop-in accepts"), `AIMED` holds short hand-written
topologies, one per clause of the host planner (plan_fusion / plan_views / view_producer_ok in host/network.c and the run-time
fall-back of host/layers.c).  Both produce cfg TEXT; `features(cfg_text)` counts what a cfg exercises from the text alone.

Work bound.  The oracle (oracle/oracle.c, one thread, exact integers) was measured at 2.5-3 GMAC/s (0.09 s for the 0.25 GMAC of
`pool_keep_view` on one core of a 2024 x86-64 server CPU), so 2 s per image would allow 5 GMAC; the sweep runs every net on six to nine
images, so random nets are cut off far below that, at MAC_CAP per image (about 0.06 s).  The two aimed nets that need a whole round of the
chip for a weights-stationary fusion (AIMED_BIG) are the only ones above it."""
import random

MAC_CAP = 150_000_000     # per image, random nets
MAX_CELLS = 48 * 48       # largest map a random net grows to
ACTS = ("leaky", "relu6", "relu", "linear")
# every admission boundary of conv_forward_impl: c % 64, c % 16, c == 128 / 256, and counts outside all of them
FILTERS = (16, 32, 64, 128, 256, 17, 24, 33, 40, 48, 96)
SIZES = (1, 1, 1, 1, 3, 3, 3, 3, 3, 5, 5, 5, 2, 4, 6, 7, 8, 9, 10, 11)
POOLS = ((2, 2), (2, 2), (2, 1), (3, 2), (5, 1), (9, 1), (13, 1))


def cdiv(a, b):
    """C's truncating division (glue_edges.cdiv's equal): the reference sizes a pool's output with it, and Python's // floors"""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


# ----------------------------------------------------------------------------------------------- cfg text
class Net:
    """cfg writer that tracks every layer's (type, channels, height, width)"""

    def __init__(self, h, w, c=3):
        self.top = f"[net]\nbatch=1\nsubdivisions=1\nwidth={w}\nheight={h}\nchannels={c}\n"
        self.secs = []
        self.shape = []   # (type, c, h, w)
        self.cur = (c, h, w)
        self.macs = 0

    def _push(self, text, ty, c, h, w):
        self.secs.append(text)
        self.shape.append((ty, c, h, w))
        self.cur = (c, h, w)
        return len(self.secs) - 1

    def conv(self, n, size, stride=1, pad=None, padding=None, act="leaky", bn=1, qs=0):
        c, h, w = self.cur
        if pad is None and padding is None:
            pad = 0 if size == 1 else 1
        p = size // 2 if pad else (padding or 0)
        oh, ow = (h + 2 * p - size) // stride + 1, (w + 2 * p - size) // stride + 1
        assert oh >= 1 and ow >= 1 and h + 2 * p >= size and w + 2 * p >= size
        self.macs += oh * ow * n * c * size * size
        t = "[convolutional]\n" + ("batch_normalize=1\n" if bn else "") + f"filters={n}\nsize={size}\nstride={stride}\n"
        t += "pad=1\n" if pad else f"padding={padding or 0}\n"
        t += f"activation={act}\nquantized=1\nquant_stop={qs}\n"
        return self._push(t, "conv", n, oh, ow)

    def maxpool(self, size, stride, qs=0, padding=None):
        """padding: the cfg's `padding=` line (both sides together, as the reference counts it); None leaves the default, size - 1"""
        c, h, w = self.cur
        pad = size - 1 if padding is None else padding
        oh, ow = cdiv(h + pad - size, stride) + 1, cdiv(w + pad - size, stride) + 1  # C truncates (ref: src/maxpool_layer.c:31-32)
        assert oh >= 1 and ow >= 1
        t = f"[maxpool]\nsize={size}\nstride={stride}\n" + ("" if padding is None else f"padding={padding}\n")
        return self._push(t + f"quantized=1\nquant_stop={qs}\n", "maxpool", c, oh, ow)

    def upsample(self, stride, qs=0):
        c, h, w = self.cur
        return self._push(f"[upsample]\nstride={stride}\nquantized=1\nquant_stop={qs}\n", "upsample", c, h * stride, w * stride)

    def route(self, layers, qs=0, absolute=False):
        i = len(self.secs)
        srcs = [x if x >= 0 else i + x for x in layers]
        h, w = self.shape[srcs[0]][2:]
        assert all(self.shape[s][2:] == (h, w) and self.shape[s][0] != "yolo" for s in srcs)
        txt = ",".join(str(s if absolute else s - i) for s in srcs)
        return self._push(f"[route]\nlayers = {txt}\nquantized=1\nquant_stop={qs}\n", "route", sum(self.shape[s][1] for s in srcs), h, w)

    def shortcut(self, frm, qs=0):
        i = len(self.secs)
        src = frm if frm >= 0 else i + frm
        assert self.shape[src][1:] == self.cur and self.shape[src][0] != "yolo"
        return self._push(f"[shortcut]\nfrom={frm}\nactivation=linear\nquantized=1\nquant_stop={qs}\n", "shortcut", *self.cur)

    def head(self, size=1, nmask=3, classes=2, bn=0, **kw):
        """quant_stop head conv + its [yolo] layer"""
        self.conv(nmask * (classes + 5), size, act="linear", bn=bn, qs=1, **kw)
        c, h, w = self.cur
        mask = ",".join(str(k) for k in range(nmask))
        anchors = ", ".join(f"{10 + 7 * k},{14 + 9 * k}" for k in range(nmask))
        return self._push(f"[yolo]\nmask = {mask}\nanchors = {anchors}\nclasses={classes}\nnum={nmask}\n", "yolo", c, h, w)

    def text(self, comment=""):
        return (f"# {comment}\n" if comment else "") + self.top + "\n" + "\n".join(self.secs)


# ------------------------------------------------------------------------------------------ random topologies
def random_net(seed):
    """Seeded random topology -> cfg text.  Deterministic: the same seed gives the same text on every run and platform."""
    rng = random.Random(0x9E3779B1 * (seed + 1))
    h = rng.choice((20, 24, 26, 27, 31, 32, 33, 36, 40))
    w = rng.choice((20, 24, 26, 27, 31, 32, 33, 36, 40)) if rng.random() < 0.5 else h
    net = Net(h, w)
    act0 = rng.choice(ACTS[:3])  # a net leans on one activation and mixes others in around it
    nheads = rng.choice((1, 1, 2, 3))
    nbody = rng.randint(7, 14)
    unroutable = set()           # 3-filter convs (4-byte cells: only a convolution reads them), yolo layers

    def act():
        return act0 if rng.random() < 0.6 else rng.choice(ACTS)

    def conv(force_1x1=False, n=None):
        c, ch, cw = net.cur
        for _ in range(64):
            size = 1 if force_1x1 else rng.choice(SIZES)
            stride = 1 if size == 1 else rng.choice((1, 1, 1, 2, 2, 3))
            pad, padding = (0, 0) if size == 1 else ((1, None) if rng.random() < 0.6 else (0, rng.randint(0, size - 1)))
            p = size // 2 if pad else padding
            if ch + 2 * p < size or cw + 2 * p < size:
                continue
            oh, ow = (ch + 2 * p - size) // stride + 1, (cw + 2 * p - size) // stride + 1
            if oh < 2 or ow < 2:
                continue
            nn = n or rng.choice(FILTERS)
            if oh * ow * nn * c * size * size > MAC_CAP // 3 or net.macs + oh * ow * nn * c * size * size > MAC_CAP:
                if n is None:
                    nn = rng.choice((16, 17, 24, 32))
                if net.macs + oh * ow * nn * c * size * size > MAC_CAP:
                    continue
            return net.conv(nn, size, stride, pad=pad or None, padding=None if pad else padding, act=act(), bn=int(rng.random() < 0.8))
        return net.conv(n or 16, 1, act=act())  # always fits: a 1x1 on the current map

    def same_map(exclude=()):
        _, ch, cw = net.cur
        return [i for i, s in enumerate(net.shape) if s[2:] == (ch, cw) and i not in unroutable and i not in exclude]

    conv()  # layer 0 reads the image
    routed = []  # producers a route already reads (reading them again is one of the features)
    for _ in range(nbody):
        c, ch, cw = net.cur
        last = len(net.secs) - 1
        kind = rng.choices(("conv", "pool", "up", "route", "shortcut", "res", "cell4"), (30, 14, 8, 18, 8, 8, 2))[0]
        qs = int(rng.random() < 0.12)
        if kind == "pool" and min(ch, cw) >= 4:
            size, stride = rng.choice(POOLS)
            if (size, stride) == (2, 2) and ch % 2 == 0 and cw % 2 == 0 and rng.random() < 0.4 and \
                    net.macs + ch * cw * 64 * (c + 9 * 128) < MAC_CAP:  # the 64 -> 64..128 conv + pool kernel's shape
                if c != 64:
                    net.conv(64, 1, act=act())
                net.conv(rng.choice((64, 96, 128)), 3, act=act())
            net.maxpool(size, stride, qs)
        elif kind == "up" and ch * cw * 4 <= MAX_CELLS:
            s = rng.choice([k for k in (2, 2, 3, 4) if ch * cw * k * k <= MAX_CELLS])
            if c % 64 and rng.random() < 0.5 and net.macs + ch * cw * c * 64 < MAC_CAP:  # give the conv + upsample fusion a candidate
                net.conv(64, 1, act=act())
                net.conv(rng.choice((32, 64)), rng.choice((1, 3)), act=act())
            net.upsample(s, qs)
        elif kind == "route":
            cand = same_map(exclude=(last,))
            arity = rng.choice((1, 2, 2, 3))
            if arity == 1 or not cand:
                pool = [i for i in range(last + 1) if i not in unroutable and net.shape[i][2] * net.shape[i][3] <= MAX_CELLS]
                net.route([rng.choice(pool)], qs, absolute=rng.random() < 0.3)
            else:
                srcs = [last] if last not in unroutable and rng.random() < 0.7 else []
                if routed and rng.random() < 0.4:  # a producer read by more than one route
                    srcs += [i for i in routed if i in cand and i not in srcs][:1]
                rest = [k for k in cand if k not in srcs]
                rng.shuffle(rest)
                srcs += rest[:max(0, arity - len(srcs))]
                if len(srcs) < 2:  # one candidate only: list it twice
                    srcs = (srcs * 2)[:2]
                rng.shuffle(srcs)
                if sum(net.shape[s][1] for s in srcs) > 512:
                    srcs = srcs[:2]
                net.route(srcs, qs, absolute=rng.random() < 0.3)
                routed += srcs
        elif kind == "shortcut":
            cand = [i for i in same_map(exclude=(last,)) if net.shape[i][1] == c]
            if cand and last not in unroutable:
                net.shortcut(rng.choice(cand) - len(net.secs) if rng.random() < 0.7 else rng.choice(cand), qs)
            else:
                conv()
        elif kind == "res" and last not in unroutable:  # a residual unit: 1x1 down, 3x3 back up, add; sometimes stacked (from = a shortcut)
            frm = last
            for _ in range(rng.choice((1, 1, 2))):
                net.conv(rng.choice((16, 32, 64)), 1, act=act())
                net.conv(c, rng.choice((3, 3, 5)), act=rng.choice(("linear", act())))
                net.shortcut(frm - len(net.secs))
                frm = len(net.secs) - 1
        elif kind == "cell4":  # a 3-filter conv: 4-byte cells, read by a conv only
            net.conv(3, rng.choice((1, 3)), act=act())
            unroutable.add(len(net.secs) - 1)
            conv()
        else:
            conv()
        if len(net.secs) - 1 in unroutable and kind != "cell4":
            conv()
    for k in range(nheads):
        c, ch, cw = net.cur
        nmask, classes = rng.choice(((3, 2), (3, 80), (2, 3), (1, 11)))  # 21, 255, 16, 16 filters
        if nmask * (classes + 5) * c * ch * cw > MAC_CAP // 2:
            nmask, classes = 3, 2
        tail = len(net.secs) - 1
        if rng.random() < 0.3 and net.macs + ch * cw * c * 48 < MAC_CAP:
            net.conv(rng.choice((32, 48, 64)), rng.choice((1, 3)), act=act())
        net.head(size=rng.choice((1, 1, 1, 3, 5)), nmask=nmask, classes=classes, bn=0)
        unroutable.add(len(net.secs) - 1)
        if k + 1 < nheads:  # the next branch starts from a tensor in front of this head, as in yolov3
            pool = [i for i in range(tail + 1) if i not in unroutable and net.shape[i][2] * net.shape[i][3] <= MAX_CELLS]
            net.route([rng.choice(pool[-4:])], absolute=rng.random() < 0.3)
            r = rng.random()
            if r < 0.4 and net.cur[1] * net.cur[2] * 4 <= MAX_CELLS:
                if net.cur[0] % 64 == 0 or rng.random() < 0.5:
                    net.conv(rng.choice((32, 64)), 1, act=act())
                net.upsample(2)
                cand = same_map(exclude=(len(net.secs) - 1,))
                if cand:
                    net.route([len(net.secs) - 1, rng.choice(cand)])
            elif r < 0.7:
                conv()
    return net.text(f"random_net({seed})")


# --------------------------------------------------------------------------------------------- aimed topologies
def _aimed():
    A = {}

    def add(name, clause, net, **kw):
        A[name] = dict(cfg=net.text(f"{name}: {clause}"), clause=clause, **kw)

    # --- views of a concatenating route
    for name, act1, clause in (("view_same_zp", "leaky", "every input of route 3 is a view, input 1 feeds a 3x3 conv directly with the route's zero point: elided"),
                               ("view_zp_differs", "relu6", "relu6 producer 1 (zp 0) feeds 3x3 conv 2 directly, route 3 has the leaky input's zp 23: "
                                                            "view refused, 16-byte copy")):
        n = Net(24, 24)
        n.conv(32, 3); n.conv(32, 3, act=act1); n.conv(16, 3); n.route([2, 1], absolute=True); n.conv(32, 3); n.head()
        add(name, clause, n)
    for name, act1, clause in (("shared_route_same_zp", "leaky", "one-input route 3 shares producer 1's tensor, 3x3 conv 4 reads its pads with the zp of "
                                                                 "route 5: both routes elided"),
                               ("shared_route_zp_differs", "relu6", "the same with a relu6 producer: view_producer_ok's second loop refuses route 5, "
                                                                    "route 3 still shares")):
        n = Net(24, 24)
        n.conv(32, 3); n.conv(32, 3, act=act1); n.conv(16, 1); n.route([1], absolute=True); n.conv(32, 3); n.route([4, 2, 1], absolute=True)
        n.conv(32, 3); n.head()
        add(name, clause, n)
    n = Net(32, 32)
    n.conv(32, 3); n.conv(32, 3, stride=2); n.maxpool(2, 1); n.conv(32, 3, stride=2); n.upsample(2); n.route([4, 2], absolute=True)
    n.conv(32, 3); n.head()
    add("view_maxpool_upsample", "stand-alone maxpool 2 and upsample 4 write into windows of route 5: elided", n)
    n = Net(32, 32)
    n.conv(32, 3); n.conv(32, 3, stride=2); n.maxpool(2, 1); n.conv(32, 3, stride=2); n.upsample(2); n.route([4, 2], absolute=True)
    n.conv(32, 3); n.maxpool(3, 2); n.conv(32, 5); n.head()
    add("glue_own_zp", "maxpool / upsample / route records with zero points of their own: 3x3 conv 3 behind maxpool 2 refuses the view, "
                       "every conv behind a glue layer pads with the glue layer's zero point", n, glue_own_zp=True)
    for s, st in ((3, 3), (4, 4)):
        n = Net(24, 24)
        n.conv(16, 3); n.conv(32, 3); n.conv(64, 3, stride=st); n.conv(32, 1); n.upsample(s); n.route([4, 1], absolute=True); n.conv(32, 3); n.head()
        add(f"fused_upsample_window_s{s}", f"1x1 conv 3 (c = 64) stores stride-{s} upsampled pixels into upsample 4's window of route 5 "
                                           "(yolov3-tiny's pattern)", n)
    # --- fusions that need a whole round of the chip (weights-stationary 128-channel kernel): large maps, AIMED_BIG
    n = Net(72, 72)
    n.conv(128, 3); n.conv(32, 3); n.maxpool(2, 2); n.conv(32, 3); n.upsample(2); n.route([1, 4], absolute=True); n.conv(32, 1); n.head()
    add("pool_keep_view", "conv 1 (c = 128) + maxpool 2 fused with fuse_pool_keep, the kept pre-pool tensor is a view of route 5; "
                          "the throughput plan refuses the fused form", n)
    n = Net(74, 74)
    n.conv(32, 3); n.conv(128, 1); n.conv(32, 3); n.shortcut(0); n.conv(16, 1); n.route([4, 0], absolute=True); n.head()
    add("fused_shortcut_from_view", "conv 2 (c = 128) + shortcut 3 fused, its `from` tensor (layer 0) is a view of route 5; "
                                    "the throughput plan refuses the fused form", n)
    # --- routes that cannot be elided
    n = Net(24, 24)
    n.conv(32, 3); n.conv(32, 3); n.conv(16, 3); n.route([2, 1], absolute=True); n.conv(16, 1); n.route([4, 1], absolute=True); n.head()
    add("producer_in_two_routes", "producer 1 is a view of route 3; route 5 lists it again and falls back to the copy, reading a window", n)
    n = Net(24, 24)
    n.conv(32, 3); n.conv(32, 3); n.route([1, 1], absolute=True); n.conv(32, 3); n.head()
    add("route_same_layer_twice", "route 2 lists layer 1 twice: not elided", n)
    n = Net(20, 20)
    n.conv(32, 3); n.conv(33, 3); n.conv(17, 3); n.route([2, 1], absolute=True); n.conv(32, 3); n.head()
    add("route_byte_copy", "17 + 33 channels: no view, and the second input starts inside a 16-byte group: byte copy", n)
    # --- shortcut fusion candidates by index
    n = Net(16, 16)
    n.conv(32, 3); n.conv(32, 3); n.conv(32, 3); n.shortcut(-2); n.conv(32, 3); n.shortcut(-1); n.head()
    add("shortcut_neighbours", "shortcut 3 adds conv 2's own input (index i - 1): candidate, refused by the launcher (c = 32); shortcut 5 adds "
                               "conv 4 to itself (index == i): never a candidate", n)
    # --- candidates by shape that the launcher refuses (general kernel)
    n = Net(16, 16)
    n.conv(64, 3); n.conv(32, 5); n.upsample(2); n.head()
    add("refused_upsample_5x5", "5x5 conv 1 on c = 64 + upsample: candidate, refused by conv_generic_forward, re-run unfused", n)
    n = Net(16, 16)
    n.conv(32, 3); n.conv(32, 5); n.shortcut(0); n.head()
    add("refused_shortcut_5x5", "5x5 conv 1 on c = 32 + shortcut: candidate, refused, re-run unfused", n)
    n = Net(16, 16)
    n.conv(48, 3); n.head(size=5)
    add("refused_yolo_5x5", "5x5 quant_stop head on c = 48 + yolo: candidate, refused, re-run unfused", n)
    n = Net(18, 18)
    n.conv(32, 3); n.conv(32, 3, padding=0); n.maxpool(2, 2); n.head()
    add("refused_pool_padding0", "3x3 padding=0 conv 1 on c = 32 (even output map) + maxpool 2/2: candidate, refused, re-run unfused", n)
    n = Net(16, 16)
    n.conv(64, 3); n.conv(96, 3); n.maxpool(2, 2); n.head()
    add("pool_64_to_96", "3x3 conv 1, 64 -> 96 channels, + maxpool 2/2: the one c % 64 == 0 shape plan_fusion admits (its own fused kernel)", n)
    n = Net(20, 24)
    n.conv(16, 3); n.conv(32, 3); n.maxpool(2, 2); n.head()
    add("pool_16_to_32", "3x3 conv 1, 16 -> 32 channels, + maxpool 2/2: fused on the table-driven kernel (conv_pool16, id 7)", n)
    n = Net(17, 17)
    n.conv(32, 3); n.conv(32, 3); n.maxpool(2, 2); n.conv(32, 3); n.maxpool(3, 2); n.head()
    add("pool_non_candidates", "3x3 conv 1 on an odd map + maxpool 2/2 and 3x3 conv 3 + maxpool 3/2: unfused from the start", n)
    # --- the general kernel and the 4-byte cells
    n = Net(20, 20)
    n.conv(32, 3); n.conv(16, 3); n.conv(32, 3); n.conv(24, 5); n.route([1, 2], absolute=True); n.conv(32, 3); n.route([5, 3], absolute=True); n.head()
    add("kxk_reads_window", "5x5 conv 3 (general kernel) reads layer 2's tensor, a window at byte offset 16 of route 4; route 6 (32 + 24) copies "
                            "16-byte groups", n)
    n = Net(16, 16)
    n.conv(16, 3); n.conv(3, 1, act="relu6"); n.conv(32, 3); n.conv(3, 3, act="linear"); n.conv(16, 5); n.head()
    add("cell4_conv_feeds_conv", "3-filter convs 1 and 3 store 4-byte cells that a 3x3 and a 5x5 conv read", n)
    n = Net(12, 12)
    n.conv(64, 3); n.conv(32, 1); n.upsample(2, qs=1); n.head()
    add("fused_upsample_quant_stop", "upsample 2 has a quant_stop float tail: conv 1 (c = 64) must not swallow it", n)
    n = Net(58, 58)
    n.conv(16, 3); n.conv(40, 3, stride=7); n.head()
    add("kxk_stride7_wide_m_tile", "a stride-7 conv on c = 16 reaches the general kernel's 128 x 64 tile through the host (the 256-pixel patch "
                                   "of 108 x 108 or 220 x 52 cells does not fit in LDS)", n)
    return A


AIMED = _aimed()
AIMED_BIG = ("pool_keep_view", "fused_shortcut_from_view")  # above MAC_CAP (see the module docstring)

# random_net seeds of the committed sweep: every net passes the liveness condition of tests/test_netgen_cpu.py (a seed that fails it is
# replaced, not excused); act_gain 4 scales the activations up so that wrapping stores occur, glue_own_zp gives glue layers own zero points
SEEDS = ((0, 1.0, False), (2, 1.0, True), (7, 4.0, False), (12, 1.0, False), (16, 1.0, False), (17, 4.0, True), (22, 1.0, True), (24, 1.0, False),
         (27, 4.0, False), (28, 1.0, False), (29, 4.0, True), (30, 1.0, True), (36, 1.0, False), (39, 4.0, False), (43, 4.0, False), (47, 4.0, False), (135, 4.0, False),
         (176, 1.0, False))


def sweep():
    """name -> dict(cfg text, weights seed, act_gain, glue_own_zp) of every net of the sweep"""
    nets = {}
    for k, (seed, gain, gzp) in enumerate(SEEDS):
        nets[f"rand{seed}"] = dict(cfg=random_net(seed), wseed=1000 + seed, act_gain=gain, glue_own_zp=gzp)
    for k, (name, a) in enumerate(AIMED.items()):
        nets[name] = dict(cfg=a["cfg"], wseed=500 + k, act_gain=a.get("act_gain", 1.0), glue_own_zp=a.get("glue_own_zp", False))
    return nets


# ---------------------------------------------------------------------------- the reference's view of the sweep
# The reference has no integer [shortcut] (the op is this build's own: a quantized shortcut kills it with a segfault or an assert of
# src/blas.c), so it runs the TWIN of a net: every [shortcut] replaced by a one-input route, a copy with the same shape, so that every
# later index holds.  tests/golden/netgen_ref.json holds the reference's tensors of the twins.
SHORTCUT_FEATURES = ("shortcut_from_convolutional", "shortcut_from_shortcut", "shortcut_from_route_input", "quant_stop_shortcut")
REF_IMAGE_SEEDS = (5, 6)  # synth_image_u8 seeds of the two images every twin is recorded on


def reference_twin(cfg_text):
    """cfg text with a one-input `[route] layers = -1` in place of each [shortcut]; its quantized / quant_stop lines are kept and the
    text is otherwise unchanged."""
    out, lines, i = [], cfg_text.split("\n"), 0
    while i < len(lines):
        if lines[i].strip().replace(" ", "") == "[shortcut]":
            out += ["[route]", "layers = -1"]
            i += 1
            while i < len(lines) and not lines[i].strip().startswith("["):
                key = lines[i].strip().replace(" ", "").partition("=")[0]
                if key in ("quantized", "quant_stop") or not lines[i].strip():
                    out.append(lines[i])
                i += 1
        else:
            out.append(lines[i])
            i += 1
    return "\n".join(out)


def _ref_extra():
    """aimed nets of the twin list only: what the sweep's own nets leave to one reading of the reference"""
    E = {}
    n = Net(24, 24)
    n.conv(32, 3); n.conv(32, 3, act="relu6"); n.conv(16, 1, act="linear"); n.route([2, 1, 0], qs=1, absolute=True); n.conv(32, 3); n.head()
    E["route_quant_stop_mixed_records"] = dict(
        cfg=n.text("route_quant_stop_mixed_records: the float tail of route 3 dequantises each input with THAT input's scale and zero "
                   "point (ref: src/route_layer.c:121-129); linear, relu6 and leaky producers, and a record of the route's own that "
                   "differs from all three"), wseed=900, act_gain=1.0, glue_own_zp=True)
    return E


REF_EXTRA = _ref_extra()


def ref_sweep():
    """name -> dict like sweep() of the nets the reference runs: the twin of every net of the sweep with the sweep's own weight seeds and
    gains, and REF_EXTRA.  AIMED_BIG stays out: its maps (72 and 74 cells wide) and work are above what the reference-pinned GPU tests allow themselves
    (48 x 48, MAC_CAP), and what those two nets aim at, fusions of a whole round of the chip, is the planner's doing, not arithmetic."""
    nets = {}
    for name, spec in sweep().items():
        if name not in AIMED_BIG:
            nets[name] = dict(spec, cfg=reference_twin(spec["cfg"]), has_shortcut="[shortcut]" in spec["cfg"])
    for name, spec in REF_EXTRA.items():
        nets[name] = dict(spec, has_shortcut=False)
    return nets


POOL_MAPS = ((1, 1), (2, 3), (5, 6), (7, 4))


def pool_nets():
    """name -> (cfg text, (size, stride, padding, h, w)) of the one-pool nets: 1x1 conv, pool, head.  Sizes 1, 2, 3, 5, strides 1..4,
    padding 0..size + 1 on POOL_MAPS; where h + padding < size (or w) the geometry is kept only if C's truncating division still gives
    one output row (the reference's and the host's parsers then accept it; Python's floor would say 0)."""
    nets = {}
    for size in (1, 2, 3, 5):
        for stride in (1, 2, 3, 4):
            for padding in range(size + 2):
                for h, w in POOL_MAPS:
                    if cdiv(h + padding - size, stride) + 1 < 1 or cdiv(w + padding - size, stride) + 1 < 1:
                        continue
                    n = Net(h, w)
                    n.conv(17, 1, act="leaky"); n.maxpool(size, stride, padding=padding); n.head()
                    nets[f"pool_k{size}_s{stride}_p{padding}_{h}x{w}"] = (n.text(), (size, stride, padding, h, w))
    return nets


def upsample_nets():
    """name -> (cfg text, (stride, h, w)) of the one-upsample nets: 1x1 conv, upsample, head; strides 1..4 on POOL_MAPS"""
    nets = {}
    for stride in (1, 2, 3, 4):
        for h, w in POOL_MAPS:
            n = Net(h, w)
            n.conv(17, 1, act="leaky"); n.upsample(stride); n.head()
            nets[f"up_s{stride}_{h}x{w}"] = (n.text(), (stride, h, w))
    return nets


ONE_LAYER_WSEED = 77


# ------------------------------------------------------------------------------------- features from the text
def parse(cfg_text):
    """[(section type, {key: value})] of the layers of a cfg text (the [net] section dropped)"""
    secs = []
    for raw in cfg_text.splitlines():
        line = raw.strip().replace(" ", "")
        if not line or line[0] in "#;":
            continue
        if line[0] == "[":
            secs.append((line.strip("[]"), {}))
        else:
            k, _, v = line.partition("=")
            secs[-1][1][k] = v
    return secs[1:]


def _map_sizes(cfg_text, secs):
    """(height, width) of every layer's output, from the text"""
    top = dict(l.replace(" ", "").split("=") for l in cfg_text.split("[convolutional]")[0].splitlines() if "=" in l and l[0] != "#")
    h, w, out = int(top["height"]), int(top["width"]), []
    for i, (t, o) in enumerate(secs):
        if t == "convolutional":
            size, stride = int(o["size"]), int(o.get("stride", 1))
            p = size // 2 if int(o.get("pad", 0)) else int(o.get("padding", 0))
            h, w = (h + 2 * p - size) // stride + 1, (w + 2 * p - size) // stride + 1
        elif t == "maxpool":
            size, stride = int(o["size"]), int(o["stride"])
            pad = int(o.get("padding", size - 1))
            h, w = cdiv(h + pad - size, stride) + 1, cdiv(w + pad - size, stride) + 1
        elif t == "upsample":
            h, w = h * int(o.get("stride", 2)), w * int(o.get("stride", 2))
        elif t == "route":
            x = int(o["layers"].split(",")[0])
            h, w = out[x if x >= 0 else i + x]
        out.append((h, w))
    return out


def features(cfg_text):
    """The set of feature names of section 1 of the sweep's specification that this cfg exercises, from its text alone."""
    secs = parse(cfg_text)
    f = set()
    srcs_of = {}
    for i, (t, o) in enumerate(secs):
        if t == "route":
            srcs_of[i] = [int(x) if int(x) >= 0 else i + int(x) for x in o["layers"].split(",")]
    read_by_routes = [s for v in srcs_of.values() for s in set(v)]
    hw = _map_sizes(cfg_text, secs)
    for i, (t, o) in enumerate(secs):
        qs = int(o.get("quant_stop", 0))
        if t == "maxpool":
            h, w = hw[i - 1]
            f.add("maxpool_on_odd_map" if (h & 1) or (w & 1) else "maxpool_on_even_map")
        if t == "convolutional":
            size, stride, n = int(o["size"]), int(o.get("stride", 1)), int(o["filters"])
            f |= {f"size{size}", f"conv_stride{stride}", f"act_{o['activation']}", f"bn{int(o.get('batch_normalize', 0))}"}
            f.add("pad1" if int(o.get("pad", 0)) else ("padding0" if int(o.get("padding", 0)) == 0 else "padding_n"))
            if size > 1 and not int(o.get("pad", 0)) and int(o.get("padding", 0)) == size - 1:
                f.add("padding_size_minus_1")
            f.add(f"filters{n}" if n in FILTERS or n in (3, 255) else ("filters_mod16" if n % 16 == 0 else "filters_odd"))
            if n == 3:
                f.add("cell4_conv")
            nxt = secs[i + 1] if i + 1 < len(secs) else ("", {})
            if nxt[0] == "maxpool" and int(nxt[1]["size"]) == 2 and int(nxt[1]["stride"]) == 2 and size == 3 and stride == 1 and \
                    64 <= n <= 128 and n % 32 == 0 and i > 0 and secs[i - 1][0] == "convolutional" and int(secs[i - 1][1]["filters"]) == 64:
                f.add("pool_64_to_64_128")
        elif t == "maxpool":
            f.add(f"maxpool{o['size']}/{o['stride']}")
            if qs:
                f.add("quant_stop_maxpool")
        elif t == "upsample":
            f.add(f"upsample{o.get('stride', 2)}")
            if qs:
                f.add("quant_stop_upsample")
        elif t == "route":
            raw = [int(x) for x in o["layers"].split(",")]
            f.add(f"route{len(raw)}")
            f.add("route_negative" if any(x < 0 for x in raw) else "route_absolute")
            if any(read_by_routes.count(s) > 1 for s in srcs_of[i]):
                f.add("producer_in_two_routes")
            if len(raw) > 1:
                acts = {secs[s][1].get("activation") for s in srcs_of[i] if secs[s][0] == "convolutional"}
                if len(acts) > 1:
                    f.add("route_mixed_activations")
                if len(set(srcs_of[i])) < len(raw):
                    f.add("route_same_layer_twice")
            if qs:
                f.add("quant_stop_route")
                if len({secs[s][1].get("activation") for s in srcs_of[i] if secs[s][0] == "convolutional"}) > 1:
                    f.add("quant_stop_route_mixed_records")  # (of the twin list: REF_EXTRA)
        elif t == "shortcut":
            frm = int(o["from"])
            frm = frm if frm >= 0 else i + frm
            f.add(f"shortcut_from_{secs[frm][0]}")
            if frm in read_by_routes:
                f.add("shortcut_from_route_input")
            if qs:
                f.add("quant_stop_shortcut")
        elif t == "yolo":
            f.add("yolo")
    f.add(f"heads{sum(t == 'yolo' for t, _ in secs)}")
    return f


REQUIRED_FEATURES = (
    [f"size{k}" for k in range(1, 12)] + ["conv_stride1", "conv_stride2", "conv_stride3", "conv_stride7", "pad1", "padding0", "padding_n", "padding_size_minus_1"] +
    [f"filters{n}" for n in FILTERS] + ["filters3", "filters255", "pool_64_to_64_128", "cell4_conv", "bn0", "bn1"] + [f"act_{a}" for a in ACTS] +
    ["maxpool_on_odd_map", "maxpool_on_even_map", "maxpool2/2", "maxpool2/1", "maxpool3/2", "maxpool5/1", "maxpool9/1", "maxpool13/1", "upsample2", "upsample3", "upsample4",
     "route1", "route2", "route3", "route_negative", "route_absolute", "producer_in_two_routes", "route_mixed_activations", "route_same_layer_twice",
     "shortcut_from_convolutional", "shortcut_from_shortcut", "shortcut_from_route_input",
     "quant_stop_maxpool", "quant_stop_upsample", "quant_stop_route", "quant_stop_shortcut", "heads1", "heads2", "heads3"])
