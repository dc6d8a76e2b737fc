"""Sites that put int8 accumulators on the edges of the fused-table epilogue: exact rounding ties, both clamps, the bounds of the half-step
index, accumulators that a float cannot hold, the one value the half-step rule cannot serve.  Shared by tests/test_requant_edges_cpu.py (plans,
the numpy model, the coverage conditions) and tests/test_gpu_requant_edges.py (the kernels).  Host only: nothing here touches a device.

Technique ("Edge accumulators"):
  dyadic scales   tensor scales are powers of two, so cs = (in * w) / out is exactly 2^-e: one accumulator in 2^e is an exact tie, the product
                  float(acc) * cs is exact and mhip_conv_i8_lut2_ok accepts the scale (the half-step table runs)
  witness table   SiLU with (conv-out, sigmoid, out) scales (2^-7, 2^-8, 2^-8): neighbouring inputs map to different bytes almost everywhere, so
                  a result that is off by one shows in the output byte; the other side of a pair and a chained stage get tables of their own
                  (WITNESS_B, WITNESS_C) so that swapped tables show
  chosen accs     a few input pixels (whole k x k neighbourhoods) are zero in every frame: there the accumulator IS the bias, and the bias vector
                  is a list of edge accumulators (edge_accs)
  third witness   evaluate() recomputes every convolution in numpy (int64 sums, float32 requantisation) from the checker's input tensor
"""
import struct

import numpy as np

import marsfile
from conftest import lcg_frame

P2 = lambda e: float(2.0 ** e)
# measured through the checker: inputs that differ from their neighbour (negative of 128, non-negative of 127); do the two lowest / highest differ
WITNESS = (P2(-7), P2(-8), P2(-8))    # 74, 126; lowest and highest both differ: a clamp that is off by one shows at either end
WITNESS_B = (P2(-6), P2(-8), P2(-7))  # 66, 126; the highest differ.  The other side of a pair / a chained stage: swapped tables show
WITNESS_C = (P2(-7), P2(-7), P2(-8))  # 92, 95; the lowest differ


def f32(x):
    return np.float32(x)


def combined_scale(s_in, s_w, s_out):
    """the reference's float32 steps: (in * w) / out"""
    return f32(f32(f32(s_in) * f32(s_w)) / f32(s_out))


def edge_accs(cs, n):
    """up to n accumulators on the epilogue's edges for combined scale cs (p = acc * cs), the essential ones first:
    p = +-0.5, +-1.5, +-2.5, 126.5, 127.5, -127.5, -128.5, 2p = +-255, +-256, +-257 (the bounds of the half-step index), 0, +-1,
    +-2^20, +-(2^24 + 1) (no float holds it), +-2^30; then each of the p values one accumulator up and down.  For a dyadic cs the p values are hit
    exactly; otherwise the nearest accumulator stands in."""
    twop = [1, -1, 3, -3, 5, -5, 253, 255, -255, -257, 256, -256, 257]
    core = [int(round(t / 2.0 / float(cs))) for t in twop]
    first = core + [0, 1, -1, 1 << 20, -(1 << 20), (1 << 24) + 1, -(1 << 24) - 1, 1 << 30, -(1 << 30)]
    near = [a + d for a in core for d in (1, -1)]
    out = []
    for a in first + near:
        if a not in out and abs(a) <= 1 << 30:
            out.append(a)
    return out[:n]


def quirk_acc(cs):
    """the accumulator a* > 0 with float32(a*) * cs == 0x3EFFFFFF (0.49999997), which the reference's float add rounds UP to 1 and
    trunc(2x) does not: mhip_conv_i8_lut2_ok refuses such a scale.  None when no accumulator lands there."""
    quirk = np.array([0x3EFFFFFF], dtype=np.uint32).view(np.float32)[0]
    a0 = int(float(quirk) / float(cs))
    a = np.arange(max(a0 - 64, 1), a0 + 64, dtype=np.int64)
    hit = a[(a.astype(np.float32) * f32(cs)) == quirk]
    return int(hit[0]) if hit.size else None


class Site:
    """one .mars file with its frames and what the tests expect of it.
    stages: per requantising stage a dict
        layer    index of the CONV2D (or ADD) layer in the file
        need     coverage conditions the stage must meet: "ties", "clamps", "wide", "relu" (see coverage())
        edges    {channel: accumulator} placed through the bias, or None"""

    def __init__(self, name, d, frames, stages, form=(), full=(), lut2=None, fusion=1, tuning=(), off=(), min_rows=0, safe=1):
        self.name, self.d, self.frames, self.stages = name, d, frames, stages
        self.form = tuple(form)      # substrings the default plan's op lines must contain (each in at least one line)
        self.full = tuple(full)
        self.lut2 = lut2             # True / False: every conv op has / no conv op has a half-step table; None: not checked
        self.fusion = fusion         # fusion level the form needs (2 for the fused bottleneck)
        self.safe = safe             # the "safe" flag of the site's first convolution (0: |acc * cs| may leave the int32 range)
        self.tuning = tuple(tuning)  # ((knob, value, default), ...) the form needs
        self.off = tuple(off)        # the switches that turn the site's fusions off, one at a time
        self.min_rows = min_rows     # launches of the rows kernel (variant 20) one run must add

    def __repr__(self):
        return self.name


class Builder:
    """a graph of convolutions whose scales are chosen from the combined scale wanted (dyadic unless told otherwise)"""

    def __init__(self, seed):
        self.G = marsfile.Graph()
        self.rng = np.random.default_rng(seed)
        self.stages = []
        self.zero = []  # (y, x) input pixels that every frame zeroes

    def input(self, h, w, c, scale=P2(-5), nchw=False):
        self.nchw = nchw
        self.x = self.G.tensor([1, c, h, w] if nchw else [1, h, w, c], fmt=marsfile.NCHW if nchw else marsfile.NHWC, scale=scale)
        self.in_shape = (h, w, c)
        return self.x

    def _act(self, shape, scale):
        return self.G.tensor(shape, fmt=marsfile.NCHW if self.nchw else marsfile.NHWC, scale=scale)

    def conv(self, x, in_c, out_c, oh, ow, k=1, stride=1, cs=P2(-4), triple=WITNESS, wr=3, act="silu", edges=False, out=None,
             need=("ties", "clamps", "wide"), bias_range=40, w_scale=None):
        """conv (+ SiLU chain / RELU layer / nothing) with combined scale cs: the weight scale follows from the input's and the convolution
        result's scales.  edges: the bias carries edge_accs(cs) in its first channels (the caller zeroes input neighbourhoods).
        Returns the result tensor."""
        G, rng = self.G, self.rng
        s_in = G.tensors[x]["scale"]
        s1 = triple[0]
        ws = float(cs) * s1 / s_in if w_scale is None else w_scale
        shape = [1, out_c, oh, ow] if self.nchw else [1, oh, ow, out_c]
        wshape = (out_c, in_c, k, k) if self.nchw else (out_c, k, k, in_c)
        wt = G.tensor(list(wshape), fmt=marsfile.OIHW if self.nchw else marsfile.OHWI, scale=ws,
                      data=rng.integers(-wr, wr + 1, wshape, dtype=np.int8))
        bias = rng.integers(-bias_range, bias_range + 1, out_c).astype(np.int32)
        placed = None
        if edges:
            cs32 = combined_scale(s_in, ws, s1)
            lst = edge_accs(cs32, out_c) if edges is True else list(edges)[:out_c]
            bias[:len(lst)] = lst
            placed = dict(enumerate(lst))
        b = G.tensor([out_c], dtype=marsfile.I32, fmt=marsfile.D1, scale=1.0, data=bias)
        if act == "silu":
            a = self._act(shape, s1)
            g = self._act(shape, triple[1])
            o = out if out is not None else self._act(shape, triple[2])
            G.conv(x, a, wt, b, (k, k), (stride, stride))
            self.stages.append(dict(layer=len(G.layers) - 1, need=set(need), edges=placed))
            G.layer(marsfile.SIGMOID, [a], [g])
            G.layer(marsfile.MUL, [a, g], [o])
            return o
        if act == "relu":
            a = self._act(shape, s1)
            o = out if out is not None else self._act(shape, s1)
            G.conv(x, a, wt, b, (k, k), (stride, stride))
            self.stages.append(dict(layer=len(G.layers) - 1, need=set(need), edges=placed))
            G.layer(marsfile.RELU, [a], [o])
            return o
        o = out if out is not None else self._act(shape, s1)
        G.conv(x, o, wt, b, (k, k), (stride, stride))
        self.stages.append(dict(layer=len(G.layers) - 1, need=set(need), edges=placed))
        return o

    def add(self, a, b, shape, s_out, need):
        o = self.G.tensor(list(shape), scale=s_out)
        self.G.layer(marsfile.ADD, [a, b], [o])
        self.stages.append(dict(layer=len(self.G.layers) - 1, need=set(need), edges=None))
        return o

    def concat(self, parts, shape, scale):
        o = self.G.tensor(list(shape), scale=scale)
        self.G.concat(parts, o)
        return o

    def zero_under(self, out_pixels, k, stride, oh, ow):
        """zero the k x k input neighbourhoods (SAME padding) of these output pixels"""
        h, w, _ = self.in_shape
        pt = max((oh - 1) * stride + k - h, 0) // 2
        pl = max((ow - 1) * stride + k - w, 0) // 2
        for (oy, ox) in out_pixels:
            for ky in range(k):
                for kx in range(k):
                    y, x = oy * stride - pt + ky, ox * stride - pl + kx
                    if 0 <= y < h and 0 <= x < w:
                        self.zero.append((y, x))

    def frames(self, B, seed, small=0):
        """B input frames: random int8 (small: values in -small .. small) with the zeroed pixels"""
        h, w, c = self.in_shape
        out = []
        for f in range(B):
            v = lcg_frame(0xED6E0000 + 64 * seed + f, h * w * c).view(np.int8).astype(np.int32)
            if small:
                v = np.mod(v, 2 * small + 1) - small
            v = v.astype(np.int8).reshape((c, h, w) if self.nchw else (h, w, c))
            for (y, x) in self.zero:
                if self.nchw:
                    v[:, y, x] = 0
                else:
                    v[y, x, :] = 0
            out.append(np.ascontiguousarray(v).view(np.uint8).reshape(-1))
        return out

    def site(self, name, outs, B=3, seed=0, small=0, **kw):
        return Site(name, self.G.serialise([self.x], outs), self.frames(B, seed, small), self.stages, **kw)


# ------------------------------------------------------------------------------------------------ the sites
def _corner_and_inside(oh, ow):
    return [(0, 0), (oh // 2, ow // 2), (oh - 1, ow - 2)]


def plain_site(name, h, w, in_c, out_c, k=1, stride=1, cs=P2(-4), wr=3, act="silu", seed=1, need=("ties", "clamps", "wide"), small=0,
               in_scale=P2(-5), triple=WITNESS, nchw=False, B=3, edges=True, **kw):
    """one convolution of the graph input with the witness table (or a RELU layer, or no table) behind it"""
    b = Builder(seed)
    x = b.input(h, w, in_c, scale=in_scale, nchw=nchw)
    oh, ow = (h + stride - 1) // stride, (w + stride - 1) // stride
    o = b.conv(x, in_c, out_c, oh, ow, k, stride, cs=cs, triple=triple, wr=wr, act=act, edges=edges, need=need)
    b.zero_under(_corner_and_inside(oh, ow), k, stride, oh, ow)
    return b.site(name, [o], B=B, seed=seed, small=small, **kw)


def slice_site(name="slice", h=16, w=16, seed=11):
    """two 1x1s write the channel slices of a concat that a 3 x 3 reads (it stays materialised)"""
    b = Builder(seed)
    x = b.input(h, w, 64)
    b.zero_under(_corner_and_inside(h, w), 1, 1, h, w)
    cat = b.G.tensor([1, h, w, 64], scale=P2(-8))
    s1 = b.conv(x, 64, 32, h, w, 1, 1, cs=P2(-4), edges=True)
    s2 = b.conv(x, 64, 32, h, w, 1, 1, cs=P2(-5), triple=(P2(-6), P2(-8), P2(-8)), wr=6, edges=True)  # (both slices at the concat's scale)
    b.G.concat([s1, s2], cat)
    o = b.conv(cat, 64, 32, h, w, 3, 1, cs=P2(-4), wr=2, triple=WITNESS_B)
    return b.site(name, [o], seed=seed, form=(" pix_stride=64",), lut2=True)


def add_site(name, c, h, w, order, table, s_out, seed, need):
    """x -> A (1x1, SiLU or no table) -> Add(A, x) in either operand order: the planner folds the Add into A's epilogue.  Operand scales 2^-5;
    s_out 2^-4 makes every odd sum a tie (negative ones must round UP), 2^-5 saturates on both sides"""
    b = Builder(seed)
    x = b.input(h, w, c, scale=P2(-5))
    b.zero_under(_corner_and_inside(h, w), 1, 1, h, w)
    trip = (P2(-7), P2(-8), P2(-5)) if table else (P2(-5), 0, 0)
    a = b.conv(x, c, c, h, w, 1, 1, cs=P2(-4) if table else P2(-5), triple=trip, wr=3 if c <= 64 else 2, act="silu" if table else "none",
               edges=True, need=("ties", "clamps", "wide"))
    o = b.add(a, x, [1, h, w, c], s_out, need) if order == 0 else b.add(x, a, [1, h, w, c], s_out, need)
    return b.site(name, [o], seed=seed, form=(" add=",), lut2=True)


def add3_site(name, c, h, w, seed, s_out=P2(-4)):
    """the bottleneck's shape: x -> 1x1 -> 3x3 -> Add(x, 3x3): the Add folds into the 3 x 3 (patch-staged at 32 channels)"""
    b = Builder(seed)
    x = b.input(h, w, c, scale=P2(-5))
    b.zero_under(_corner_and_inside(h, w), 1, 1, h, w)
    t = b.conv(x, c, c, h, w, 1, 1, cs=P2(-4), edges=True, wr=4 if c == 32 else 3)
    u = b.conv(t, c, c, h, w, 3, 1, cs=P2(-4), triple=(P2(-6), P2(-8), P2(-5)), wr=2 if c == 32 else 1)
    o = b.add(x, u, [1, h, w, c], s_out, ("ties",) if s_out == P2(-4) else ("clamps",))
    return b.site(name, [o], seed=seed, form=(" add=",), lut2=True)


def split_site(name, in_c=32, h=16, w=16, stride=1, seed=21, chain=0):
    """x -> A: 3 x 3 SiLU to 64 channels -> cv1, cv2: SiLU 1x1s to 32 channels each (fuse_split) [-> D: a SiLU 1x1 32 -> 32 on side `chain`]"""
    b = Builder(seed)
    ih, iw = (h, w) if stride == 1 else (2 * h, 2 * w)
    x = b.input(ih, iw, in_c)
    b.zero_under(_corner_and_inside(h, w), 3, stride, h, w)
    t = b.conv(x, in_c, 64, h, w, 3, stride, cs=P2(-5), wr=2 if in_c >= 32 else 3, edges=True)
    t1, t2, td = (WITNESS, WITNESS_B, WITNESS_C) if chain != 2 else (WITNESS_B, WITNESS_C, WITNESS)  # every stage has the two-ended table once
    cv1 = b.conv(t, 64, 32, h, w, 1, 1, cs=P2(-4), triple=t1, wr=4)
    cv2 = b.conv(t, 64, 32, h, w, 1, 1, cs=P2(-3), triple=t2, wr=2)
    outs = [cv1, cv2]
    form = [" split_next"]
    full = []
    off = ["MARS_HIP_NO_SPLIT"]
    if chain:
        d = b.conv(cv1 if chain == 1 else cv2, 32, 32, h, w, 1, 1, cs=P2(-4), triple=td, wr=5)
        outs.append(d)
        full = [" split_chain %d" % chain]
        off = ["MARS_HIP_NO_CHAIN", "MARS_HIP_NO_SPLIT"]
    return b.site(name, outs, seed=seed, form=form, full=full, lut2=True, off=off)


def both_site(name, in_c=128, h=12, w=12, seed=31, tail="outputs", side=1, cat=False):
    """cv1, cv2: SiLU 1x1s from in_c to 64 channels each as one tile (pair_both) over the graph input or (cat) over the never-materialised
    concat({a 3 x 3 of x, x}); tail "chain": a SiLU 1x1 64 -> 64 reads side `side` alone (elided), "chain_out": the side is an output too"""
    b = Builder(seed)
    if cat:
        c = in_c // 2
        x = b.input(h, w, c, scale=P2(-8))
        b.zero_under([(h // 2, w // 2)], 3, 1, h, w)
        first = b.conv(x, c, c, h, w, 3, 1, cs=P2(-5), wr=2, edges=True)
        src = b.concat([first, x], [1, h, w, in_c], P2(-8))
    else:
        x = src = b.input(h, w, in_c)
        b.zero_under(_corner_and_inside(h, w), 1, 1, h, w)
    wr = 2 if in_c >= 128 else 3
    t1, t2, td = (WITNESS, WITNESS_B, WITNESS_C) if side == 1 else (WITNESS_B, WITNESS_C, WITNESS)
    cv1 = b.conv(src, in_c, 64, h, w, 1, 1, cs=P2(-4), triple=t1, wr=wr, edges=not cat)
    cv2 = b.conv(src, in_c, 64, h, w, 1, 1, cs=P2(-5), triple=t2, wr=2 * wr, edges=not cat)
    outs = [cv1, cv2]
    form = [" pair_both"]
    off = ["MARS_HIP_NO_BOTH"]
    if tail.startswith("chain"):
        s, other = (cv1, cv2) if side == 1 else (cv2, cv1)
        d = b.conv(s, 64, 64, h, w, 1, 1, cs=P2(-4), triple=td, wr=3)
        outs = [other, d] + ([s] if tail == "chain_out" else [])
        form += [" both_chain=%d" % side] + ([" both_elide"] if tail == "chain" else [])
        off = ["MARS_HIP_NO_BOTH_CHAIN", "MARS_HIP_NO_BOTH"]
    if cat:
        form += [" seg=2"]
    return b.site(name, outs, seed=seed, form=form, lut2=True, off=off)


def pair_site(name="pair", h=12, w=12, seed=41):
    """sides of 32 channels over a plain input: the side-by-side pair kernel"""
    b = Builder(seed)
    x = b.input(h, w, 64)
    b.zero_under(_corner_and_inside(h, w), 1, 1, h, w)
    cv1 = b.conv(x, 64, 32, h, w, 1, 1, cs=P2(-4), triple=WITNESS, wr=3, edges=True)
    cv2 = b.conv(x, 64, 32, h, w, 1, 1, cs=P2(-5), triple=WITNESS_B, wr=6, edges=True)
    return b.site(name, [cv1, cv2], seed=seed, form=(" pair_next",), lut2=True)


def c3_site(name, c=32, h=16, w=16, shortcut=True, seed=51, fusion=1):
    """a C3 block: x (2c) -> cv1, cv2 (c each); one bottleneck (1x1, 3x3, optional Add) on cv1's branch; cv3 over concat({m, cv2}).
    fusion 1: the 3 x 3 takes cv3 (fuse_post); fusion 2: it takes the bottleneck's 1x1 in front instead (fuse_bottleneck)"""
    b = Builder(seed)
    x = b.input(h, w, 2 * c)
    b.zero_under(_corner_and_inside(h, w), 1, 1, h, w)
    cv1 = b.conv(x, 2 * c, c, h, w, 1, 1, cs=P2(-4), triple=(P2(-7), P2(-8), P2(-7)), wr=3, edges=True)
    cv2 = b.conv(x, 2 * c, c, h, w, 1, 1, cs=P2(-5), triple=WITNESS_B, wr=6, edges=True)
    t = b.conv(cv1, c, c, h, w, 1, 1, cs=P2(-4), triple=WITNESS, wr=8 if c == 32 else 6)
    u = b.conv(t, c, c, h, w, 3, 1, cs=P2(-4), triple=(P2(-6), P2(-8), P2(-7)), wr=2 if c == 32 else 1)
    if shortcut:
        u = b.add(cv1, u, [1, h, w, c], P2(-6), ("ties",))
    cat = b.concat([u, cv2], [1, h, w, 2 * c], P2(-8))
    cv3 = b.conv(cat, 2 * c, 2 * c, h, w, 1, 1, cs=P2(-4), triple=WITNESS_C, wr=3 if c == 32 else 2)
    form = [" pre" if fusion == 2 else " post_next"] + ([" add="] if shortcut else [])  # (a 3 x 3 that takes the 1x1 in front does not take cv3)
    off = ["MARS_HIP_BOTTLENECK_LIMIT" if fusion == 2 else "MARS_HIP_NO_POST"]
    return b.site(name, [cv3, cv1], seed=seed, form=form, lut2=True, off=off, fusion=fusion)


def slow_table_site(name="slow_table", h=16, w=16, seed=61):
    """a combined scale the half-step table cannot serve (1 / 640: accumulator 320 gives 0.49999997): the 6-instruction table path, with
    +-a* and their neighbours in the bias.  The reference rounds +-a* to +-1."""
    s_in, s_w, s1 = 0.04, 1.0 / 64, 0.4
    cs = combined_scale(s_in, s_w, s1)
    a = quirk_acc(cs)
    assert a is not None, "no accumulator reaches 0x3EFFFFFF at this scale: pick another one"
    b = Builder(seed)
    x = b.input(h, w, 64, scale=s_in)
    b.zero_under(_corner_and_inside(h, w), 1, 1, h, w)
    lst = [a, -a, a + 1, a - 1, -a - 1, -a + 1] + edge_accs(cs, 58)
    o = b.conv(x, 64, 64, h, w, 1, 1, cs=None, triple=(s1, P2(-8), P2(-8)), wr=127, act="silu", edges=lst, need=("clamps", "wide"),
               w_scale=s_w, bias_range=2000)
    s = b.site(name, [o], seed=seed, lut2=False)
    s.quirk = a
    return s


def rows_slow_site(name="rows_slow", seed=62):
    """20 x 20, 128 -> 128, 3 x 3 with the scale the half-step table cannot serve and NO table behind it: the requant_safe branch of the rows
    kernel (variant 20), which declines a layer that has a table without its half-step form"""
    s_in, s_w, s1 = 0.04, 1.0 / 64, 0.4
    cs = combined_scale(s_in, s_w, s1)
    b = Builder(seed)
    x = b.input(20, 20, 128, scale=s_in)
    b.zero_under(_corner_and_inside(20, 20), 3, 1, 20, 20)
    a = quirk_acc(cs)
    lst = [a, -a, a + 1, a - 1, -a - 1, -a + 1] + edge_accs(cs, 58)
    o = b.conv(x, 128, 128, 20, 20, 3, 1, cs=None, triple=(s1, 0, 0), wr=40, act="none", edges=lst, need=("clamps", "wide"), w_scale=s_w,
               bias_range=2000)
    s = b.site(name, [o], seed=seed, tuning=(("variant", 20, 0),), min_rows=1)
    s.quirk = a
    return s


def all_sites():
    """name -> constructor; built lazily (some take a moment)"""
    S = {}

    def reg(fn, name, *a, **kw):
        S[name] = lambda: fn(name, *a, **kw)

    reg(plain_site, "k1_16x16", 16, 16, 64, 64, lut2=True)
    reg(plain_site, "k1_5x5", 5, 5, 64, 64, seed=2, lut2=True)
    reg(plain_site, "k3_s1", 16, 16, 64, 64, k=3, cs=P2(-5), wr=2, seed=3, lut2=True)
    reg(plain_site, "k3_s2", 32, 32, 64, 64, k=3, stride=2, cs=P2(-5), wr=2, seed=4, lut2=True)
    reg(plain_site, "k3_c128", 16, 16, 128, 128, k=3, cs=P2(-5), wr=1, seed=5, lut2=True)
    reg(plain_site, "rows", 20, 20, 128, 128, k=3, cs=P2(-5), wr=1, seed=6, lut2=True, tuning=(("variant", 20, 0),), min_rows=1)
    S["rows_slow"] = rows_slow_site
    reg(plain_site, "stem", 32, 32, 3, 32, k=6, stride=2, cs=P2(-4), wr=4, seed=7, lut2=True)
    reg(plain_site, "patch_c16", 32, 32, 16, 64, k=3, stride=2, cs=P2(-4), wr=2, seed=8, lut2=True)
    reg(plain_site, "oc255", 16, 16, 64, 255, cs=P2(-4), seed=9, lut2=True)
    reg(plain_site, "nchw", 16, 16, 64, 64, cs=P2(-4), seed=10, nchw=True)
    S["slice"] = slice_site
    S["slow_table"] = slow_table_site
    reg(plain_site, "unsafe_ties", 16, 16, 64, 64, cs=1.5, in_scale=1.0, wr=3, small=3, seed=12,
        need=("ties", "clamps", "wide"), safe=0)
    reg(plain_site, "unsafe_overflow", 16, 16, 64, 64, cs=4.0, in_scale=1.0, wr=1, small=3, seed=13,
        need=("clamps", "wide", "overflow"), safe=0)
    reg(plain_site, "relu", 16, 16, 64, 64, act="relu", seed=14, need=("relu", "clamps", "wide"), lut2=True)
    reg(plain_site, "no_table", 16, 16, 64, 64, act="none", seed=15)
    for c in (32, 128):
        for order in (0, 1):
            reg(add_site, "add_c%d_o%d_lut" % (c, order), c, 16, 16, order, True, P2(-4), 70 + c + order, ("ties",))
            reg(add_site, "add_c%d_o%d_plain" % (c, order), c, 16, 16, order, False, P2(-4), 80 + c + order, ("ties",))
        reg(add_site, "add_c%d_sat" % c, c, 16, 16, 0, True, P2(-5), 90 + c, ("clamps",))
        reg(add3_site, "add3_c%d" % c, c, 16, 16, 100 + c)
    reg(add3_site, "add3_c32_sat", 32, 16, 16, 133, s_out=P2(-5))
    reg(split_site, "split_s1", 32, 16, 16, 1, 21)
    reg(split_site, "split_s2", 16, 16, 16, 2, 22)
    reg(split_site, "split_chain1", 32, 16, 16, 1, 23, chain=1)
    reg(split_site, "split_chain2", 32, 16, 16, 2, 24, chain=2)
    S["pair"] = pair_site
    reg(both_site, "both", 128, 12, 12, 31)
    reg(both_site, "both_chain1_elided", 128, 12, 12, 32, tail="chain", side=1)
    reg(both_site, "both_chain2_kept", 64, 12, 12, 33, tail="chain_out", side=2)
    reg(both_site, "both_cat", 128, 12, 12, 34, cat=True)
    reg(c3_site, "post_add", 32, 16, 16, True, 51)
    reg(c3_site, "post", 64, 16, 16, False, 52)
    reg(c3_site, "pre_add", 32, 16, 16, True, 53, fusion=2)
    reg(c3_site, "pre", 32, 16, 16, False, 54, fusion=2)
    return S


# ------------------------------------------------------------------------------------------------ the numpy model
def _conv_params(layer):
    kh, kw, sh, sw, _, _, pad = struct.unpack_from("<7I", layer["params"], 0)
    act, wid, bid = struct.unpack_from("<3I", layer["params"], 48)
    return kh, kw, sh, sw, pad, act, wid, bid


def _blob(d, hdr, t, dtype):
    return np.frombuffer(d, dtype=dtype, count=t["size"] // np.dtype(dtype).itemsize, offset=hdr["woff"] + t["off"])


def conv_acc(d, parsed, li, x_bytes):
    """int64 accumulators [oh, ow, oc] of CONV2D layer li over the input bytes x_bytes (NHWC, or NCHW where the input is tagged so)"""
    hdr, tensors, layers = parsed
    L = layers[li]
    kh, kw, sh, sw, pad, act, wid, bid = _conv_params(L)
    ti, to = tensors[L["ins"][0]], tensors[L["outs"][0]]
    nchw = ti["fmt"] != marsfile.NHWC
    if nchw:
        ic, ih, iw = ti["shape"][1:4]
        oc, oh, ow = to["shape"][1:4]
        x = np.frombuffer(x_bytes, dtype=np.int8)[:ic * ih * iw].reshape(ic, ih, iw).transpose(1, 2, 0).astype(np.int64)
        wt = _blob(d, hdr, tensors[wid], np.int8).reshape(oc, ic, kh, kw).transpose(0, 2, 3, 1).astype(np.int64)
    else:
        ih, iw, ic = ti["shape"][1:4]
        oh, ow, oc = to["shape"][1:4]
        x = np.frombuffer(x_bytes, dtype=np.int8)[:ih * iw * ic].reshape(ih, iw, ic).astype(np.int64)
        wt = _blob(d, hdr, tensors[wid], np.int8).reshape(oc, kh, kw, ic).astype(np.int64)
    pt = pl = 0
    if pad == marsfile.PAD_SAME:
        pt, pl = ((oh - 1) * sh + kh - ih) // 2, ((ow - 1) * sw + kw - iw) // 2
    acc = np.zeros((oh, ow, oc), dtype=np.int64)
    if bid != marsfile.NONE:
        acc += _blob(d, hdr, tensors[bid], np.int32).astype(np.int64)[None, None, :]
    if kh == 1 and kw == 1 and sh == 1 and sw == 1 and pt == 0 and pl == 0:
        acc += (x.reshape(-1, ic) @ wt.reshape(oc, ic).T).reshape(oh, ow, oc)
    else:
        xp = np.zeros((ih + 2 * kh + sh * oh, iw + 2 * kw + sw * ow, ic), dtype=np.int64)  # zeros wherever a tap leaves the image
        oy0, ox0 = kh, kw
        xp[oy0:oy0 + ih, ox0:ox0 + iw] = x
        for ky in range(kh):
            for kx in range(kw):
                y0, x0 = oy0 - pt + ky, ox0 - pl + kx
                tap = xp[y0:y0 + sh * oh:sh, x0:x0 + sw * ow:sw]
                acc += (tap.reshape(-1, ic) @ wt[:, ky, kx, :].T).reshape(oh, ow, oc)
    assert np.abs(acc).max() < 2 ** 31, "the reference's int32 sum would wrap"
    cs = combined_scale(ti["scale"], tensors[wid]["scale"], to["scale"])
    return acc, cs, act, nchw


def requant(acc, cs, relu=False):
    """the reference's float32 steps: trunc(p + copysign(0.5, p)) with x86's out-of-range result, clamped; -> (q, p)"""
    p = acc.astype(np.float32) * f32(cs)
    biased = p + np.where(p >= 0, f32(0.5), f32(-0.5)).astype(np.float32)
    ok = (biased >= f32(-2147483648.0)) & (biased < f32(2147483648.0))
    r = np.where(ok, np.trunc(np.where(ok, biased, 0)).astype(np.int64), -(1 << 31))
    q = np.clip(r, -128, 127)
    if relu:
        q = np.maximum(q, 0)
    return q.astype(np.int8), p, r


def add_model(a, b, sa, sb, so):
    """the reference's int8 Add: sat8(trunc((a * sa + b * sb) * (1 / so) + 0.5)); -> (bytes, t)"""
    inv = f32(1.0) / f32(so)
    y = a.astype(np.float32) * f32(sa) + b.astype(np.float32) * f32(sb)
    t = (y * inv).astype(np.float32)
    r = np.trunc(t + f32(0.5)).astype(np.int64)
    return np.clip(r, -128, 127).astype(np.int8), t


def table_after(orc, parsed, li):
    """the 256-entry map (index q + 128) that follows conv layer li before its result is stored -- the SiLU chain or an activation layer evaluated
    by the checker over all 256 inputs -- with the tensor that receives it; (None, conv-out tensor) when nothing follows"""
    hdr, tensors, layers = parsed
    t1 = layers[li]["outs"][0]
    nxt = [l for l in layers[li + 1:li + 3]]
    G = marsfile.Graph()
    x = G.tensor([1, 1, 1, 256], scale=tensors[t1]["scale"])
    if len(nxt) == 2 and nxt[0]["type"] == marsfile.SIGMOID and nxt[0]["ins"][0] == t1 and nxt[1]["type"] == marsfile.MUL \
            and set(nxt[1]["ins"]) == {t1, nxt[0]["outs"][0]}:
        g = G.tensor([1, 1, 1, 256], scale=tensors[nxt[0]["outs"][0]]["scale"])
        o = G.tensor([1, 1, 1, 256], scale=tensors[nxt[1]["outs"][0]]["scale"])
        G.layer(marsfile.SIGMOID, [x], [g])
        G.layer(marsfile.MUL, [x, g] if nxt[1]["ins"][0] == t1 else [g, x], [o])
        t_out = nxt[1]["outs"][0]
    elif nxt and nxt[0]["type"] == marsfile.RELU and nxt[0]["ins"][0] == t1:
        o = G.tensor([1, 1, 1, 256], scale=tensors[nxt[0]["outs"][0]]["scale"])
        G.layer(marsfile.RELU, [x], [o])
        t_out = nxt[0]["outs"][0]
    else:
        return None, t1
    g = orc.Graph(G.serialise([x], [o]))
    g.set_input(0, np.arange(-128, 128).astype(np.int8).tobytes())
    assert g.run() == 0
    return g.tensor(o).view(np.int8).copy(), t_out


def coverage(p, r, q, tab, relu=False):
    """counts of one conv stage from the numpy accumulators and the checker's table alone.  A tie (frac |p| == 0.5) is WITNESSED when the table
    maps q and q - sign(p) -- what rounding toward zero would give -- to different bytes."""
    ap = np.abs(p)
    tie = (ap - np.floor(ap)) == f32(0.5)
    inr = np.abs(r) <= 128
    T = (lambda v: tab[np.clip(v, -128, 127) + 128]) if tab is not None else (lambda v: np.clip(v, -128, 127))
    lo = 0 if relu else -128
    qq = q.astype(np.int64)
    other = np.maximum(np.clip(qq - np.sign(p).astype(np.int64), -128, 127), lo)
    wit = tie & inr & (T(qq) != T(other))
    return dict(ties_pos=int((wit & (p > 0)).sum()), ties_neg=int((wit & (p < 0)).sum()),
                raw_ties_neg=int((tie & (p < 0) & inr).sum()),
                clamp_hi=int((r > 127).sum()), clamp_lo=int((r < -128).sum()), wide=int((np.abs(p.astype(np.float64) * 2) >= 256).sum()),
                small_neg=int(((p < 0) & (p > -1)).sum()), overflow=int((r == -(1 << 31)).sum()), n=int(p.size))


def evaluate(orc, site):
    """run the checker on every frame, restate every stage in numpy and compare, count the coverage.
    -> (per frame {tensor: bytes} of every activation, per stage summed counts)"""
    parsed = marsfile.parse(site.d)
    hdr, tensors, layers = parsed
    acts = [i for i, t in enumerate(tensors) if t["size"] == 0]
    per_frame = []
    for x in site.frames:
        g = orc.Graph(site.d)
        g.set_input(0, x.tobytes())
        assert g.run() == 0
        per_frame.append({ti: g.tensor(ti) for ti in acts})
        g.close()
    cov = []
    for st in site.stages:
        L = layers[st["layer"]]
        tot = {}
        if L["type"] == marsfile.CONV2D:
            tab, t_out = table_after(orc, parsed, st["layer"])
            relu_layer = tab is not None and layers[st["layer"] + 1]["type"] == marsfile.RELU
            for f, T in enumerate(per_frame):
                acc, cs, act, nchw = conv_acc(site.d, parsed, st["layer"], T[L["ins"][0]].tobytes())
                q, p, r = requant(acc, cs, relu=act == 1)
                lay = (lambda v: v.transpose(2, 0, 1)) if nchw else (lambda v: v)
                want = T[L["outs"][0]].view(np.int8)
                assert np.array_equal(lay(q).reshape(-1), want), (site.name, st["layer"], f, int((lay(q).reshape(-1) != want).sum()))
                if tab is not None:
                    assert np.array_equal(lay(tab[q.astype(np.int64) + 128]).reshape(-1), T[t_out].view(np.int8)), (site.name, st["layer"], f)
                for ch, a in (st["edges"] or {}).items():
                    assert (acc[:, :, ch] == a).any(), "%s: edge accumulator %d (channel %d) is nowhere in frame %d" % (site.name, a, ch, f)
                for k, v in coverage(p, r, q, tab, relu=relu_layer or act == 1).items():
                    tot[k] = tot.get(k, 0) + v
            tot["cs"] = float(cs)
        else:
            ta, tb, to = (tensors[i] for i in (L["ins"][0], L["ins"][1], L["outs"][0]))
            for f, T in enumerate(per_frame):
                a, b = T[L["ins"][0]].view(np.int8), T[L["ins"][1]].view(np.int8)
                out, t = add_model(a, b, ta["scale"], tb["scale"], to["scale"])
                assert np.array_equal(out, T[L["outs"][0]].view(np.int8)), (site.name, st["layer"], f)
                tie = (t - np.floor(t)) == f32(0.5)
                r = np.trunc(t + f32(0.5))
                c = dict(ties_pos=int((tie & (t > 0) & (t < 127)).sum()), ties_neg=int((tie & (t < 0) & (t > -128)).sum()),
                         clamp_hi=int((r > 127).sum()), clamp_lo=int((r < -128).sum()), n=int(t.size))
                for k, v in c.items():
                    tot[k] = tot.get(k, 0) + v
        cov.append(tot)
    return per_frame, cov


def check_needs(site, cov):
    """the coverage conditions of every stage (asserts)"""
    for st, c in zip(site.stages, cov):
        need, tag = st["need"], (site.name, st["layer"], c)
        if "ties" in need:
            assert c["ties_pos"] >= 32 and c["ties_neg"] >= 32, tag
        if "relu" in need:  # behind a ReLU a negative tie rounds to 0 either way: positive ties witnessed (q = 1 against 0), negative ones present
            assert c["ties_pos"] >= 32 and c["raw_ties_neg"] >= 32 and c["small_neg"] >= 32, tag
        if "clamps" in need:
            assert c["clamp_hi"] >= 16 and c["clamp_lo"] >= 16, tag
        if "wide" in need:
            assert c["wide"] >= 8, tag
        if "overflow" in need:
            assert c["overflow"] >= 3, tag
