"""Operands for the float32 convolutions at the edges the random [-1, 1] cases never reach, and what each f32_mfma mode must give for
them -- host only, shared by tests/test_f32_edges_cpu.py (the generators and expectations against the CPU oracle) and
tests/test_gpu_f32_edges.py (the kernels against the expectations).  DESIGN.md "Float operand edges" has the reasoning.

PIECE MODEL.  Modes 3 and 4 cut every float into bf16 pieces by round-to-nearest-even, hi = bf16(x), mid = bf16(x - hi), lo = x - hi - mid
(both subtractions exact), and sum a product from piece products, each exact in float32:
    mode 3 (two pieces)    hi*hi + hi*mid + mid*hi
    mode 4 (three pieces)  those + mid*mid + hi*lo + lo*hi
    modes 0 and 2          the full product (float32 FMA chains: the reference's order / the f32 matrix cores)
An INPUT value bf16 would round to +-inf (|x| >= 2^128 - 2^119, or an infinity) keeps a finite hi piece and its LAST piece is the infinity
(two pieces: hi saturates at the largest bf16; three: hi = mid = 0): the last piece of an input meets only the weights' hi piece, so the sum
sees inf * w once.  (Weights that large are out of scope: the host packers keep hi = inf.)  A producer that writes records (hi | mid of its
result) rounds its output to two pieces; two_piece() does the same.

EXACT CLASSES.  Operands are integers (times a power of two), chosen so that, per output element, sum over the kept piece pairs of
|piece_x| |piece_w| + |bias| (+ |residual|) < 2^24: every piece product and every partial sum IN ANY ORDER is then an integer below 2^24 in
the common unit, i.e. exact in float32, and the result must equal the integer sum of the kept piece products bit for bit whatever the
summation order, tile shape or MFMA internals.  expected() asserts the condition for every element.
    A   x in [-255, 255], w in [-15, 15]            one piece each: every mode exact -- addressing, taps, halos, K padding
    B   x in [-8191, 8191], w in {+-1, +-2}         the input's mid plane is read and meets the right weight plane
    B'  B with the roles swapped                    the packed weights' mid plane
    C   |x| up to 2^20, w in {0, +-1}, <= 8 non-zeros per output channel    mode 4 = the full sum (lo planes); mode 3 = the sum over
                                                    two-piece-rounded inputs: the expectation differs between the modes
Each class also runs as (x * 2^-s, w * 2^s), s in SCALES: power-of-two scaling commutes with every rounding while all pieces stay normal,
so the expected BITS are those of s = 0.  Operands small enough for a piece to be a bf16 subnormal are out of scope.
"""
import numpy as np

EXACT_CLASSES = ("A", "B", "Bp", "C")
SCALES = (0, 64, -64)
LIMIT = float(1 << 24)
FLT_MAX = np.float32(3.4028234663852886e38)
BF16_MAX = np.float32(2.0 ** 128 - 2.0 ** 120)  # the largest finite bf16
SPECIALS = (("+inf", np.float32(np.inf)), ("-inf", np.float32(-np.inf)), ("nan", np.float32(np.nan)), ("+fltmax", FLT_MAX), ("-fltmax", -FLT_MAX))
KEPT = {3: ((0, 0), (0, 1), (1, 0)), 4: ((0, 0), (0, 1), (1, 0), (1, 1), (0, 2), (2, 0)), 0: None, 2: None}  # (input piece, weight piece); None: full product


# ---------------------------------------------------------------------------------------------------------------- pieces
def bf16_rne(x):
    """float32 -> the nearest bf16 value (ties to even) as float32; a NaN stays one, |x| >= 2^128 - 2^119 gives inf"""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000)
    nan = (b & 0x7FFFFFFF) > 0x7F800000
    r = np.where(nan, (b | 0x400000) & 0xFFFF0000, r)
    return r.astype(np.uint32).view(np.float32).reshape(np.shape(x))


def pieces(x, npl=3):
    """x -> [hi, mid, lo][:npl] (float32 arrays).  A value bf16 would round to +-inf keeps a finite hi and the LAST piece is the infinity: with two
    pieces hi saturates at the largest bf16 and the residual is +-inf by itself, with three hi = mid = 0 and lo = bf16(x).  A NaN: some piece is NaN."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        fin = np.abs(x) < np.float32(2.0 ** 128 - 2.0 ** 119)  # (False for a NaN)
        if npl == 2:
            hi = bf16_rne(np.where(np.isnan(x), x, np.clip(x, -BF16_MAX, BF16_MAX)))
            return [hi, bf16_rne((x - hi).astype(np.float32))]
        hi = bf16_rne(np.where(fin, x, np.float32(0)))
        r1 = np.where(fin, x - hi, np.float32(0)).astype(np.float32)
        mid = bf16_rne(r1)
        lo = np.where(fin, r1 - mid, bf16_rne(x)).astype(np.float32)
    return [hi, mid, lo]


def two_piece(x):
    """what a record (hi | mid) holds of x"""
    hi, mid = pieces(x, 2)
    with np.errstate(invalid="ignore", over="ignore"):
        return (hi + mid).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- geometry
class Geom:
    """one convolution: [ic][h][w] -> [oc][oh][ow], square kernel k, stride st, pad "same" (top = left = total // 2, as the planner derives
    it from the graph) or "valid" """

    def __init__(self, h, w, ic, oc, k, st, pad="same"):
        self.h, self.w, self.ic, self.oc, self.k, self.st = h, w, ic, oc, k, st
        if pad == "same":
            self.oh, self.ow = (h + st - 1) // st, (w + st - 1) // st
            self.pt = max(0, (self.oh - 1) * st + k - h) // 2
            self.pl = max(0, (self.ow - 1) * st + k - w) // 2
        else:
            self.oh, self.ow = (h - k) // st + 1, (w - k) // st + 1
            self.pt = self.pl = 0
        self.K = ic * k * k

    def cols(self, x):
        """[ic * h * w] -> float64 [oh * ow][K], k = (ic, ky, kx) as OIHW weights flatten; zeros outside the image"""
        g = self
        x = np.asarray(x, dtype=np.float64).reshape(g.ic, g.h, g.w)
        pb = max(0, (g.oh - 1) * g.st + g.k - g.h - g.pt)
        pr = max(0, (g.ow - 1) * g.st + g.k - g.w - g.pl)
        xp = np.pad(x, ((0, 0), (g.pt, pb), (g.pl, pr)))
        win = np.lib.stride_tricks.sliding_window_view(xp, (g.k, g.k), axis=(1, 2))[:, ::g.st, ::g.st][:, :g.oh, :g.ow]  # [ic][oh][ow][k][k]
        return np.ascontiguousarray(win.transpose(1, 2, 0, 3, 4)).reshape(g.oh * g.ow, g.K)

    def conv(self, x, w):
        """float64 [oc][oh * ow] = w (x) x, no bias"""
        return np.asarray(w, dtype=np.float64).reshape(self.oc, self.K) @ self.cols(x).T


def split_geom(shape):
    h, w, ic, oc, k, st, pad, B, silu = shape
    return Geom(h, w, ic, oc, k, st, pad)


def patch_geom(shape):
    h, w, ic, oc, k, st, B, silu, add = shape
    return Geom(h, w, ic, oc, k, st)


def stem_geom(shape):
    h, w, ic, oc, k, B, silu = shape
    return Geom(h, w, ic, oc, k, 2)


GEOMS = {"split": split_geom, "patch": patch_geom, "stem": stem_geom}


# ---------------------------------------------------------------------------------------------------------------- exact classes
def exact_operands(cls, g, rng, nframes=2, nonzero_w=False):
    """-> (frames: list of float32 [ic * h * w], weights float32 [oc][ic][k][k], bias float32 [oc]) of class cls, unscaled (s = 0)"""
    n, wshape = g.ic * g.h * g.w, (g.oc, g.ic, g.k, g.k)
    big = lambda size: rng.integers(-8191, 8192, size)  # noqa: E731
    small = lambda size: rng.choice(np.array([-2, -1, 1, 2]), size)  # noqa: E731
    if cls == "A":
        xs = [rng.integers(-255, 256, n) for _ in range(nframes)]
        w = rng.integers(-15, 16, wshape)
        if nonzero_w:
            w = np.where(w == 0, 7, w)
    elif cls == "B":
        xs, w = [big(n) for _ in range(nframes)], small(wshape)
    elif cls == "Bp":
        xs, w = [small(n) for _ in range(nframes)], big(wshape)
    elif cls == "C":
        xs = [rng.integers(-(1 << 20), (1 << 20) + 1, n) for _ in range(nframes)]
        w = np.zeros((g.oc, g.K), dtype=np.int64)
        for oc in range(g.oc):
            nz = rng.choice(g.K, size=min(7, g.K), replace=False)
            w[oc, nz] = rng.choice(np.array([-1, 1]), nz.size)
        w = w.reshape(wshape)
    else:
        raise ValueError(cls)
    bias = rng.integers(-1000, 1001, g.oc)
    return [q.astype(np.float32) for q in xs], w.astype(np.float32), bias.astype(np.float32)


def scaled(xs, w, s):
    """(x * 2^-s, w * 2^s): the same products, magnitudes 2^s away from 1"""
    return [np.ldexp(q, -s).astype(np.float32) for q in xs], np.ldexp(w, s).astype(np.float32)


def expected(g, x, w, bias, mode, resid=None):
    """the float32 [oc][oh * ow] a convolution in `mode` must give for one frame of an exact class (x, w may be scaled), by the piece model in
    float64 (exact: every term and partial sum is an integer below 2^53); asserts the class's condition, sum |piece products| + |bias| (+
    |residual|) < 2^24 for every element"""
    kept = KEPT[mode]
    b = np.asarray(bias, dtype=np.float64).reshape(g.oc, 1)
    r = 0.0 if resid is None else np.asarray(resid, dtype=np.float64).reshape(g.oc, -1)
    if kept is None:
        groups = [(np.asarray(x, dtype=np.float64), np.asarray(w, dtype=np.float64))]
    else:
        px, pw = pieces(x, 3), pieces(w, 3)
        groups = []
        for i in sorted({i for i, _ in kept}):  # input piece i times the sum of the weight pieces it is kept with (exact: they do not overlap)
            groups.append((px[i].astype(np.float64), sum(pw[j].astype(np.float64) for ii, j in kept if ii == i)))
    tot = sum(g.conv(a, c) for a, c in groups) + b + r
    if kept is None:
        mass = g.conv(np.abs(groups[0][0]), np.abs(groups[0][1]))
    else:
        mass = sum(g.conv(np.abs(px[i].astype(np.float64)), np.abs(pw[j].astype(np.float64))) for i, j in kept)
    mass = mass + np.abs(b) + np.abs(r)
    assert mass.max() < LIMIT, "not an exact class: sum of |piece products| reaches %g" % mass.max()
    out = tot.astype(np.float32)
    assert (out.astype(np.float64) == tot).all()
    return out


def same_floats(got, want):
    """element-wise: the same bits, or both NaN"""
    a, b = np.ascontiguousarray(got).view(np.float32).reshape(-1), np.ascontiguousarray(want).view(np.float32).reshape(-1)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


# ---------------------------------------------------------------------------------------------------------------- non-finite classes
def positions(g, nframes, f=0):
    """name -> (frame, channel, y, x) of the one special value: every place a gather, a halo, a frame boundary or a padded tap could go wrong"""
    h, w, ic = g.h, g.w, g.ic
    yo, xo = (h // 2) | 1, (w // 2) | 1  # odd row / column: under stride 2 (even pad) the LAST real tap of the window left of / above it ends one before
    pos = {
        "interior": (f, 0, h // 2, w // 2),
        "top-left": (f, 0, 0, 0), "top-right": (f, 0, 0, w - 1), "bottom-left": (f, 0, h - 1, 0), "bottom-right": (f, 0, h - 1, w - 1),
        "frame-last": (f, ic - 1, h - 1, w - 1),
        "last-channel": (f, ic - 1, h // 2, w // 2),
    }
    if nframes > f + 1:
        pos["next-frame-first"] = (f + 1, 0, 0, 0)
    if g.st == 2:  # the pixel right of (below) a window's last real tap: the padded tap of the stride-2 gathers sits on it with weight 0
        pos["right-of-window"] = (f, 0, h // 2 & ~1, xo)
        pos["below-window"] = (f, 0, yo, w // 2 & ~1)
    return pos


POSITION_NAMES = ("interior", "top-left", "top-right", "bottom-left", "bottom-right", "frame-last", "last-channel", "next-frame-first",
                  "right-of-window", "below-window")


def poisoned(g, clean, w, pos_cyx, special, mode):
    """clean = this mode's expectation for the frame without the special; -> with it at (channel, y, x): outputs whose TRUE window holds it are NaN
    (NaN) or sign(w) * inf (+-inf; +-FLT_MAX in modes 3 / 4, whose hi piece rounds to inf), in modes 0 / 2 FLT_MAX gives float32(FLT_MAX * w)
    (every other term is below its last bit); every other output keeps its bits"""
    c, y, x = pos_cyx
    ind = np.zeros((g.ic, g.h, g.w))
    ind[c, y, x] = 1.0
    wtap = g.conv(ind, w)  # the weight the special meets in each output's window, 0 where the window does not hold it
    assert (np.asarray(w) != 0).all()
    out = clean.copy()
    hit = wtap != 0
    with np.errstate(over="ignore", invalid="ignore"):
        if np.isnan(special):
            val = np.full(wtap.shape, np.nan, dtype=np.float32)
        elif np.isinf(special) or mode in (3, 4):
            val = (np.sign(wtap) * np.sign(special) * np.inf).astype(np.float32)
        else:
            val = np.float32(special) * wtap.astype(np.float32)
    out[hit] = val[hit]
    return out, hit


def with_specials(g, x, w, clean_of):
    """the general form of poisoned(): x may hold any number of +-inf / NaN.  An output is NaN where its window holds a NaN, an infinity on a zero
    weight or infinite terms of both signs; +-inf where it holds infinite terms of one sign; else clean_of(x with the specials zeroed)"""
    x = np.asarray(x, dtype=np.float32)
    w = np.asarray(w, dtype=np.float64)
    pinf, ninf, nan = np.isposinf(x).astype(float), np.isneginf(x).astype(float), np.isnan(x).astype(float)
    up = g.conv(pinf, w > 0) + g.conv(ninf, w < 0)
    down = g.conv(pinf, w < 0) + g.conv(ninf, w > 0)
    bad = g.conv(nan, np.ones_like(w)) + g.conv(pinf + ninf, w == 0)
    out = clean_of(np.where(np.isfinite(x), x, np.float32(0))).copy()
    out[up > 0] = np.inf
    out[down > 0] = -np.inf
    out[(bad > 0) | ((up > 0) & (down > 0))] = np.nan
    return out, (up > 0) | (down > 0) | (bad > 0)


# ---------------------------------------------------------------------------------------------------------------- bound class
def bound_operands(g, rng, nframes=2):
    """magnitudes log-uniform over 2^-20 .. 2^20, random signs, dense weights"""
    def draw(size):
        return (np.exp2(rng.uniform(-20, 20, size)) * rng.choice(np.array([-1.0, 1.0]), size)).astype(np.float32)
    return [draw(g.ic * g.h * g.w) for _ in range(nframes)], draw((g.oc, g.ic, g.k, g.k)), draw(g.oc)


def c_mode(mode, K):
    """worst-case |got - ref64| / A: what the kept products drop (a two-piece residual <= 2^-17 |x| on either side, the dropped mid * mid <=
    2^-16 |x w|; with three pieces 2^-22) + one ulp (not half: the MFMA's internal rounding is not specified) per accumulated term"""
    return {3: 2.0 ** -15 + (3 * K + 2) * 2.0 ** -23, 4: 2.0 ** -22 + (6 * K + 2) * 2.0 ** -23, 2: (K + 2) * 2.0 ** -23, 0: (K + 2) * 2.0 ** -24}[mode]


def ref64(g, x, w, bias):
    """-> (float64 convolution of the float32 operands, A = sum |x| |w| + |bias|), each [oc][oh * ow]"""
    b = np.asarray(bias, dtype=np.float64).reshape(g.oc, 1)
    x, w = np.asarray(x, dtype=np.float64), np.asarray(w, dtype=np.float64)
    return g.conv(x, w) + b, g.conv(np.abs(x), np.abs(w)) + np.abs(b)


# ---------------------------------------------------------------------------------------------------------------- SiLU
def silu_grid():
    """every NORMAL bf16 value with |v| <= 104 (2^-126 upward), and +-0 (float32).  bf16 subnormals are left out: the pre-activation reaches the
    SiLU through the matrix cores as a bf16 piece, and subnormal pieces are out of scope (module docstring)"""
    bits = np.arange(0x10000, dtype=np.uint32) << 16
    v = bits.view(np.float32)
    a = np.abs(v)
    keep = (a == 0) | ((a >= 2.0 ** -126) & (a <= 104))
    return v[keep].copy()


def silu64(v):
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(over="ignore"):
        return v / (1.0 + np.exp(-v))


def silu_fast_bound(v):
    """|got - silu64(v)| allowed for the three-product kernels' SiLU (v_exp_f32 of v * -1.4427, v_rcp_f32), at any v: relative 2^-23 (|v| + 4) -- the
    argument's rounding, scaled by |v| through the exponential, + 1 ulp each for exp and rcp + two more roundings -- and 2^-120 absolute:
    below v = -88.7 the exponential overflows and the kernel returns -0 where the true value is about -2e-37"""
    v = np.asarray(v, dtype=np.float64)
    return 2.0 ** -23 * (np.abs(v) + 4) * np.abs(silu64(v)) + 2.0 ** -120


def one_hot_weights(g):
    """out channel o reads input channel o % ic at tap (o // ic) % (k * k), weight 1: the pre-activation IS one input value"""
    w = np.zeros((g.oc, g.ic, g.k * g.k), dtype=np.float32)
    centre = (g.k // 2) * g.k + g.k // 2
    for o in range(g.oc):
        w[o, o % g.ic, (centre + o // g.ic) % (g.k * g.k)] = 1.0
    return w.reshape(g.oc, g.ic, g.k, g.k)
