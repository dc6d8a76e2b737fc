"""The element-wise and batch-norm layers restated in numpy float32, and the case tables of tests/test_elt_cpu.py and tests/test_gpu_elt.py.

One rounding per operation, in the order of the reference loops (mars_runtime.c :742-771 sigmoid, :818-835 / :885-902 int8 mul / add,
:807-816 / :874-883 the float forms, :1066-1086 ReLU / leaky, :1115-1154 batch-norm).  The float sigmoid takes expf from the host's libm
through ctypes: numpy's exp is not glibc's.  Every case builder asserts, on the CPU, that its case holds what it is there for (ties,
clamps, subnormals, operands at which a fused or reciprocal form gives another byte), so that no case can quietly stop testing anything;
the count a builder measured stands in a comment beside its case.  Nothing here needs a GPU or the oracle."""
import ctypes
import ctypes.util
import functools
from fractions import Fraction

import numpy as np

F = np.float32
I8, U8, U32 = np.int8, np.uint8, np.uint32
INT_MIN = -(1 << 31)
QUIET = dict(over="ignore", under="ignore", invalid="ignore", divide="ignore")


def f32(v):
    return np.asarray(v, dtype=F)


def bits(x):
    return np.ascontiguousarray(x, dtype=F).view(U32)


def from_bits(u):
    return np.ascontiguousarray(u, dtype=U32).view(F)


def is_subnormal(x):
    x = f32(x)
    return (x != 0) & (np.abs(x) < F(2.0 ** -126))


# ---- the arithmetic ----------------------------------------------------------------------------------------------------------------------------
def trunc_x86(v, saturating=False):
    """(int32_t)v as x86's cvttss2si gives it: NaN, v >= 2^31 and v < -2^31 -> INT_MIN.  saturating = the conversion the device has in
    hardware (NaN -> 0, clamped to the int32 range): what a kernel without trunc_x86's second line would compute"""
    v = f32(v)
    ok = (v >= F(-2147483648.0)) & (v < F(2147483648.0))  # (false for NaN)
    out = np.full(v.shape, INT_MIN, dtype=np.int64)
    out[ok] = np.trunc(v[ok]).astype(np.int64)
    if saturating:
        out[~ok & (v > 0)] = (1 << 31) - 1
        out[np.isnan(v)] = 0
    return out


def q8(t, saturating=False):
    """(int32_t)(t + 0.5f), then the clamp to [-128, 127]"""
    with np.errstate(**QUIET):
        return np.clip(trunc_x86(f32(t) + F(0.5), saturating), -128, 127).astype(I8)


def scale_or_one(s):
    """`s > 0 ? s : 1.0f`: 0, negative and NaN scales fall back to 1"""
    s = F(s)
    return s if s > 0 else F(1.0)


def inv_of(so):
    """the binaries' factor: 1.0f / (so > 0 ? so : 1.0f)"""
    with np.errstate(**QUIET):
        return F(1.0) / scale_or_one(so)


def fma32(a, b, c):
    """a * b + c rounded once (through float64: exact while the operands' exponents lie within 2^29 of each other; builders confirm the
    witnesses they keep with is_nearest)"""
    with np.errstate(**QUIET):
        return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F)


def is_nearest(r, exact):
    """r (a finite float32) is the one float32 nearest to the Fraction `exact`, with no tie"""
    r = F(r)
    lo, hi = np.nextafter(r, F(-np.inf)), np.nextafter(r, F(np.inf))
    if not (np.isfinite(lo) and np.isfinite(hi)):
        return False
    d = abs(Fraction(float(r)) - exact)
    return d < abs(Fraction(float(lo)) - exact) and d < abs(Fraction(float(hi)) - exact)


def binary_i8(is_mul, a, b, sa, sb, inv, form="plain", saturating=False):
    """int8 MUL / ADD.  form: "plain" (the reference), or what a subtly wrong kernel would compute: "fma_a" = a * sa + vb fused (add only),
    "fma_half" = y * inv + 0.5 fused, "div" = y / so in place of y * inv (so = 1 / inv is passed as inv)"""
    with np.errstate(**QUIET):
        va, vb = f32(a).astype(F) * F(sa), f32(b).astype(F) * F(sb)
        if is_mul:
            y = va * vb
        else:
            y = fma32(f32(a), F(sa), vb) if form == "fma_a" else va + vb
        if form == "div":
            return q8(y / F(inv), saturating)
        if form == "fma_half":
            return np.clip(trunc_x86(fma32(y, F(inv), F(0.5)), saturating), -128, 127).astype(I8)
        return q8(y * F(inv), saturating)


_expf = None


def expf(x):
    """the host libm's expf, element by element"""
    global _expf
    if _expf is None:
        m = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
        m.expf.restype, m.expf.argtypes = ctypes.c_float, [ctypes.c_float]
        _expf = m.expf
    x = f32(x)
    return np.array(list(map(_expf, x.reshape(-1).tolist())), dtype=F).reshape(x.shape)


def sigmoid_f32(x):
    with np.errstate(**QUIET):
        return F(1.0) / (F(1.0) + expf(-f32(x)))


def relu_f32(x, alpha, form="plain"):
    """x > 0 ? x : x * alpha: -0.0 for negative x at alpha 0, NaN for NaN.  form "max" = max(x, 0) style (x > 0 ? x : 0)"""
    x = f32(x)
    with np.errstate(**QUIET):
        return np.where(x > 0, x, F(0.0) if form == "max" else x * F(alpha)).astype(F)


def binary_f32(op, a, b):
    """op 0 add, 1 mul, 2 sub"""
    with np.errstate(**QUIET):
        return (f32(a) + f32(b), f32(a) * f32(b), f32(a) - f32(b))[op]


def sigmoid_table(in_scale, out_scale):
    """int8 sigmoid of all 256 bytes -> table[q + 128].  in_scale as it stands (negative, NaN); out_scale falls back to 1 when not > 0"""
    q = np.arange(-128, 128).astype(F)
    with np.errstate(**QUIET):
        return q8(sigmoid_f32(q * F(in_scale)) / scale_or_one(out_scale))


def relu_table(leaky):
    """ReLU and ReLU6 alike (no upper clamp); leaky: (int32_t)(q * 0.01f), then only the lower clamp"""
    q = np.arange(-128, 128)
    neg = np.maximum(trunc_x86(q.astype(F) * F(0.01)), -128) if leaky else np.zeros(256, np.int64)
    return np.where(q > 0, q, neg).astype(I8)


def unary_i8(kind, x, in_scale=1.0, out_scale=1.0):
    """kind: sigmoid / relu / relu6 / leaky on int8 bytes"""
    tab = sigmoid_table(in_scale, out_scale) if kind == "sigmoid" else relu_table(kind == "leaky")
    return tab[np.asarray(x, dtype=I8).astype(np.int32) + 128]


def _per_channel(v, n, c, hw, default):
    v = np.full(c, default, dtype=F) if v is None else f32(v)
    return np.broadcast_to(v.reshape(1, c, 1), (n, c, hw))


def bn_i8_elements(x, sc, bi, in_scale, out_scale, form="plain", saturating=False):
    """one int8 batch-norm result per element of the (broadcast) arrays x, sc, bi; the scales as the layer uses them (already > 0)"""
    with np.errstate(**QUIET):
        xf = np.asarray(x).astype(F) * F(in_scale)
        y = fma32(xf, sc, bi) if form == "fma" else xf * f32(sc) + f32(bi)
        t = y * (F(1.0) / F(out_scale)) if form == "recip" else y / F(out_scale)
    return q8(t, saturating)


def batchnorm_i8(x, n, c, hw, s, b, in_scale, out_scale, form="plain", saturating=False):
    """[n][c][hw] int8.  s / b None = 1 / 0.  Both scales fall back to 1 when not > 0; the result is y / out_scale, a true division.
    form "recip" = y * (1 / out_scale), "fma" = x * sc + bi fused"""
    x = np.asarray(x, dtype=I8).reshape(n, c, hw)
    sc, bi = _per_channel(s, n, c, hw, 1.0), _per_channel(b, n, c, hw, 0.0)
    return bn_i8_elements(x, sc, bi, scale_or_one(in_scale), scale_or_one(out_scale), form, saturating).reshape(-1)


def batchnorm_f32(x, n, c, hw, s, b, form="plain"):
    x = f32(x).reshape(n, c, hw)
    sc, bi = _per_channel(s, n, c, hw, 1.0), _per_channel(b, n, c, hw, 0.0)
    with np.errstate(**QUIET):
        return (fma32(x, sc, bi) if form == "fma" else x * sc + bi).reshape(-1)


# ---- comparing --------------------------------------------------------------------------------------------------------------------------------
def differing(got, want, dtype):
    """indices at which got differs from want.  Floats: where want is NaN only NaN-ness is compared (the rule of test_decode_odd_scales);
    every other bit, the sign of zero included, must match.  Bytes: every bit"""
    if dtype == "f32":
        g, w = np.ascontiguousarray(got).reshape(-1).view(U8).view(F), np.ascontiguousarray(want).reshape(-1).view(U8).view(F)
        assert g.shape == w.shape, (g.shape, w.shape)
        nan = np.isnan(w)
        return np.flatnonzero(np.where(nan, ~np.isnan(g), g.view(U32) != w.view(U32)))
    g, w = np.ascontiguousarray(got).reshape(-1).view(U8), np.ascontiguousarray(want).reshape(-1).view(U8)
    assert g.shape == w.shape, (g.shape, w.shape)
    return np.flatnonzero(g != w)


def assert_same(what, got, want, dtype):
    bad = differing(got, want, dtype)
    if len(bad):
        view = (lambda v: np.ascontiguousarray(v).reshape(-1).view(U8).view(U32)) if dtype == "f32" else (lambda v: np.ascontiguousarray(v).reshape(-1).view(U8))
        g, w = view(got), view(want)
        raise AssertionError("%s: %d of %d differ; first (index, got, want): %s"
                             % (what, len(bad), len(w), [(int(i), hex(int(g[i])), hex(int(w[i]))) for i in bad[:6]]))


# ---- int8 binary: all 65 536 pairs in every scale class ------------------------------------------------------------------------------------------
def all_pairs():
    """a[i] = i / 256 - 128, b[i] = i % 256 - 128"""
    v = np.arange(-128, 128, dtype=np.int32)
    return np.repeat(v, 256).astype(I8), np.tile(v, 256).astype(I8)


P2, ODD_SO = F(2.0 ** -4), F(0.02)
# class -> (add scales, mul scales) as (sa, sb, inv), and the output scale a graph gives that inv with (None: no tensor scale does)
BINARY_CLASSES = {
    "P2": (((P2, P2, F(8.0)),) * 2, F(2.0 ** -3)),
    "ODD": (((F(0.05), F(0.031), F(1.0) / ODD_SO),) * 2, ODD_SO),
    "HUGE": (((F(3e18), F(3e18), F(1.0)),) * 2, F(1.0)),
    "INF": (((F(np.inf), F(1.0), F(1.0)),) * 2, F(1.0)),
    "NAN": (((F(np.nan), F(1.0), F(1.0)),) * 2, F(1.0)),
    "INVINF": (((F(0.05), F(0.05), F(np.inf)),) * 2, F(2.0 ** -149)),  # 1 / 2^-149 overflows
    "NEGINV": (((F(0.05), F(0.05), F(-20.0)),) * 2, None),             # a negative output scale falls back to 1: launcher only
    "DENORM": (((F(2.0 ** -133), F(2.0 ** -133), F(2.0 ** 127)), (F(2.0 ** -67), F(2.0 ** -67), F(2.0 ** 127))), F(2.0 ** -127)),
    # at 2^-67 a product a b 2^-134 is subnormal only while |a b| < 256: 2 450 such results are non-zero.  At 2^-69 it is one while
    # |a b| < 4096, and 14 972 are: the class that holds the count of 10 000 for the multiply
    "DENORM_DEEP": (((F(2.0 ** -134), F(2.0 ** -134), F(2.0 ** 127)), (F(2.0 ** -69), F(2.0 ** -69), F(2.0 ** 127))), F(2.0 ** -127)),
}
BINARY_CASES = [(c, m) for c in BINARY_CLASSES for m in (0, 1)]


def binary_id(case):
    return "%s_%s" % (case[0], "mul" if case[1] else "add")


@functools.lru_cache(maxsize=None)
def binary_case(cls, is_mul):
    """-> (a, b, sa, sb, inv, want) over all pairs.  Measured (add / mul), asserted below with the issue's minimum counts:
      P2           exact ties t + 0.5 = k + 0.5: 16 256 / 2 560 positive, 16 512 / 2 560 negative   (add has 32 768 in all)
      ODD          fused a * sa + vb: 142 bytes change; fused y * inv + 0.5: 2; y / so: 54 / 12; 39 438 / 43 821 results clamp
      HUGE         32 385 / 32 513 positive overflows become -128 through INT_MIN (a saturating conversion: +127)
      DENORM       38 014 / 2 450 non-zero results from subnormal operands (add) or a subnormal product (mul)
      DENORM_DEEP  20 481 / 14 972 of them"""
    a, b = all_pairs()
    sa, sb, inv = BINARY_CLASSES[cls][0][is_mul]
    want = binary_i8(is_mul, a, b, sa, sb, inv)
    with np.errstate(**QUIET):
        va, vb = a.astype(F) * sa, b.astype(F) * sb
        y = va * vb if is_mul else va + vb
        t = y * inv
    if cls == "P2":  # everything is exact: t is a multiple of 1/2
        tie = (t * F(2)) % F(2) == 1
        assert (tie & (t > 0)).sum() >= 1000 and (tie & (t < 0)).sum() >= 1000, (cls, is_mul)
        assert is_mul or tie.sum() == 32768
        assert (want > 0).any() and (want < 0).any()
        # a tie rounds up, towards +inf, on both sides of zero (trunc(t + 0.5)): checked against the exact value
        k = np.flatnonzero(tie & (np.abs(t) < 100))
        assert np.array_equal(want[k].astype(np.float64), np.trunc(t[k].astype(np.float64) + 0.5))
    elif cls == "ODD":
        assert (want == 127).any() and (want == -128).any()
        so = BINARY_CLASSES[cls][1]
        assert (binary_i8(is_mul, a, b, sa, sb, so, form="div") != want).sum() >= 1
        if not is_mul:
            fa = np.flatnonzero(binary_i8(0, a, b, sa, sb, inv, form="fma_a") != want)
            fh = np.flatnonzero(binary_i8(0, a, b, sa, sb, inv, form="fma_half") != want)
            assert len(fa) >= 1 and len(fh) >= 1
            i = int(fa[0])  # the witness, confirmed in exact arithmetic: the fused sum is another float than the twice-rounded one
            exact = Fraction(int(a[i])) * Fraction(float(sa)) + Fraction(float(vb[i]))
            fused = fma32(a[i], sa, vb[i])
            assert is_nearest(fused, exact) and fused != y[i]
            i = int(fh[0])
            exact = Fraction(float(y[i])) * Fraction(float(inv)) + Fraction(1, 2)
            fused = fma32(y[i], inv, F(0.5))
            assert is_nearest(fused, exact) and fused != t[i] + F(0.5)
    elif cls == "HUGE":
        nz = (a.astype(np.int32) * b != 0) if is_mul else (a.astype(np.int32) + b != 0)  # the exact result is not 0 (the issue names (0, 0) alone)
        assert (want[nz] == -128).all() and (want[~nz] == 0).all()
        pos = nz & (t > 0)
        assert pos.sum() >= 1000 and (t[pos] + F(0.5) >= F(2147483648.0)).all()           # through INT_MIN, not through the upper clamp:
        assert (binary_i8(is_mul, a, b, sa, sb, inv, saturating=True)[pos] == 127).all()  # a saturating conversion gives +127 there
    elif cls in ("INF", "NAN"):
        assert (want == -128).all()  # the 0 * inf row (a = 0) included: NaN -> INT_MIN
        assert (binary_i8(is_mul, a, b, sa, sb, inv, saturating=True) != want).any()
    elif cls in ("DENORM", "DENORM_DEEP"):
        sub = (is_subnormal(y) if is_mul else is_subnormal(va) | is_subnormal(vb))
        assert ((want != 0) & sub).sum() >= (2000 if (cls, is_mul) == ("DENORM", 1) else 10000), ((want != 0) & sub).sum()
        assert not binary_i8(is_mul, a, b, F(0), F(0), inv).any()  # what flushed operands give: all zero
    return a, b, sa, sb, inv, want


# output scales the host turns into inv: 0, negative and NaN -> 1.0; 2^-127 -> 2^127, finite
HOST_OUT_SCALES = {"so_zero": F(0.0), "so_neg": F(-0.02), "so_nan": F(np.nan), "so_denorm": F(2.0 ** -127)}


# ---- int8 unary: all 256 bytes, every kind, a set of (in_scale, out_scale) -----------------------------------------------------------------------
UNARY_SCALES = {
    "usual": (F(0.05), F(1 / 127.0)), "p2": (F(2.0 ** -4), F(2.0 ** -7)), "wide": (F(0.31), F(0.0123)),
    "in_neg": (F(-0.05), F(1 / 127.0)), "in_nan": (F(np.nan), F(1 / 127.0)), "in_inf": (F(np.inf), F(1 / 127.0)),
    "out_zero": (F(0.05), F(0.0)), "out_neg": (F(0.05), F(-1 / 127.0)), "out_nan": (F(0.05), F(np.nan)), "out_denorm": (F(0.05), F(2.0 ** -127)),
}
UNARY_CASES = [("sigmoid", s) for s in UNARY_SCALES] + [(k, s) for k in ("relu", "relu6", "leaky") for s in ("usual", "out_neg")]


def unary_bytes(frame):
    """all 256 bytes, each twice, in an order of its own per frame"""
    return np.random.default_rng(900 + frame).permutation(np.tile(np.arange(-128, 128), 2)).astype(I8)


def check_unary_tables():
    """what the tables are there for: measured 107 distinct sigmoid bytes at "usual", 94 at "p2"; the fallbacks to 1.0 give 0 / 1 only"""
    assert len(set(sigmoid_table(*UNARY_SCALES["usual"]).tolist())) >= 100 and len(set(sigmoid_table(*UNARY_SCALES["p2"]).tolist())) >= 90
    for k in ("out_zero", "out_neg", "out_nan"):
        assert set(sigmoid_table(*UNARY_SCALES[k]).tolist()) == {0, 1}
    assert (sigmoid_table(*UNARY_SCALES["out_denorm"]) == -128).all()     # y / 2^-127 >= 2^31 -> INT_MIN
    assert (sigmoid_table(*UNARY_SCALES["in_nan"]) == -128).all()
    assert sigmoid_table(*UNARY_SCALES["in_neg"])[0] > sigmoid_table(*UNARY_SCALES["in_neg"])[255]
    lk = relu_table(True)
    assert lk[0] == -1 and lk[28] == -1 and lk[29] == 0 and lk[128] == 0 and lk[255] == 127  # -128 .. -100 -> -1
    assert relu_table(False)[127] == 0 and relu_table(False)[200] == 72


# ---- int8 batch-norm -----------------------------------------------------------------------------------------------------------------------------
BN_N, BN_HW = 2, 256
SEARCH_CHANNELS = 65536
SPECIAL_SC_BI = [(np.nan, 0.25), (1.5, np.inf), (1.5, -np.inf), (3e30, 0.0), (-3e30, 1.0), (2.0 ** -140, 0.5), (2.0 ** -149, -2.0 ** -140)]


def bn_planes(c, seed):
    """[2][c][256] int8: every byte value in every channel plane, in an order of its own"""
    rng = np.random.default_rng(seed)
    return np.stack([rng.permutation(256) for _ in range(BN_N * c)]).astype(np.int32).reshape(BN_N, c, BN_HW) - 128


@functools.lru_cache(maxsize=None)
def bn_search(in_scale, out_scale, seed):
    """seeded search over SEARCH_CHANNELS random (sc, bi) for channels in which, at some byte, a reciprocal multiply gives another result
    than the division, and channels in which a fused x * sc + bi does -> (sc, bi, kinds) of the kept channels, at most 6 of each kind.
    Only elements whose t + 0.5 lies within 2^-9 of an integer inside the clamps can change, so only those are tried in the other forms.
    Measured: 13 / 7 channels found at (0.05, 0.037), 38 / 9 at (0.02, 0.0213).  A kept fused witness is confirmed in exact arithmetic."""
    rng = np.random.default_rng(seed)
    sc = (rng.random(SEARCH_CHANNELS, dtype=F) * F(3) - F(1.5)).astype(F)
    bi = (rng.random(SEARCH_CHANNELS, dtype=F) * F(4) - F(2)).astype(F)
    q = np.arange(-128, 128, dtype=np.int32).reshape(1, 256)
    with np.errstate(**QUIET):
        u = ((q.astype(F) * F(in_scale)) * sc.reshape(-1, 1) + bi.reshape(-1, 1)) / F(out_scale) + F(0.5)
    ch, qi = np.nonzero((np.abs(u - np.rint(u)) < F(2.0 ** -9)) & (np.abs(u) < 200))
    plain = bn_i8_elements(q[0, qi], sc[ch], bi[ch], in_scale, out_scale)
    keep, kinds = [], []
    for form in ("recip", "fma"):
        hit = np.flatnonzero(bn_i8_elements(q[0, qi], sc[ch], bi[ch], in_scale, out_scale, form=form) != plain)
        found = []
        for k in hit:
            c, xf = int(ch[k]), F(q[0, qi[k]]) * F(in_scale)
            if c in found or c in keep:
                continue
            if form == "fma" and not is_nearest(fma32(xf, sc[c], bi[c]), Fraction(float(xf)) * Fraction(float(sc[c])) + Fraction(float(bi[c]))):
                continue
            found.append(c)
        assert len(found) >= 4, (form, len(found))
        keep += found[:6]
        kinds += [form] * len(found[:6])
    return sc[keep], bi[keep], tuple(kinds)


BN_I8_NAMES = ("ties", "searched_a", "searched_b", "no_s", "no_b", "no_s_no_b", "in_zero", "in_neg", "in_nan", "out_zero", "out_neg", "out_nan")


@functools.lru_cache(maxsize=None)
def bn_i8_cases():
    """name -> dict(x [2][c][256], c, s, b (None = missing), in_scale, out_scale, want)"""
    out = {}

    def add(name, c, s, b, isc, osc, seed):
        x = bn_planes(c, seed).astype(I8)
        s = None if s is None else f32(s).copy()
        b = None if b is None else f32(b).copy()
        out[name] = dict(x=x, c=c, s=s, b=b, in_scale=F(isc), out_scale=F(osc), want=batchnorm_i8(x, BN_N, c, BN_HW, s, b, isc, osc))
        return out[name]

    # exact ties: y / out_scale = (q sc + k) / 2 with k odd.  Measured: 1 070 positive and 1 068 negative ties inside the clamps, of 4 096 results
    sc = f32([1, -1, 0.5, 3, -0.25, 1, 2, -2])
    bi = f32([1, 3, -5, 7, 9, -11, 13, -1]) * F(2.0 ** -4)
    k = add("ties", 8, sc, bi, 2.0 ** -4, 2.0 ** -3, 11)
    t = (k["x"].astype(np.float64) * 2.0 ** -4 * sc.astype(np.float64).reshape(1, 8, 1) + bi.astype(np.float64).reshape(1, 8, 1)) * 8.0
    tie = (t * 2) % 2 == 1
    assert (tie & (t > 0) & (t < 127)).sum() >= 1000 and (tie & (t < 0) & (t > -128)).sum() >= 1000
    inside = tie & (np.abs(t) < 127)
    assert np.array_equal(k["want"].reshape(t.shape)[inside], np.floor(t[inside] + 0.5))  # ties go up
    # searched channels, then the special ones
    for name, isc, osc, seed in (("searched_a", 0.05, 0.037, 21), ("searched_b", 0.02, 0.0213, 22)):
        s, b, kinds = bn_search(isc, osc, seed)
        if name == "searched_a":
            s = np.concatenate([s, f32([q[0] for q in SPECIAL_SC_BI])])
            b = np.concatenate([b, f32([q[1] for q in SPECIAL_SC_BI])])
        k = add(name, len(s), s, b, isc, osc, seed)
        for form in ("recip", "fma"):  # at least 4 kept channels of each kind change a byte of THIS case
            other = batchnorm_i8(k["x"], BN_N, k["c"], BN_HW, s, b, isc, osc, form=form)
            per_ch = (other != k["want"]).reshape(BN_N, k["c"], BN_HW).any(axis=(0, 2))
            assert per_ch[[i for i, q in enumerate(kinds) if q == form]].all() and per_ch.sum() >= 4, (name, form)
    sp = out["searched_a"]
    w = sp["want"].reshape(BN_N, sp["c"], BN_HW)[:, -len(SPECIAL_SC_BI):]
    assert (w[:, 0] == -128).all() and (w[:, 1] == -128).all() and (w[:, 2] == -128).all()  # NaN, +inf and -inf alike
    assert (batchnorm_i8(sp["x"], BN_N, sp["c"], BN_HW, sp["s"], sp["b"], 0.05, 0.037, saturating=True) != sp["want"]).any()
    assert set(np.unique(w[:, 3]).tolist()) == {-128, 0}  # sc = 3e30: both signs overflow to -128, x = 0 stays 0
    # the forms with s, b, or both missing; the scale fall-backs; a single channel and a single pixel
    s, b = out["searched_a"]["s"][:5], out["searched_a"]["b"][:5]
    add("no_s", 5, None, b, 0.05, 0.037, 31)
    add("no_b", 5, s, None, 0.05, 0.037, 32)
    add("no_s_no_b", 5, None, None, 0.05, 0.037, 33)
    for name, isc, osc in (("in_zero", 0.0, 0.037), ("in_neg", -0.05, 0.037), ("in_nan", np.nan, 0.037),
                           ("out_zero", 0.05, 0.0), ("out_neg", 0.05, -0.037), ("out_nan", 0.05, np.nan)):
        k = add(name, 5, s, b, isc, osc, 34)
        one = batchnorm_i8(k["x"], BN_N, 5, BN_HW, s, b, 1.0 if name.startswith("in") else 0.05, 0.037 if name.startswith("in") else 1.0)
        assert np.array_equal(k["want"], one)
    assert tuple(out) == BN_I8_NAMES
    return out


# ---- float32 --------------------------------------------------------------------------------------------------------------------------------
def sweep_1021():
    """every 1021st bit pattern of the 32-bit space"""
    return from_bits(np.arange(0, 1 << 32, 1021, dtype=np.uint64).astype(U32))


@functools.lru_cache(maxsize=None)
def f32_binary_operands():
    """256 floats: +-0, the smallest and largest subnormals, FLT_MIN, 1, 1 +- ulp, FLT_MAX, +-inf, a NaN, and seeded random bit patterns
    of every exponent class (exponent field 0, 1 .. 254 and 255)"""
    special = [0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00800000, 0x80800000, 0x3F800000, 0xBF800000,
               0x3F800001, 0x3F7FFFFF, 0xBF800001, 0xBF7FFFFF, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F800000, 0xFF800000, 0x7FC00000]
    rng = np.random.default_rng(404)
    n = 256 - len(special)
    expo = np.concatenate([np.zeros(20), np.full(6, 255), rng.integers(1, 255, n - 66), [1, 2, 23, 24, 253, 254] * 5 + [126, 127, 128, 102, 103, 104, 149, 150, 151, 127]])
    assert len(expo) == n
    u = (rng.integers(0, 2, n).astype(np.uint64) << 31) | (expo.astype(np.uint64) << 23) | rng.integers(0, 1 << 23, n).astype(np.uint64)
    v = from_bits(np.concatenate([np.array(special, dtype=np.uint64), u]).astype(U32))
    assert len(v) == 256 and np.isnan(v).sum() >= 2 and is_subnormal(v).sum() >= 20 and np.isinf(v).sum() >= 2
    return v


@functools.lru_cache(maxsize=None)
def f32_binary_case():
    """all 65 536 pairs -> (a, b, [add, mul, sub]).  Measured: 3 537 NaN sums, 3 930 subnormal products, 5 840 infinite products from
    finite operands, 11 153 zero products of either sign from non-zero operands"""
    v = f32_binary_operands()
    a, b = np.repeat(v, 256), np.tile(v, 256)
    want = [binary_f32(op, a, b) for op in range(3)]
    assert np.isnan(want[0]).sum() >= 1000 and is_subnormal(want[1]).sum() >= 1000
    assert (np.isinf(want[1]) & np.isfinite(a) & np.isfinite(b)).sum() >= 1000
    assert ((want[1] == 0) & (a != 0) & (b != 0)).sum() >= 100 and (bits(want[2]) == 0x80000000).any()
    return a, b, want


RELU_ALPHAS = (F(0.0), F(0.01))
TINY_END = 0x04800000  # the bit pattern of 2^-118: every x below it has a subnormal x * 0.01f or none at all


@functools.lru_cache(maxsize=None)
def f32_relu_sweep():
    """every 1021st pattern, and every 37th pattern with |x| < 2^-118 (both signs): what the graph-level tests run; the launcher test adds
    EVERY pattern with |x| < 2^-118 (tiny_patterns).  Measured over 8 287 575 floats: 4 135 571 results of -0.0 and 16 433 NaN at alpha 0; 2 011 631 subnormal
    results at alpha 0.01, 1 541 762 of them from normal x"""
    t = np.arange(0, TINY_END, 37, dtype=np.uint64)
    x = np.concatenate([sweep_1021(), from_bits(t.astype(U32)), from_bits((t | 0x80000000).astype(U32))])
    r0, r1 = relu_f32(x, RELU_ALPHAS[0]), relu_f32(x, RELU_ALPHAS[1])
    assert (bits(r0) == 0x80000000).sum() >= 1000 and np.isnan(r0).sum() >= 1000 and np.isnan(r1).sum() >= 1000
    assert is_subnormal(r1).sum() >= 1000 and (is_subnormal(r1) & ~is_subnormal(x)).sum() >= 1000  # x * 0.01f going subnormal
    assert (bits(relu_f32(x, 0, form="max")) != bits(r0)).sum() >= 1000
    return x


def tiny_patterns(negative):
    """EVERY pattern with |x| < 2^-118 of one sign: 75 497 472 floats"""
    u = np.arange(0, TINY_END, dtype=U32)
    if negative:
        u |= U32(0x80000000)
    return from_bits(u)


SIG_BANDS = {"neg": (-104.0, -87.0), "pos": (87.0, 104.0)}


def sigmoid_band(which):
    """EVERY pattern of x in [-104, -87] / [87, 104]: 2 228 225 floats each.  The band of subnormal results (x in (-88.723, -87.336)),
    the overflow of expf to inf and the -0x1.9fe368p6f / 0x1.62e42ep6f cut-offs of expf_exact"""
    lo, hi = SIG_BANDS[which]
    u0, u1 = sorted((int(bits(F(lo))[0]), int(bits(F(hi))[0])))
    return from_bits(np.arange(u0, u1 + 1, dtype=np.uint64).astype(U32))


def sigmoid_sweep():
    """every 1021st pattern, and every 64th pattern of +-[2^-7, 96]"""
    u = np.arange(0x3C000000, 0x42C00000 + 1, 64, dtype=np.uint64)
    return np.concatenate([sweep_1021(), from_bits(u.astype(U32)), from_bits((u | 0x80000000).astype(U32))])


SIGMOID_CASES = ("sweep", "neg", "pos")


@functools.lru_cache(maxsize=None)
def f32_sigmoid_case(which):
    """-> (x, want), computed once (the libm calls take a few seconds).  Measured: 181 704 subnormal results in "neg" and 2 002 409 of 0.0 below
    them, 1.0 throughout "pos"; the sweep (7 745 575 floats) has 16 433 NaN and 3 017 subnormal results"""
    x = sigmoid_sweep() if which == "sweep" else sigmoid_band(which)
    want = sigmoid_f32(x)
    if which == "neg":
        assert is_subnormal(want).sum() >= 100000 and (bits(want) == 0).any() and (want >= F(2.0 ** -126)).any()
    elif which == "pos":
        assert (want == 1).all()
    else:
        assert (want == 1).any() and (bits(want) == 0).any() and np.isnan(want).sum() >= 1000 and len(np.unique(bits(want))) > 100000
    want.setflags(write=False)
    return x, want


BN_F32_SHAPES = [(2, 7, 5, 9), (1, 64, 16, 16)]


@functools.lru_cache(maxsize=None)
def bn_f32_case(shape, special=False):
    """-> dict(x, n, c, hw, s, b, want): random data in (-4, 4), sc in (-1.5, 1.5), bi in (-2, 2).  Measured: a fused multiply-add changes
    17.6% / 25.6% of the results.  special: the first channels take SPECIAL_SC_BI"""
    n, c, h, w = shape
    rng = np.random.default_rng(n * 1000 + c)
    x = (rng.random(n * c * h * w, dtype=F) * F(8) - F(4)).astype(F)
    s = (rng.random(c, dtype=F) * F(3) - F(1.5)).astype(F)
    b = (rng.random(c, dtype=F) * F(4) - F(2)).astype(F)
    if special:
        k = min(c, len(SPECIAL_SC_BI))
        s[:k], b[:k] = f32([q[0] for q in SPECIAL_SC_BI[:k]]), f32([q[1] for q in SPECIAL_SC_BI[:k]])
        x[::5] = from_bits(np.random.default_rng(c).integers(0, 1 << 32, len(x[::5]), dtype=np.uint64).astype(U32))  # any bit pattern
    want = batchnorm_f32(x, n, c, h * w, s, b)
    if not special:
        assert (bits(batchnorm_f32(x, n, c, h * w, s, b, form="fma")) != bits(want)).mean() >= 0.01
    else:
        assert np.isnan(want).any() and np.isinf(want).any()
    return dict(x=x, n=n, c=c, hw=h * w, s=s, b=b, want=want)


# ---- one-layer graphs: every case above that a .mars file can express ------------------------------------------------------------------------
# name -> (file bytes, [input index -> frame -> array], output tensor, "i8" / "f32", frame -> expected output).  Two frames each: the second
# holds the first one's elements in reverse order (batch-norm: planes of its own), so that no frame mix-up cancels.  Scales stand on the
# tensors; batch-norm parameters are weight tensors; the binaries take two graph inputs.
def _graph_binary(dtype, is_mul, n, sa=1.0, sb=1.0, so=1.0):
    import marsfile as M
    G = M.Graph()
    shape = [1, 1, n // 256, 256]
    kw = dict(dtype=M.F32, fmt=M.NCHW) if dtype == "f32" else {}
    a, b, o = G.tensor(shape, scale=float(sa), **kw), G.tensor(shape, scale=float(sb), **kw), G.tensor(shape, scale=float(so), **kw)
    G.layer(M.MUL if is_mul else M.ADD, [a, b], [o])
    return G.serialise([a, b], [o]), o


def _graph_unary(dtype, kind, n, in_scale=1.0, out_scale=1.0):
    import marsfile as M
    G = M.Graph()
    kw = dict(dtype=M.F32, fmt=M.NCHW) if dtype == "f32" else {}
    a, o = G.tensor([1, 1, 1, n], scale=float(in_scale), **kw), G.tensor([1, 1, 1, n], scale=float(out_scale), **kw)
    G.layer(dict(sigmoid=M.SIGMOID, relu=M.RELU, relu6=M.RELU6, leaky=M.LEAKY)[kind], [a], [o])
    return G.serialise([a], [o]), o


def _graph_bn(dtype, shape, s, b, in_scale=1.0, out_scale=1.0, fmt=None):
    import marsfile as M
    G = M.Graph()
    kw = dict(dtype=M.F32 if dtype == "f32" else M.I8, fmt=M.NCHW if fmt is None else fmt)
    a = G.tensor(list(shape), scale=float(in_scale), **kw)
    ts = M.NONE if s is None else G.tensor([shape[1]], dtype=M.F32, fmt=M.D1, data=f32(s))
    tb = M.NONE if b is None else G.tensor([shape[1]], dtype=M.F32, fmt=M.D1, data=f32(b))
    o = G.tensor(list(shape), scale=float(out_scale), **kw)
    G.layer(M.BATCHNORM, [a, ts, tb], [o])
    return G.serialise([a], [o]), o


def _rev(x):
    return np.ascontiguousarray(x[::-1])


@functools.lru_cache(maxsize=None)
def graph_case(name):
    """-> dict(d, inputs = [per input: [frame 0, frame 1]], out, dtype, want = [frame 0, frame 1])"""
    fam, _, rest = name.partition("/")
    if fam == "bin_i8":
        cls, _, op = rest.rpartition("_")
        is_mul = int(op == "mul")
        if cls in HOST_OUT_SCALES:  # the host's rule for the output scale, at ODD's operand scales
            a, b = all_pairs()
            (sa, sb, _), so = BINARY_CLASSES["ODD"][0][is_mul], HOST_OUT_SCALES[cls]
            inv = inv_of(so)
            assert np.isfinite(inv) and (inv == 1 or cls == "so_denorm")
            want = binary_i8(is_mul, a, b, sa, sb, inv)
        else:
            a, b, sa, sb, inv, want = binary_case(cls, is_mul)
            so = BINARY_CLASSES[cls][1]
            assert bits(inv_of(so)) == bits(inv), (cls, "the graph's output scale does not give the class's inv")
        d, o = _graph_binary("i8", is_mul, len(a), sa, sb, so)
        return dict(d=d, inputs=[[a, _rev(a)], [b, _rev(b)]], out=o, dtype="i8", want=[want, _rev(want)])
    if fam == "unary_i8":
        kind, _, sk = rest.partition("_")
        isc, osc = UNARY_SCALES[sk]
        xs = [unary_bytes(0), unary_bytes(1)]
        d, o = _graph_unary("i8", kind, len(xs[0]), isc, osc)
        return dict(d=d, inputs=[xs], out=o, dtype="i8", want=[unary_i8(kind, x, isc, osc) for x in xs])
    if fam == "bn_i8":
        nhwc = rest.endswith("@nhwc")  # tagged NHWC: the reference still indexes [n][c][h][w]
        k = bn_i8_cases()[rest.replace("@nhwc", "")]
        xs = [k["x"], bn_planes(k["c"], 7000 + k["c"]).astype(I8)]
        import marsfile as M
        d, o = _graph_bn("i8", (BN_N, k["c"], 16, 16), k["s"], k["b"], k["in_scale"], k["out_scale"], M.NHWC if nhwc else None)
        return dict(d=d, inputs=[[x.reshape(-1) for x in xs]], out=o, dtype="i8",
                    want=[batchnorm_i8(x, BN_N, k["c"], BN_HW, k["s"], k["b"], k["in_scale"], k["out_scale"]) for x in xs])
    if fam == "bin_f32":
        a, b, want = f32_binary_case()
        op = ("add", "mul").index(rest)
        d, o = _graph_binary("f32", op, len(a))
        return dict(d=d, inputs=[[a, _rev(a)], [b, _rev(b)]], out=o, dtype="f32", want=[want[op], _rev(want[op])])
    if fam == "relu_f32":
        x = f32_relu_sweep()
        want = relu_f32(x, RELU_ALPHAS[rest == "leaky"])
        d, o = _graph_unary("f32", rest, len(x))
        return dict(d=d, inputs=[[x, _rev(x)]], out=o, dtype="f32", want=[want, _rev(want)])
    if fam == "sigmoid_f32":
        x, want = f32_sigmoid_case(rest)
        d, o = _graph_unary("f32", "sigmoid", len(x))
        return dict(d=d, inputs=[[x, _rev(x)]], out=o, dtype="f32", want=[want, _rev(want)])
    if fam == "bn_f32":
        i, _, sp = rest.partition("_")
        shape = BN_F32_SHAPES[int(i)]
        k = bn_f32_case(shape, sp == "special")
        xs = [k["x"], _rev(k["x"])]
        d, o = _graph_bn("f32", shape, k["s"], k["b"])
        return dict(d=d, inputs=[xs], out=o, dtype="f32", want=[batchnorm_f32(x, k["n"], k["c"], k["hw"], k["s"], k["b"]) for x in xs])
    raise KeyError(name)


GRAPH_CASES = (["bin_i8/%s_%s" % (c, op) for c in list(BINARY_CLASSES) + list(HOST_OUT_SCALES) if BINARY_CLASSES.get(c, (0, 1))[1] is not None
                for op in ("add", "mul")]
               + ["unary_i8/%s_%s" % q for q in UNARY_CASES]
               + ["bn_i8/" + n for n in BN_I8_NAMES + ("ties@nhwc", "searched_a@nhwc")]
               + ["bin_f32/add", "bin_f32/mul", "relu_f32/relu", "relu_f32/leaky"] + ["sigmoid_f32/" + w for w in SIGMOID_CASES]
               + ["bn_f32/0", "bn_f32/1", "bn_f32/0_special", "bn_f32/1_special"])
BIG_GRAPHS = ("relu_f32", "sigmoid_f32")  # millions of floats: run with the smallest slack behind the tensors
