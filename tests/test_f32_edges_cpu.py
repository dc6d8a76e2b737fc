"""tests/f32edges.py against the CPU oracle and against Python integers -- no GPU.  What tests/test_gpu_f32_edges.py holds the kernels to
is proven here first: the exact classes' generators and their < 2^24 condition (the oracle, float32 in the reference's order, gives the
int64 full product bit for bit), the piece model (modes 3 / 4 / records differ from the full product exactly where class C says), the
non-finite expectations of modes 0 / 2 (the oracle's own output), and the bound class (the oracle inside c_0 * A)."""
import numpy as np
import pytest

import f32edges as fe
import f32shapes

NONFINITE = [("split", f32shapes.SPLIT[0]), ("split", f32shapes.SPLIT[1]), ("split", f32shapes.SPLIT[3]),
             ("patch", f32shapes.PATCH[0]), ("patch", f32shapes.PATCH[3]), ("stem", f32shapes.STEM[0])]
BUILD = {"split": f32shapes.split_case, "patch": f32shapes.patch_case, "stem": f32shapes.stem_case}
ALL = [(fam, shape) for fam, shapes, _ in f32shapes.FAMILIES for shape in shapes]


def ids(v):
    return f32shapes.shape_id(*v) if isinstance(v, tuple) and isinstance(v[0], str) else str(v)


def seed_of(fam, shape, cls):
    return [sum(int(q) if not isinstance(q, str) else len(q) for q in shape), len(fam), fe.EXACT_CLASSES.index(cls) if cls in fe.EXACT_CLASSES else 9]


def run_oracle(orc, case, x, r=None):
    g = orc.Graph(case["d"])
    g.set_input(0, np.ascontiguousarray(x, dtype=np.float32).tobytes())
    if r is not None:
        g.set_input(1, np.ascontiguousarray(r, dtype=np.float32).tobytes())
    assert g.run() == 0
    out = g.tensor(case["out"]).view(np.float32).copy()
    g.close()
    return out


@pytest.mark.parametrize("cls", fe.EXACT_CLASSES)
@pytest.mark.parametrize("fs", ALL, ids=ids)
def test_exact_classes_oracle_is_the_integer_sum(orc, fs, cls):
    """every shape, every exact class, unscaled and scaled by 2^+-64: the oracle equals the integer full product bit for bit (and expected()
    has asserted the < 2^24 condition for every mode's kept products on the way)"""
    fam, shape = fs
    g = fe.GEOMS[fam](shape)
    xs, w, bias = fe.exact_operands(cls, g, np.random.default_rng(seed_of(fam, shape, cls)), nframes=1)
    add = fam == "patch" and shape[8]
    r = np.random.default_rng(5).integers(-1000, 1001, g.oc * g.oh * g.ow).astype(np.float32) if add else None
    want = {m: fe.expected(g, xs[0], w, bias, m, r) for m in (0, 3, 4)}
    for s in fe.SCALES:
        sx, sw = fe.scaled(xs, w, s)
        if s:
            for m in (0, 3, 4):  # the claim the GPU test relies on: the scaled operands' expectation has the bits of s = 0
                assert np.array_equal(fe.expected(g, sx[0], sw, bias, m, r).view(np.uint32), want[m].view(np.uint32)), (s, m)
            if g.K * g.oh * g.ow * g.oc > 50e6:
                continue  # (the oracle on the large shapes: once)
        case = BUILD[fam](shape, weights=sw, bias=bias, silu=False)
        got = run_oracle(orc, case, sx[0], r)
        assert fe.same_floats(got, want[0]).all(), "scale 2^%d" % s


def int_conv(g, x, w):
    """the convolution in Python integers (object arrays): no float anywhere"""
    cols = g.cols(x).astype(np.int64).astype(object)
    return np.asarray(w, dtype=np.float64).reshape(g.oc, g.K).astype(np.int64).astype(object) @ cols.T


@pytest.mark.parametrize("cls", fe.EXACT_CLASSES)
def test_piece_model_against_python_integers(cls):
    """modes 3, 4 and the record rounding against sums of piece products in Python integers: they differ from the full product exactly where
    class C says they must (mode 3 and records drop the input's lo piece; mode 4 drops nothing), nowhere in A, B, B'"""
    g = fe.Geom(7, 9, 3, 5, 3, 1)
    xs, w, bias = fe.exact_operands(cls, g, np.random.default_rng(11), nframes=1)
    x = xs[0]
    px, pw = fe.pieces(x), fe.pieces(w)
    for a in px + pw:
        assert (a == np.round(a)).all()
    assert (sum(p.astype(np.float64) for p in px) == x).all() and (sum(p.astype(np.float64) for p in pw) == w.astype(np.float64)).all()
    b = bias.astype(np.int64).astype(object).reshape(g.oc, 1)
    full = int_conv(g, x, w) + b
    for mode in (0, 2, 3, 4):
        kept = fe.KEPT[mode]
        want = full if kept is None else sum(int_conv(g, px[i], pw[j]) for i, j in kept) + b
        got = fe.expected(g, x, w, bias, mode)
        assert (got.astype(np.float64).astype(np.int64).astype(object) == want).all(), mode
        differs = bool((want != full).any())
        assert differs == (cls == "C" and mode == 3), (cls, mode)
    rec = fe.two_piece(x)
    assert bool((rec != x).any()) == (cls == "C")
    if cls == "C":  # mode 3 on x = the full product on what a record holds of x (the weights are one piece)
        assert np.array_equal(fe.expected(g, x, w, bias, 3), fe.expected(g, rec, w, bias, 0))
    if cls in ("B", "C"):
        assert (px[1] != 0).mean() > 0.8  # the mid plane is populated
    if cls == "Bp":
        assert (pw[1] != 0).mean() > 0.8


def test_pieces_of_non_finite_values():
    """an infinity: every piece but the last stays finite, the last is the infinity (so that it meets the weights' hi piece only).  FLT_MAX: with two
    pieces hi + mid = 2^128 (inf once summed in float32), with three lo = inf.  2^128 - 2^119, the smallest value bf16 rounds to inf: two pieces hold
    it exactly (hi saturates), three give inf."""
    edge = np.float32(2.0 ** 128 - 2.0 ** 119)
    x = np.array([np.inf, -np.inf, fe.FLT_MAX, -fe.FLT_MAX, edge, np.nan, 2.0 ** 127 * 1.98], dtype=np.float32)
    hi, mid = fe.pieces(x, 2)
    assert (np.abs(hi[:5]) == fe.BF16_MAX).all() and np.isposinf(mid[0]) and np.isneginf(mid[1])
    assert mid[2] == np.float32(2.0 ** 120) and mid[3] == -mid[2] and float(hi[2]) + float(mid[2]) == 2.0 ** 128 and float(hi[4]) + float(mid[4]) == float(edge)
    h3, m3, l3 = fe.pieces(x, 3)
    assert (h3[:5] == 0).all() and (m3[:5] == 0).all() and np.isposinf(l3[[0, 2, 4]]).all() and np.isneginf(l3[[1, 3]]).all()
    for p in ((hi, mid), (h3, m3, l3)):
        assert any(np.isnan(a[5]) for a in p) and np.isfinite(p[0][6]) and p[0][6] != 0
    assert fe.bf16_rne(np.float32(1.00390625)) == np.float32(1.0) and fe.bf16_rne(np.float32(1.01171875)) == np.float32(1.015625)  # ties to even


@pytest.mark.parametrize("fs", NONFINITE, ids=ids)
def test_non_finite_expectations_are_the_oracles(orc, fs):
    """modes 0 and 2 share one expectation: the special value reaches exactly the outputs whose window holds it, as NaN, sign(w) * inf or
    float32(FLT_MAX * w), and nothing else moves -- the oracle's own output, position by position, special by special"""
    fam, shape = fs
    g = fe.GEOMS[fam](shape)
    xs, w, bias = fe.exact_operands("A", g, np.random.default_rng(seed_of(fam, shape, "A")), nframes=1, nonzero_w=True)
    case = BUILD[fam](shape, weights=w, bias=bias, silu=False)
    clean = fe.expected(g, xs[0], w, bias, 0)
    for name, (f, c, y, x) in fe.positions(g, 2).items():
        for sname, sv in fe.SPECIALS:
            q = xs[0].copy().reshape(g.ic, g.h, g.w)
            q[c, y, x] = sv
            want, hit = fe.poisoned(g, clean, w, (c, y, x), sv, 0)
            assert hit.any() and not hit.all()
            got = run_oracle(orc, case, q.reshape(-1))
            assert fe.same_floats(got, want).all(), (name, sname)


@pytest.mark.parametrize("fs", NONFINITE, ids=ids)
def test_bound_class_holds_for_the_oracle(orc, fs):
    fam, shape = fs
    g = fe.GEOMS[fam](shape)
    xs, w, bias = fe.bound_operands(g, np.random.default_rng(seed_of(fam, shape, "bound")), nframes=1)
    case = BUILD[fam](shape, weights=w, bias=bias, silu=False)
    ref, A = fe.ref64(g, xs[0], w, bias)
    got = run_oracle(orc, case, xs[0]).astype(np.float64).reshape(ref.shape)
    ratio = np.abs(got - ref) / (fe.c_mode(0, g.K) * A)
    assert ratio.max() <= 1.0, ratio.max()


def test_silu_grid_and_bound():
    v = fe.silu_grid()
    assert v.size > 33000 and (v == 0).sum() == 2 and np.signbit(v[v == 0]).sum() == 1 and np.abs(v).max() == 104 and np.abs(v[v != 0]).min() == 2.0 ** -126
    assert (fe.bf16_rne(v) == v).all()
    assert (fe.silu_fast_bound(v) >= 2.0 ** -120).all()


@pytest.mark.parametrize("px", [2, 210])
def test_virtual_concat_expectations_are_the_oracles(orc, px):
    """the graph of the virtual-concat GPU tests: with_specials() over the oracle's own concat tensor gives the oracle's output, for a special
    among the concat's first-run pixels and behind them"""
    import marsfile
    h, w, c, oc, B = f32shapes.VC
    g = fe.Geom(h, w, 2 * c, oc, 1, 1)
    rng = np.random.default_rng(3)
    x = rng.integers(-15, 16, h * w).astype(np.float32)
    wa, wb = rng.choice(np.arange(1, 16), c), -rng.choice(np.arange(1, 16), c)
    wr = rng.integers(-15, 16, (oc, 2 * c))
    wr = np.where(wr == 0, 7, wr)
    br = rng.integers(-1000, 1001, oc)
    d, cat = f32shapes.vcat_graph(wa, wb, wr, br)
    out_id = marsfile.parse(d)[0]["outputs"][0]
    for sname, sv in fe.SPECIALS[:3]:
        q = x.copy()
        q[px] = sv
        o = orc.Graph(d)
        o.set_input(0, q.tobytes())
        assert o.run() == 0
        ct, out = o.tensor(cat).view(np.float32).copy(), o.tensor(out_id).view(np.float32).copy()
        o.close()
        want, hit = fe.with_specials(g, ct, wr, lambda z: fe.expected(g, z, wr, br, 0))
        assert hit.any() and not hit.all() and fe.same_floats(out, want).all(), sname
