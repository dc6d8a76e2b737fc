"""The arithmetic of csrc/hip/eltwise.hip over its full operand domain: binary_i8_kernel, f32_kernel (add, mul, sub, sigmoid, ReLU, leaky
ReLU) and bn_kernel (int8 and float32) one launcher call at a time against tests/eltref.py, and the same cases as one-layer graphs against
the CPU oracle, which is what tests the host code of mars_plan.c that feeds them (plan_unary's tables, plan_binary's 1 / so, plan_batchnorm's
scale rules).  Every comparison is bit for bit; where the expected float is NaN only NaN-ness is compared.  The sigmoid's expected values
come from the host libm, so test_sigmoid_f32 is the device sweep of csrc/expf_exact.h.

Operands live in the guarded allocations of tests/test_gpu_move.py ([256 guard bytes][payload][256 guard bytes], outputs pre-filled with
0x5A): the guards, the bytes between frames and outside a slice must still hold the sentinel, and inputs must be unchanged.  Refusals are
asserted only where the launcher returns before any launch.  tests/test_elt_cpu.py pins eltref and the cases without a GPU."""
import ctypes as C

import numpy as np
import pytest

import eltref as E
import moveref as R
from test_gpu_move import SENT, align16, hbm, same, sentinel, strided  # noqa: F401  (hbm: a fixture)

pytestmark = pytest.mark.gpu

F, I8, U8 = np.float32, np.int8, np.uint8
FRAMES = 3


@pytest.fixture
def dev(hbm):
    """hbm with the prototypes of the five launchers tests/test_gpu_move.py does not declare"""
    P, Z, I, Fl = C.c_void_p, C.c_size_t, C.c_int, C.c_float
    for n, a in (("mhip_batchnorm_i8", [P, Z, P, Z, I, I, I, I, P, P, Fl, Fl]),
                 ("mhip_batchnorm_f32", [P, Z, P, Z, I, I, I, I, P, P]),
                 ("mhip_sigmoid_f32", [P, Z, P, Z, I, Z]),
                 ("mhip_binary_f32", [I, P, Z, P, Z, P, Z, I, Z]),
                 ("mhip_relu_f32", [P, Z, P, Z, I, Z, Fl])):
        f = getattr(hbm.L, n)
        f.restype, f.argtypes = I, a
    return hbm


def off16(stride):
    """the next multiple of 4 from `stride` on that is no multiple of 16"""
    return stride + 4 if stride % 16 == 0 else stride


def raw(x):
    return np.ascontiguousarray(x).reshape(-1).view(U8)


def image(frames, stride):
    """what an output allocation must hold: frames[f] at f * stride, the sentinel everywhere else"""
    return strided([raw(x) for x in frames], stride, SENT)


# ---- mhip_binary_i8: every class x op through each of its code paths ------------------------------------------------------------------------------
# aligned  = pointers and strides multiples of 16, dense: 16-byte body;  plus1 = every pointer + 1: byte path;
# slice16  = slice output (run 16, pix_stride 48, ch_off 16): one 16-byte store per thread;  slice12 = (12, 40, 20): byte by byte
BIN_PATHS = {"aligned": (0, 0, 0, 0), "plus1": (1, 0, 0, 0), "slice16": (0, 16, 48, 16), "slice12": (0, 12, 40, 20)}


@pytest.mark.parametrize("case", E.BINARY_CASES, ids=E.binary_id)
def test_binary_i8(dev, case):
    """all 65 536 pairs, 2 frames (the second in reverse order); the same case through all paths gives the same bytes, all equal to eltref"""
    cls, is_mul = case
    a, b, sa, sb, inv, want = E.binary_case(cls, is_mul)
    dense = {}
    for path, (off, run, ps, choff) in BIN_PATHS.items():
        pad = (-len(a)) % run if run else 0  # n % run == 0: the first pairs once more behind the last
        xa, xb, w = (np.concatenate([v, v[:pad]]) for v in (a, b, want))
        n = len(xa)
        fa, fb, fw = [xa, xa[::-1]], [xb, xb[::-1]], [w, w[::-1]]
        npix = n // run if run else 0
        frame_out = npix * ps if run else n
        sa_, sb_, so_ = n + 16, n + 32, align16(frame_out) + 48
        da, db = dev(strided(fa, sa_, (1,)), off, guard=R.random_bytes(2, 512)), dev(strided(fb, sb_, (3,)), off, guard=R.random_bytes(4, 512))
        d = dev(sentinel(2 * so_), off)
        assert dev.L.mhip_binary_i8(is_mul, da.ptr, sa_, db.ptr, sb_, d.ptr, so_, 2, n, float(sa), float(sb), float(inv), run, ps, choff) == 0
        exp = sentinel(2 * so_).view(I8)
        for f in range(2):
            if run:
                R.place(exp[f * so_:], fw[f], npix, run, ps, choff)
            else:
                exp[f * so_:f * so_ + n] = fw[f]
        what = "binary_i8 %s %s" % (E.binary_id(case), path)
        got = d.read(what)
        same(what, got, exp)
        da.unchanged(what)
        db.unchanged(what)
        g0 = got[:frame_out].view(I8)
        dense[path] = (g0.reshape(npix, ps)[:, choff:choff + run].reshape(-1) if run else g0)[:len(a)]
    for path in BIN_PATHS:
        same("binary_i8 %s: %s against aligned" % (E.binary_id(case), path), dense[path], dense["aligned"])


# ---- mhip_batchnorm_i8 / mhip_batchnorm_f32 -----------------------------------------------------------------------------------------------------
def dev_params(dev, v):
    return None if v is None else dev(E.f32(v))


def ptr(d):
    return None if d is None else d.ptr


def run_bn_i8(dev, what, xs, n, c, hw, s, b, isc, osc, in_gap=7, out_gap=13):
    """frames xs at strides that are no multiples of 16; -> nothing, asserts"""
    total = n * c * hw
    is_, os_ = total + in_gap, total + out_gap
    a = dev(strided([raw(x) for x in xs], is_, (5,)), guard=R.random_bytes(6, 512))
    ds, db = dev_params(dev, s), dev_params(dev, b)
    d = dev(sentinel(len(xs) * os_))
    assert dev.L.mhip_batchnorm_i8(a.ptr, is_, d.ptr, os_, len(xs), n, c, hw, ptr(ds), ptr(db), float(isc), float(osc)) == 0
    same(what, d.read(what), image([E.batchnorm_i8(x, n, c, hw, s, b, isc, osc) for x in xs], os_))
    for q in (a, ds, db):
        if q is not None:
            q.unchanged(what)


@pytest.mark.parametrize("name", E.BN_I8_NAMES)
def test_batchnorm_i8(dev, name):
    """[2, C, 16, 16] with every int8 value in every channel: exact ties, searched channels in which a reciprocal multiply or a fused
    multiply-add gives another byte, NaN / inf / 3e30 / subnormal parameters, s / b missing, the scales not > 0 as the planner passes them"""
    k = E.bn_i8_cases()[name]
    xs = [k["x"], E.bn_planes(k["c"], 7000 + k["c"]).astype(I8), k["x"][::-1]]
    # plan_batchnorm replaces scales that are not > 0 by 1.0 before the launch; the launcher itself takes what it is given
    run_bn_i8(dev, "batchnorm_i8 " + name, xs, E.BN_N, k["c"], E.BN_HW, k["s"], k["b"], E.scale_or_one(k["in_scale"]), E.scale_or_one(k["out_scale"]))


# (n, c, hw, s given, b given)
BN_LAYOUT = [(2, 3, 1, True, True), (1, 1, 300, True, True), (2, 5, 7, True, False), (1, 1, 1, False, False), (3, 2, 257, False, True)]


@pytest.mark.parametrize("case", BN_LAYOUT, ids=lambda c: "x".join(str(int(q)) for q in c))
def test_batchnorm_layout(dev, case):
    """hw = 1, c = 1, n > 1, more than one block, null s / b: which channel an element takes, int8 and float32"""
    n, c, hw, has_s, has_b = case
    rng = np.random.default_rng(n * 100 + c * 10 + hw)
    s = (rng.random(c, dtype=F) * F(3) - F(1.5)) if has_s else None
    b = (rng.random(c, dtype=F) * F(4) - F(2)) if has_b else None
    total = n * c * hw
    run_bn_i8(dev, "batchnorm_i8 layout %s" % (case,), [rng.integers(-128, 128, total).astype(I8) for _ in range(FRAMES)], n, c, hw, s, b, F(0.05), F(0.037))
    run_bn_f32(dev, "batchnorm_f32 layout %s" % (case,), [(rng.random(total, dtype=F) * F(8) - F(4)) for _ in range(FRAMES)], n, c, hw, s, b)


def run_bn_f32(dev, what, xs, n, c, hw, s, b):
    """frames at byte strides that are multiples of 4 and not of 16"""
    total = n * c * hw
    is_, os_ = off16(4 * total + 4), off16(4 * total + 8)
    a = dev(strided([raw(x) for x in xs], is_, (7,)), guard=R.random_bytes(8, 512))
    ds, db = dev_params(dev, s), dev_params(dev, b)
    d = dev(sentinel(len(xs) * os_))
    assert dev.L.mhip_batchnorm_f32(a.ptr, is_, d.ptr, os_, len(xs), n, c, hw, ptr(ds), ptr(db)) == 0
    E.assert_same(what, d.read(what), image([E.batchnorm_f32(x, n, c, hw, s, b) for x in xs], os_), "f32")
    for q in (a, ds, db):
        if q is not None:
            q.unchanged(what)


@pytest.mark.parametrize("special", [False, True], ids=["random", "special"])
@pytest.mark.parametrize("shape", E.BN_F32_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_batchnorm_f32(dev, shape, special):
    """random data (a fused multiply-add would change 17.6% / 25.6% of the results), then NaN / inf / 3e30 / subnormal parameters on
    arbitrary bit patterns"""
    k = E.bn_f32_case(shape, special)
    xs = [k["x"], k["x"][::-1], np.roll(k["x"], 3)]
    run_bn_f32(dev, "batchnorm_f32 %s" % (shape,), xs, k["n"], k["c"], k["hw"], k["s"], k["b"])


def test_batchnorm_refusals(dev):
    a, d, p = dev(np.zeros(256, U8)), dev(sentinel(256)), dev(np.ones(4, F))
    L = dev.L
    for n, c, hw in ((0, 2, 2), (2, 0, 2), (2, 2, 0), (-1, 2, 2)):
        assert L.mhip_batchnorm_i8(a.ptr, 64, d.ptr, 64, 1, n, c, hw, p.ptr, p.ptr, 1.0, 1.0) == -1
        assert L.mhip_batchnorm_f32(a.ptr, 64, d.ptr, 64, 1, n, c, hw, p.ptr, p.ptr) == -1
    assert L.mhip_batchnorm_i8(None, 64, d.ptr, 64, 1, 1, 2, 2, p.ptr, p.ptr, 1.0, 1.0) == -1
    assert L.mhip_batchnorm_i8(a.ptr, 64, None, 64, 1, 1, 2, 2, p.ptr, p.ptr, 1.0, 1.0) == -1
    assert L.mhip_batchnorm_i8(a.ptr, 64, d.ptr, 64, 0, 1, 2, 2, p.ptr, p.ptr, 1.0, 1.0) == -1
    assert L.mhip_batchnorm_f32(None, 64, d.ptr, 64, 1, 1, 2, 2, p.ptr, p.ptr) == -1
    assert L.mhip_batchnorm_f32(a.ptr, 64, None, 64, 1, 1, 2, 2, p.ptr, p.ptr) == -1
    assert L.mhip_batchnorm_f32(a.ptr, 64, d.ptr, 64, 0, 1, 2, 2, p.ptr, p.ptr) == -1
    same("batchnorm refusals", d.read("refusals"), sentinel(256))


# ---- f32_kernel: mhip_binary_f32, mhip_relu_f32, mhip_sigmoid_f32 -----------------------------------------------------------------------------------
SMALL_N = [1, 3, 4, 5, 1027]  # a thread owns 4 floats, a block 1024: below, at and above both


def run_f32(dev, what, call, ins, want, frames=2, check_inputs=True, fill=None):
    """ins: per operand its frames; 2 frames at a byte stride of 4 n + 4, every pointer 4 bytes off a 16-byte boundary.  call(pointers and
    strides of the operands, then of the output, frames, n) -> the launcher's return value"""
    n = len(want[0])
    stride = 4 * n + 4
    ds = [dev(strided([raw(x) for x in fr], stride, (11 + i,) if fill is None else fill), 4, guard=R.random_bytes(12 + i, 512)) for i, fr in enumerate(ins)]
    d = dev(sentinel(frames * stride), 4)
    args = [q for x in ds for q in (x.ptr, stride)]
    assert call(*args, d.ptr, stride, frames, n) == 0
    E.assert_same(what, d.read(what), image(want, stride), "f32")
    for x in ds:
        if check_inputs:
            x.unchanged(what)
        x.free()
    d.free()


def small_operands(n, k):
    v = E.f32_binary_operands()
    return np.resize(np.roll(v, 7 * k), n)


@pytest.mark.parametrize("op", [0, 1, 2], ids=["add", "mul", "sub"])
def test_binary_f32(dev, op):
    """all 65 536 pairs of 256 floats (zeros, subnormals, FLT_MIN, 1 +- ulp, FLT_MAX, inf, NaN, every exponent class), then the small counts"""
    a, b, want = E.f32_binary_case()
    call = lambda *q: dev.L.mhip_binary_f32(op, *q)  # noqa: E731
    run_f32(dev, "binary_f32 op %d" % op, call, [[a, a[::-1]], [b, b[::-1]]], [want[op], want[op][::-1]])
    for n in SMALL_N:
        xa, xb = [small_operands(n, 0), small_operands(n, 1)], [small_operands(n, 2), small_operands(n, 3)]
        run_f32(dev, "binary_f32 op %d n %d" % (op, n), call, [xa, xb], [E.binary_f32(op, p, q) for p, q in zip(xa, xb)])


def test_binary_f32_refusals(dev):
    a, d = dev(np.zeros(256, U8)), dev(sentinel(256))
    for op in (-1, 3, 4):  # 3 and 4 are the kernel's sigmoid and ReLU: not reachable through this launcher
        assert dev.L.mhip_binary_f32(op, a.ptr, 64, a.ptr, 64, d.ptr, 64, 1, 8) == -1
    assert dev.L.mhip_binary_f32(0, a.ptr, 64, None, 64, d.ptr, 64, 1, 8) == -1
    assert dev.L.mhip_binary_f32(0, None, 64, a.ptr, 64, d.ptr, 64, 1, 8) == -1
    assert dev.L.mhip_binary_f32(0, a.ptr, 64, a.ptr, 64, None, 64, 1, 8) == -1
    assert dev.L.mhip_binary_f32(0, a.ptr, 64, a.ptr, 64, d.ptr, 64, 0, 8) == -1
    assert dev.L.mhip_relu_f32(None, 64, d.ptr, 64, 1, 8, 0.0) == -1 and dev.L.mhip_sigmoid_f32(a.ptr, 64, None, 64, 1, 8) == -1
    same("f32 refusals", d.read("refusals"), sentinel(256))


@pytest.mark.parametrize("alpha", E.RELU_ALPHAS, ids=["relu", "leaky"])
def test_relu_f32_sweep(dev, alpha):
    """every 1021st bit pattern and a 37th of the tiny ones: -0.0 for negative x, NaN for NaN (x > 0 ? x : x * alpha), then the small counts"""
    x = E.f32_relu_sweep()
    call = lambda *q: dev.L.mhip_relu_f32(*q, float(alpha))  # noqa: E731
    want = E.relu_f32(x, alpha)
    run_f32(dev, "relu_f32 alpha %g" % alpha, call, [[x, x[::-1]]], [want, want[::-1]])
    for n in SMALL_N:
        xs = [small_operands(n, 4), small_operands(n, 5)]
        run_f32(dev, "relu_f32 alpha %g n %d" % (alpha, n), call, [xs], [E.relu_f32(v, alpha) for v in xs])


@pytest.mark.parametrize("negative", [True, False], ids=["negative", "positive"])
@pytest.mark.parametrize("alpha", E.RELU_ALPHAS, ids=["relu", "leaky"])
def test_relu_f32_every_tiny_pattern(dev, alpha, negative):
    """EVERY pattern with |x| < 2^-118 of one sign, one launch: x * 0.01f is subnormal or rounds to zero for all of them"""
    x = E.tiny_patterns(negative)
    want = E.relu_f32(x, alpha)
    if negative and alpha:
        assert E.is_subnormal(want).sum() >= 1000 and (E.bits(want) == 0x80000000).any()  # (the smallest round to -0.0)
    run_f32(dev, "relu_f32 alpha %g tiny" % alpha, lambda *q: dev.L.mhip_relu_f32(*q, float(alpha)), [[x]], [want], frames=1, check_inputs=False, fill=0xA5)


@pytest.mark.parametrize("which", E.SIGMOID_CASES)
def test_sigmoid_f32(dev, which):
    """the device build of expf_exact.h, its double FMAs, the double -> float conversion into subnormals and the 1 / (1 + e) behind it,
    against the host libm: the sweeps, then EVERY pattern of [-104, -87] / [87, 104] in one launch per band"""
    x, want = E.f32_sigmoid_case(which)
    call = dev.L.mhip_sigmoid_f32
    if which == "sweep":
        run_f32(dev, "sigmoid_f32 sweep", call, [[x, x[::-1]]], [want, want[::-1]])
        for n in SMALL_N:
            xs = [small_operands(n, 6), small_operands(n, 7)]
            run_f32(dev, "sigmoid_f32 n %d" % n, call, [xs], [E.sigmoid_f32(v) for v in xs])
    else:
        run_f32(dev, "sigmoid_f32 band " + which, call, [[x]], [want], frames=1)


# ---- the same cases as one-layer graphs: mars_plan.c's tables and scale rules ---------------------------------------------------------------------
@pytest.mark.parametrize("name", E.GRAPH_CASES)
def test_elt_graph(gpu, orc, name):
    """gpu.Model(batch 2, fusion 0) against the CPU oracle on every tensor, and against eltref on the output: plan_unary's tables over all
    256 bytes x kind x scales, plan_binary's 1 / (so > 0 ? so : 1), plan_batchnorm's fall-backs and its [n][c][h][w] walk of an NHWC tag"""
    import marsfile
    k = E.graph_case(name)
    _, tensors, _ = marsfile.parse(k["d"])
    big = name.split("/")[0] in E.BIG_GRAPHS
    m = gpu.Model(k["d"], batch=2, fusion=0)
    try:
        for i, frames in enumerate(k["inputs"]):
            for f in range(2):
                m.input_view(i)[f] = raw(frames[f])
        m.run()
        for f in range(2):
            g = orc.Graph(k["d"], **(dict(slack_mult=1, slack_add=4096) if big else {}))
            for i, frames in enumerate(k["inputs"]):
                g.set_input(i, raw(frames[f]).tobytes())
            assert g.run() == 0
            for ti, t in enumerate(tensors):
                if t["size"] == 0 and marsfile.tensor_nbytes(t):
                    E.assert_same("%s frame %d tensor %d" % (name, f, ti), m.read_tensor(ti, frame=f), g.tensor(ti), k["dtype"])
            g.close()
            E.assert_same("%s frame %d against eltref" % (name, f), m.read_tensor(k["out"], frame=f), k["want"][f], k["dtype"])
    finally:
        m.close()
