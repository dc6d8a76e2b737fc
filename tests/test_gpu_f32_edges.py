"""The float32 convolution kernels (conv_f32_split / conv_f32_patch / conv_f32_stem, the pair form) at the operands the random [-1, 1]
cases never reach, in modes 3 (two bf16 pieces, three products), 4 (three pieces, six products), 2 (f32 matrix cores) and 0 (the
reference's order): tests/f32edges.py says what each mode must give and tests/test_f32_edges_cpu.py proves those expectations on the CPU.
* exact classes: integer operands (times 2^+-64) whose every piece product and partial sum is exact -- the result equals the integer sum
  of the mode's kept piece products BIT FOR BIT in every frame; a piece plane read from the wrong slot, a cross term dropped on one K
  step, a tap off by one all show at zero tolerance;
* non-finite classes: one +-inf / NaN / +-FLT_MAX in one frame reaches exactly the outputs whose window holds it;
* bound class: magnitudes 2^-20 .. 2^20 against a float64 convolution within c_mode * sum |x| |w| per element;
* the three-product kernels' fast SiLU against float64, the six-product mode's against the oracle bit for bit.
The launch counters prove that each case ran the kernel it is meant for."""
import ctypes as C

import numpy as np
import pytest

import f32edges as fe
import f32shapes
import marsfile

pytestmark = pytest.mark.gpu

MODES = (3, 4, 2, 0)
BUILD = {"split": f32shapes.split_case, "patch": f32shapes.patch_case, "stem": f32shapes.stem_case}
ALL = [(fam, shape) for fam, shapes, _ in f32shapes.FAMILIES for shape in shapes]
SUBSET = [("split", f32shapes.SPLIT[0]), ("split", f32shapes.SPLIT[1]), ("split", f32shapes.SPLIT[3]),  # one per gather form: 0, 1, 2
          ("patch", f32shapes.PATCH[0]), ("patch", f32shapes.PATCH[3]), ("stem", f32shapes.STEM[0])]   # stride 1, stride 2; the stem


def ids(v):
    return f32shapes.shape_id(*v) if isinstance(v, tuple) and isinstance(v[0], str) else str(v)


def seed_of(fam, shape, tag):
    return [sum(int(q) if not isinstance(q, str) else len(q) for q in shape), len(fam), sum(ord(ch) for ch in tag)]


def batch_of(fam, shape):
    B = shape[7] if fam == "split" else shape[6] if fam == "patch" else shape[5]
    return min(B, 5) if B == 37 else B  # (the 37 short frames: 5 keep several frame boundaries per tile)


def runs_of(fam):
    """(mode, persist_slots): the patch and stem kernels also with three workgroups walking all tiles"""
    return ((3, 0), (3, 3), (4, 0), (2, 0), (0, 0)) if fam in ("patch", "stem") else tuple((m, 0) for m in MODES)


def declined(fam, shape):
    """the one shape conv_f32_split does not take (stride 2 onto an odd output width): modes 3 and 4 fall back to the f32 matrix cores"""
    return fam == "split" and shape[5] == 2 and fe.GEOMS[fam](shape).ow % 2 == 1


def arithmetic(fam, shape, mode):
    """the mode whose kept products the kernel that runs this shape in `mode` sums (f32edges.KEPT)"""
    return 0 if mode == 2 or declined(fam, shape) else mode


def own_launches(fam, shape, mode):
    """how often the family's own kernel must run for this shape in this mode (tests/test_gpu_graph.py test_conv_f32_*_shapes)"""
    if fam == "split":
        h, w, ic, oc, k, st, pad, B, silu = shape
        stem = mode == 3 and ic == 3 and k == 6
        return 1 if mode in (3, 4) and not declined(fam, shape) and not stem else 0
    if fam == "patch":
        return 1 if mode == 3 else 0
    k = shape[4]
    return 1 if mode == 3 and k * k // 2 <= 20 and ((k - 2) // 2) % 2 == 0 else 0


@pytest.fixture
def tuned(gpu):
    gpu.set_tuning("dual_stream_min_batch", 0)  # one launch over the whole batch
    yield gpu
    gpu.set_tuning("f32_mfma", 1)
    gpu.set_tuning("persist_slots", 0)
    gpu.set_tuning("dual_stream_min_batch", 64)


class Runner:
    """a loaded model in one mode; run(frames[, resid]) -> float32 [B][oc * oh * ow], counting the family's kernel"""

    def __init__(self, gpu, fam, case, B, mode, slots=0):
        self.count = getattr(gpu.lib(), "mhip_conv_f32_%s_launches" % fam)
        self.count.restype = C.c_ulong
        gpu.set_tuning("f32_mfma", mode)
        gpu.set_tuning("persist_slots", slots)
        self.m, self.B, self.launched = gpu.Model(case["d"], batch=B), B, None

    def run(self, frames, resid=None):
        for f in range(self.B):
            self.m.input_view(0)[f] = np.ascontiguousarray(frames[f % len(frames)], dtype=np.float32).view(np.uint8)
            if resid is not None:
                self.m.input_view(1)[f] = np.ascontiguousarray(resid[f % len(resid)], dtype=np.float32).view(np.uint8)
        n0 = self.count()
        self.m.run()
        if self.launched is None:  # (the first run: later ones may replay a captured graph, which the host-side counters do not see)
            self.launched = self.count() - n0
        return self.m.output_view(0).copy().view(np.float32)

    def close(self):
        self.m.close()


@pytest.mark.parametrize("cls", fe.EXACT_CLASSES)
@pytest.mark.parametrize("fs", ALL, ids=ids)
def test_exact_classes_bit_for_bit(tuned, fs, cls):
    fam, shape = fs
    g = fe.GEOMS[fam](shape)
    B = batch_of(fam, shape)
    xs, w, bias = fe.exact_operands(cls, g, np.random.default_rng(seed_of(fam, shape, cls)), nframes=2)
    add = fam == "patch" and shape[8]
    rs = [np.random.default_rng(5 + i).integers(-1000, 1001, g.oc * g.oh * g.ow).astype(np.float32) for i in range(2)] if add else None
    want = {m: [fe.expected(g, xs[i], w, bias, m, rs[i] if add else None) for i in range(2)] for m in (0, 3, 4)}
    for s in fe.SCALES:  # (x * 2^-s, w * 2^s): the same expected bits (test_f32_edges_cpu.py checks that claim)
        sx, sw = fe.scaled(xs, w, s)
        case = BUILD[fam](shape, weights=sw, bias=bias, silu=False)
        for mode, slots in runs_of(fam):
            r = Runner(tuned, fam, case, B, mode, slots)
            got = r.run(sx, rs)
            r.close()
            assert r.launched == own_launches(fam, shape, mode), "mode %d: conv_f32_%s launched %d time(s)" % (mode, fam, r.launched)
            for f in range(B):
                ok = fe.same_floats(got[f], want[arithmetic(fam, shape, mode)][f % 2])
                assert ok.all(), "class %s scale 2^%d mode %d slots %d frame %d: %d of %d values differ" % (cls, s, mode, slots, f, int((~ok).sum()), ok.size)


def pair_graph(h, w, ic, oc, weights, biases):
    """C3's cv1 + cv2: two 1 x 1 convolutions over one tensor (tests/test_gpu_graph.py test_conv_f32_pairs, smallest shape), no SiLU"""
    G = marsfile.Graph()
    F, N = marsfile.F32, marsfile.NCHW
    x = G.tensor([1, ic, h, w], dtype=F, fmt=N)
    outs = []
    for wd, bd in zip(weights, biases):
        a = G.tensor([1, oc, h, w], dtype=F, fmt=N)
        wt = G.tensor([oc, ic, 1, 1], dtype=F, fmt=marsfile.OIHW, data=np.ascontiguousarray(wd, dtype=np.float32).reshape(oc, ic, 1, 1))
        b = G.tensor([oc], dtype=F, fmt=marsfile.D1, data=np.ascontiguousarray(bd, dtype=np.float32))
        G.conv(x, a, wt, b, (1, 1), (1, 1))
        outs.append(a)
    return G.serialise([x], outs)


@pytest.mark.parametrize("cls", ["A", "B"])
def test_exact_classes_pair_form(tuned, cls):
    """the pair form of conv_f32_split (one launch, two weight sets) on classes A and B: both outputs bit for bit, modes 3 and 4"""
    h, w, ic, oc, B = 20, 20, 64, 32, 3
    g = fe.Geom(h, w, ic, oc, 1, 1)
    rng = np.random.default_rng(seed_of("pair", (h, w, ic, oc), cls))
    xs, w1, b1 = fe.exact_operands(cls, g, rng, nframes=2)
    _, w2, b2 = fe.exact_operands(cls, g, rng, nframes=1)
    count = tuned.lib().mhip_conv_f32_pair_launches
    count.restype = C.c_ulong
    for s in fe.SCALES:
        sx, sw1 = fe.scaled(xs, w1, s)
        _, sw2 = fe.scaled(xs, w2, s)
        d = pair_graph(h, w, ic, oc, (sw1, sw2), (b1, b2))
        for mode in (3, 4):
            tuned.set_tuning("f32_mfma", mode)
            m = tuned.Model(d, batch=B)
            for f in range(B):
                m.input_view(0)[f] = sx[f % 2].view(np.uint8)
            n0 = count()
            m.run()
            assert count() - n0 == 1, "mode %d: the pair form launched %d time(s)" % (mode, count() - n0)
            got = [m.output_view(k).copy().view(np.float32) for k in range(2)]
            m.close()
            for k, (wk, bk) in enumerate(((w1, b1), (w2, b2))):
                for f in range(B):
                    ok = fe.same_floats(got[k][f], fe.expected(g, xs[f % 2], wk, bk, mode))
                    assert ok.all(), "class %s scale 2^%d mode %d output %d frame %d: %d values differ" % (cls, s, mode, k, f, int((~ok).sum()))


def chain_operands(cls, g1, g2, rng):
    """producer and consumer operands for a conv -> conv chain whose SECOND convolution is of class cls: the producer's output (small
    integers times few +-1 weights) lands in the class's input range -- B: up to 8191, most values with a non-zero mid piece"""
    n = g1.ic * g1.h * g1.w
    xmax, w2 = (15, rng.integers(-15, 16, (g2.oc, g2.ic, g2.k, g2.k))) if cls == "A" else (127, rng.choice(np.array([-2, -1, 1, 2]), (g2.oc, g2.ic, g2.k, g2.k)))
    xs = [rng.integers(-xmax, xmax + 1, n).astype(np.float32) for _ in range(2)]
    w1 = rng.integers(-1, 2, (g1.oc, g1.ic, g1.k, g1.k)).astype(np.float32)
    b1 = (rng.integers(-60, 61, g1.oc) if cls == "A" else rng.integers(2000, 4001, g1.oc) * rng.choice(np.array([-1, 1]), g1.oc)).astype(np.float32)
    b2 = rng.integers(-1000, 1001, g2.oc).astype(np.float32)
    return xs, w1, b1, w2.astype(np.float32), b2


REC = (20, 20, 64, 32, 16, 3)  # h, w, c0 -> (1 x 1) c1 -> (3 x 3) c2, batch: the smallest shape of tests/test_gpu_graph.py test_conv_f32_record_pairs


def rec_graph(w1, b1, w2, b2):
    """-> (file bytes, the tensor between the two convolutions: in record format under f32_mfma = 3)"""
    h, w, c0, c1, c2, B = REC
    G = marsfile.Graph()
    F, N = marsfile.F32, marsfile.NCHW
    x = G.tensor([1, c0, h, w], dtype=F, fmt=N)
    t = G.tensor([1, c1, h, w], dtype=F, fmt=N)
    o = G.tensor([1, c2, h, w], dtype=F, fmt=N)
    f32 = lambda a, shape: np.ascontiguousarray(a, dtype=np.float32).reshape(shape)  # noqa: E731
    G.conv(x, t, G.tensor([c1, c0, 1, 1], dtype=F, fmt=marsfile.OIHW, data=f32(w1, (c1, c0, 1, 1))), G.tensor([c1], dtype=F, fmt=marsfile.D1, data=f32(b1, c1)), (1, 1), (1, 1), pad=marsfile.PAD_SAME)
    G.conv(t, o, G.tensor([c2, c1, 3, 3], dtype=F, fmt=marsfile.OIHW, data=f32(w2, (c2, c1, 3, 3))), G.tensor([c2], dtype=F, fmt=marsfile.D1, data=f32(b2, c2)), (3, 3), (1, 1), pad=marsfile.PAD_SAME)
    return G.serialise([x], [o]), t


def rec_counters(gpu):
    counts = {}
    for name in ("prec", "recin"):
        counts[name] = getattr(gpu.lib(), "mhip_conv_f32_%s_launches" % name)
        counts[name].restype = C.c_ulong
    return lambda: sum(c() for c in counts.values())


def test_non_finite_through_a_record(tuned):
    """+-inf / NaN / +-FLT_MAX in frame 1 of the chain's input: the producer (weights 2 or 3: every channel of that pixel becomes +inf, -inf or
    NaN in every mode) writes them as RECORDS in mode 3 -- a saturated hi piece and the infinity in mid -- and the 3 x 3 reader (weights of one
    sign per output channel) must give sign * inf / NaN on the 3 x 3 pixels around it and the clean bits elsewhere; the tensor between them reads
    back as the expected floats.  Modes 4, 2 and 0 (no records) must agree."""
    h, w, c0, c1, c2, B = REC
    g1, g2 = fe.Geom(h, w, c0, c1, 1, 1), fe.Geom(h, w, c1, c2, 3, 1)
    rng = np.random.default_rng(seed_of("rec", REC, "nonfinite"))
    xs = [rng.integers(-15, 16, c0 * h * w).astype(np.float32) for _ in range(2)]
    w1, b1 = rng.integers(2, 4, (c1, c0)), rng.integers(-60, 61, c1)
    w2 = rng.integers(1, 16, (c2, c1, 3, 3)) * rng.choice(np.array([-1, 1]), (c2, 1, 1, 1))
    b2 = rng.integers(-1000, 1001, c2)
    d, t = rec_graph(w1, b1, w2, b2)
    readers = rec_counters(tuned)
    at = (5 * h + h // 2) * w + w // 2  # channel 5, the centre pixel
    bad = []
    for mode, slots in ((3, 0), (3, 3), (4, 0), (2, 0), (0, 0)):
        tuned.set_tuning("f32_mfma", mode)
        tuned.set_tuning("persist_slots", slots)
        m = tuned.Model(d, batch=B)
        ar = 0 if mode == 2 else mode
        first = True
        for sname, sv in fe.SPECIALS:
            frames = [xs[f % 2] for f in range(B)]
            frames[1] = frames[1].copy()
            frames[1][at] = sv
            for f in range(B):
                m.input_view(0)[f] = frames[f].view(np.uint8)
            n0 = readers()
            m.run()
            if first:
                assert readers() - n0 == (1 if mode == 3 else 0), (mode, readers() - n0)
                first = False
            got = m.output_view(0).copy().view(np.float32)
            for f in range(B):
                model_x = frames[f].copy()
                model_x[np.abs(model_x) == fe.FLT_MAX] *= np.float32(np.inf)  # (times a weight of at least 2: inf in every arithmetic)
                t1, hit1 = fe.with_specials(g1, model_x, w1, lambda q: fe.expected(g1, q, w1, b1, ar))
                want, hit = fe.with_specials(g2, t1.reshape(-1), w2, lambda q: fe.expected(g2, q, w2, b2, ar))
                assert hit.sum() == (9 * c2 if f == 1 else 0) and (np.isnan(sv) or np.isinf(want[hit]).all())
                ok = fe.same_floats(got[f], want)
                back = fe.same_floats(m.read_tensor(t, frame=f).view(np.float32), t1) if f == 1 else ok
                if not (ok.all() and back.all()):
                    bad.append("mode %d slots %d %s frame %d: %d outputs differ, %d values of the tensor between" % (mode, slots, sname, f, int((~ok).sum()), int((~back).sum())))
        m.close()
    assert not bad, "\n".join(bad)


def test_record_write_read_round_trip_at_the_edges(tuned):
    """mars_hip_write_tensor cuts floats into records on the host as the kernels do on the device: a tensor in record format reads back as hi + mid
    -- two-piece rounding (2^20 + 2^10 + 1 loses its last bit: the proof that the tensor IS in record format), +-inf as +-inf (a saturated hi, the infinity
    in mid), +-FLT_MAX as +-inf (hi + mid = 2^128), 2^128 - 2^119 exactly, NaN as NaN"""
    h, w, c0, c1, c2, B = REC
    rng = np.random.default_rng(seed_of("rec", REC, "roundtrip"))
    d, t = rec_graph(rng.integers(-1, 2, (c1, c0)), np.zeros(c1), rng.integers(-2, 3, (c2, c1, 3, 3)), np.zeros(c2))
    tuned.set_tuning("f32_mfma", 3)
    m = tuned.Model(d, batch=B)
    m.run()
    probe = rng.integers(-(1 << 20), 1 << 20, c1 * h * w).astype(np.float32)
    edge = [np.inf, -np.inf, fe.FLT_MAX, -fe.FLT_MAX, 2.0 ** 128 - 2.0 ** 119, -(2.0 ** 128 - 2.0 ** 119), np.nan, 2.0 ** 20 + 2.0 ** 10 + 1, 0.0, -0.0, 2.0 ** -100]
    where = rng.choice(probe.size, len(edge), replace=False)
    probe[where] = np.array(edge, dtype=np.float32)
    m.write_tensor(t, probe.view(np.uint8), frame=1)
    back = m.read_tensor(t, frame=1).view(np.float32)
    m.close()
    want = fe.two_piece(probe)
    assert np.isposinf(want[where[[0, 2]]]).all() and np.isneginf(want[where[[1, 3]]]).all() and want[where[4]] == probe[where[4]] and want[where[7]] != probe[where[7]]
    ok = fe.same_floats(back, want)
    assert ok.all(), "%d values differ; the edge values read back as %r" % (int((~ok).sum()), back[where].tolist())


@pytest.mark.parametrize("cls", ["A", "B"])
def test_exact_classes_record_pair(tuned, cls):
    """1 x 1 -> 3 x 3 with the tensor between them in record format (hi | mid pieces, mode 3: the smallest shape of tests/test_gpu_graph.py
    test_conv_f32_record_pairs, no SiLU): the producer's results here fit two pieces, so the record holds them exactly and the chain must
    equal the integer chain bit for bit -- the record writer's piece order, the reader's LDS-DMA ring, the pieces' pairing; the counters
    prove that mode 3 took a record reader and the other modes did not"""
    h, w, c0, c1, c2, B = REC
    g1, g2 = fe.Geom(h, w, c0, c1, 1, 1), fe.Geom(h, w, c1, c2, 3, 1)
    xs, w1, b1, w2, b2 = chain_operands(cls, g1, g2, np.random.default_rng(seed_of("rec", (h, w, c0, c1, c2), cls)))
    want = {}
    for mode in (0, 3, 4):
        want[mode] = []
        for q in xs:
            t1 = fe.expected(g1, q, w1, b1, mode)
            assert np.array_equal(fe.two_piece(t1), t1) and (cls == "A" or (fe.pieces(t1, 2)[1] != 0).mean() > 0.5)
            want[mode].append(fe.expected(g2, t1.reshape(-1), w2, b2, mode))
    readers_now = rec_counters(tuned)
    for s in fe.SCALES:  # the consumer's operands scaled: (t1 * 2^-s through the producer's weights, w2 * 2^s)
        d, _ = rec_graph(np.ldexp(w1, -s), np.ldexp(b1, -s), np.ldexp(w2, s), b2)
        for mode, slots in ((3, 0), (3, 3), (4, 0), (2, 0), (0, 0)):
            tuned.set_tuning("f32_mfma", mode)
            tuned.set_tuning("persist_slots", slots)
            m = tuned.Model(d, batch=B)
            for f in range(B):
                m.input_view(0)[f] = xs[f % 2].view(np.uint8)
            n0 = readers_now()
            m.run()
            readers = readers_now() - n0
            got = m.output_view(0).copy().view(np.float32)
            m.close()
            assert readers == (1 if mode == 3 else 0), "mode %d: %d record reader launch(es)" % (mode, readers)
            for f in range(B):
                ok = fe.same_floats(got[f], want[0 if mode == 2 else mode][f % 2])
                assert ok.all(), "class %s scale 2^%d mode %d slots %d frame %d: %d values differ" % (cls, s, mode, slots, f, int((~ok).sum()))


NONFINITE = [(fam, shape, name) for fam, shape in SUBSET for name in fe.positions(fe.GEOMS[fam](shape), batch_of(fam, shape), 1)]


@pytest.mark.parametrize("fsp", NONFINITE, ids=lambda v: f32shapes.shape_id(v[0], v[1]) + "-" + v[2])
def test_non_finite_reaches_its_window_only(tuned, fsp):
    """class-A frames (every weight non-zero), one special value in frame 1 (or the first pixel of frame 2): outputs whose true window holds
    it are NaN / sign(w) * inf (+-FLT_MAX: inf in modes 3 and 4, whose hi piece rounds to inf; float32(FLT_MAX * w) in modes 0 and 2), every
    other output of every frame keeps the bits of the clean run"""
    fam, shape, name = fsp
    g = fe.GEOMS[fam](shape)
    B = batch_of(fam, shape)
    xs, w, bias = fe.exact_operands("A", g, np.random.default_rng(seed_of(fam, shape, "A")), nframes=2, nonzero_w=True)
    case = BUILD[fam](shape, weights=w, bias=bias, silu=False)
    pf, c, y, x = fe.positions(g, B, 1)[name]
    clean = {m: [fe.expected(g, xs[i], w, bias, m) for i in range(2)] for m in (0, 3, 4)}
    bad = []
    for mode, slots in runs_of(fam):
        r = Runner(tuned, fam, case, B, mode, slots)
        for sname, sv in fe.SPECIALS:
            frames = [xs[f % 2] for f in range(B)]
            q = frames[pf].copy().reshape(g.ic, g.h, g.w)
            q[c, y, x] = sv
            frames[pf] = q.reshape(-1)
            got = r.run(frames)
            assert r.launched == own_launches(fam, shape, mode), (mode, r.launched)
            for f in range(B):
                want = clean[arithmetic(fam, shape, mode)][f % 2]
                if f == pf:
                    want, hit = fe.poisoned(g, want, w, (c, y, x), sv, arithmetic(fam, shape, mode))
                    assert hit.any() and not hit.all()
                ok = fe.same_floats(got[f], want)
                if not ok.all():
                    a = got[f][~ok.reshape(-1)]
                    bad.append("mode %d slots %d %s frame %d: %d values differ (%d NaN, %d inf among them)" % (
                        mode, slots, sname, f, int((~ok).sum()), int(np.isnan(a).sum()), int(np.isinf(a).sum())))
        r.close()
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("fs", SUBSET, ids=ids)
def test_bound_class(tuned, fs):
    """magnitudes log-uniform over 2^-20 .. 2^20, dense weights: |got - float64 convolution| <= c_mode * (sum |x| |w| + |bias|) per element;
    prints the largest err / bound per mode (DESIGN.md "Float operand edges" records them)"""
    fam, shape = fs
    g = fe.GEOMS[fam](shape)
    B = batch_of(fam, shape)
    xs, w, bias = fe.bound_operands(g, np.random.default_rng(seed_of(fam, shape, "bound")), nframes=2)
    case = BUILD[fam](shape, weights=w, bias=bias, silu=False)
    refs = [fe.ref64(g, q, w, bias) for q in xs]
    worst = {}
    for mode, slots in runs_of(fam):
        r = Runner(tuned, fam, case, B, mode, slots)
        got = r.run(xs)
        r.close()
        assert r.launched == own_launches(fam, shape, mode), (mode, r.launched)
        for f in range(B):
            ref, A = refs[f % 2]
            ratio = np.abs(got[f].astype(np.float64).reshape(ref.shape) - ref) / (fe.c_mode(mode, g.K) * A)
            worst[(mode, slots)] = max(worst.get((mode, slots), 0.0), float(ratio.max()))
    print("f32 bound class %s: max err / bound %s" % (f32shapes.shape_id(fam, shape), " ".join("mode%d/%d=%.4f" % (m, sl, v) for (m, sl), v in worst.items())))
    assert all(np.isfinite(v) and v <= 1.0 for v in worst.values()), worst


# ---- the virtual concat (mars_plan.c virtual_concat_f32, conv_f32_vcat.hip): a 1 x 1 convolution over a float CONCAT that is never
# materialised -- conv_f32_split on a view of the concat's last input, the first pixels of every plane recomputed by the head launch.
# The concat's inputs are 1 x 1 convolutions of ONE channel with single-piece weights and no bias: exact in every mode (one term each), so
# the concat holds the same floats whatever the mode and the reader alone is under test.
VC, vcat_graph = f32shapes.VC, f32shapes.vcat_graph


def vcat_run(gpu, orc, d, cat, xs, modes=MODES):
    """-> (the oracle's concat tensor per frame -- the reader's true operand --, {mode: float32 [B][oc * h * w]}); modes 3 and 4 must plan the view + head launch"""
    B = VC[4]
    cats = []
    for q in xs:
        o = orc.Graph(d)
        o.set_input(0, np.ascontiguousarray(q, dtype=np.float32).tobytes())
        assert o.run() == 0
        cats.append(o.tensor(cat).view(np.float32).copy())
        o.close()
    got = {}
    for mode in modes:
        gpu.set_tuning("f32_mfma", mode)
        virtual = any(" conv_f32_vhead " in l for l in gpu.describe_plan(d))
        assert virtual == (mode in (3, 4)), (mode, virtual)
        m = gpu.Model(d, batch=B)
        for f in range(B):
            m.input_view(0)[f] = np.ascontiguousarray(xs[f % len(xs)], dtype=np.float32).view(np.uint8)
        m.run()
        got[mode] = m.output_view(0).copy().view(np.float32)
        m.close()
    return cats, got


@pytest.mark.parametrize("cls", ["A", "B"])
def test_exact_classes_virtual_concat(tuned, orc, cls):
    h, w, c, oc, B = VC
    g = fe.Geom(h, w, 2 * c, oc, 1, 1)
    rng = np.random.default_rng(seed_of("vcat", VC, cls))
    if cls == "A":
        xs = [rng.integers(-15, 16, h * w).astype(np.float32) for _ in range(2)]
        wa, wb = rng.choice(np.arange(1, 16), c), -rng.choice(np.arange(1, 16), c)
        wr = rng.integers(-15, 16, (oc, 2 * c))
    else:
        xs = [rng.integers(-8191, 8192, h * w).astype(np.float32) for _ in range(2)]
        wa, wb = rng.choice(np.array([-1, 1]), c), rng.choice(np.array([-1, 1]), c)
        wr = rng.choice(np.array([-2, -1, 1, 2]), (oc, 2 * c))
    br = rng.integers(-1000, 1001, oc)
    want = None
    for s in fe.SCALES:  # the reader's operands scaled: the concat through its producers' weights
        d, cat = vcat_graph(np.ldexp(wa.astype(np.float32), -s), np.ldexp(wb.astype(np.float32), -s), np.ldexp(wr.astype(np.float32), s), br)
        cats, got = vcat_run(tuned, orc, d, cat, xs)
        if want is None:  # (the concat holds at most two pieces per value and the weights one: every mode keeps the full product)
            assert cls == "A" or (fe.pieces(cats[0], 2)[1] != 0).mean() > 0.1
            want = [fe.expected(g, q, wr, br, 3) for q in cats]
            assert all(np.array_equal(fe.expected(g, q, wr, br, 0), wq) for q, wq in zip(cats, want))
        for mode in MODES:
            for f in range(B):
                ok = fe.same_floats(got[mode][f], want[f % 2])
                assert ok.all(), "class %s scale 2^%d mode %d frame %d: %d values differ" % (cls, s, mode, f, int((~ok).sum()))


VC_WHERE = {"head-pixel": (1, 2), "interior": (1, (VC[0] // 2) * VC[1] + VC[1] // 2), "top-left": (1, 0), "top-right": (1, VC[1] - 1),
            "bottom-left": (1, (VC[0] - 1) * VC[1]), "frame-last": (1, VC[0] * VC[1] - 1), "next-frame-first": (2, 0)}  # (frame, pixel of the graph input)


@pytest.mark.parametrize("where", list(VC_WHERE))
def test_non_finite_through_the_virtual_concat(tuned, orc, where):
    """one +-inf / NaN / +-FLT_MAX in the graph input: among the head launch's pixels, behind them, at the corners, as the last pixel of frame 1
    (the end of the shifted planes and the head launch's extra plane) and the first of frame 2 (the first pixel behind the head pixels, the
    frame boundary of the view).  The producers' weights are at least 2 in magnitude, so that they carry the value into every channel of its
    pixel as +-inf in every mode (FLT_MAX * 2 overflows whatever the arithmetic); the byte-wise concat copies some of those, and the reader must
    give NaN / +-inf exactly where its true operand -- the oracle's concat tensor -- says, and the clean bits everywhere else, in every frame."""
    h, w, c, oc, B = VC
    g = fe.Geom(h, w, 2 * c, oc, 1, 1)
    rng = np.random.default_rng(seed_of("vcat", VC, where))
    xs = [rng.integers(-15, 16, h * w).astype(np.float32) for _ in range(B)]
    wa, wb = rng.choice(np.arange(2, 16), c), -rng.choice(np.arange(2, 16), c)
    wr = rng.integers(-15, 16, (oc, 2 * c))
    wr = np.where(wr == 0, 7, wr)
    br = rng.integers(-1000, 1001, oc)
    d, cat = vcat_graph(wa, wb, wr, br)
    pf, px = VC_WHERE[where]
    bad = []
    for sname, sv in fe.SPECIALS:
        frames = [q.copy() for q in xs]
        frames[pf][px] = sv
        cats, got = vcat_run(tuned, orc, d, cat, frames)
        for f in range(B):
            want, hit = fe.with_specials(g, cats[f], wr, lambda q: fe.expected(g, q, wr, br, 0))
            assert hit.any() == (f == pf) and not hit.all(), (sname, f)
            for mode in MODES:
                ok = fe.same_floats(got[mode][f], want)
                if not ok.all():
                    bad.append("mode %d %s frame %d: %d values differ" % (mode, sname, f, int((~ok).sum())))
    assert not bad, "\n".join(bad)


def test_bound_class_virtual_concat(tuned, orc):
    """the concat holds +-m 2^e (m <= 15, e in -20 .. 20: exact products of the one-channel producers), the reader's weights are log-uniform
    over 2^-20 .. 2^20: the bound class on the view + head launch"""
    h, w, c, oc, B = VC
    g = fe.Geom(h, w, 2 * c, oc, 1, 1)
    rng = np.random.default_rng(seed_of("vcat", VC, "bound"))
    xs = [(np.exp2(rng.integers(-20, 21, h * w)) * rng.choice(np.array([-1.0, 1.0]), h * w)).astype(np.float32) for _ in range(2)]
    wa, wb = rng.choice(np.arange(1, 16), c), -rng.choice(np.arange(1, 16), c)
    _, wr, br = fe.bound_operands(g, rng, nframes=1)
    d, cat = vcat_graph(wa, wb, wr, br)
    cats, got = vcat_run(tuned, orc, d, cat, xs)
    worst = {}
    for mode in MODES:
        for f in range(B):
            ref, A = fe.ref64(g, cats[f % 2], wr, br)
            ratio = np.abs(got[mode][f].astype(np.float64).reshape(ref.shape) - ref) / (fe.c_mode(mode, g.K) * A)
            worst[mode] = max(worst.get(mode, 0.0), float(ratio.max()))
    print("f32 bound class virtual concat: max err / bound %s" % " ".join("mode%d=%.4f" % kv for kv in worst.items()))
    assert all(np.isfinite(v) and v <= 1.0 for v in worst.values()), worst


SILU = [("split", (32, 32, 32, 32, 1, 1, "same", 2, True)), ("patch", (40, 40, 32, 32, 3, 1, 2, True, False)), ("stem", (128, 192, 3, 32, 6, 3, True))]


@pytest.mark.parametrize("fs", SILU, ids=ids)
def test_silu_sweep(tuned, orc, fs):
    """the fused SiLU of each kernel that has silu_fast, through one-hot weights (the pre-activation is one input value, exact): v over EVERY normal
    bf16 value with |v| <= 104 -- 2^-126 upward, where a rescaled form loses bits, to -104, where the exponential has overflowed -- and +-0
    (f32edges.silu_grid says why bf16 subnormals are left out); the test asserts that every one of them is a pre-activation of some output.
    Mode 3 against float64 v / (1 + exp(-v)) within 2^-23 (|v| + 4) relative + 2^-120; mode 4 (the libm-exact form) equal to the oracle bit for bit."""
    fam, shape = fs
    g = fe.GEOMS[fam](shape)
    B = batch_of(fam, shape)
    grid = fe.silu_grid()
    rng = np.random.default_rng(3)
    n = g.ic * g.h * g.w
    assert B * n >= grid.size
    xs = [rng.permutation(np.resize(grid, n)).astype(np.float32) for _ in range(B)] if fam == "stem" else np.split(rng.permutation(np.resize(grid, B * n)).astype(np.float32), B)
    w = fe.one_hot_weights(g)
    case = BUILD[fam](shape, weights=w, bias=np.zeros(g.oc, dtype=np.float32), silu=True)
    pre = [g.conv(q, w) for q in xs]  # exact: one term each
    seen = np.unique(np.concatenate([p.reshape(-1) for p in pre]))  # (-0 arrives as +0: the accumulator starts at a +0 bias)
    assert np.isin(grid.astype(np.float64), seen).all(), "%d grid values reach no output" % int((~np.isin(grid.astype(np.float64), seen)).sum())
    oracle = []
    for q in xs:
        o = orc.Graph(case["d"])
        o.set_input(0, q.tobytes())
        assert o.run() == 0
        oracle.append(o.tensor(case["out"]).view(np.float32).copy())
        o.close()
    for mode in (3, 4):
        r = Runner(tuned, fam, case, B, mode)
        got = r.run(xs)
        r.close()
        assert r.launched == own_launches(fam, shape, mode), (mode, r.launched)
        for f in range(B):
            if mode == 4:
                ok = fe.same_floats(got[f], oracle[f])
                assert ok.all(), "mode 4 frame %d: %d values differ from the oracle" % (f, int((~ok).sum()))
                continue
            v = pre[f].reshape(-1)
            err = np.abs(got[f].astype(np.float64) - fe.silu64(v))
            ratio = err / fe.silu_fast_bound(v)
            small = np.abs(v) < 2.0 ** -20
            i, j = int(np.argmax(ratio)), int(np.argmax(np.where(small, ratio, -1)))
            print("f32 silu_fast %s frame %d: max err / bound %.4f at v = %r; below 2^-20: %.4f at v = %r" % (fam, f, ratio[i], float(v[i]), ratio[j], float(v[j])))
            assert np.isfinite(got[f]).all() and ratio[i] <= 1.0, "frame %d: v = %r got %r want %r" % (f, float(v[i]), float(got[f][i]), float(fe.silu64(v[i])))
