"""tests/moveref.py pinned, without a GPU: for every pool, concat and upsample case of tests/test_gpu_move.py the one-layer graph (NHWC, or
NCHW-tagged for the *_nchwq cases) runs on the CPU oracle -- and on the compiled reference where it was built -- and moveref has to give the
same bytes for every frame.  Then the cases themselves: no pool case may pass with a window one row or column off, and no case of the
binary_i8 layout test sits on a rounding tie."""
import numpy as np
import pytest

import marsfile
import moveref as R
import test_gpu_move as T

I8 = np.int8


@pytest.fixture(params=["oracle", "reference"])
def engine(request):
    """a graph runner: the restated oracle, or the reference's own layer functions (skipped where oracle/_ref was not built)"""
    if request.param == "oracle":
        return request.getfixturevalue("orc").Graph
    return request.getfixturevalue("ref").O2Model


def run_graph(engine, d, inputs, tensors):
    g = engine(d)
    for i, x in enumerate(inputs):
        g.set_input(i, np.asarray(x).tobytes())
    assert g.run() == 0
    out = [g.tensor(t).view(I8) for t in tensors]
    g.close()
    return out


def pool_graph(fmt, in_h, in_w, ch, out_h, out_w, kh, kw, sh, sw, n=1):
    G = marsfile.Graph()
    x = G.tensor([1, in_h, in_w, ch], fmt=fmt)
    outs, cur = [], x
    for _ in range(n):
        o = G.tensor([1, out_h, out_w, ch], fmt=fmt)
        G.pool(cur, o, (kh, kw), (sh, sw))
        outs.append(o)
        cur = o
    return G.serialise([x], outs), outs


def same(what, got, want):
    got, want = np.asarray(got).view(np.uint8), np.asarray(want).view(np.uint8)
    assert got.shape == want.shape and np.array_equal(got, want), (what, int((got != want).sum()) if got.shape == want.shape else (got.shape, want.shape))


# ---- moveref against the oracle / the reference -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", list(T.MAXPOOL))
def test_maxpool_cases(engine, cid):
    args = T.MAXPOOL[cid][0]
    d, outs = pool_graph(marsfile.NHWC, *args)
    for f, (x, want) in enumerate(zip(T.maxpool_frames(cid), T.maxpool_want(cid))):
        same((cid, f), run_graph(engine, d, [x], outs)[0], want)


@pytest.mark.parametrize("case", T.POOL_CHAIN, ids=T.name_of)
def test_pool_chain_cases(engine, case):
    h, w, ch, kh, kw, n, frames = case
    d, outs = pool_graph(marsfile.NHWC, h, w, ch, h, w, kh, kw, 1, 1, n)
    want = T.chain_want(case)
    for f, x in enumerate(T.chain_frames(case)):
        got = run_graph(engine, d, [x], outs)
        for i in range(n):
            same((case, "stage", i, "frame", f), got[i], want[i][f])


@pytest.mark.parametrize("cid", list(T.MAXPOOLQ))
def test_maxpool_nchwq_cases(engine, cid):
    """[1, C, H, W] tagged NCHW: kh runs over channels, kw over map rows -- this comparison is what fixes that reading"""
    c, h, w, kh, kw = T.MAXPOOLQ[cid]
    d, outs = pool_graph(marsfile.NCHW, c, h, w, c, h, kh, kw, 1, 1)
    for f, x in enumerate(T.maxpoolq_frames(cid)):
        want = R.maxpool_q(x, c, h, w, kh, kw)
        same((cid, f), run_graph(engine, d, [x], outs)[0], want)
        same((cid, f, "pixels x channels and back"), R.from_pxc(R.to_pxc(want, c, h, w), c, h, w), want)


@pytest.mark.parametrize("cid", list(T.CONCAT))
def test_concat_slice_cases(engine, cid):
    """the slice under test as one input of a whole CONCAT: inputs of ch_off, in_c (and the rest of out_c, if any) channels"""
    (out_h, out_w, in_c, out_c, ch_off), _ = T.CONCAT[cid]
    parts = ([ch_off] if ch_off else []) + [in_c] + ([out_c - ch_off - in_c] if out_c > ch_off + in_c else [])
    assert sum(parts) == out_c and 1 <= len(parts) <= 4
    k_under_test = 1 if ch_off else 0
    G = marsfile.Graph()
    ins = [G.tensor([1, out_h, out_w, c]) for c in parts]
    o = G.tensor([1, out_h, out_w, out_c])
    G.concat(ins, o)
    d = G.serialise(ins, [o])
    npix = out_h * out_w
    for f in range(T.COPY_FRAMES):
        xs = [T.copy_frames(cid, T.COPY_FRAMES, npix * c, 0 if k == k_under_test else 1 + k)[f] for k, c in enumerate(parts)]
        got = run_graph(engine, d, xs, [o])[0]
        same((cid, f), got, R.concat(xs, parts, out_h, out_w, out_c))
        alone = np.full(npix * out_c, T.SENT, dtype=np.uint8).view(I8)  # the GPU test's expectation: this slice alone in a sentinel buffer
        R.concat_slice(alone, xs[k_under_test], out_h, out_w, in_c, out_c, ch_off)
        mine = np.zeros(npix * out_c, dtype=bool).reshape(npix, out_c)
        mine[:, ch_off:ch_off + in_c] = True
        same((cid, f, "slice"), alone[mine.reshape(-1)], got[mine.reshape(-1)])
        assert (alone[~mine.reshape(-1)].view(np.uint8) == T.SENT).all()


@pytest.mark.parametrize("case", T.CONCATQ, ids=T.name_of)
def test_concat_nchwq_cases(engine, case):
    in_cs, H, W, _ = case
    G = marsfile.Graph()
    ins = [G.tensor([1, c, H, W], fmt=marsfile.NCHW) for c in in_cs]
    o = G.tensor([1, sum(in_cs), H, W], fmt=marsfile.NCHW)
    G.concat(ins, o, axis=1)
    d = G.serialise(ins, [o])
    for f, xs in enumerate(T.concatq_frames(case)):
        want = R.concat_q(xs, in_cs, H, W)
        same((case, f), run_graph(engine, d, xs, [o])[0], want)
        # the flat rule the kernel's comment states: out[f + k W] = in_k[f], later inputs win, zeros behind an input's end
        flat = np.zeros(len(want) + len(in_cs) * W, dtype=I8)
        for k, x in enumerate(xs):
            src = np.zeros(len(want), dtype=I8)
            src[:len(x)] = x
            flat[k * W:k * W + len(want)] = src
        same((case, f, "flat rule"), flat[:len(want)], want)


@pytest.mark.parametrize("cid", list(T.UPSAMPLE))
def test_upsample_cases(engine, cid):
    (in_h, in_w, ch, out_h, out_w, sh, sw), _ = T.UPSAMPLE[cid]
    G = marsfile.Graph()
    x = G.tensor([1, in_h, in_w, ch])
    o = G.tensor([1, out_h, out_w, ch])
    G.upsample(x, o, sh, sw)
    d = G.serialise([x], [o])
    for f, v in enumerate(T.copy_frames(cid, T.COPY_FRAMES, in_h * in_w * ch)):
        same((cid, f), run_graph(engine, d, [v], [o])[0], R.upsample(v, in_h, in_w, ch, out_h, out_w, sh, sw))


@pytest.mark.parametrize("cid", list(T.UPSAMPLEQ))
def test_upsample_nchwq_cases(engine, cid):
    (ci, hi, wi), (co, ho, wo), sh, sw = T.UPSAMPLEQ[cid]
    G = marsfile.Graph()
    x = G.tensor([1, ci, hi, wi], fmt=marsfile.NCHW)
    o = G.tensor([1, co, ho, wo], fmt=marsfile.NCHW)
    G.upsample(x, o, sh, sw)
    d = G.serialise([x], [o])
    for f, v in enumerate(T.copy_frames(cid, T.COPY_FRAMES, ci * hi * wi)):
        want = R.upsample_q(v, ci, hi, wi, co, ho, wo, sh, sw)
        assert len(want) == co * ho * wo and not want[co * ho * wi:].any()  # behind the written extent: 0
        same((cid, f), run_graph(engine, d, [v], [o])[0], want)


# ---- moveref's own helpers, by hand -------------------------------------------------------------------------------------------------------------
def test_layout_helpers_by_hand():
    x = np.arange(24, dtype=I8)  # C = 2, H = 3, W = 4: element (c, h, w) = 12 c + 4 h + w
    p = R.to_pxc(x, 2, 3, 4)
    assert p.tolist()[:6] == [0, 12, 1, 13, 2, 14] and p[2 * (1 * 4 + 2) + 1] == 12 + 4 + 2
    assert np.array_equal(R.from_pxc(p, 2, 3, 4), x)
    r = R.nchw_to_nhwc_pad(np.arange(6, dtype=I8), 2, 3, 4)  # [2][3] -> [3][4]
    assert r.tolist() == [0, 3, 0, 0, 1, 4, 0, 0, 2, 5, 0, 0]
    assert R.unpad_rows(np.arange(12, dtype=I8), 3, 2, 4).tolist() == [0, 1, 4, 5, 8, 9]
    dst = np.full(12, 90, dtype=I8)
    R.place(dst, np.array([1, 2, 3, 4], dtype=I8), 2, 2, 6, 3)
    assert dst.tolist() == [90, 90, 90, 1, 2, 90, 90, 90, 90, 3, 4, 90]
    # pool: 1 x 3 map of one channel, window 1 x 2, clipped at the right edge; an empty window (map of height 0 rows read) is -128
    assert R.maxpool(np.array([5, -7, -128], dtype=I8), 1, 3, 1, 1, 3, 1, 2, 1, 1).tolist() == [5, -7, -128]
    assert R.maxpool(np.array([-1, 0, 127, -128], dtype=I8), 2, 2, 1, 1, 1, 2, 2, 1, 1).tolist() == [127]
    # upsample: 1 x 2 -> 1 x 5 by 2: columns 0 0 1 1 and the clamp
    assert R.upsample(np.array([7, 9], dtype=I8), 1, 2, 1, 1, 5, 1, 2).tolist() == [7, 7, 9, 9, 9]
    # concat: two inputs of 1 and 2 channels, 2 pixels; the second input one byte short reads 0
    assert R.concat([np.array([1, 2], dtype=I8), np.array([3, 4, 5], dtype=I8)], [1, 2], 1, 2, 3).tolist() == [1, 3, 4, 2, 5, 0]


def test_pool_frame_kinds():
    x = R.pool_frames(5, 3, 6, 5, 16)
    assert len({v.tobytes() for v in x}) == 3
    peaks = x[1]
    assert 1 <= (peaks != -128).sum() <= 12 and peaks[peaks != -128].min() >= -100
    signs = x[2].reshape(30, 16)
    assert set(signs.reshape(-1).tolist()) == {-128, 127, -1, 0, 1}
    assert signs[0, :5].view(np.uint8).tolist() == [0x80, 0x7F, 0xFF, 0x00, 0x01] and signs[1, 0] == 127 and signs[0, 5] == -128
    for c in range(16):  # one channel meets both signs in any two neighbouring pixels
        assert len(set(signs[:5, c].tolist())) == 5


# ---- the cases bite ---------------------------------------------------------------------------------------------------------------------------
def mutations(k, extent):
    """a window extent one less (k > 1 and k <= the map's extent) and one more (k + 1 <= the map's extent)"""
    return ([k - 1] if k > 1 and k <= extent else []) + ([k + 1] if k + 1 <= extent else [])


def assert_window_bites(what, frames, pool, kh, kw, ext_h, ext_w):
    """pool(x, kh, kw) -> bytes.  Every mutated window must change at least one output byte on the case's own frames"""
    want = [pool(x, kh, kw) for x in frames]
    tried = 0
    for mkh, mkw in [(m, kw) for m in mutations(kh, ext_h)] + [(kh, m) for m in mutations(kw, ext_w)]:
        got = [pool(x, mkh, mkw) for x in frames]
        changed = sum(int((np.asarray(g) != np.asarray(w)).sum()) for g, w in zip(got, want))
        assert changed > 0, "%s would pass with a %d x %d window in place of %d x %d" % (what, mkh, mkw, kh, kw)
        tried += 1
    return tried


@pytest.mark.parametrize("cid", list(T.MAXPOOL))
def test_maxpool_cases_tell_windows_apart(cid):
    in_h, in_w, ch, out_h, out_w, kh, kw, sh, sw = T.MAXPOOL[cid][0]
    assert_window_bites(cid, T.maxpool_frames(cid), lambda x, a, b: R.maxpool(x, in_h, in_w, ch, out_h, out_w, a, b, sh, sw), kh, kw, in_h, in_w)


@pytest.mark.parametrize("case", T.POOL_CHAIN, ids=T.name_of)
def test_pool_chain_cases_tell_windows_apart(case):
    h, w, ch, kh, kw, n, frames = case

    def chain(x, a, b):
        return np.concatenate([s[0] for s in T.chain_want(case, [x], a, b)])

    assert_window_bites(case, T.chain_frames(case), chain, kh, kw, h, w)


@pytest.mark.parametrize("cid", list(T.MAXPOOLQ))
def test_maxpool_nchwq_cases_tell_windows_apart(cid):
    c, h, w, kh, kw = T.MAXPOOLQ[cid]
    assert_window_bites(cid, T.maxpoolq_frames(cid), lambda x, a, b: R.maxpool_q(x, c, h, w, a, b), kh, kw, c, h)


def test_copy_case_frames_all_differ():
    """a seed of its own per frame and per input: no mix-up of frames or inputs can cancel"""
    for case in T.CONCATQ:
        xs = [x.tobytes()[:16 * case[1] * case[2]] for per_frame in T.concatq_frames(case) for x in per_frame]
        assert len(set(xs)) == len(xs), case
    for cid in list(T.CONCAT) + list(T.UPSAMPLE):
        assert len({x.tobytes() for x in T.copy_frames(cid, T.COPY_FRAMES, 48)}) == T.COPY_FRAMES


@pytest.mark.parametrize("is_mul", [0, 1], ids=["add", "mul"])
@pytest.mark.parametrize("cid", list(T.BINARY))
def test_binary_i8_cases_have_no_ties(orc, cid, is_mul):
    """binary_case asserts the distance to a tie itself; here also: the plain formula is the oracle's MUL / ADD on those bytes"""
    a, b, want = T.binary_case(cid, is_mul)
    n = len(a[0])
    G = marsfile.Graph()
    F = np.float32
    ta, tb = G.tensor([1, 1, 1, n], scale=float(F(T.BIN_SA))), G.tensor([1, 1, 1, n], scale=float(F(T.BIN_SB)))
    to = G.tensor([1, 1, 1, n], scale=0.0675)
    G.layer(marsfile.MUL if is_mul else marsfile.ADD, [ta, tb], [to])
    d = G.serialise([ta, tb], [to])
    assert abs(float(F(1.0) / F(0.0675)) - T.BIN_INV) < 1e-5
    for f in range(T.COPY_FRAMES):
        same((cid, is_mul, f), run_graph(orc.Graph, d, [a[f], b[f]], [to])[0], want[f])
