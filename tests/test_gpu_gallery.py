"""Gallery match on the device (include/mars_hip.h, "Gallery match"): mars_yolo_match_vectors over channel counts, gallery sizes around the
launcher's chunk length, query counts and top_k; ties across chunks; the extremes of the arithmetic; the device's 1 / sqrtf over a sweep of
qq; the threshold; the pooled sums of a loaded model; the chain detector -> crops -> second model -> classify -> match -> identities per
detection, and its ordering.  The expected values come from the numpy restatement of tests/test_gallery_cpu.py (checked there by hand);
every comparison is bit-exact."""
import numpy as np
import pytest

import cases
from conftest import lcg_frame
from test_gallery_cpu import F, ident_np, match_np, quantise_np
from test_gpu_classify import head_graph
from test_gpu_roi import FRAME_SEED, Chain, second_stage

pytestmark = pytest.mark.gpu


def same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert got.tobytes() == want.tobytes(), (what, got.reshape(-1)[:8], want.reshape(-1)[:8])


def vectors(seed, n, c, shift=0):
    """cases.i8 bytes widened to int32 (shift: a common factor, which the rule ignores)"""
    return (cases.i8(seed, n * c).astype(np.int32) << shift).reshape(n, c)


def gallery_of(gpu, rows_i32, ids=None, capacity=None):
    c = rows_i32.shape[1]
    g = gpu.Gallery(c, capacity or len(rows_i32))
    ids = np.arange(len(rows_i32), dtype=np.int32) * 3 + 5 if ids is None else ids
    g.add(rows_i32, ids)
    assert g.count() == len(rows_i32)
    return g, np.asarray(ids, dtype=np.int32)


def check(gpu, g, gal, ids, q, ks, what, min_score=0.0):
    c = gal.shape[1]
    want, want_rows = match_np(gal, ids, q, c, 8, min_score)
    for k in ks:
        top, rows = gpu.match_vectors(g, q, gpu.match_opts(top_k=k, min_score=min_score))
        same(rows, np.ascontiguousarray(want_rows[:, :k]), (what, k, "rows"))
        same(top, np.ascontiguousarray(want[:, :k]), (what, k))
    return want, want_rows


CH = None


def chunk(gpu):
    global CH
    if CH is None:
        CH = gpu.match_chunk(1)
        assert gpu.match_chunk(CH + 1) == CH and gpu.match_chunk(3 * CH + 5) == CH
    return CH


# (C, G, N): every C, G and N of the lists once at least; G = None: one chunk + 1, G = -1: three chunks + 5
# (the last two: more than one tile of 64 queries over more than one chunk, with the queries in registers and without)
SHAPES = [(1, 3, 3), (5, 1, 1), (5, 17, 17), (64, 16, 65), (64, None, 17), (65, -1, 3), (81, 17, 65), (4096, 3, 3), (4096, 16, 17),
          (64, -1, 65), (81, None, 65)]


@pytest.mark.parametrize("shape", SHAPES, ids=["c%d_g%s_n%d" % s for s in SHAPES])
def test_match_vectors(gpu, shape):
    c, G, n = shape
    G = chunk(gpu) + 1 if G is None else 3 * chunk(gpu) + 5 if G == -1 else G
    gal = vectors(0x6A110000 + c, G, c, shift=c % 7)
    gal[np.abs(gal).max(axis=1) == 0, 0] = 1  # (no null rows: C = 1 meets a zero byte now and then)
    q = vectors(0x6A120000 + c * 3 + n, n, c, shift=11)
    g, ids = gallery_of(gpu, gal)
    want, rows = check(gpu, g, gal, ids, q, (1, 3, 8), shape)
    if G < 8:  # fewer rows than top_k: the entries behind the last row are empty
        assert (rows[:, G:] == -1).all() and (want["cls"][:, G:] == -1).all() and (want["score"][:, G:] == 0).all()
    top, _ = gpu.match_vectors(g, q)  # no options: top_k = 1
    same(top, np.ascontiguousarray(want[:, :1]), (shape, "default options"))
    g.close()


def test_ties_come_back_in_row_order_across_chunks(gpu):
    """the same row at index 2, at the last index of chunk 0 and at the first of chunk 1: equal keys, returned as rows 2, ch - 1, ch"""
    ch = chunk(gpu)
    gal = vectors(0x6A130000, ch + 40, 64)
    hit = gal[2].copy()
    gal[ch - 1] = hit
    gal[ch] = hit * 3  # the same direction: the same int8 row
    q = np.stack([hit, vectors(0x6A130001, 1, 64)[0], -hit])
    g, ids = gallery_of(gpu, gal)
    want, rows = check(gpu, g, gal, ids, q, (3, 8), "ties")
    assert rows[0, :3].tolist() == [2, ch - 1, ch] and want["score"][0, 0] == want["score"][0, 1] == want["score"][0, 2]
    assert (want["score"][2] <= 0).all() or set(rows[2].tolist()).isdisjoint({2, ch - 1, ch})  # the negated query: those rows rank last
    top, r = gpu.match_vectors(g, q, gpu.match_opts(top_k=8))
    assert r[0, :3].tolist() == [2, ch - 1, ch] and top["score"][0, 0] == top["score"][0, 1] == top["score"][0, 2]
    g.close()


def test_extremes(gpu):
    """all-(+max) query and row at C = 4096: dot = 127 * 127 * 4096 = 66 064 384, above 2^24; the negated row last; a null query between
    two real ones"""
    c = 4096
    gal = np.stack([np.full(c, 2 ** 31 - 1, dtype=np.int32), vectors(0x6A140000, 1, c)[0], np.full(c, -2 ** 31, dtype=np.int32)])
    q = np.stack([np.full(c, 77, dtype=np.int32), np.zeros(c, dtype=np.int32), vectors(0x6A140001, 1, c)[0]])
    g, ids = gallery_of(gpu, gal)
    want, rows = check(gpu, g, gal, ids, q, (1, 3, 8), "extremes")
    assert quantise_np(gal[:1], c)[1][0] == 66064384
    assert rows[0, :3].tolist() == [0, 1, 2] and abs(float(want["score"][0, 0]) - 1.0) < 1e-6 and abs(float(want["score"][0, 2]) + 1.0) < 1e-6
    assert (rows[1] == -1).all() and (want["cls"][1] == -1).all() and (want["score"][1] == 0).all()  # the null query
    assert (rows[2, :3] >= 0).all()
    alone, _ = gpu.match_vectors(g, q[2:], gpu.match_opts(top_k=3))  # its neighbour is unaffected by it
    same(alone, np.ascontiguousarray(want[2:, :3]), "beside a null query")
    g.close()


def test_square_root_sweep(gpu):
    """qinv = 1.0f / sqrtf((float)qq) on the device over more than 1000 distinct qq: C = 2 queries (127 k, t k), t = 0 .. 127, and 1000
    random C = 64 queries, each against one fixed row; the scores equal numpy's correctly rounded ones"""
    seen = set()
    for c, q in ((2, np.array([[127 * (t % 5 + 1), t * (t % 5 + 1)] for t in range(128)], dtype=np.int32)),
                 (64, np.random.default_rng(0x6A15).integers(-2 ** 20, 2 ** 20, (1000, 64)).astype(np.int32))):
        gal = vectors(0x6A150000 + c, 1, c)
        gal[0, 0] = 100
        g, ids = gallery_of(gpu, gal)
        check(gpu, g, gal, ids, q, (1,), ("sqrt", c))
        seen |= {(c, int(x)) for x in quantise_np(q, c)[1]}
        g.close()
    assert len(seen) >= 1000


def test_threshold_at_a_returned_score(gpu):
    gal, q = vectors(0x6A160000, 40, 64), vectors(0x6A160001, 3, 64)
    g, ids = gallery_of(gpu, gal)
    want, rows = check(gpu, g, gal, ids, q, (8,), "no threshold")
    pos = [(i, k) for i in range(3) for k in range(8) if want["score"][i, k] > 0]
    i, k = pos[len(pos) // 2]
    s = want["score"][i, k]
    at, at_rows = check(gpu, g, gal, ids, q, (8,), "at the score", min_score=s)
    assert at_rows[i, k] == rows[i, k] and at["score"][i, k] == s  # kept
    up = np.nextafter(s, F(2))
    above, above_rows = check(gpu, g, gal, ids, q, (8,), "above the score", min_score=up)
    assert above_rows[i, k] == -1 and above["cls"][i, k] == -1 and above["score"][i, k] == 0
    g.close()


def test_gallery_lifecycle_and_refusals_on_the_device(gpu):
    BAD_FILE, BAD_TENSOR = gpu.MARS_ERR_INVALID_FILE, gpu.MARS_ERR_INVALID_TENSOR

    def refused(code, fn, *a, **kw):
        with pytest.raises(gpu.MarsError) as ei:
            fn(*a, **kw)
        assert ei.value.code == code

    g = gpu.Gallery(5, 4)
    assert g.count() == 0
    refused(BAD_TENSOR, gpu.match_vectors, g, np.ones((1, 5), dtype=np.int32))          # an empty gallery
    refused(BAD_FILE, g.add, np.ones((2, 5), dtype=np.int32), [1, -1])                  # a negative id
    refused(BAD_TENSOR, g.add, np.array([[1, 2, 3, 4, 5], [0, 0, 0, 0, 0]]), [1, 2])    # a null vector
    assert g.count() == 0                                                               # all or none
    g.add(vectors(0x6A170000, 3, 5), [7, 7, 9])                                         # rows may share an id
    refused(BAD_TENSOR, g.add, vectors(0x6A170001, 2, 5), [1, 2])                       # more rows than the capacity holds
    assert g.count() == 3
    top, rows = gpu.match_vectors(g, vectors(0x6A170000, 3, 5), gpu.match_opts(top_k=2))
    assert rows[:, 0].tolist() == [0, 1, 2] and top["cls"][:, 0].tolist() == [7, 7, 9]
    g.clear()
    assert g.count() == 0
    g.add(vectors(0x6A170002, 4, 5), [1, 2, 3, 4])
    same(gpu.match_vectors(g, vectors(0x6A170003, 2, 5), gpu.match_opts(top_k=8))[0],
         match_np(vectors(0x6A170002, 4, 5), [1, 2, 3, 4], vectors(0x6A170003, 2, 5), 5, 8)[0], "after clear")
    g.close()


# ---- through a model ---------------------------------------------------------------------------------------------------------------------
def test_match_through_a_model(gpu):
    """the head of a loaded model at batch 3: classify_device -> match_device -> match_results equals the restatement on classify_results'
    sums; again after two more rows were added"""
    C_ = 81
    d, mid, out = head_graph(C_, False)
    m = gpu.Model(d, batch=3)
    nb = m.input_view(0).shape[1]
    for f in range(3):
        m.input_view(0)[f] = lcg_frame(0x6A180000 + f, nb)
    m.run()
    gal = vectors(0x6A180010, 20, C_, shift=4)
    g, _ = gallery_of(gpu, gal[:18], ids=np.arange(18) + 100, capacity=32)
    other = gpu.Gallery(64, 4)
    other.add(vectors(1, 1, 64), [0])
    with pytest.raises(gpu.MarsError) as ei:
        m.match_results(3)  # nothing pending
    assert ei.value.code == gpu.MARS_ERR_INVALID_TENSOR
    with pytest.raises(gpu.MarsError) as ei:
        m.match_device(g, top_k=3)  # no classify results
    assert ei.value.code == gpu.MARS_ERR_INVALID_TENSOR
    m.classify_device(top_k=3)
    with pytest.raises(gpu.MarsError) as ei:
        m.match_device(other, top_k=3)  # 64 channels against C = 81
    assert ei.value.code == gpu.MARS_ERR_INVALID_TENSOR
    m.match_device(g, top_k=3)
    with pytest.raises(ValueError):
        m.match_results(1)  # the library would copy 3 entries per frame into arrays of 1
    top, rows = m.match_results(3)
    assert m.match_results()[0].tobytes() == top.tobytes()  # sized by the enqueued top_k
    _, sums = m.classify_results(3)
    want, want_rows = match_np(gal[:18], np.arange(18) + 100, sums, C_, 3)
    same(top, want, "model")
    same(rows, want_rows, "model rows")
    sums[1] = sums[1] * 0 + gal[19] * 5  # a query that will find row 19 once it is enrolled
    g.add(gal[18:], [300, 301])
    assert g.count() == 20
    m.classify_device(top_k=3)
    top2, rows2 = m.match(g, top_k=8, min_score=0.05)
    _, sums2 = m.classify_results(3)
    want2, want_rows2 = match_np(gal, list(range(100, 118)) + [300, 301], sums2, C_, 8, 0.05)
    same(top2, want2, "after add")
    same(rows2, want_rows2, "after add, rows")
    t, r = gpu.match_vectors(g, sums[1:2])
    assert r.tolist() == [[19]] and t["cls"].tolist() == [[301]]
    m.pipe_open()
    with pytest.raises(gpu.MarsError) as ei:
        m.match_device(g)  # an open pipe
    assert ei.value.code == gpu.MARS_ERR_INVALID_TENSOR
    m.pipe_close()
    other.close()
    g.close()
    m.close()


# ---- the chain ---------------------------------------------------------------------------------------------------------------------------
def one_round(c, dst, g, buf):
    """detector -> crops -> second model -> classify -> match -> labels and identities; nothing waits"""
    c.detect(buf)
    dst.crop_detections(c.det, buf.ptr, c.opts(), device=True)
    dst.run_device(sync=False)
    dst.classify_device(top_k=3)
    dst.match_device(g, top_k=3)
    c.det.label_detections(dst)


def fetch(c, dst):
    dets = c.det.detect_results()
    rois, _ = dst.roi_results()
    top, rows = dst.match_results(3)
    _, sums = dst.classify_results(3)
    return dets, rois, top, rows, sums, c.det.identity_results()


@pytest.fixture(scope="module")
def chain(gpu):
    d2, tin, tout, nhwc = second_stage(gpu, "shipped")
    c = Chain(gpu)
    dst = gpu.Model(d2, batch=8)
    gal = vectors(0x6A190000, 50, 64, shift=9) + 40000  # pooled sums of the shipped file lean to one side; so do these rows
    g, ids = gallery_of(gpu, gal, ids=np.arange(50) + 1000)
    yield c, dst, g, gal, ids
    g.close()
    dst.close()
    c.close()


def test_chain_identities(gpu, chain):
    c, dst, g, gal, ids = chain
    nv, buf = c.frames(FRAME_SEED)
    with pytest.raises(gpu.MarsError) as ei:
        c.det.identity_results()  # nothing pending
    assert ei.value.code == gpu.MARS_ERR_INVALID_TENSOR
    one_round(c, dst, g, buf)
    labels = c.det.label_results()
    c.det.identify_detections(dst)
    dets, rois, top, rows, sums, idents = fetch(c, dst)
    assert len(rois) == 8 and sum(len(x) for x in dets) > 8
    want, want_rows = match_np(gal, ids, sums, 64, 3)
    same(top, want, "chain top")
    same(rows, want_rows, "chain rows")
    same(idents, ident_np(rois, top[:, 0], [len(x) for x in dets]), "identities")
    assert int((idents["cls"] >= 1000).sum()) == 8
    without = [(f, i) for f, x in enumerate(dets) for i in range(len(x)) if idents[f, i]["cls"] < 0]
    assert len(without) >= 1 and all(idents[f, i]["score"] == 0 for f, i in without)
    same(c.det.label_results(), labels, "labels beside identities")  # the identify call left them alone
    assert labels.tobytes() != idents.tobytes()
    with pytest.raises(gpu.MarsError) as ei:
        dst.identify_detections(dst)
    assert ei.value.code == gpu.MARS_ERR_INVALID_TENSOR
    stranger = Chain(gpu)  # another detector: the crops in dst were not cut out of its detections
    with pytest.raises(gpu.MarsError) as ei:
        stranger.det.identify_detections(dst)
    assert ei.value.code == gpu.MARS_ERR_INVALID_TENSOR
    with pytest.raises(gpu.MarsError) as ei:
        c.det.identify_detections(stranger.det)  # no crop call ever wrote into that model
    assert ei.value.code == gpu.MARS_ERR_INVALID_TENSOR
    stranger.close()
    same(c.det.identity_results(), idents, "identities after the refusals")


def test_chain_rounds_back_to_back(gpu, chain):
    """two full rounds on different frames enqueued without a host wait: what is read afterwards is the second round's"""
    c, dst, g, gal, ids = chain
    (nv_a, buf_a), (nv_b, buf_b) = c.frames(FRAME_SEED), c.frames(FRAME_SEED + 32)
    one_round(c, dst, g, buf_b)
    c.det.identify_detections(dst)
    ref = fetch(c, dst)
    one_round(c, dst, g, buf_a)
    c.det.identify_detections(dst)
    one_round(c, dst, g, buf_b)
    c.det.identify_detections(dst)
    got = fetch(c, dst)
    for a, b in zip(got[0], ref[0]):
        assert a.tobytes() == b.tobytes()
    for k, what in ((1, "rois"), (2, "top"), (3, "rows"), (4, "sums"), (5, "identities")):
        assert got[k].tobytes() == ref[k].tobytes(), what
    one_round(c, dst, g, buf_a)
    c.det.identify_detections(dst)
    assert fetch(c, dst)[4].tobytes() != ref[4].tobytes()  # other frames, other sums
