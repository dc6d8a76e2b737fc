"""Raw anchor-free DFL heads decoded on the device (mars_hip_detect_dfl), bit for bit against a numpy restatement of the decode
(include/mars_hip.h "anchor-free DFL heads": float32, every operation rounded on its own, both tables from libm's expf) followed by the
reference's NMS."""
import ctypes as C
import ctypes.util
import os

import numpy as np
import pytest

import marsfile
from conftest import lcg_frame
from test_gpu_yolo_heads import letterbox_map, nms, sig_table

pytestmark = pytest.mark.gpu

MODELS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "models")
F32 = np.float32

_libm = C.CDLL(ctypes.util.find_library("m"))
_libm.expf.restype = C.c_float
_libm.expf.argtypes = [C.c_float]


def e_table(scale):
    """E[d] = expf(-((float)d * scale)), d = 0 .. 255"""
    s = F32(scale)
    return np.array([F32(_libm.expf(float(-(F32(d) * s)))) for d in range(256)], dtype=F32)


def decode_dfl(heads, det_dtype, conf=0.25):
    """heads: [(box int8 [4 R][H][W], cls int8 [nc][H][W], box scale, class scale, stride)] in prediction order -> (the candidate records,
    the first 1000; the number of candidates)"""
    conf = F32(conf)
    out = []
    for box, cls, bs, cs, stride in heads:
        nc, H, W = cls.shape
        R = box.shape[0] // 4
        sg, E = sig_table(cs), e_table(bs)
        cl = cls.reshape(nc, H * W).astype(np.int32)
        best = np.argmax(cl, axis=0)  # the first class of largest byte
        c = sg[cl[best, np.arange(H * W)] + 128]
        idx = np.nonzero(c >= conf)[0]
        q = box.reshape(4, R, H * W)[:, :, idx].astype(np.int32)
        e = E[q.max(axis=1)[:, None, :] - q]
        den, num = e[:, 0].copy(), np.zeros((4, len(idx)), dtype=F32)
        for i in range(1, R):
            den = den + e[:, i]
        for i in range(R):
            num = num + F32(i) * e[:, i]
        dist = num / den
        assert dist.dtype == F32
        ax, ay = (idx % W).astype(F32) + F32(0.5), (idx // W).astype(F32) + F32(0.5)
        x1, y1, x2, y2 = ax - dist[0], ay - dist[1], ax + dist[2], ay + dist[3]
        rec = np.zeros(len(idx), dtype=det_dtype)
        rec["x"] = ((x1 + x2) * F32(0.5)) * F32(stride)
        rec["y"] = ((y1 + y2) * F32(0.5)) * F32(stride)
        rec["w"] = (x2 - x1) * F32(stride)
        rec["h"] = (y2 - y1) * F32(stride)
        rec["conf"] = c[idx]
        rec["cls"] = best[idx]
        out.append(rec)
    all_ = np.concatenate(out)
    return all_[:1000], len(all_)


def _conv(G, rng, x, out, oc, ic, k, s, nchw):
    if nchw:
        w = G.tensor([oc, ic, k, k], fmt=marsfile.OIHW, scale=0.01, data=rng.integers(-127, 128, (oc, ic, k, k), dtype=np.int8))
    else:
        w = G.tensor([oc, k, k, ic], scale=0.01, data=rng.integers(-127, 128, (oc, k, k, ic), dtype=np.int8))
    G.conv(x, out, w, k=(k, k), s=(s, s))


def dfl_graph(nc, R, nchw, in_c=16):
    """32 x 32 x in_c input; head 0: box + class 1x1 convolutions at 32 x 32, their concat a graph output; head 1: the same with stride 2
    at 16 x 16, its concat read only by a RESHAPE.  NHWC tags at fusion >= 1: the convolutions write slices of the concats; NCHW tags:
    planes (head 0) / pixels x channels where the channel counts allow (head 1).  -> file, [(box, class, concat, grid, stride)]"""
    rng = np.random.default_rng(nc * 64 + R * 2 + nchw)
    G = marsfile.Graph()
    fmt = marsfile.NCHW if nchw else marsfile.NHWC
    shp = (lambda c, h, w: [1, c, h, w]) if nchw else (lambda c, h, w: [1, h, w, c])
    x = G.tensor(shp(in_c, 32, 32), fmt=fmt, scale=0.05)
    heads = []
    for hw, s in ((32, 1), (16, 2)):
        b = G.tensor(shp(4 * R, hw, hw), fmt=fmt, scale=0.25)
        c = G.tensor(shp(nc, hw, hw), fmt=fmt, scale=0.25)
        _conv(G, rng, x, b, 4 * R, in_c, 1, s, nchw)
        _conv(G, rng, x, c, nc, in_c, 1, s, nchw)
        cat = G.tensor(shp(4 * R + nc, hw, hw), fmt=fmt, scale=0.25)
        G.concat([b, c], cat, axis=1 if nchw else 3)
        heads.append((b, c, cat, hw, s))
    G.layer(marsfile.RESHAPE, [heads[1][2]], [G.tensor([0, 0, 0, 0])])
    return G.serialise([x], [heads[0][2]]), heads


def head_bytes(gpu, m, f, b, c, cat, nchw):
    """the (box [4 R][H][W], class [nc][H][W]) bytes of frame f: the tensors themselves (mars_hip_read_tensor: the reference's bytes in the
    tag's order) or, where the plan keeps them only as slices of the concat's buffer (NHWC), the concat output's channels"""
    db, dc = m.tensor_desc(b), m.tensor_desc(c)
    if nchw:
        return tuple(m.read_tensor(t, f).view(np.int8).reshape(d.shape[1], d.shape[2], d.shape[3]) for t, d in ((b, db), (c, dc)))
    H, W, cb, cc = db.shape[1], db.shape[2], db.shape[3], dc.shape[3]
    try:
        return (m.read_tensor(b, f).view(np.int8).reshape(H, W, cb).transpose(2, 0, 1), m.read_tensor(c, f).view(np.int8).reshape(H, W, cc).transpose(2, 0, 1))
    except gpu.MarsError:
        o = m.read_tensor(cat, f).view(np.int8).reshape(H, W, cb + cc).transpose(2, 0, 1)
        return o[:cb], o[cb:]


def expected(gpu, m, f, heads, nchw, conf, box_scale=None, cls_scale=None, thresh=0.45):
    hs = []
    for b, c, cat, _, s in heads:
        bb, cb = head_bytes(gpu, m, f, b, c, cat, nchw)
        hs.append((np.ascontiguousarray(bb), np.ascontiguousarray(cb), box_scale or m.tensor_desc(b).scale, cls_scale or m.tensor_desc(c).scale, s))
    cand, raw = decode_dfl(hs, gpu.DET_DTYPE, conf)
    return nms(cand, thresh), raw


def fill(m, seed):
    nb = m.input_view(0).shape[1]
    for f in range(m.batch):
        m.input_view(0)[f] = lcg_frame(seed + f, nb)


def same(got, want, what):
    for f, (g, w) in enumerate(zip(got, want)):
        assert len(g) == len(w) and g.tobytes() == w.tobytes(), (what, f, len(g), len(w))


@pytest.mark.parametrize("fusion", [0, 1])
@pytest.mark.parametrize("nchw", [False, True])
@pytest.mark.parametrize("nc, R", [(1, 16), (3, 16), (80, 16), (3, 8), (80, 8)])
def test_hand_built_graphs(gpu, nc, R, nchw, fusion):
    """graph -> heads -> boxes at batch 1, 3 and 66 (two streams): the tensors' own scales (saturating: the cap) and gentle overrides
    with a threshold that few cells pass"""
    d, heads = dfl_graph(nc, R, nchw)
    assert gpu.find_yolo_dfl_heads(d) == ([(b, c, s) for b, c, _, _, s in heads], nc, R)
    m = gpu.Model(d, batch=1, fusion=fusion)
    few = 0
    for B in (1, 3, 66):
        m.set_batch(B)
        fill(m, 0xDF100000 + 1000 * B)
        m.run()
        for kw in (dict(conf=0.25), dict(conf=0.7 if nc < 80 else 0.78, box_scales=0.05, cls_scales=0.01)):
            got = m.detect_dfl(**kw)
            exp = [expected(gpu, m, f, heads, nchw, kw["conf"], kw.get("box_scales"), kw.get("cls_scales")) for f in range(B)]
            same(got, [e[0] for e in exp], (nc, R, nchw, fusion, B, kw))
            few += sum(0 < e[1] < 1000 for e in exp)
    assert few > 0
    m.close()


def _write_heads(gpu, m, f, heads, nchw, arrs):
    """arrs: per head (box [4 R][H][W], class [nc][H][W]) int8, written where the decode reads them"""
    for (b, c, cat, hw, _), (ab, ac) in zip(heads, arrs):
        def put(t, a):
            a = np.ascontiguousarray(a if nchw else a.transpose(1, 2, 0))
            return gpu.lib().mars_hip_write_tensor(m.p, t, f, a.ctypes.data, a.size)
        if put(b, ab) != 0 or put(c, ac) != 0:
            assert not nchw and put(cat, np.concatenate([ab, ac])) == 0


@pytest.mark.parametrize("nchw", [False, True])
def test_chosen_bytes(gpu, nchw):
    """decode only, bytes written into the heads: class ties (the first wins), all bins equal, one bin at +127 and the rest at -128 under
    a large scale (E underflows to 0), no candidate at all, and more than 1000 candidates (the first 1000 are kept)"""
    nc, R = 3, 16
    d, heads = dfl_graph(nc, R, nchw)
    m = gpu.Model(d, batch=5)
    fill(m, 1)
    m.run()
    rng = np.random.default_rng(5)
    frames = []
    for f in range(5):
        arrs = []
        for _, _, _, hw, _ in heads:
            ab = rng.integers(-128, 128, (4 * R, hw, hw), dtype=np.int8)
            ac = rng.integers(-128, 128, (nc, hw, hw), dtype=np.int8)
            if f == 0:    # ties between classes 1 and 2, class 0 below
                ac[1] = ac[2] = np.maximum(ac[1], 0)
                ac[0] = -128
            elif f == 1:  # all bins equal: dist = 7.5 on every side
                ab[:] = rng.integers(-128, 128, (1, hw, hw), dtype=np.int8)
            elif f == 2:  # one bin at +127, the rest at -128
                ab[:] = -128
                pos = rng.integers(0, R, (4, hw, hw))
                for s in range(4):
                    np.put_along_axis(ab[s * R:(s + 1) * R], pos[s][None], 127, axis=0)
            elif f == 3:  # nothing passes
                ac[:] = -128
            else:         # everything passes
                ac[:] = 127
            arrs.append((ab, ac))
        _write_heads(gpu, m, f, heads, nchw, arrs)
        frames.append(arrs)
    for bs, cs, conf in ((0.05, 0.02, 0.6), (1.0, 0.02, 0.6), (3.0, 0.05, 0.25)):
        got = m.detect_dfl(conf=conf, box_scales=bs, cls_scales=cs)
        raws = []
        for f in range(5):
            hs = [(ab, ac, bs, cs, s) for (ab, ac), (_, _, _, _, s) in zip(frames[f], heads)]
            cand, raw = decode_dfl(hs, gpu.DET_DTYPE, conf)
            raws.append(raw)
            want = nms(cand, 0.45)
            assert got[f].tobytes() == want.tobytes(), (nchw, bs, cs, conf, f)
            if f == 0:
                assert len(cand) > 0 and set(cand["cls"]) == {1}
            if f == 1:  # 120 / 16 = 7.5 on both sides, times the stride (1 or 2)
                assert len(cand) > 0 and set(cand["w"]) <= {F32(15), F32(30)} and set(cand["h"]) <= {F32(15), F32(30)}
        assert raws[3] == 0 and len(got[3]) == 0 and raws[4] == 32 * 32 + 16 * 16 and raws[0] > 0
    assert e_table(3.0)[255] == 0
    m.close()


def _nu():
    with open(os.path.join(MODELS, "yolov5nu.mars"), "rb") as fh:
        return fh.read()


NU_HEADS = [(323, 336, 8), (350, 363, 16), (377, 390, 32)]


def _expected_model(gpu, m, f, heads, conf, box_scale=None, cls_scale=None, nchw=True):
    return expected(gpu, m, f, [(b, c, None, None, s) for b, c, s in heads], nchw, conf, box_scale, cls_scale)[0]


def test_shipped_yolov5nu(gpu):
    """yolov5nu.mars at batch 8 on LCG frames: its own scales (1.0), the 0.1 overrides, and explicit tensor lists"""
    d = _nu()
    assert gpu.find_yolo_dfl_heads(d) == (NU_HEADS, 80, 16)
    B = 8
    m = gpu.Model(d, batch=B)
    fill(m, 0x4EAD0000)
    m.run()
    got = m.detect_dfl()
    same(got, [_expected_model(gpu, m, f, NU_HEADS, 0.25) for f in range(B)], "own scales")
    got = m.detect_dfl(box_scales=0.1, cls_scales=0.1)
    same(got, [_expected_model(gpu, m, f, NU_HEADS, 0.25, 0.1, 0.1) for f in range(B)], "0.1")
    assert sum(len(g) for g in got) > 0
    same(m.detect_dfl(heads=NU_HEADS, reg_max=16, box_scales=0.1, cls_scales=0.1), got, "explicit lists")
    same(m.detect_dfl(heads=[h[:2] for h in NU_HEADS], box_scales=[0.1] * 4, cls_scales=[0.1] * 4), got, "explicit lists, default strides")
    m.close()


def _twin_heads(gpu, d):
    hdr, _, _ = marsfile.parse(d)
    return [(b, c, o, None, s) for (b, c, s), o in zip(gpu.find_yolo_dfl_heads(d)[0], hdr["outputs"])]


@pytest.mark.parametrize("nchw", [False, True])
def test_twin_640(gpu, nchw):
    """the 640 x 640 dfl twin at batch 8: some boxes per frame, far fewer than the cap"""
    d = gpu.synth_model(width_x16=4, input_hw=640, nchw_int8=nchw, seed=1, head="dfl")
    heads = _twin_heads(gpu, d)
    B = 8
    m = gpu.Model(d, batch=B)
    fill(m, 0x5EED0000)
    m.run()
    got = m.detect_dfl()
    exp = [expected(gpu, m, f, heads, nchw, 0.25) for f in range(B)]
    same(got, [e[0] for e in exp], nchw)
    assert all(0 < e[1] <= 250 for e in exp), [e[1] for e in exp]
    m.close()


def camera_dfl_graph():
    """NCHW int8 [1, 3, 64, 64] camera input -> 3x3 stride-2 conv to 16 x 32 x 32 -> two DFL heads: 32 x 32 (stride 2), its concat read only
    by a RESHAPE (internal tensors), and 16 x 16 (stride 4), its concat the graph output.  The heads follow the input."""
    rng = np.random.default_rng(78)
    G = marsfile.Graph()
    N = marsfile.NCHW
    x = G.tensor([1, 3, 64, 64], fmt=N, scale=1.0 / 128)
    t1 = G.tensor([1, 16, 32, 32], fmt=N, scale=0.02)
    _conv(G, rng, x, t1, 16, 3, 3, 2, True)
    heads = []
    for hw, s in ((32, 1), (16, 2)):
        b, c = G.tensor([1, 64, hw, hw], fmt=N, scale=0.08), G.tensor([1, 80, hw, hw], fmt=N, scale=0.02)
        _conv(G, rng, t1, b, 64, 16, 1, s, True)
        _conv(G, rng, t1, c, 80, 16, 1, s, True)
        cat = G.tensor([1, 144, hw, hw], fmt=N, scale=0.08)
        G.concat([b, c], cat, axis=1)
        heads.append((b, c, cat, hw, 2 * s))
    G.layer(marsfile.RESHAPE, [heads[0][2]], [G.tensor([0, 0, 0, 0])])
    return G.serialise([x], [heads[1][2]]), heads


CAM_CONF = 0.45  # the camera graph's class bytes saturate: every cell passes, the cap decides


def _camera_frames(n, w, h, seed):
    return [lcg_frame(seed + i, w * h * 3).reshape(h, w, 3) for i in range(n)]


def test_letterbox_mapping(gpu):
    d, heads = camera_dfl_graph()
    B = 2
    m = gpu.Model(d, batch=B)
    m.preprocess(np.stack(_camera_frames(B, 1280, 720, 0xCA0000)))
    m.run_device()
    plain = m.detect_dfl(conf=CAM_CONF)
    same(plain, [expected(gpu, m, f, heads, True, CAM_CONF)[0] for f in range(B)], "plain")
    mapped = m.detect_dfl(conf=CAM_CONF, src=(1280, 720))
    for f in range(B):
        assert len(plain[f]) > 0
        assert mapped[f].tobytes() == letterbox_map(plain[f], 1280, 720, 64, 64).tobytes(), f
    m.close()


@pytest.mark.parametrize("camera", [False, True])
def test_pipe(gpu, camera):
    """the pipe with dfl_heads, plain and camera mode, 5 different batches of 2 (three in flight over one set of internal head tensors):
    every batch equals the synchronous path"""
    d, _ = camera_dfl_graph()
    B, W, H, N = 2, 1280, 720, 5
    m = gpu.Model(d, batch=B)
    nb = m.input_view(0).shape[1]
    if camera:
        batches = [np.stack(_camera_frames(B, W, H, 0xB0B0 * 8 + 16 * k)).reshape(B, -1) for k in range(N)]
    else:
        batches = [np.stack([lcg_frame(0xD0D0 * 8 + 16 * k + f, nb) for f in range(B)]) for k in range(N)]
    want = []
    for k in range(N):
        if camera:
            m.preprocess(batches[k].reshape(B, H, W, 3))
            m.run_device()
            want.append(m.detect_dfl(conf=CAM_CONF, src=(W, H)))
        else:
            m.input_view(0)[:] = batches[k]
            m.run()
            want.append(m.detect_dfl(conf=CAM_CONF))
        assert all(len(w) > 0 for w in want[-1])
    assert camera or len({want[k][0].tobytes() for k in range(N)}) == N
    m.pipe_open(download_outputs=False, detect=True, camera=(W, H) if camera else None, dfl_heads=gpu.yolo_dfl_heads(conf=CAM_CONF))
    got = []
    for k in range(N):
        if k >= 3:
            got.append(m.pipe_wait()[1])
        m.pipe_input_view(0)[:] = batches[k]
        m.pipe_submit()
    while len(got) < N:
        got.append(m.pipe_wait()[1])
    m.pipe_close()
    for k in range(N):
        same(got[k], want[k], (camera, k))
    m.close()


def test_async_hand_off(gpu):
    """run_device_async(A) -> detect_dfl_device -> mars_run(B) in a loop: the decode of A reads tensors that B's graph overwrites; the layers
    of B that write them wait, so every batch's boxes equal run / sync / detect"""
    d, _ = camera_dfl_graph()
    B = 64
    m = gpu.Model(d, batch=B)
    nb = m.input_view(0).shape[1]
    xs = [[lcg_frame(0xA0A00000 + 0x100000 * k + f, nb) for f in range(B)] for k in range(3)]
    want = []
    for k in range(3):
        for f in range(B):
            m.input_view(0)[f] = xs[k][f]
        m.run()
        want.append(m.detect_dfl(conf=CAM_CONF))
    assert all(want[0][f].tobytes() != want[1][f].tobytes() for f in range(B))
    for f in range(B):
        m.input_view(0)[f] = xs[0][f]
    m.upload()
    for k in range(3):
        m.run_device(sync=False)
        m.detect_dfl_device(conf=CAM_CONF)
        nxt = xs[(k + 1) % 3]
        for f in range(B):
            m.input_view(0)[f] = nxt[f]
        m.run()  # upload + graph of the next batch on the main stream, no host wait in between
        same(m.detect_results(), want[k], k)
        m.upload()
    m.close()


def test_cross_refusals(gpu):
    """the anchor calls refuse DFL tensors, the DFL calls refuse anchor heads and bad configurations, the pipe refuses both options"""
    INV = gpu.MARS_ERR_INVALID_TENSOR
    m = gpu.Model(_nu())
    for heads in (None, [323], [336], [337]):
        with pytest.raises(gpu.MarsError) as e:
            m.detect_heads(heads=heads)
        assert e.value.code == INV, heads
    for kw in (dict(heads=[(337, 336)]), dict(heads=[(323, 363)]), dict(reg_max=8), dict(box_scales=-1.0), dict(heads=[(323, 9999)]),
               dict(heads=[(1, 336)])):
        with pytest.raises(gpu.MarsError) as e:
            m.detect_dfl(**kw)
        assert e.value.code == INV, kw
    with pytest.raises(gpu.MarsError) as e:
        m.pipe_open(download_outputs=False, detect=True, heads=True, dfl_heads=True)
    assert e.value.code == INV
    m.close()
    with open(os.path.join(MODELS, "yolov5n_int8.mars"), "rb") as fh:
        m = gpu.Model(fh.read())
    for kw in (dict(), dict(heads=[(313, 335)])):
        with pytest.raises(gpu.MarsError) as e:
            m.detect_dfl(**kw)
        assert e.value.code == INV, kw
    m.close()
