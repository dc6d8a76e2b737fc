"""Raw anchor-based YOLOv5 Detect heads decoded on the device (mars_hip_detect_heads), bit for bit against a numpy restatement of
the decode (float32, every operation rounded on its own, the sigmoid table from libm's expf) followed by the reference's NMS."""
import ctypes as C
import ctypes.util
import os

import numpy as np
import pytest

import marsfile
from conftest import lcg_frame

pytestmark = pytest.mark.gpu

MODELS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "models")
F32 = np.float32
DEFAULT_ANCHORS = [[[10, 13], [16, 30], [33, 23]], [[30, 61], [62, 45], [59, 119]], [[116, 90], [156, 198], [373, 326]]]

_libm = C.CDLL(ctypes.util.find_library("m"))
_libm.expf.restype = C.c_float
_libm.expf.argtypes = [C.c_float]


def sig_table(scale):
    """sig[q + 128] = 1.0f / (1.0f + expf((-(float)q) * scale))"""
    s = F32(scale)
    return np.array([F32(1.0) / (F32(1.0) + F32(_libm.expf(float(F32(-float(q)) * s)))) for q in range(-128, 128)], dtype=F32)


def nms(dets, thresh):
    import refbind
    if refbind.available():
        return refbind.nms(dets, thresh)
    import orcbind
    return orcbind.nms(dets, thresh)


def decode_heads(heads, det_dtype, conf=0.25):
    """heads: [(int8 [C][H][W], scale, stride, anchors [3][2])] in prediction order -> the candidate records, the first 1000"""
    conf = F32(conf)
    out = []
    for arr, scale, stride, anchors in heads:
        Cn, H, W = arr.shape
        nc = Cn // 3 - 5
        R = 5 + nc
        sg = sig_table(scale)
        for a in range(3):
            blk = arr[a * R:(a + 1) * R].reshape(R, H * W).astype(np.int32)
            obj = sg[blk[4] + 128]
            best = np.argmax(blk[5:], axis=0)  # the first class of largest byte
            qb = blk[5:][best, np.arange(H * W)]
            c = obj * sg[qb + 128]
            idx = np.nonzero(~(obj < conf) & ~(c < conf))[0]
            rec = np.zeros(len(idx), dtype=det_dtype)
            gx, gy = (idx % W).astype(F32), (idx // W).astype(F32)
            s = [sg[blk[k, idx] + 128] for k in range(4)]
            rec["x"] = (((s[0] * F32(2.0)) - F32(0.5)) + gx) * F32(stride)
            rec["y"] = (((s[1] * F32(2.0)) - F32(0.5)) + gy) * F32(stride)
            tw, th = s[2] * F32(2.0), s[3] * F32(2.0)
            rec["w"] = (tw * tw) * F32(anchors[a][0])
            rec["h"] = (th * th) * F32(anchors[a][1])
            rec["conf"] = c[idx]
            rec["cls"] = best[idx]
            out.append(rec)
    return np.concatenate(out)[:1000]


def letterbox_map(dets, src_w, src_h, tw, th):
    """mars_preproc.c's letterbox geometry, then x' = (x - px) * rx, w' = w * rx (y, h alike)"""
    scale = min(F32(tw) / F32(src_w), F32(th) / F32(src_h))
    nw, nh = int(F32(src_w) * scale), int(F32(src_h) * scale)
    px, py = F32((tw - nw) // 2), F32((th - nh) // 2)
    rx, ry = F32(src_w) / F32(nw), F32(src_h) / F32(nh)
    d = dets.copy()
    d["x"] = (d["x"] - px) * rx
    d["y"] = (d["y"] - py) * ry
    d["w"] = d["w"] * rx
    d["h"] = d["h"] * ry
    return d


def _conv(G, rng, x, out, oc, ic, k, s, nchw):
    if nchw:
        w = G.tensor([oc, ic, k, k], fmt=marsfile.OIHW, scale=0.01, data=rng.integers(-127, 128, (oc, ic, k, k), dtype=np.int8))
    else:
        w = G.tensor([oc, k, k, ic], scale=0.01, data=rng.integers(-127, 128, (oc, k, k, ic), dtype=np.int8))
    G.conv(x, out, w, k=(k, k), s=(s, s))


def head_graph(nc, nchw, scales):
    """32 x 32 x 16 input; head 0: 1x1 stride 1 -> 32 x 32, a graph output; head 1: 1x1 stride 2 -> 16 x 16, read only by a RESHAPE.
    NHWC tags: head 0 rows at a 16-byte pitch (256 for 255 channels), head 1 dense rows.  NCHW tags: head 0 planes, head 1 held
    pixels x channels at a 16-byte pitch."""
    rng = np.random.default_rng(nc * 2 + nchw)
    Cn = 3 * (5 + nc)
    G = marsfile.Graph()
    fmt = marsfile.NCHW if nchw else marsfile.NHWC
    shp = (lambda c, h, w: [1, c, h, w]) if nchw else (lambda c, h, w: [1, h, w, c])
    x = G.tensor(shp(16, 32, 32), fmt=fmt, scale=0.05)
    h0 = G.tensor(shp(Cn, 32, 32), fmt=fmt, scale=scales[0])
    h1 = G.tensor(shp(Cn, 16, 16), fmt=fmt, scale=scales[1])
    _conv(G, rng, x, h0, Cn, 16, 1, 1, nchw)
    _conv(G, rng, x, h1, Cn, 16, 1, 2, nchw)
    G.layer(marsfile.RESHAPE, [h1], [G.tensor([0, 0, 0, 0])])
    return G.serialise([x], [h0]), (h0, h1)


@pytest.mark.parametrize("nchw", [False, True])
@pytest.mark.parametrize("nc", [1, 3, 80])
def test_kernel_synthetic_heads(gpu, nc, nchw):
    """random head bytes written straight into the heads, in every device layout (NHWC dense / at pitch 256, NCHW planes, NCHW-tagged
    held pixels x channels), three frames: a saturating scale (every sigmoid 0.5, all ties: > 1000 candidates, the cap), an
    ordinary one, and a high threshold (few candidates)"""
    Cn = 3 * (5 + nc)
    for scales, conf in (((1e-12, 1e-12), 0.25), ((0.06, 0.045), 0.25), ((0.06, 0.045), 0.9)):
        d, tids = head_graph(nc, nchw, scales)
        m = gpu.Model(d, batch=3)
        anchors = [[[3, 4], [5, 6], [7, 9]], [[11, 12], [13, 17], [19, 23]]]
        rng = np.random.default_rng(nc * 7 + nchw)
        want = []
        for f in range(3):
            heads = []
            for k, (ti, hw) in enumerate(zip(tids, (32, 16))):
                arr = rng.integers(-128, 128, (Cn, hw, hw), dtype=np.int8)
                ref_bytes = arr if nchw else arr.transpose(1, 2, 0)  # the reference's bytes in the tag's order
                assert gpu.lib().mars_hip_write_tensor(m.p, ti, f, np.ascontiguousarray(ref_bytes).ctypes.data, arr.size) == 0
                heads.append((arr, scales[k], 32 // hw, anchors[k]))
            cand = decode_heads(heads, gpu.DET_DTYPE, conf)
            if scales[0] < 1e-6:
                assert len(cand) == 1000
            want.append(nms(cand, 0.45))
        got = m.detect_heads(heads=[(tids[0], 1), (tids[1], 2)], anchors=anchors, conf=conf, thresh=0.45)
        for f in range(3):
            assert len(got[f]) == len(want[f]), (nc, nchw, scales, conf, f)
            assert got[f].tobytes() == want[f].tobytes(), (nc, nchw, scales, conf, f)
        m.close()


def test_invalid_heads(gpu):
    """a weight, a tensor of a channel count that is no 3 * (5 + nc), no heads at all: MARS_ERR_INVALID_TENSOR"""
    d, tids = head_graph(3, False, (0.05, 0.05))
    m = gpu.Model(d)
    for heads in ([3], [0], [tids[0], 99]):
        with pytest.raises(gpu.MarsError) as e:
            m.detect_heads(heads=heads)
        assert e.value.code == gpu.MARS_ERR_INVALID_TENSOR
    m.close()
    m = gpu.Model(gpu.synth_model(tiny=True, input_hw=160))
    with pytest.raises(gpu.MarsError) as e:
        m.detect_heads()
    assert e.value.code == gpu.MARS_ERR_INVALID_TENSOR
    m.close()


def _shipped():
    with open(os.path.join(MODELS, "yolov5n_int8.mars"), "rb") as fh:
        return fh.read()


def _expected_from_tensors(gpu, m, f, heads, conf):
    """the numpy decode of frame f's heads as mars_hip_read_tensor returns them (the reference's [C][H][W] bytes)"""
    hs = []
    for k, (ti, stride, nc) in enumerate(heads):
        dsc = m.tensor_desc(ti)
        arr = m.read_tensor(ti, f).view(np.int8).reshape(dsc.shape[1], dsc.shape[2], dsc.shape[3])
        hs.append((arr, dsc.scale, stride, DEFAULT_ANCHORS[k]))
    return decode_heads(hs, gpu.DET_DTYPE, conf)


def test_shipped_model(gpu):
    """the shipped yolov5n_int8.mars at batch 8 on LCG frames: its three internal heads decoded on the device equal the numpy decode
    of the same heads read back, followed by the reference's NMS"""
    d = _shipped()
    heads = gpu.find_yolo_heads(d)
    assert heads == [(313, 8, 80), (335, 16, 80), (357, 32, 80)]
    B = 8
    m = gpu.Model(d, batch=B)
    nb = m.input_view(0).shape[1]
    for f in range(B):
        m.input_view(0)[f] = lcg_frame(0x4EAD0000 + f, nb)
    m.run()
    for conf in (0.25, 0.01):
        got = m.detect_heads(conf=conf)
        for f in range(B):
            want = nms(_expected_from_tensors(gpu, m, f, heads, conf), 0.45)
            assert got[f].tobytes() == want.tobytes(), (conf, f)
    assert sum(len(g) for g in got) > 0
    m.close()


def camera_graph():
    """NCHW int8 [1, 3, 64, 64] input (a camera input for the front-end) -> 3x3 stride-2 conv to 16 x 32 x 32 -> two 255-channel 1x1
    heads: 32 x 32 (stride 2) read only by a RESHAPE -- an internal tensor held pixels x channels at pitch 256, as in the shipped
    file -- and 16 x 16 (stride 4), the graph output.  Unlike the shipped file's (whose int8 heads saturate to the same few values
    for every frame), these heads follow the input."""
    rng = np.random.default_rng(77)
    G = marsfile.Graph()
    N = marsfile.NCHW
    x = G.tensor([1, 3, 64, 64], fmt=N, scale=1.0 / 128)
    t1 = G.tensor([1, 16, 32, 32], fmt=N, scale=0.02)
    _conv(G, rng, x, t1, 16, 3, 3, 2, True)
    h0 = G.tensor([1, 255, 32, 32], fmt=N, scale=0.08)
    h1 = G.tensor([1, 255, 16, 16], fmt=N, scale=0.08)
    _conv(G, rng, t1, h0, 255, 16, 1, 1, True)
    _conv(G, rng, t1, h1, 255, 16, 1, 2, True)
    G.layer(marsfile.RESHAPE, [h0], [G.tensor([0, 0, 0, 0])])
    return G.serialise([x], [h1]), [(h0, 2, 80), (h1, 4, 80)]


def test_camera_graph_heads(gpu):
    """the synthetic camera graph's heads are found, decode bit-exactly and differ from frame to frame"""
    d, heads = camera_graph()
    assert gpu.find_yolo_heads(d) == heads
    B = 3
    m = gpu.Model(d, batch=B)
    nb = m.input_view(0).shape[1]
    for f in range(B):
        m.input_view(0)[f] = lcg_frame(0xCA3E0000 + f, nb)
    m.run()
    got = m.detect_heads()
    for f in range(B):
        want = nms(_expected_from_tensors(gpu, m, f, heads, 0.25), 0.45)
        assert len(want) > 0 and got[f].tobytes() == want.tobytes(), f
    assert got[0].tobytes() != got[1].tobytes()
    m.close()


def _camera_frames(n, w, h, seed):
    return [lcg_frame(seed + i, w * h * 3).reshape(h, w, 3) for i in range(n)]


def test_letterbox_mapping(gpu):
    """preprocess(1280 x 720 frames) -> run -> detect_heads(src=(1280, 720)): the unmapped result mapped in numpy"""
    d = _shipped()
    B = 2
    m = gpu.Model(d, batch=B)
    frames = np.stack(_camera_frames(B, 1280, 720, 0xCA0000))
    m.preprocess(frames)
    m.run_device()
    plain = m.detect_heads(conf=0.01)
    mapped = m.detect_heads(conf=0.01, src=(1280, 720))
    for f in range(B):
        assert len(plain[f]) > 0
        assert mapped[f].tobytes() == letterbox_map(plain[f], 1280, 720, 640, 640).tobytes(), f
    m.close()


@pytest.mark.parametrize("model", ["shipped", "synthetic"])
def test_pipe_camera_heads(gpu, model):
    """camera-mode pipe with heads set, 5 batches of 2 (three in flight, four slots, one set of internal head tensors): every batch
    equals preprocess -> run -> detect_heads with boxes in camera pixels (the synthetic graph's heads differ from batch to batch, so
    a decode that read another batch's heads would show)"""
    d = _shipped() if model == "shipped" else camera_graph()[0]
    B, W, H, N = 2, 1280, 720, 5
    batches = [np.stack(_camera_frames(B, W, H, 0xB0B0 * 8 + 16 * k)) for k in range(N)]
    m = gpu.Model(d, batch=B)
    want = []
    for k in range(N):
        m.preprocess(batches[k])
        m.run_device()
        want.append(m.detect_heads(conf=0.01, src=(W, H)))
        assert all(len(w) > 0 for w in want[-1])
    m.pipe_open(download_outputs=False, detect=True, camera=(W, H), heads=gpu.yolo_heads(conf=0.01))
    got = []
    for k in range(N):
        if k >= 3:
            got.append(m.pipe_wait()[1])
        m.pipe_input_view(0)[:] = batches[k].reshape(B, -1)
        m.pipe_submit()
    while len(got) < N:
        got.append(m.pipe_wait()[1])
    m.pipe_close()
    for k in range(N):
        for f in range(B):
            assert got[k][f].tobytes() == want[k][f].tobytes(), (k, f)
    if model == "synthetic":
        assert len({want[k][0].tobytes() for k in range(N)}) == N
    m.close()


def test_overlap_keeps_first_batch(gpu):
    """run_device_async(A) -> detect_heads_device -> mars_run(B): the decode of A reads heads that B's graph overwrites; the
    head-writing layers of B wait for it, so A's boxes come out unchanged"""
    d, _ = camera_graph()
    B = 64
    m = gpu.Model(d, batch=B)
    nb = m.input_view(0).shape[1]
    xa = [lcg_frame(0xA0A00000 + f, nb) for f in range(B)]
    xb = [lcg_frame(0xB0B00000 + f, nb) for f in range(B)]
    for f in range(B):
        m.input_view(0)[f] = xa[f]
    m.run()
    want = m.detect_heads(conf=0.01)
    for f in range(B):
        m.input_view(0)[f] = xb[f]
    m.run()
    want_b = m.detect_heads(conf=0.01)
    assert all(want[f].tobytes() != want_b[f].tobytes() for f in range(B))
    for f in range(B):
        m.input_view(0)[f] = xa[f]
    m.upload()
    for _ in range(2):
        m.run_device(sync=False)
        m.detect_heads_device(conf=0.01)
        for f in range(B):
            m.input_view(0)[f] = xb[f]
        m.run()  # upload B + graph B on the main stream, no host wait in between
        got = m.detect_results()
        for f in range(B):
            assert got[f].tobytes() == want[f].tobytes(), f
        for f in range(B):
            m.input_view(0)[f] = xa[f]
        m.upload()
    m.close()
