"""Instance masks on the device (mars_hip_detect_seg, mars_yolo_masks), bit for bit against the numpy restatement of include/mars_hip.h
"Instance masks" (tests/segref.py).  The expected detections and their origins come from the DFL restatement of tests/test_gpu_yolo_dfl.py
and a literal restatement of the reference's exchange sort + greedy NMS that carries each record's index (checked against the reference's
own NMS wherever it is used)."""
import ctypes as C

import numpy as np
import pytest

import marsfile
import segref
from conftest import lcg_frame
from test_gpu_yolo_dfl import _conv, _write_heads, decode_dfl, head_bytes
from test_gpu_yolo_heads import letterbox_map, nms, sig_table

pytestmark = pytest.mark.gpu

F32 = np.float32
R, NC = 4, 3  # reg_max and classes of the hand-built graphs


def origins_dfl(heads, conf):
    """the prediction index (cells of the heads before + cell) of every candidate decode_dfl(heads) lists, in its order"""
    out, base = [], 0
    for _, cls, _, cs, _ in heads:
        nc, H, W = cls.shape
        cl = cls.reshape(nc, H * W).astype(np.int32)
        c = sig_table(cs)[cl[np.argmax(cl, axis=0), np.arange(H * W)] + 128]
        out.append(base + np.nonzero(c >= F32(conf))[0])
        base += H * W
    return np.concatenate(out)[:1000]


def sort_nms_idx(cand, thresh):
    """indices into cand of the records the reference's `for i: for j > i: if d[j].conf > d[i].conf swap` + greedy class-wise suppression keeps,
    in its order; the IoU in the tail's float32 expression order"""
    n = len(cand)
    conf, idx = cand["conf"].tolist(), list(range(n))
    for i in range(n):
        for j in range(i + 1, n):
            if conf[j] > conf[i]:
                conf[i], conf[j], idx[i], idx[j] = conf[j], conf[i], idx[j], idx[i]
    d = cand[idx]
    x, y, w, h, cls = d["x"], d["y"], d["w"], d["h"], d["cls"]
    x1, y1, x2, y2, area = x - w / F32(2), y - h / F32(2), x + w / F32(2), y + h / F32(2), w * h
    removed, keep = np.zeros(n, dtype=bool), []
    for i in range(n):
        if removed[i]:
            continue
        keep.append(idx[i])
        iw = np.maximum(F32(0), np.minimum(x2[i], x2) - np.maximum(x1[i], x1))
        ih = np.maximum(F32(0), np.minimum(y2[i], y2) - np.maximum(y1[i], y1))
        inter = iw * ih
        uni = ((area[i] + area) - inter) + F32(1e-6)
        hit = (inter / uni > F32(thresh)) & (cls == cls[i])
        hit[:i + 1] = False
        removed |= hit
    return np.array(keep, dtype=np.int64)


def seg_graph(nm, nchw, S, in_c=16):
    """S x S x in_c input -> a chain of 1x1 stride-2 convolutions down to S / 32; DFL heads (box 4 R, class NC, concat) and a coefficient
    convolution of nm channels at S / 8, S / 16 and S / 32, prototypes of nm channels at S / 4.  The four header outputs: the concats and
    the prototypes; every coefficient tensor is read by a RESHAPE alone.  -> file, [(box, class, concat, grid, stride)], [coef], proto"""
    rng = np.random.default_rng(nm * 4 + nchw * 2 + (S > 64))
    G = marsfile.Graph()
    fmt = marsfile.NCHW if nchw else marsfile.NHWC
    shp = (lambda c, h, w: [1, c, h, w]) if nchw else (lambda c, h, w: [1, h, w, c])
    x = G.tensor(shp(in_c, S, S), fmt=fmt, scale=0.05)
    feat, t, sc = {}, x, 0.25  # every convolution's output scale is 3 x its input's: the int8 spread stays near 40 steps
    for s in (2, 4, 8, 16, 32):
        n = G.tensor(shp(in_c, S // s, S // s), fmt=fmt, scale=sc)
        _conv(G, rng, t, n, in_c, in_c, 1, 2, nchw)
        feat[s], t, sc = (n, sc), n, sc * 3
    heads, coefs = [], []
    for s in (8, 16, 32):
        g, (p, ps) = S // s, feat[s]
        b = G.tensor(shp(4 * R, g, g), fmt=fmt, scale=ps * 3)
        c = G.tensor(shp(NC, g, g), fmt=fmt, scale=ps * 3)
        _conv(G, rng, p, b, 4 * R, in_c, 1, 1, nchw)
        _conv(G, rng, p, c, NC, in_c, 1, 1, nchw)
        cat = G.tensor(shp(4 * R + NC, g, g), fmt=fmt, scale=ps * 3)
        G.concat([b, c], cat, axis=1 if nchw else 3)
        cf = G.tensor(shp(nm, g, g), fmt=fmt, scale=ps * 3)
        _conv(G, rng, p, cf, nm, in_c, 1, 1, nchw)
        G.layer(marsfile.RESHAPE, [cf], [G.tensor([0, 0, 0, 0])])
        heads.append((b, c, cat, g, s))
        coefs.append(cf)
    pr = G.tensor(shp(nm, S // 4, S // 4), fmt=fmt, scale=feat[4][1] * 3)
    _conv(G, rng, feat[4][0], pr, nm, in_c, 1, 1, nchw)
    return G.serialise([x], [h[2] for h in heads] + [pr]), heads, coefs, pr


def chw_bytes(m, t, f, nchw):
    """tensor t of frame f as int8 [C][H][W] (mars_hip_read_tensor: the reference's bytes in the tag's order)"""
    s = m.tensor_desc(t).shape
    a = m.read_tensor(t, f).view(np.int8)
    return a.reshape(s[1], s[2], s[3]) if nchw else a.reshape(s[1], s[2], s[3]).transpose(2, 0, 1)


def expected_frame(gpu, hs, coef_arrs, coef_scales, proto_arr, proto_scale, S, conf, thresh=0.45, **seg):
    """hs as decode_dfl takes them -> (kept records, mask records, mask words, prediction indices of the kept records)"""
    cand, _ = decode_dfl(hs, gpu.DET_DTYPE, conf)
    org = origins_dfl(hs, conf)
    assert len(org) == len(cand)
    keep = sort_nms_idx(cand, thresh)
    kept = cand[keep]
    assert kept.tobytes() == nms(cand.copy(), thresh).tobytes(), "the test's own sort + NMS differs from the reference's"
    cells = np.cumsum([0] + [h[1].shape[1] * h[1].shape[2] for h in hs])
    rows, scales = [], []
    for o in org[keep]:
        k = int(np.searchsorted(cells, o, side="right")) - 1
        rows.append(coef_arrs[k].reshape(coef_arrs[k].shape[0], -1)[:, o - cells[k]])
        scales.append(F32(coef_scales[k]) * F32(proto_scale))
    recs, words = segref.mask_frame(kept, rows, scales, proto_arr, S, S, **seg)
    return kept, recs, words, org[keep]


def check(got, want, what):
    dets, recs, words, pw = got
    for f, (kept, wr, ww, _) in enumerate(want):
        assert dets[f].tobytes() == kept.tobytes(), (what, f, "detections")
        assert recs[f].tobytes() == wr.tobytes(), (what, f, recs[f], wr)
        assert np.array_equal(words[f], ww), (what, f, "words")
    assert words.shape[0] == len(want) and (pw + 31) // 32 == words.shape[-1]


def fill(m, seed, zero_frame=None):
    nb = m.input_view(0).shape[1]
    for f in range(m.batch):
        m.input_view(0)[f] = 0 if f == zero_frame else lcg_frame(seed + f, nb)


DFL_KW = dict(conf=0.6, box_scales=0.05, cls_scales=0.02)  # an all-zero input gives class bytes of 0: confidence 0.5, no candidate


def model_expected(gpu, m, heads, coefs, pr, nchw, S, seg_kw, dfl_kw=DFL_KW):
    want = []
    for f in range(m.batch):
        hs = []
        for b, c, cat, _, s in heads:
            bb, cb = head_bytes(gpu, m, f, b, c, cat, nchw)
            hs.append((np.ascontiguousarray(bb), np.ascontiguousarray(cb), dfl_kw["box_scales"], dfl_kw["cls_scales"], s))
        ca = [np.ascontiguousarray(chw_bytes(m, t, f, nchw)) for t in coefs]
        want.append(expected_frame(gpu, hs, ca, [m.tensor_desc(t).scale for t in coefs], np.ascontiguousarray(chw_bytes(m, pr, f, nchw)),
                                   m.tensor_desc(pr).scale, S, dfl_kw["conf"], **seg_kw))
    return want


@pytest.mark.parametrize("fusion", [0, 1])
@pytest.mark.parametrize("nchw", [False, True])
@pytest.mark.parametrize("nm", [1, 4, 32, 33, 64])
def test_hand_built_graphs(gpu, nm, nchw, fusion):
    """graph -> heads -> boxes -> masks at batch 3 (frame 1 has no detection), 64 x 64 (prototypes 16 x 16) and 160 x 160 (40 x 40)"""
    for S in (64, 160):
        d, heads, coefs, pr = seg_graph(nm, nchw, S)
        m = gpu.Model(d, batch=3, fusion=fusion)
        fill(m, 0x5E600000 + S, zero_frame=1)
        m.run()
        plain = m.detect_dfl(**DFL_KW)
        for seg_kw in (dict(max_per_frame=16), dict(max_per_frame=3, logit_min=5000.0)):
            got = m.detect_seg(gpu.seg_opts(coefs, pr, **seg_kw), **DFL_KW)
            want = model_expected(gpu, m, heads, coefs, pr, nchw, S, seg_kw)
            check(got, want, (nm, nchw, fusion, S, seg_kw))
            assert all(a.tobytes() == b.tobytes() for a, b in zip(got[0], plain))
            assert len(want[1][0]) == 0 and not got[2][1].any() and (got[1][1]["det"] == -1).all()
            assert len(want[0][0]) > 3 and want[0][1]["area"].max() > 0
            assert got[2].shape == (3, seg_kw["max_per_frame"], S // 4, (S // 4 + 31) // 32) and got[3] == S // 4
        m.close()


def test_result_block_grows_and_is_reused(gpu):
    """one model, max_per_frame 1 -> 64 (the cap: the result block has to grow) -> 1 (the larger block is kept and holds the smaller layout):
    every call's boxes and masks are the restatement's, the stage's device time is there after each, and nothing can be fetched before the first"""
    S, nm, nchw = 64, 4, False
    d, heads, coefs, pr = seg_graph(nm, nchw, S)
    m = gpu.Model(d, batch=3)
    with pytest.raises(gpu.MarsError) as e:
        m.mask_results()
    assert e.value.code == gpu.MARS_ERR_INVALID_TENSOR and gpu.lib().mars_hip_mask_ms(m.p) < 0
    fill(m, 0x5E600000 + S, zero_frame=1)
    m.run()
    for n in (1, 64, 1):
        seg_kw = dict(max_per_frame=n)
        got = m.detect_seg(gpu.seg_opts(coefs, pr, **seg_kw), **DFL_KW)
        want = model_expected(gpu, m, heads, coefs, pr, nchw, S, seg_kw)
        check(got, want, ("growth", n))
        assert got[2].shape == (3, n, S // 4, 1) and len(want[0][0]) > 1
        assert gpu.lib().mars_hip_mask_ms(m.p) >= 0
    m.close()


@pytest.mark.parametrize("nchw", [False, True])
@pytest.mark.parametrize("nm", [4, 32])
def test_chosen_bytes(gpu, nm, nchw):
    """bytes written into the heads, the coefficient tensors and the prototypes: every cell its own coefficient row, two class-byte levels over
    all cells (the tail's tie-queue replay decides the order), more kept boxes than max_per_frame, a min_conf between the two levels, dots
    of exactly 0 inside the rectangles; the same masks with and without src = (w, h), the detections those of detect_dfl"""
    S, B = 64, 3
    d, heads, coefs, pr = seg_graph(nm, nchw, S)
    m = gpu.Model(d, batch=B)
    fill(m, 7)
    m.run()
    rng = np.random.default_rng(17 + nm)
    frames = []
    for f in range(B):
        arrs, ca = [], []
        for _, _, _, g, _ in heads:
            ab = rng.integers(-128, 128, (4 * R, g, g), dtype=np.int8)
            ac = rng.integers(-128, 128, (NC, g, g), dtype=np.int8)
            if f == 0:
                ac[:] = -128
                ac[1] = np.where(rng.integers(0, 2, (g, g)) == 1, 40, 20)
            elif f == 1:
                ac[:] = -128  # nothing passes
            arrs.append((ab, ac))
            ca.append(rng.integers(-128, 128, (nm, g, g), dtype=np.int8))
        rows = np.concatenate([a.reshape(nm, -1) for a in ca], axis=1).T
        assert len({r.tobytes() for r in rows}) == len(rows) == 84
        pa = rng.integers(-128, 128, (nm, S // 4, S // 4), dtype=np.int8)
        ys, xs = np.mgrid[0:S // 4, 0:S // 4]
        pa[:, (xs + ys) % 3 == 0] = 0
        _write_heads(gpu, m, f, heads, nchw, arrs)
        for t, a in zip(coefs + [pr], ca + [pa]):
            m.write_tensor(t, a if nchw else a.transpose(1, 2, 0), f)
        frames.append((arrs, ca, pa))
    kw = dict(conf=0.6, box_scales=0.3, cls_scales=0.05)
    cs, ps = [0.5, 0.25, 0.125], 0.0625
    mid = float(sig_table(0.05)[30 + 128])  # between the confidences of bytes 20 and 40
    plain, mapped = m.detect_dfl(**kw), m.detect_dfl(src=(1280, 720), **kw)
    for seg_kw in (dict(max_per_frame=5), dict(max_per_frame=64, min_conf=mid), dict(max_per_frame=16, logit_min=-3.0)):
        want = []
        for f in range(B):
            arrs, ca, pa = frames[f]
            hs = [(ab, ac, kw["box_scales"], kw["cls_scales"], s) for (ab, ac), (_, _, _, _, s) in zip(arrs, heads)]
            want.append(expected_frame(gpu, hs, ca, cs, pa, ps, S, kw["conf"], **seg_kw))
        kept0, recs0 = want[0][0], want[0][1]
        taken = int((recs0["det"] >= 0).sum())
        assert len(set(kept0["conf"])) == 2 and len(kept0) > 5 and len(want[1][0]) == 0
        if "min_conf" in seg_kw:
            assert 0 < taken < len(kept0) and taken == int((kept0["conf"] >= F32(mid)).sum())
        else:
            assert taken == min(len(kept0), seg_kw["max_per_frame"])
        zero_inside = sum(1 for r in recs0[:taken] for y in range(r["y0"], r["y1"]) for x in range(r["x0"], r["x1"]) if (x + y) % 3 == 0)
        assert zero_inside > 0 and recs0["area"].max() > 0
        opts = gpu.seg_opts(coefs, pr, coef_scales=cs, proto_scale=ps, **seg_kw)
        got = m.detect_seg(opts, **kw)
        check(got, want, (nm, nchw, seg_kw))
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got[0], plain))
        got2 = m.detect_seg(opts, src=(1280, 720), **kw)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got2[0], mapped))
        assert all(a.tobytes() == letterbox_map(b, 1280, 720, S, S).tobytes() for a, b in zip(got2[0], plain))
        assert got2[1].tobytes() == got[1].tobytes() and np.array_equal(got2[2], got[2])
    m.close()


@pytest.mark.parametrize("nm", [1, 4, 32, 33, 64])
@pytest.mark.parametrize("ph, pw", [(16, 16), (40, 40), (5, 33)])
def test_host_pointer_form(gpu, nm, ph, pw):
    rng = np.random.default_rng(nm * 100 + pw)
    proto = rng.integers(-128, 128, (nm, ph, pw), dtype=np.int8)
    proto[:, ph // 2, pw // 2] = 0
    for n in (0, 1, 16, 17, 64):
        coefs = rng.integers(-128, 128, (n, nm), dtype=np.int8)
        boxes = np.zeros(n, dtype=gpu.DET_DTYPE)
        boxes["x"], boxes["y"] = rng.uniform(-8, 72, n), rng.uniform(-8, 72, n)
        boxes["w"], boxes["h"] = rng.uniform(0, 70, n), rng.uniform(0, 70, n)
        boxes["conf"] = rng.uniform(0, 1, n)
        if n:
            boxes[0] = (32, 32, 64, 64, 0.0, 0)  # the whole map, a confidence of 0: the host form takes every box
        for lm in (0.0, 0.7):
            recs, words = gpu.masks(coefs, proto, boxes, 64, 64, 0.01, lm)
            if n == 0:
                assert recs.shape == (0,) and words.shape == (0, ph, (pw + 31) // 32)
                continue
            wr, ww = segref.mask_frame(boxes, coefs, [0.01] * n, proto, 64, 64, logit_min=lm, max_per_frame=n, take_all=True)
            assert recs.tobytes() == wr.tobytes(), (nm, ph, pw, n, lm)
            assert np.array_equal(words, ww), (nm, ph, pw, n, lm)
            assert np.array_equal(gpu.unpack_masks(words, pw), segref.unpack(ww, pw))
    for bad in (dict(s=0.0), dict(s=-1.0), dict(s=float("nan")), dict(lm=float("inf")), dict(in_w=0)):
        with pytest.raises(ValueError):
            gpu.masks(np.zeros((1, nm), np.int8), proto, np.zeros(1, gpu.DET_DTYPE), bad.get("in_w", 64), 64, bad.get("s", 0.01), bad.get("lm", 0.0))


def test_host_pointer_form_limits(gpu):
    box = np.zeros(1, gpu.DET_DTYPE)
    with pytest.raises(ValueError):
        gpu.masks(np.zeros((1, 65), np.int8), np.zeros((65, 4, 4), np.int8), box, 64, 64, 0.01)
    with pytest.raises(ValueError):
        gpu.masks(np.zeros((65, 4), np.int8), np.zeros((4, 4, 4), np.int8), np.zeros(65, gpu.DET_DTYPE), 64, 64, 0.01)


def test_async_hand_off(gpu):
    """run_device_async(A) -> detect_seg_device -> mars_run(B) with no host wait in between: the tail of A reads head, coefficient and prototype
    tensors that B's graph overwrites; the layers of B that write them wait, so every batch's boxes and masks equal run / sync / detect_seg"""
    S, B, nm = 64, 16, 32
    d, heads, coefs, pr = seg_graph(nm, True, S)
    m = gpu.Model(d, batch=B)
    nb = m.input_view(0).shape[1]
    xs = [[lcg_frame(0xA5A00000 + 0x100000 * k + f, nb) for f in range(B)] for k in range(3)]
    opts = gpu.seg_opts(coefs, pr, max_per_frame=8)
    want = []
    for k in range(3):
        for f in range(B):
            m.input_view(0)[f] = xs[k][f]
        m.run()
        want.append(m.detect_seg(opts, **DFL_KW))
    assert sum(want[0][1][f].tobytes() != want[1][1][f].tobytes() for f in range(B)) > B // 2
    check(want[2], model_expected(gpu, m, heads, coefs, pr, True, S, dict(max_per_frame=8)), "sync")
    for f in range(B):
        m.input_view(0)[f] = xs[0][f]
    m.upload()
    for k in range(3):
        m.run_device(sync=False)
        m.detect_seg_device(opts, **DFL_KW)
        nxt = xs[(k + 1) % 3]
        for f in range(B):
            m.input_view(0)[f] = nxt[f]
        m.run()  # upload + graph of the next batch on the main stream, no host wait in between
        dets = m.detect_results()
        recs, words, _ = m.mask_results()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(dets, want[k][0])), k
        assert recs.tobytes() == want[k][1].tobytes() and np.array_equal(words, want[k][2]), k
        m.upload()
    assert gpu.lib().mars_hip_mask_ms(m.p) > 0
    m.close()


def test_refusals(gpu):
    INV = gpu.MARS_ERR_INVALID_TENSOR
    S = 64
    d, heads, coefs, pr = seg_graph(4, False, S)
    m = gpu.Model(d, batch=2)
    with pytest.raises(gpu.MarsError) as e:
        m.mask_results()  # before any seg call
    assert e.value.code == INV
    fill(m, 3)
    m.run()
    d8, heads8, coefs8, pr8 = seg_graph(8, False, S)  # the same tensor numbering, other channel counts
    assert (coefs8, pr8) == (coefs, pr)
    hdr, tensors, _ = marsfile.parse(d)
    weight = next(i for i, t in enumerate(tensors) if t["size"])
    box0, cls0 = heads[0][0], heads[0][1]
    bad = [
        dict(max_per_frame=65), dict(max_per_frame=-1),
        dict(coef_scales=-1.0), dict(proto_scale=-0.5), dict(coef_scales=float("nan")), dict(proto_scale=float("inf")),
        dict(logit_min=float("nan")), dict(min_conf=float("inf")),
        dict(coefs=[coefs[1], coefs[0], coefs[2]]),   # a coefficient grid that differs from its head's
        dict(coefs=[coefs[0], coefs[1], box0]),       # 16 channels on head 0's grid: not nm, not head 2's grid
        dict(proto=box0),                              # nm would be 16: the coefficient tensors have 4
        dict(proto=weight), dict(coefs=[weight, coefs[1], coefs[2]]),
        dict(proto=hdr["inputs"][0]),                  # a graph input: no convolution wrote it
        dict(proto=9999), dict(proto=-1), dict(coefs=[coefs[0], coefs[1], 9999]),
    ]
    for kw in bad:
        o = gpu.seg_opts(kw.pop("coefs", coefs), kw.pop("proto", pr), **kw)
        with pytest.raises(gpu.MarsError) as e:
            m.detect_seg_device(o, **DFL_KW)
        assert e.value.code == INV, kw
    with pytest.raises(gpu.MarsError) as e:
        m.detect_seg_device(None, **DFL_KW)
    assert e.value.code == INV
    with pytest.raises(gpu.MarsError) as e:  # what detect_dfl refuses
        m.detect_seg_device(gpu.seg_opts(coefs, pr), heads=[(cls0, box0)])
    assert e.value.code == INV
    with pytest.raises(gpu.MarsError) as e:
        m.mask_results()  # still none
    assert e.value.code == INV
    m.pipe_open(download_outputs=False, detect=True, dfl_heads=gpu.yolo_dfl_heads(**DFL_KW))
    with pytest.raises(gpu.MarsError) as e:
        m.detect_seg_device(gpu.seg_opts(coefs, pr), **DFL_KW)
    assert e.value.code == INV
    m.pipe_close()
    m.run()
    m.detect_seg(gpu.seg_opts(coefs, pr), **DFL_KW)  # and the good configuration passes
    m.close()
    d65, _, coefs65, pr65 = seg_graph(65, False, S)  # nm > 64
    m = gpu.Model(d65, batch=1)
    fill(m, 3)
    m.run()
    with pytest.raises(gpu.MarsError) as e:
        m.detect_seg_device(gpu.seg_opts(coefs65, pr65), **DFL_KW)
    assert e.value.code == INV
    m.close()


def test_twin_160(gpu):
    """synth_model(head="seg") at 160 x 160, batch 2: graph -> found heads -> masks, through the C entry point that fetches everything"""
    S, B = 160, 2
    d = gpu.synth_model(width_x16=4, input_hw=S, seed=1, head="seg")
    hdr, _, _ = marsfile.parse(d)
    coefs, pr = gpu.seg_twin_tensors(d)
    heads = [(b, c, o, None, s) for (b, c, s), o in zip(gpu.find_yolo_dfl_heads(d)[0], hdr["outputs"])]
    m = gpu.Model(d, batch=B)
    fill(m, 0x5EED0000)
    m.run()
    conf = 0.1
    opts = gpu.seg_opts(coefs, pr)
    dets = np.zeros((B, gpu.MAX_DET), dtype=gpu.DET_DTYPE)
    counts = np.zeros(B, dtype=np.int32)
    recs = np.zeros((B, 16), dtype=gpu.MASK_DTYPE)
    words = np.zeros((B, 16, S // 4, 2), dtype=np.uint32)
    rc = gpu.lib().mars_hip_detect_seg(m.p, C.byref(gpu.yolo_dfl_heads(conf=conf)), C.byref(opts), dets.ctypes.data,
                                       counts.ctypes.data_as(C.POINTER(C.c_int)), recs.ctypes.data, words.ctypes.data)
    assert rc == 0
    kw = dict(conf=conf, box_scales=m.tensor_desc(heads[0][0]).scale, cls_scales=m.tensor_desc(heads[0][1]).scale)
    assert all(m.tensor_desc(b).scale == kw["box_scales"] and m.tensor_desc(c).scale == kw["cls_scales"] for b, c, _, _, _ in heads)
    want = model_expected(gpu, m, heads, coefs, pr, False, S, dict(max_per_frame=16), kw)
    check(([dets[f, :counts[f]] for f in range(B)], recs, words, S // 4), want, "twin")
    assert sum(len(w[0]) for w in want) > 0 and sum(int(w[1]["area"].sum()) for w in want) > 0
    m.close()
