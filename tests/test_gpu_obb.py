"""Oriented boxes on the device (mars_hip_detect_obb, mars_yolo_obb_nms), byte for byte against the numpy restatement of include/mars_hip.h
"Oriented boxes" (tests/obbref.py) on the bytes the model holds.  Every comparison is byte equality."""
import ctypes as C

import numpy as np
import pytest

import marsfile
import obbref
from conftest import lcg_frame
from test_gpu_pose import chw_bytes, fill, pose_graph
from test_gpu_yolo_dfl import _write_heads, head_bytes
from test_roi_cpu import roi_crop_np, roi_select_np

pytestmark = pytest.mark.gpu

F32 = np.float32
R, NC = 4, 3  # reg_max and classes of the hand-built graphs (tests/test_gpu_pose.py)
DFL_KW = dict(conf=0.6, box_scales=0.05, cls_scales=0.02)  # an all-zero input gives class bytes of 0: confidence 0.5, no candidate
CAP_KW = dict(conf=0.3, box_scales=0.05, cls_scales=0.02)  # ... and a threshold below it: nearly every cell is a candidate


def obb_graph(nchw, S, nm=0, f32_extra=False):
    """the hand-built DFL graph of tests/test_gpu_pose.py with a "keypoint" convolution of ONE channel per scale: the angle tensors, each
    read by a RESHAPE alone.  -> file, [(box, class, concat, grid, stride)], [angle tensor], [coefficient tensor], prototype tensor"""
    return pose_graph(1, 1, nchw, S, nm=nm, f32_extra=f32_extra)


def frame_heads(gpu, m, f, heads, angs, nchw, dfl_kw, ang_scales=None):
    hs = []
    for k, ((b, c, cat, _, s), t) in enumerate(zip(heads, angs)):
        bb, cb = head_bytes(gpu, m, f, b, c, cat, nchw)
        a = ang_scales[k] if ang_scales is not None else m.tensor_desc(t).scale
        hs.append((np.ascontiguousarray(bb), np.ascontiguousarray(cb), np.ascontiguousarray(chw_bytes(m, t, f, nchw))[0], dfl_kw["box_scales"],
                   dfl_kw["cls_scales"], a, s))
    return hs


def model_expected(gpu, m, heads, angs, nchw, S, dfl_kw=DFL_KW, ang_scales=None, agnostic=False, src=None, thresh=0.45):
    """the expectation of every frame from the bytes the model holds: [(obb records, enclosing rectangles, candidates)]"""
    return [obbref.frame(frame_heads(gpu, m, f, heads, angs, nchw, dfl_kw, ang_scales), dfl_kw["conf"], thresh, agnostic, src, (S, S))
            for f in range(m.batch)]


def check(got, want, what):
    dets, boxes = got
    assert len(dets) == len(boxes) == len(want)
    for f, (wb, wd, _) in enumerate(want):
        assert len(boxes[f]) == len(dets[f]) == len(wb), (what, f, "counts", len(boxes[f]), len(dets[f]), len(wb))
        assert boxes[f].tobytes() == wb.tobytes(), (what, f, "obb records")
        assert dets[f].tobytes() == wd.tobytes(), (what, f, "detections")


@pytest.mark.parametrize("fusion", [0, None])
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("S", [64, 256])
@pytest.mark.parametrize("nchw", [False, True])
def test_hand_built_graphs(gpu, nchw, S, batch, fusion):
    """graph -> heads -> oriented boxes.  S = 64: 84 predictions (partial waves), frame 1 of a batch of 3 has no candidate.  S = 256: 1 344
    predictions and a threshold low enough that the 1 000-candidate cap bites"""
    d, heads, angs, _, _ = obb_graph(nchw, S)
    m = gpu.Model(d, batch=batch, fusion=fusion)
    fill(m, 0x0BB00000 + S, zero_frame=1 if S == 64 else None)
    m.run()
    kw = DFL_KW if S == 64 else CAP_KW
    got = m.detect_obb(gpu.obb_opts(angs), **kw)
    want = model_expected(gpu, m, heads, angs, nchw, S, kw)
    check(got, want, (nchw, S, batch, fusion))
    assert sum(len(w[0]) for w in want) > 0
    if S == 256:
        assert all(w[2] > 1000 for w in want), [w[2] for w in want]  # the cap bites
        assert any(len(set(w[0]["angle"].tolist())) > 8 for w in want)
    elif batch == 3:
        assert len(want[1][0]) == 0 and len(got[1][1]) == 0
    # the prediction index names the cell the box was made from
    cells = np.cumsum([0] + [g * g for _, _, _, g, _ in heads])
    for wb, _, _ in want:
        assert ((wb["pred"] >= 0) & (wb["pred"] < cells[-1])).all()
    m.close()


def test_result_block_follows_the_batch(gpu):
    """one model at batch 1 -> 3 -> 1 (mars_hip_set_batch between the calls): the result block and the angle tables inside it are there for
    every batch, every call's boxes are the restatement's, the stage's device time is there after each, and nothing can be fetched before
    the first"""
    S, nchw = 64, False
    d, heads, angs, _, _ = obb_graph(nchw, S)
    m = gpu.Model(d, batch=1)
    with pytest.raises(gpu.MarsError) as e:
        m.obb_results()
    assert e.value.code == gpu.MARS_ERR_INVALID_TENSOR and m.obb_ms() < 0
    for batch in (1, 3, 1):
        m.set_batch(batch)
        fill(m, 0x0BB00000 + S, zero_frame=1)
        m.run()
        got = m.detect_obb(gpu.obb_opts(angs), **DFL_KW)
        want = model_expected(gpu, m, heads, angs, nchw, S, DFL_KW)
        check(got, want, ("growth", batch))
        assert len(want) == batch and len(want[0][0]) > 0
        assert m.obb_ms() >= 0
    m.close()


def test_flags_and_overrides(gpu):
    """angle_scales overrides, MARS_OBB_AGNOSTIC on and off, src = 1280 x 720, nms_thresh 0.3 and 0.7: one graph, many calls"""
    S, nchw = 128, False
    d, heads, angs, _, _ = obb_graph(nchw, S)
    m = gpu.Model(d, batch=2)
    fill(m, 0x0BB10000)
    m.run()
    kw = dict(DFL_KW, conf=0.52)
    own = [m.tensor_desc(t).scale for t in angs]
    over = [0.05, 0.02, 0.01]
    kept = {}
    for name, ang_scales, agn, src, th in (("plain", None, False, None, 0.45), ("scales", over, False, None, 0.45), ("agnostic", None, True, None, 0.45),
                                           ("src", None, False, (1280, 720), 0.45), ("t0.3", None, False, None, 0.3), ("t0.7", None, False, None, 0.7),
                                           ("all", over, True, (1280, 720), 0.7)):
        o = gpu.obb_opts(angs, angle_scales=ang_scales, agnostic=agn)
        call_kw = dict(kw, thresh=th, **({"src": src} if src else {}))
        got = m.detect_obb(o, **call_kw)
        want = model_expected(gpu, m, heads, angs, nchw, S, kw, ang_scales, agn, src, th)
        check(got, want, name)
        kept[name] = [w[0] for w in want]
    assert over != own
    assert any(a["angle"].tobytes() != b["angle"].tobytes() for a, b in zip(kept["plain"], kept["scales"])), "the overrides change no angle"
    assert any(a["pred"].tolist() != b["pred"].tolist() for a, b in zip(kept["plain"], kept["agnostic"])), "the flag changes nothing on this input"
    assert all(len(a) <= len(b) for a, b in zip(kept["agnostic"], kept["plain"]))
    assert any(len(a) < len(b) < len(c) for a, b, c in zip(kept["t0.3"], kept["plain"], kept["t0.7"]))
    for a, b in zip(kept["plain"], kept["src"]):  # the mapping moves the boxes and leaves the angle, the order and the kept set
        assert a["pred"].tolist() == b["pred"].tolist() and np.array_equal(a["angle"], b["angle"]) and not np.array_equal(a["x"], b["x"])
        assert np.array_equal(b["w"], a["w"] * F32(10.0)) and np.array_equal(b["h"], a["h"] * F32(10.0))  # 128 from 1280: BOTH sides by rx = 10
    m.close()


def crafted(n, ncls, seed, levels=4):
    """n boxes on a square field of side 12 sqrt(n) (about as crowded for every n), sides 5 .. 40, every angle of the rule's range, confidences from a few levels only (the index tie-break
    decides), classes 0 .. ncls - 1 spread so that more classes than buckets share a bucket"""
    rng = np.random.default_rng(seed)
    b = np.zeros(n, dtype=obbref.OBB_DTYPE)
    b["x"], b["y"] = rng.uniform(0, 12 * n ** 0.5, n), rng.uniform(0, 12 * n ** 0.5, n)
    b["w"], b["h"] = rng.uniform(5, 40, n), rng.uniform(5, 40, n)
    b["angle"] = rng.uniform(-np.pi / 4, 3 * np.pi / 4, n)
    b["conf"] = rng.choice(np.linspace(0.3, 0.9, levels), n)
    b["cls"] = rng.integers(0, ncls, n)
    if ncls > 128:  # half of the boxes in classes 1 and 129: one bucket (class & 127), two classes that must not suppress each other
        b["cls"][:n // 2] = rng.choice([1, 129], n // 2)
    b["pred"] = rng.permutation(n) + 1000
    return b


@pytest.mark.parametrize("ncls", [1, 130])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_obb_nms_lists(gpu, n, ncls):
    b = crafted(n, ncls, n * 7 + ncls)
    for T, agn in ((0.45, False), (0.3, True)):
        got = gpu.obb_nms(b, T, agnostic=agn)
        want = obbref.nms_list(b, T, agn)
        assert got.tobytes() == want.tobytes(), (n, ncls, T, agn, len(got), len(want))
    if n >= 63:
        want = obbref.nms_list(b, 0.45)
        assert len(want) < n and len(set(want["conf"].tolist())) < len(want)  # something is suppressed, and ties are kept side by side
        if ncls == 130:  # classes 1 and 129 share a bucket and do not suppress each other: taking them for one class keeps fewer
            merged = b.copy()
            merged["cls"][merged["cls"] == 129] = 1
            assert len(obbref.nms_list(merged, 0.45)) < len(want)
    assert gpu.obb_nms(b, 0.0).tobytes() == obbref.nms_list(b, 0.45).tobytes()  # a threshold of 0 is the default


def one(x, y, w, h, angle, conf, cls=0, pred=0):
    b = np.zeros(1, dtype=obbref.OBB_DTYPE)
    b[0] = (x, y, w, h, conf, cls, angle, pred)
    return b


def test_obb_nms_chain_zero_area_and_refusals(gpu):
    # A - B - C along a line, 20 x 20, 6 apart: A suppresses B, B would suppress C, A does not: C survives
    A, B, Cc = one(0, 0, 20, 20, 0.2, 0.9, pred=1), one(6, 0, 20, 20, 0.2, 0.8, pred=2), one(12, 0, 20, 20, 0.2, 0.7, pred=3)
    assert obbref.nms_list(np.concatenate([A, B]))["pred"].tolist() == [1] and obbref.nms_list(np.concatenate([B, Cc]))["pred"].tolist() == [2]
    assert obbref.nms_list(np.concatenate([A, Cc]))["pred"].tolist() == [1, 3]
    chain = np.concatenate([Cc, A, B])  # (not in order: the sort puts A first)
    got = gpu.obb_nms(chain)
    assert got["pred"].tolist() == [1, 3] and got.tobytes() == obbref.nms_list(chain).tobytes()
    # zero-area boxes: a comparison with a NaN operand is false, they suppress nothing and are not suppressed
    # (angle 0: sn = 0, so b = c = d = 0 exactly and the 10 x 0 pairs meet 0 / 0, not rounding noise)
    z = np.concatenate([one(5, 5, 0, 0, 0.0, 0.9, pred=1), one(5, 5, 0, 0, 0.0, 0.8, pred=2), one(5, 5, 10, 0, 0.0, 0.7, pred=3),
                        one(5, 5, 10, 0, 0.0, 0.6, pred=4), one(5, 5, 10, 10, 0.0, 0.5, pred=5), one(5, 5, 10, 10, 0.0, 0.4, pred=6)])
    got = gpu.obb_nms(z)
    assert got.tobytes() == obbref.nms_list(z).tobytes() and got["pred"].tolist() == [1, 2, 3, 4, 5]
    assert len(gpu.obb_nms(np.zeros(0, dtype=obbref.OBB_DTYPE))) == 0
    for bad in (one(0, 0, 1, 1, 0, float("nan")), one(0, 0, 1, 1, 0, -0.5), one(0, 0, 1, 1, 0, -0.0)):
        with pytest.raises(ValueError):
            gpu.obb_nms(np.concatenate([A, bad]))
    for kw in (dict(flags=2), dict(thresh=-0.1), dict(thresh=float("nan"))):
        with pytest.raises(ValueError):
            gpu.obb_nms(A, **kw)
    with pytest.raises(ValueError):
        gpu.obb_nms(crafted(1001, 1, 5))


def upright_iou(a, b):
    """the axis-aligned IoU of two mars_det_t records"""
    iw = min(a["x"] + a["w"] / 2, b["x"] + b["w"] / 2) - max(a["x"] - a["w"] / 2, b["x"] - b["w"] / 2)
    ih = min(a["y"] + a["h"] / 2, b["y"] + b["h"] / 2) - max(a["y"] - a["h"] / 2, b["y"] - b["h"] / 2)
    inter = max(iw, 0) * max(ih, 0)
    return inter / (a["w"] * a["h"] + b["w"] * b["h"] - inter)


def test_rotation_is_real(gpu):
    """two thin boxes, 40 x 2, about one centre: crossing at 90 degrees (angles -pi / 4 and pi / 4, the ends of the rule's first quarter) both
    are kept, parallel one is suppressed.  Their enclosing upright rectangles are the same square in the first case: an axis-aligned NMS
    of those suppresses the crossing pair too, so it fails here"""
    q = F32(np.pi / 4)
    cross = np.concatenate([one(50, 50, 40, 2, -q, 0.9, pred=1), one(50, 50, 40, 2, q, 0.8, pred=2)])
    par = np.concatenate([one(50, 50, 40, 2, q, 0.9, pred=1), one(50, 50, 40, 2, q, 0.8, pred=2)])
    for T in (0.3, 0.45, 0.7):
        assert gpu.obb_nms(cross, T)["pred"].tolist() == [1, 2]
        assert gpu.obb_nms(par, T)["pred"].tolist() == [1]
    e = obbref.enclosing(cross, obbref.cosf(cross["angle"]), obbref.sinf(cross["angle"]))
    assert upright_iou(e[0], e[1]) > 0.99
    # a near miss: parallel and half a length apart along their axis they still overlap; two widths apart across it they do not
    ux, uy = float(np.cos(q)), float(np.sin(q))
    along = np.concatenate([par[:1], one(50 + 10 * ux, 50 + 10 * uy, 40, 2, q, 0.8, pred=2)])
    across = np.concatenate([par[:1], one(50 - 4 * uy, 50 + 4 * ux, 40, 2, q, 0.8, pred=2)])
    assert gpu.obb_nms(along, 0.3).tobytes() == obbref.nms_list(along, 0.3).tobytes() and len(obbref.nms_list(along, 0.3)) == 1
    assert gpu.obb_nms(across, 0.3).tobytes() == obbref.nms_list(across, 0.3).tobytes() and len(obbref.nms_list(across, 0.3)) == 2


@pytest.mark.parametrize("nchw", [False, True])
def test_angle_extremes_on_written_bytes(gpu, nchw):
    """bytes written into the heads and the angle tensors: angle bytes of -128 and 127 side by side (the ends of both tables) among random
    ones, sharp box bins (small boxes, few suppressed), class bytes at two levels (ties), under an angle scale that does not saturate"""
    S = 64
    d, heads, angs, _, _ = obb_graph(nchw, S)
    m = gpu.Model(d, batch=2)
    fill(m, 5)
    m.run()
    rng = np.random.default_rng(41 + nchw)
    for f in range(2):
        arrs = []
        for (_, _, _, g, _), t in zip(heads, angs):
            ab = np.full((4 * R, g, g), -128, dtype=np.int8)
            pos = rng.integers(0, 3, (4, g, g))
            for s in range(4):
                np.put_along_axis(ab[s * R:(s + 1) * R], pos[s][None], 127, axis=0)
            ac = np.full((NC, g, g), -128, dtype=np.int8)
            np.put_along_axis(ac, rng.integers(0, NC, (1, g, g)), np.where(rng.integers(0, 2, (1, g, g)) == 1, 40, 20).astype(np.int8), axis=0)
            aa = rng.integers(-128, 128, (1, g, g), dtype=np.int8)
            aa[0, 0, 0::2], aa[0, 0, 1::2] = -128, 127
            arrs.append((ab, ac))
            m.write_tensor(t, aa if nchw else aa.transpose(1, 2, 0), f)
        _write_heads(gpu, m, f, heads, nchw, arrs)
    kw = dict(conf=0.55, box_scales=0.3, cls_scales=0.05)
    scales = [0.02, 0.03, 0.04]
    got = m.detect_obb(gpu.obb_opts(angs, angle_scales=scales), **kw)
    want = model_expected(gpu, m, heads, angs, nchw, S, kw, scales)
    check(got, want, nchw)
    _, at, _, _ = obbref.tables(scales[0])
    angles = np.concatenate([w[0]["angle"] for w in want])
    assert at[0] in angles and at[255] in angles and len(set(angles.tolist())) > 20
    m.close()


def test_downstream_crop_stage(gpu):
    """mars_hip_detect_results after the call holds the enclosing rectangles (check()), and mars_hip_crop_detections_device takes them: the
    second model's input equals the ROI restatement's crops of those rectangles"""
    S, W, H = 64, 98, 62
    d, heads, angs, _, _ = obb_graph(False, S)
    m = gpu.Model(d, batch=2)
    fill(m, 0x0BB20000)
    m.run()
    kw = dict(DFL_KW, conf=0.52)
    got = m.detect_obb(gpu.obb_opts(angs), src=(W, H), **kw)
    check(got, model_expected(gpu, m, heads, angs, False, S, kw, src=(W, H)), "src")
    d2 = gpu.synth_model(tiny=True, input_hw=160, seed=5)
    hdr, tensors, _ = marsfile.parse(d2)
    tin = hdr["inputs"][0]
    nhwc = tensors[tin]["fmt"] == marsfile.NHWC
    dst = gpu.Model(d2, batch=4)
    frames = np.stack([lcg_frame(0x201000 + f, W * H * 3) for f in range(2)])
    buf = gpu.DeviceBuffer(frames)
    m.detect_obb_device(gpu.obb_opts(angs), src=(W, H), **kw)
    dst.crop_detections(m, buf.ptr, gpu.roi_opts(W, H), device=True)
    rois, dropped = dst.roi_results()
    kept, want_dropped = roi_select_np(got[0], W, H, 4)
    assert len(kept) > 0 and [tuple(int(v) for v in r) for r in rois] == kept and dropped == want_dropped
    for k, (f, i, x0, y0, x1, y1) in enumerate(kept):
        want = roi_crop_np(frames[f].reshape(H, W, 3), (x0, y0, x1, y1), 160, 160, nhwc)
        assert np.array_equal(dst.read_tensor(tin, frame=k)[:want.size].view(np.int8), want), k
    buf.free()
    dst.close()
    m.close()


@pytest.mark.parametrize("nchw", [False, True])
def test_seg_and_obb_on_one_model(gpu, nchw):
    """a graph with a seg head and angle tensors: seg then obb, and obb then seg, each leaves the other's block alone; the detections are
    the last call's"""
    S, nm = 64, 32
    d, heads, angs, coefs, pr = obb_graph(nchw, S, nm=nm)
    m = gpu.Model(d, batch=3)
    fill(m, 0x0BB30000, zero_frame=1)
    m.run()
    so, oo = gpu.seg_opts(coefs, pr, max_per_frame=8), gpu.obb_opts(angs)
    obb_kw = dict(DFL_KW, conf=0.55)
    seg_alone = m.detect_seg(so, **DFL_KW)
    obb_alone = m.detect_obb(oo, **obb_kw)
    check(obb_alone, model_expected(gpu, m, heads, angs, nchw, S, obb_kw), "alone")
    assert (seg_alone[1]["det"] >= 0).any() and sum(len(b) for b in obb_alone[1]) > 0
    for first in ("seg", "obb"):
        for who in (first, "obb" if first == "seg" else "seg"):
            if who == "seg":
                m.detect_seg_device(so, **DFL_KW)
            else:
                m.detect_obb_device(oo, **obb_kw)
        dets = m.detect_results()
        last = obb_alone[0] if first == "seg" else seg_alone[0]
        assert all(a.tobytes() == b.tobytes() for a, b in zip(dets, last)), first
        recs, words, _ = m.mask_results()
        assert recs.tobytes() == seg_alone[1].tobytes() and np.array_equal(words, seg_alone[2]), first
        assert all(a.tobytes() == b.tobytes() for a, b in zip(m.obb_results(), obb_alone[1])), first
    m.close()


def test_second_run_and_async_hand_off(gpu):
    """run_device_async(A) -> detect_obb_device -> mars_run(B) with no host wait in between: the tail of A reads head and angle tensors that
    B's graph overwrites; the layers of B that write them wait, so every batch's boxes equal run / sync / detect_obb"""
    S, B = 64, 8
    d, heads, angs, _, _ = obb_graph(True, S)
    m = gpu.Model(d, batch=B)
    nb = m.input_view(0).shape[1]
    xs = [[lcg_frame(0x0BB40000 + 0x100000 * k + f, nb) for f in range(B)] for k in range(3)]
    opts = gpu.obb_opts(angs)
    want = []
    for k in range(3):
        for f in range(B):
            m.input_view(0)[f] = xs[k][f]
        m.run()
        want.append(m.detect_obb(opts, **DFL_KW))
    check(want[2], model_expected(gpu, m, heads, angs, True, S), "sync")
    assert sum(want[0][1][f].tobytes() != want[1][1][f].tobytes() for f in range(B)) > B // 2
    for f in range(B):
        m.input_view(0)[f] = xs[0][f]
    m.upload()
    for k in range(3):
        m.run_device(sync=False)
        m.detect_obb_device(opts, **DFL_KW)
        nxt = xs[(k + 1) % 3]
        for f in range(B):
            m.input_view(0)[f] = nxt[f]
        m.run()  # upload + graph of the next batch on the main stream, no host wait in between
        dets, boxes = m.detect_results(), m.obb_results()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(dets, want[k][0])), k
        assert all(a.tobytes() == b.tobytes() for a, b in zip(boxes, want[k][1])), k
        m.upload()
    assert m.obb_ms() > 0
    m.close()


def test_option_errors(gpu):
    """every refusal of mars_hip_detect_obb_device.  (A partly written tensor is a concat's output under the planner's row-split fusions, so
    it has at least two channels: the channel check below stands for it.)"""
    INV = gpu.MARS_ERR_INVALID_TENSOR
    S = 64
    d, heads, angs, _, _ = obb_graph(False, S, f32_extra=True)
    m = gpu.Model(d, batch=2)
    with pytest.raises(gpu.MarsError) as e:
        m.obb_results()  # before any obb call
    assert e.value.code == INV
    assert m.obb_ms() < 0
    fill(m, 3)
    m.run()
    hdr, tensors, _ = marsfile.parse(d)
    weight = next(i for i, t in enumerate(tensors) if t["size"])
    box0, cls0 = heads[0][0], heads[0][1]
    f32 = len(tensors) - 1
    assert tensors[f32]["dtype"] == marsfile.F32 and tensors[f32]["shape"] == tensors[angs[0]]["shape"]
    bad = [
        dict(angles=[f32, angs[1], angs[2]]),       # not int8 (the right shape)
        dict(angles=[angs[0], angs[1], cls0]),      # not 1 channel (3, on head 0's grid)
        dict(angles=[box0, angs[1], angs[2]]),      # not 1 channel (16, the right grid)
        dict(angles=[angs[1], angs[0], angs[2]]),   # a grid that differs from its head's
        dict(angles=[weight, angs[1], angs[2]]),    # weights
        dict(angles=[hdr["inputs"][0], angs[1], angs[2]]),  # no addressable bytes: no convolution wrote it
        dict(angles=[angs[0], angs[1], 9999]), dict(angles=[-1, angs[1], angs[2]]),
        dict(angle_scales=-1.0), dict(angle_scales=float("nan")), dict(angle_scales=float("inf")), dict(angle_scales=[0.5, -0.5, 0.5]),
        dict(flags=2), dict(flags=0x80000000), dict(flags=3),
    ]
    for kw in bad:
        what = dict(kw)
        o = gpu.obb_opts(kw.pop("angles", angs), **kw)
        with pytest.raises(gpu.MarsError) as e:
            m.detect_obb_device(o, **DFL_KW)
        assert e.value.code == INV, what
    with pytest.raises(gpu.MarsError) as e:
        m.detect_obb_device(None, **DFL_KW)  # NULL options
    assert e.value.code == INV
    with pytest.raises(gpu.MarsError) as e:  # what detect_dfl refuses
        m.detect_obb_device(gpu.obb_opts(angs), heads=[(cls0, box0)])
    assert e.value.code == INV
    with pytest.raises(gpu.MarsError) as e:
        m.obb_results()  # still none
    assert e.value.code == INV
    m.pipe_open(download_outputs=False, detect=True, dfl_heads=gpu.yolo_dfl_heads(**DFL_KW))
    with pytest.raises(gpu.MarsError) as e:
        m.detect_obb_device(gpu.obb_opts(angs), **DFL_KW)  # an open pipe
    assert e.value.code == INV
    m.pipe_close()
    m.run()
    m.detect_obb(gpu.obb_opts(angs), **DFL_KW)  # and the good configuration passes
    m.close()


def test_twin_640(gpu):
    """synth_model(head="obb") at 640 x 640, batch 2: graph -> found heads -> oriented boxes, through the C entry point that fetches everything"""
    S, B = 640, 2
    d = gpu.synth_model(width_x16=4, input_hw=S, seed=1, head="obb")
    hdr, _, _ = marsfile.parse(d)
    angs = gpu.obb_twin_tensors(d)
    heads = [(b, c, o, None, s) for (b, c, s), o in zip(gpu.find_yolo_dfl_heads(d)[0], hdr["outputs"])]
    m = gpu.Model(d, batch=B)
    fill(m, 0x5EED0000)
    m.run()
    conf = 0.1
    dets = np.zeros((B, gpu.MAX_DET), dtype=gpu.DET_DTYPE)
    counts = np.zeros(B, dtype=np.int32)
    boxes = np.zeros((B, gpu.MAX_DET), dtype=gpu.OBB_DTYPE)
    rc = gpu.lib().mars_hip_detect_obb(m.p, C.byref(gpu.yolo_dfl_heads(conf=conf)), C.byref(gpu.obb_opts(angs)), dets.ctypes.data,
                                       counts.ctypes.data_as(C.POINTER(C.c_int)), boxes.ctypes.data)
    assert rc == 0
    kw = dict(conf=conf, box_scales=m.tensor_desc(heads[0][0]).scale, cls_scales=m.tensor_desc(heads[0][1]).scale)
    assert all(m.tensor_desc(b).scale == kw["box_scales"] and m.tensor_desc(c).scale == kw["cls_scales"] for b, c, _, _, _ in heads)
    want = model_expected(gpu, m, heads, angs, False, S, kw)
    check(([dets[f, :counts[f]] for f in range(B)], [boxes[f, :counts[f]] for f in range(B)]), want, "twin")
    assert all(len(w[0]) > 0 for w in want) and len({w[0].tobytes() for w in want}) == B
    assert m.obb_ms() > 0
    m.close()
