"""Pose keypoints on the device (mars_hip_detect_pose, mars_yolo_keypoints), byte for byte against the numpy restatement of include/mars_hip.h
"Pose keypoints" (tests/poseref.py).  The expected detections and their origins come from the DFL restatement of tests/test_gpu_yolo_dfl.py
and the index-carrying sort + NMS of tests/test_gpu_yolo_seg.py.  Every comparison is byte equality."""
import ctypes as C

import numpy as np
import pytest

import marsfile
import poseref
from conftest import lcg_frame
from test_gpu_yolo_dfl import _conv, _write_heads, decode_dfl, head_bytes
from test_gpu_yolo_heads import letterbox_map, nms, sig_table
from test_gpu_yolo_seg import origins_dfl, sort_nms_idx

pytestmark = pytest.mark.gpu

F32 = np.float32
R, NC = 4, 3  # reg_max and classes of the hand-built graphs
DFL_KW = dict(conf=0.6, box_scales=0.05, cls_scales=0.02)  # an all-zero input gives class bytes of 0: confidence 0.5, no candidate
SHAPES = [(17, 3), (1, 2), (5, 3), (32, 3)]  # the stock export; two channels; 15 channels (no multiple of 4 or 16); the cap


def pose_graph(K, D, nchw, S, nm=0, in_c=16, f32_extra=False):
    """S x S x in_c input -> a chain of 1x1 stride-2 convolutions down to S / 32; DFL heads (box 4 R, class NC, concat) and a keypoint
    convolution of K * D channels at S / 8, S / 16 and S / 32, each keypoint tensor read by a RESHAPE alone; the concats are the outputs.
    nm > 0: a seg head too (a coefficient convolution of nm channels per scale, prototypes at S / 4 as the fourth output).
    f32_extra: one more tensor, float32, K * D channels on head 0's grid, that no layer touches (its index: the last tensor's).
    -> file, [(box, class, concat, grid, stride)], [keypoint tensor], [coefficient tensor], prototype tensor"""
    rng = np.random.default_rng(K * 16 + D * 4 + nchw * 2 + (S > 64) + 1000 * nm)
    G = marsfile.Graph()
    fmt = marsfile.NCHW if nchw else marsfile.NHWC
    shp = (lambda c, h, w: [1, c, h, w]) if nchw else (lambda c, h, w: [1, h, w, c])
    x = G.tensor(shp(in_c, S, S), fmt=fmt, scale=0.05)
    feat, t, sc = {}, x, 0.25  # every convolution's output scale is 3 x its input's: the int8 spread stays near 40 steps
    for s in (2, 4, 8, 16, 32):
        n = G.tensor(shp(in_c, S // s, S // s), fmt=fmt, scale=sc)
        _conv(G, rng, t, n, in_c, in_c, 1, 2, nchw)
        feat[s], t, sc = (n, sc), n, sc * 3
    heads, kpts, coefs = [], [], []
    for s in (8, 16, 32):
        g, (p, ps) = S // s, feat[s]
        b = G.tensor(shp(4 * R, g, g), fmt=fmt, scale=ps * 3)
        c = G.tensor(shp(NC, g, g), fmt=fmt, scale=ps * 3)
        _conv(G, rng, p, b, 4 * R, in_c, 1, 1, nchw)
        _conv(G, rng, p, c, NC, in_c, 1, 1, nchw)
        cat = G.tensor(shp(4 * R + NC, g, g), fmt=fmt, scale=ps * 3)
        G.concat([b, c], cat, axis=1 if nchw else 3)
        kp = G.tensor(shp(K * D, g, g), fmt=fmt, scale=ps * 3 / 64)
        _conv(G, rng, p, kp, K * D, in_c, 1, 1, nchw)
        G.layer(marsfile.RESHAPE, [kp], [G.tensor([0, 0, 0, 0])])
        heads.append((b, c, cat, g, s))
        kpts.append(kp)
        if nm:
            cf = G.tensor(shp(nm, g, g), fmt=fmt, scale=ps * 3)
            _conv(G, rng, p, cf, nm, in_c, 1, 1, nchw)
            G.layer(marsfile.RESHAPE, [cf], [G.tensor([0, 0, 0, 0])])
            coefs.append(cf)
    outs, pr = [h[2] for h in heads], None
    if f32_extra:
        G.tensor(shp(K * D, S // 8, S // 8), dtype=marsfile.F32, fmt=fmt)
    if nm:
        pr = G.tensor(shp(nm, S // 4, S // 4), fmt=fmt, scale=feat[4][1] * 3)
        _conv(G, rng, feat[4][0], pr, nm, in_c, 1, 1, nchw)
        outs.append(pr)
    return G.serialise([x], outs), heads, kpts, coefs, pr


def chw_bytes(m, t, f, nchw):
    """tensor t of frame f as int8 [C][H][W] (mars_hip_read_tensor: the reference's bytes in the tag's order)"""
    s = m.tensor_desc(t).shape
    a = m.read_tensor(t, f).view(np.int8)
    return a.reshape(s[1], s[2], s[3]) if nchw else a.reshape(s[1], s[2], s[3]).transpose(2, 0, 1)


def expected_frame(gpu, hs, kpt_arrs, kpt_scales, K, D, S, conf, thresh=0.45, src=None, **pose):
    """hs as decode_dfl takes them -> (the detections mars_hip_detect_results gives, pose records, keypoints, the kept list's heads)"""
    cand, _ = decode_dfl(hs, gpu.DET_DTYPE, conf)
    org = origins_dfl(hs, conf)
    assert len(org) == len(cand)
    keep = sort_nms_idx(cand, thresh)
    kept = cand[keep]
    assert kept.tobytes() == nms(cand.copy(), thresh).tobytes(), "the test's own sort + NMS differs from the reference's"
    recs, kp = poseref.pose_frame(kept["conf"], org[keep], kpt_arrs, kpt_scales, [h[4] for h in hs], K, D, src=src, in_hw=(S, S), **pose)
    cells = np.cumsum([0] + [a.shape[1] * a.shape[2] for a in kpt_arrs])
    return (letterbox_map(kept, src[0], src[1], S, S) if src else kept), recs, kp, np.searchsorted(cells, org[keep], side="right") - 1


def model_expected(gpu, m, heads, kpts, nchw, S, K, D, pose_kw, dfl_kw=DFL_KW, kpt_scales=None, src=None):
    """the expectation of every frame from the bytes the model holds"""
    want = []
    for f in range(m.batch):
        hs = []
        for b, c, cat, _, s in heads:
            bb, cb = head_bytes(gpu, m, f, b, c, cat, nchw)
            hs.append((np.ascontiguousarray(bb), np.ascontiguousarray(cb), dfl_kw["box_scales"], dfl_kw["cls_scales"], s))
        ka = [np.ascontiguousarray(chw_bytes(m, t, f, nchw)) for t in kpts]
        ks = kpt_scales if kpt_scales is not None else [m.tensor_desc(t).scale for t in kpts]
        want.append(expected_frame(gpu, hs, ka, ks, K, D, S, dfl_kw["conf"], src=src, **pose_kw))
    return want


def check(got, want, what):
    dets, recs, kp = got
    assert recs.shape[0] == kp.shape[0] == len(want) and recs.shape[1] == kp.shape[1]
    for f, (kept, wr, wk, _) in enumerate(want):
        assert dets[f].tobytes() == kept.tobytes(), (what, f, "detections")
        assert recs[f].tobytes() == wr.tobytes(), (what, f, recs[f], wr)
        assert kp[f].tobytes() == wk.tobytes(), (what, f, "keypoints")


def fill(m, seed, zero_frame=None):
    nb = m.input_view(0).shape[1]
    for f in range(m.batch):
        m.input_view(0)[f] = 0 if f == zero_frame else lcg_frame(seed + f, nb)


GRAPH_SEED = 0x905E0000
HAND_BUILT = [{}, dict(max_per_frame=1), dict(max_per_frame=256, min_conf=0.62)]  # the default of 32; the smallest; the cap and a cut-off


def hand_built_preconditions(want_by_kw):
    """what the 64 x 64 graphs must reach (a failure here is a failure of the test's inputs): a frame that keeps detections of two heads, a
    frame that keeps more than max_per_frame, a cut-off above some kept confidences and below others, an empty frame"""
    w32, w1, wcut = want_by_kw
    assert any(len(set(w[3].tolist())) >= 2 for w in w32), "no frame keeps detections of two heads"
    assert any(len(w[0]) > 1 for w in w1), "no frame keeps more than max_per_frame = 1"
    assert any(0 < int((w[1]["det"] >= 0).sum()) < len(w[0]) for w in wcut), "min_conf cuts nothing or everything"
    assert len(w32[1][0]) == 0 and (w32[1][1]["det"] == -1).all() and not w32[1][2].view(np.uint8).any()


@pytest.mark.parametrize("nchw", [False, True])
@pytest.mark.parametrize("K, D", SHAPES)
def test_hand_built_graphs(gpu, K, D, nchw):
    """graph -> heads -> boxes -> keypoints at batch 3 (frame 1 has no candidate) on a 64 x 64 input, grids 8 / 4 / 2"""
    S = 64
    d, heads, kpts, _, _ = pose_graph(K, D, nchw, S)
    m = gpu.Model(d, batch=3)
    fill(m, GRAPH_SEED + K, zero_frame=1)
    m.run()
    plain = m.detect_dfl(**DFL_KW)
    wants = []
    for kw in HAND_BUILT:
        got = m.detect_pose(gpu.pose_opts(kpts, num_kpt=K, kpt_dim=D, **kw), **DFL_KW)
        want = model_expected(gpu, m, heads, kpts, nchw, S, K, D, kw)
        check(got, want, (K, D, nchw, kw))
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got[0], plain)), "detect_results after a pose call differs from detect_dfl"
        assert got[1].shape == (3, kw.get("max_per_frame", 32)) and got[2].shape == (3, kw.get("max_per_frame", 32), K)
        wants.append(want)
    hand_built_preconditions(wants)
    # kpt_dim = 0 means 3
    if D == 3:
        got = m.detect_pose(gpu.pose_opts(kpts, num_kpt=K), **DFL_KW)
        check(got, wants[0], "kpt_dim 0")
    m.close()


def test_result_block_grows_and_is_reused(gpu):
    """one model, max_per_frame 1 -> 256 (the cap: the result block has to grow, and the visibility tables inside it go up again) -> 1 (the
    larger block is kept and holds the smaller layout): every call's boxes and keypoints are the restatement's, the stage's device time is
    there after each, and nothing can be fetched before the first"""
    S, K, D, nchw = 64, 17, 3, False
    d, heads, kpts, _, _ = pose_graph(K, D, nchw, S)
    m = gpu.Model(d, batch=3)
    with pytest.raises(gpu.MarsError) as e:
        m.pose_results()
    assert e.value.code == gpu.MARS_ERR_INVALID_TENSOR and m.pose_ms() < 0
    fill(m, GRAPH_SEED + K, zero_frame=1)
    m.run()
    for n in (1, 256, 1):
        kw = dict(max_per_frame=n)
        got = m.detect_pose(gpu.pose_opts(kpts, num_kpt=K, kpt_dim=D, **kw), **DFL_KW)
        want = model_expected(gpu, m, heads, kpts, nchw, S, K, D, kw)
        check(got, want, ("growth", n))
        assert got[1].shape == (3, n) and got[2].shape == (3, n, K) and any(len(w[0]) > 1 for w in want)
        assert m.pose_ms() >= 0
    m.close()


def many_kept_frames(rng, heads, K, D):
    """bytes for three frames of a 128 x 128 graph (336 cells): frame 0 -- every cell a candidate at one of two class-byte levels (the tail's
    tie-queue replay decides the order), every box distribution one sharp bin near the cell (small boxes: few are suppressed); frame 1 --
    nothing passes; frame 2 -- random bytes"""
    frames = []
    for f in range(3):
        arrs, ka = [], []
        for _, _, _, g, _ in heads:
            ab = rng.integers(-128, 128, (4 * R, g, g), dtype=np.int8)
            ac = rng.integers(-128, 128, (NC, g, g), dtype=np.int8)
            if f == 0:
                ab[:] = -128
                pos = rng.integers(0, 2, (4, g, g))
                for s in range(4):
                    np.put_along_axis(ab[s * R:(s + 1) * R], pos[s][None], 127, axis=0)
                ac[:] = -128
                np.put_along_axis(ac, rng.integers(0, NC, (1, g, g)), np.where(rng.integers(0, 2, (1, g, g)) == 1, 40, 20).astype(np.int8), axis=0)
            elif f == 1:
                ac[:] = -128
            arrs.append((ab, ac))
            ka.append(rng.integers(-128, 128, (K * D, g, g), dtype=np.int8))
        frames.append((arrs, ka))
    return frames


MANY_KW = dict(conf=0.6, box_scales=0.3, cls_scales=0.05)
MANY_SCALES = [0.5, 0.25, 0.125]  # per-head overrides


def many_kept_cases():
    mid = float(sig_table(0.05)[30 + 128])  # between the confidences of bytes 20 and 40
    return [(dict(max_per_frame=256), None, None), (dict(max_per_frame=1), None, None), (dict(), MANY_SCALES, None),
            (dict(max_per_frame=256, min_conf=mid), MANY_SCALES, None), (dict(max_per_frame=100), MANY_SCALES, (1280, 720))]


def many_kept_expected(gpu, frames, heads, kpts_desc_scales, K, D, S, pose_kw, scales, src):
    want = []
    for arrs, ka in frames:
        hs = [(ab, ac, MANY_KW["box_scales"], MANY_KW["cls_scales"], s) for (ab, ac), (_, _, _, _, s) in zip(arrs, heads)]
        want.append(expected_frame(gpu, hs, ka, scales if scales is not None else kpts_desc_scales, K, D, S, MANY_KW["conf"], src=src, **pose_kw))
    return want


def many_kept_preconditions(wants):
    """the ballot prefix crosses a 64-record boundary with records on both sides, the cut at max_per_frame falls inside a later round, and the
    cut-off leaves more than 64 and fewer than all"""
    w256, w1, w32, wcut, w100 = wants
    n0 = len(w256[0][0])
    assert n0 > 256 and int((w256[0][1]["det"] >= 0).sum()) == 256, n0  # more kept than the largest max_per_frame: four full rounds of 64
    assert len(set(w256[0][0]["conf"])) == 2 and len(set(w256[0][3].tolist())) == 3
    assert int((w32[0][1]["det"] >= 0).sum()) == 32 and int((w100[0][1]["det"] >= 0).sum()) == 100 and w1[0][1]["det"].tolist() == [0]
    assert 64 < int((wcut[0][1]["det"] >= 0).sum()) < n0
    assert len(w256[1][0]) == 0 and len(w256[2][0]) > 0


@pytest.mark.parametrize("nchw", [False, True])
def test_many_kept(gpu, nchw):
    """bytes written into the heads and the keypoint tensors of a 128 x 128 graph: more than 64 kept records in one frame, max_per_frame of 1,
    32 (the default), 100 and 256, a min_conf between the two confidence levels, per-head kpt_scales against the tensors' own, and
    src = 1280 x 720 (boxes and keypoints both mapped)"""
    K, D, S = 17, 3, 128
    d, heads, kpts, _, _ = pose_graph(K, D, nchw, S)
    m = gpu.Model(d, batch=3)
    fill(m, 7)
    m.run()
    frames = many_kept_frames(np.random.default_rng(29 + nchw), heads, K, D)
    for f, (arrs, ka) in enumerate(frames):
        _write_heads(gpu, m, f, heads, nchw, arrs)
        for t, a in zip(kpts, ka):
            m.write_tensor(t, a if nchw else a.transpose(1, 2, 0), f)
    own = [m.tensor_desc(t).scale for t in kpts]
    plain, mapped = m.detect_dfl(**MANY_KW), m.detect_dfl(src=(1280, 720), **MANY_KW)
    wants = []
    for pose_kw, scales, src in many_kept_cases():
        want = many_kept_expected(gpu, frames, heads, own, K, D, S, pose_kw, scales, src)
        kw = dict(MANY_KW, src=src) if src else MANY_KW
        got = m.detect_pose(gpu.pose_opts(kpts, num_kpt=K, kpt_dim=D, kpt_scales=scales, **pose_kw), **kw)
        check(got, want, (nchw, pose_kw, scales, src))
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got[0], mapped if src else plain))
        wants.append(want)
    many_kept_preconditions(wants)
    # the mapping moves x and y and leaves v, and the overrides change the numbers
    unmapped = many_kept_expected(gpu, frames, heads, own, K, D, S, dict(max_per_frame=100), MANY_SCALES, None)
    assert np.array_equal(unmapped[0][2]["v"], wants[4][0][2]["v"]) and not np.array_equal(unmapped[0][2]["x"], wants[4][0][2]["x"])
    assert wants[0][0][2][:32].tobytes() != wants[2][0][2].tobytes()
    m.close()


def test_second_run_and_async_hand_off(gpu):
    """a second mars_run + pose call gives the second batch's keypoints; and run_device_async(A) -> detect_pose_device -> mars_run(B) with no
    host wait in between: the tail of A reads head and keypoint tensors that B's graph overwrites; the layers of B that write them wait, so
    every batch's boxes and keypoints equal run / sync / detect_pose"""
    S, B, K, D = 64, 8, 17, 3
    d, heads, kpts, _, _ = pose_graph(K, D, True, S)
    m = gpu.Model(d, batch=B)
    nb = m.input_view(0).shape[1]
    xs = [[lcg_frame(0xA5B00000 + 0x100000 * k + f, nb) for f in range(B)] for k in range(3)]
    opts = gpu.pose_opts(kpts, num_kpt=K, max_per_frame=8)
    want = []
    for k in range(3):
        for f in range(B):
            m.input_view(0)[f] = xs[k][f]
        m.run()
        want.append(m.detect_pose(opts, **DFL_KW))
        check(want[k], model_expected(gpu, m, heads, kpts, True, S, K, D, dict(max_per_frame=8)), ("sync", k))
    assert sum(want[0][2][f].tobytes() != want[1][2][f].tobytes() for f in range(B)) > B // 2
    for f in range(B):
        m.input_view(0)[f] = xs[0][f]
    m.upload()
    for k in range(3):
        m.run_device(sync=False)
        m.detect_pose_device(opts, **DFL_KW)
        nxt = xs[(k + 1) % 3]
        for f in range(B):
            m.input_view(0)[f] = nxt[f]
        m.run()  # upload + graph of the next batch on the main stream, no host wait in between
        dets = m.detect_results()
        recs, kp = m.pose_results()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(dets, want[k][0])), k
        assert recs.tobytes() == want[k][1].tobytes() and kp.tobytes() == want[k][2].tobytes(), k
        m.upload()
    assert m.pose_ms() > 0
    m.close()


@pytest.mark.parametrize("nchw", [False, True])
def test_seg_and_pose_on_one_model(gpu, nchw):
    """a graph with both heads: seg then pose, and pose then seg, each gives the bytes it gives alone (separate blocks, each call its own tail)"""
    S, K, D, nm = 64, 17, 3, 32
    d, heads, kpts, coefs, pr = pose_graph(K, D, nchw, S, nm=nm)
    m = gpu.Model(d, batch=3)
    fill(m, GRAPH_SEED + 99, zero_frame=1)
    m.run()
    so, po = gpu.seg_opts(coefs, pr, max_per_frame=8), gpu.pose_opts(kpts, num_kpt=K, max_per_frame=8)
    pose_kw = dict(DFL_KW, conf=0.55)  # the two calls run different tails: the detections are those of the last one
    seg_alone = m.detect_seg(so, **DFL_KW)
    pose_alone = m.detect_pose(po, **pose_kw)
    check(pose_alone, model_expected(gpu, m, heads, kpts, nchw, S, K, D, dict(max_per_frame=8), pose_kw), "alone")
    assert (seg_alone[1]["det"] >= 0).any() and (pose_alone[1]["det"] >= 0).any()
    assert any(a.tobytes() != b.tobytes() for a, b in zip(seg_alone[0], pose_alone[0]))
    for first in ("seg", "pose"):
        for who in ((first, "pose" if first == "seg" else "seg")):
            if who == "seg":
                m.detect_seg_device(so, **DFL_KW)
            else:
                m.detect_pose_device(po, **pose_kw)
        dets = m.detect_results()
        last = pose_alone if first == "seg" else seg_alone
        assert all(a.tobytes() == b.tobytes() for a, b in zip(dets, last[0])), first
        recs, words, _ = m.mask_results()
        assert recs.tobytes() == seg_alone[1].tobytes() and np.array_equal(words, seg_alone[2]), first
        precs, kp = m.pose_results()
        assert precs.tobytes() == pose_alone[1].tobytes() and kp.tobytes() == pose_alone[2].tobytes(), first
    m.close()


@pytest.mark.parametrize("K, D", [(17, 3), (1, 2), (32, 3)])
def test_host_pointer_form(gpu, K, D):
    rng = np.random.default_rng(K * 4 + D)
    for n in (0, 1, 64, 65, 256):
        rows = rng.integers(-128, 128, (n, K * D), dtype=np.int8)
        gx, gy = rng.integers(0, 80, n), rng.integers(0, 80, n)
        stride = rng.choice([8, 16, 32], n)
        got = gpu.keypoints(rows, K, D, gx, gy, stride, 0.07)
        assert got.shape == (n, K)
        for i in range(n):
            assert got[i].tobytes() == poseref.keypoints(rows[i], K, D, gx[i], gy[i], stride[i], 0.07).tobytes(), (K, D, n, i)
    one = (np.zeros((1, K * D), np.int8), K, D, [0], [0], [8])
    for s in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            gpu.keypoints(*one, s)
    z = np.zeros(257, np.int32)
    for bad in ((np.zeros((257, K * D), np.int8), K, D, z, z, z), (np.zeros((1, 33 * 3), np.int8), 33, 3, [0], [0], [8]),
                (np.zeros((1, 4), np.int8), 1, 4, [0], [0], [8]), (np.zeros((1, 1), np.int8), 1, 1, [0], [0], [8])):
        with pytest.raises(ValueError):
            gpu.keypoints(*bad, 0.07)


def test_refusals(gpu):
    INV = gpu.MARS_ERR_INVALID_TENSOR
    S, K, D = 64, 5, 3
    d, heads, kpts, _, _ = pose_graph(K, D, False, S, f32_extra=True)
    m = gpu.Model(d, batch=2)
    with pytest.raises(gpu.MarsError) as e:
        m.pose_results()  # before any pose call
    assert e.value.code == INV
    assert m.pose_ms() < 0
    fill(m, 3)
    m.run()
    hdr, tensors, _ = marsfile.parse(d)
    weight = next(i for i, t in enumerate(tensors) if t["size"])
    box0, cls0 = heads[0][0], heads[0][1]
    f32 = len(tensors) - 1
    assert tensors[f32]["dtype"] == marsfile.F32 and tensors[f32]["shape"] == tensors[kpts[0]]["shape"]
    bad = [
        dict(kpts=[f32, kpts[1], kpts[2]]),       # a float32 tensor of the right shape
        dict(max_per_frame=257), dict(max_per_frame=-1),
        dict(num_kpt=0), dict(num_kpt=33), dict(num_kpt=-5), dict(kpt_dim=1), dict(kpt_dim=4), dict(kpt_dim=-3),
        dict(num_kpt=4), dict(num_kpt=6), dict(kpt_dim=2), dict(num_kpt=15, kpt_dim=2),  # K * D is not the 15 channels
        dict(kpt_scales=-1.0), dict(kpt_scales=float("nan")), dict(kpt_scales=float("inf")), dict(kpt_scales=[0.5, -0.5, 0.5]),
        dict(min_conf=float("nan")), dict(min_conf=float("inf")),
        dict(kpts=[kpts[1], kpts[0], kpts[2]]),   # a keypoint grid that differs from its head's
        dict(kpts=[kpts[0], kpts[1], cls0]),      # 3 channels on head 0's grid
        dict(kpts=[weight, kpts[1], kpts[2]]),    # weights
        dict(kpts=[hdr["inputs"][0], kpts[1], kpts[2]]),  # a graph input: no convolution wrote it
        dict(kpts=[kpts[0], kpts[1], 9999]), dict(kpts=[-1, kpts[1], kpts[2]]),
    ]
    for kw in bad:
        what = dict(kw)
        o = gpu.pose_opts(kw.pop("kpts", kpts), **dict(dict(num_kpt=K, kpt_dim=D), **kw))
        with pytest.raises(gpu.MarsError) as e:
            m.detect_pose_device(o, **DFL_KW)
        assert e.value.code == INV, what
    with pytest.raises(gpu.MarsError) as e:
        m.detect_pose_device(None, **DFL_KW)  # NULL options
    assert e.value.code == INV
    with pytest.raises(gpu.MarsError) as e:  # what detect_dfl refuses
        m.detect_pose_device(gpu.pose_opts(kpts, num_kpt=K), heads=[(cls0, box0)])
    assert e.value.code == INV
    with pytest.raises(gpu.MarsError) as e:
        m.pose_results()  # still none
    assert e.value.code == INV
    m.pipe_open(download_outputs=False, detect=True, dfl_heads=gpu.yolo_dfl_heads(**DFL_KW))
    with pytest.raises(gpu.MarsError) as e:
        m.detect_pose_device(gpu.pose_opts(kpts, num_kpt=K), **DFL_KW)
    assert e.value.code == INV
    m.pipe_close()
    m.run()
    m.detect_pose(gpu.pose_opts(kpts, num_kpt=K), **DFL_KW)  # and the good configuration passes
    m.close()


def test_twin_160(gpu):
    """synth_model(head="pose") at 160 x 160, batch 2: graph -> found heads -> keypoints, through the C entry point that fetches everything"""
    S, B, K, D = 160, 2, 17, 3
    d = gpu.synth_model(width_x16=4, input_hw=S, seed=1, head="pose")
    hdr, _, _ = marsfile.parse(d)
    kpts = gpu.pose_twin_tensors(d)
    heads = [(b, c, o, None, s) for (b, c, s), o in zip(gpu.find_yolo_dfl_heads(d)[0], hdr["outputs"])]
    m = gpu.Model(d, batch=B)
    fill(m, 0x5EED0000)
    m.run()
    conf = 0.1
    dets = np.zeros((B, gpu.MAX_DET), dtype=gpu.DET_DTYPE)
    counts = np.zeros(B, dtype=np.int32)
    recs = np.zeros((B, 32), dtype=gpu.POSE_DTYPE)
    kp = np.zeros((B, 32, K), dtype=gpu.KPT_DTYPE)
    rc = gpu.lib().mars_hip_detect_pose(m.p, C.byref(gpu.yolo_dfl_heads(conf=conf)), C.byref(gpu.pose_opts(kpts)), dets.ctypes.data,
                                        counts.ctypes.data_as(C.POINTER(C.c_int)), recs.ctypes.data, kp.ctypes.data)
    assert rc == 0
    kw = dict(conf=conf, box_scales=m.tensor_desc(heads[0][0]).scale, cls_scales=m.tensor_desc(heads[0][1]).scale)
    assert all(m.tensor_desc(b).scale == kw["box_scales"] and m.tensor_desc(c).scale == kw["cls_scales"] for b, c, _, _, _ in heads)
    want = model_expected(gpu, m, heads, kpts, False, S, K, D, {}, kw)
    check(([dets[f, :counts[f]] for f in range(B)], recs, kp), want, "twin")
    assert sum(len(w[0]) for w in want) > 0 and len({bytes(w[2][0]) for w in want}) == B
    same = m.detect_dfl(conf=conf)
    assert all(a.tobytes() == b[0].tobytes() for a, b in zip(same, want))
    m.close()
