"""Second-stage labels on the device (include/mars_hip.h, "Second-stage labels"): mars_yolo_classify_maps, the classifier head of a loaded
model in every layout a tensor can have on the device, the chain detector -> crops -> classifier -> labels per detection, and its ordering.
The expected values come from the numpy restatement of tests/test_classify_cpu.py (checked there by hand); every comparison is bit-exact."""
import numpy as np
import pytest

import cases
import marsfile
from conftest import lcg_frame
from test_classify_cpu import classify_np, label_np
from test_gpu_roi import FRAME_SEED, Chain, second_stage

pytestmark = pytest.mark.gpu

KS = (1, 3, 8)
# C x H x W, maps per call.  One pixel; odd everything; 16-byte rows; rows no multiple of 4; one pixel of many channels (column tiles);
# the channel limit; the shipped shape, the only one whose frames are split over several workgroups
SHAPES = [(1, 1, 1, 3), (5, 3, 5, 3), (64, 20, 20, 3), (81, 7, 9, 3), (300, 1, 1, 3), (4096, 2, 2, 2), (64, 160, 160, 2)]


def same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert got.tobytes() == want.tobytes(), (what, got.reshape(-1)[:8], want.reshape(-1)[:8])


def check_maps(gpu, maps, c, h, w, scale, what):
    """both layouts, every K, plain and softmax scores, against one restatement per (layout, score kind)"""
    n = maps.size // (c * h * w)
    planar = maps.reshape(n, c, h * w)
    for nhwc in (False, True):
        m = np.ascontiguousarray(planar.transpose(0, 2, 1)) if nhwc else planar
        for softmax in (False, True):
            want, want_sums = classify_np(m, c, h, w, nhwc, scale, 8, softmax)
            for k in KS:
                top, sums = gpu.classify_maps(m, c, h, w, nhwc, scale, gpu.cls_opts(top_k=k, softmax=softmax))
                same(sums, want_sums, (what, nhwc, softmax, k, "sums"))
                same(top, np.ascontiguousarray(want[:, :k]), (what, nhwc, softmax, k))
    return want


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%dx%d" % s[:3] for s in SHAPES])
def test_classify_maps(gpu, shape):
    c, h, w, n = shape
    maps = cases.i8(0xC1A55000 + c * 7 + h, n * c * h * w)
    want = check_maps(gpu, maps, c, h, w, 0.043, shape)
    if c == 5:  # more entries than channels: the three behind the last channel are {-1, 0}
        assert (want["cls"][:, 5:] == -1).all() and (want["score"][:, 5:] == 0).all() and (want["cls"][:, :5] >= 0).all()
    top, _ = gpu.classify_maps(np.ascontiguousarray(maps.reshape(n, c, h * w).transpose(0, 2, 1)), c, h, w, True, 0.043)  # no options: top_k = 1
    same(top["cls"], np.ascontiguousarray(want["cls"][:, :1]), (shape, "default options"))


@pytest.mark.parametrize("value", [-128, 127])
def test_classify_maps_extreme_bytes(gpu, value):
    """every byte at one end of the range: small maps in both layouts, and the largest grid (2^24 pixels), where the sum of -128s is
    exactly -2^31, the last int32"""
    check_maps(gpu, np.full(2 * 5 * 3 * 5, value, dtype=np.int8), 5, 3, 5, 0.5, value)
    check_maps(gpu, np.full(64 * 160 * 160, value, dtype=np.int8), 64, 160, 160, 0.01, value)
    big = np.full(4096 * 4096, value, dtype=np.int8)
    top, sums = gpu.classify_maps(big, 1, 4096, 4096, False, 0.25, gpu.cls_opts(top_k=3))
    assert sums.tolist() == [[value * 4096 * 4096]] and top["cls"].tolist() == [[0, -1, -1]]
    assert top["score"][0, 0] == np.float32(value) * np.float32(0.25)


def test_classify_maps_ties_keep_channel_order(gpu):
    """constant channels, the largest sum shared by channels 2, 7 and 40: the order is 2, 7, 40"""
    v = (np.arange(64) % 23 - 5).astype(np.int8)
    v[[2, 7, 40]] = 50
    maps = np.repeat(v[:, None], 20 * 20, axis=1)  # [c][h * w]
    want = check_maps(gpu, maps, 64, 20, 20, 0.1, "ties")
    assert want["cls"][0, :3].tolist() == [2, 7, 40]
    assert want["score"][0, 0] == want["score"][0, 1] == want["score"][0, 2]


# ---- through a model ---------------------------------------------------------------------------------------------------------------------
def head_graph(C, nchw):
    """16 x 16 x 16 input -> 3 x 3 stride-2 convolution (16 channels at 8 x 8) -> 1 x 1 convolution to C channels, the graph output.
    -> (file, internal tensor, output tensor)"""
    rng = np.random.default_rng(C * 2 + nchw)
    G = marsfile.Graph()
    fmt = marsfile.NCHW if nchw else marsfile.NHWC
    shp = (lambda c, h, w: [1, c, h, w]) if nchw else (lambda c, h, w: [1, h, w, c])

    def conv(x, out, oc, ic, k, s):
        if nchw:
            wt = G.tensor([oc, ic, k, k], fmt=marsfile.OIHW, scale=0.01, data=rng.integers(-127, 128, (oc, ic, k, k), dtype=np.int8))
        else:
            wt = G.tensor([oc, k, k, ic], scale=0.01, data=rng.integers(-127, 128, (oc, k, k, ic), dtype=np.int8))
        G.conv(x, out, wt, k=(k, k), s=(s, s))

    x = G.tensor(shp(16, 16, 16), fmt=fmt, scale=0.05)
    mid = G.tensor(shp(16, 8, 8), fmt=fmt, scale=0.5)
    out = G.tensor(shp(C, 8, 8), fmt=fmt, scale=0.37)
    conv(x, mid, 16, 16, 3, 2)
    conv(mid, out, C, 16, 1, 1)
    return G.serialise([x], [out]), mid, out


def frames_of(m, t, batch):
    return np.stack([m.read_tensor(t, frame=f) for f in range(batch)])


@pytest.mark.parametrize("fusion", [0, 1])
@pytest.mark.parametrize("nchw", [False, True], ids=["nhwc", "nchw"])
@pytest.mark.parametrize("C", [10, 64, 81])
def test_classify_through_a_model(gpu, C, nchw, fusion):
    """the head of a loaded model at batch 3: row-pitch outputs (10, 81 channels under the NHWC tag), dense rows, planes, and -- tensor= --
    the internal tensor (pixels x channels under the NCHW tag at fusion 1)"""
    d, mid, out = head_graph(C, nchw)
    m = gpu.Model(d, batch=3, fusion=fusion)
    nb = m.input_view(0).shape[1]
    for f in range(3):
        m.input_view(0)[f] = lcg_frame(0xC1A60000 + 16 * C + f, nb)
    m.run()
    for t, c, scale in ((out, C, 0.37), (mid, 16, 0.5)):
        bytes_ = frames_of(m, t, 3)
        assert len({b.tobytes() for b in bytes_}) == 3
        for softmax in (False, True):
            want, want_sums = classify_np(bytes_, c, 8, 8, not nchw, scale, 3, softmax)
            kw = dict(tensor=t) if t == mid else dict(output_index=0)
            top, sums = m.classify(top_k=3, softmax=softmax, **kw)
            same(sums, want_sums, (C, nchw, fusion, t, "sums"))
            same(top, want, (C, nchw, fusion, t, softmax))
        want, _ = classify_np(bytes_, c, 8, 8, not nchw, 0.02, 8, True)  # a scale of the caller's
        top, _ = m.classify(top_k=8, softmax=True, scale=0.02, want_sums=False, **kw)
        same(top, want, (C, nchw, fusion, t, "scale"))
    m.run_device()  # the run after a tail: its layers that write the pooled tensors wait for it, the results do not change
    same(m.classify(top_k=8, softmax=True, scale=0.02, tensor=mid)[0], want, "after another run")
    m.close()


def test_result_block_grows_and_is_reused(gpu):
    """one model, top_k 1 -> 8 (the cap: the result block has to grow) -> 1 (the larger block is kept and holds the smaller layout): every
    call's entries and sums are the restatement's, and nothing can be fetched before the first.  (The classify stage records no events of
    its own: there is no device time to ask for)"""
    C_, nchw = 10, False
    d, mid, out = head_graph(C_, nchw)
    m = gpu.Model(d, batch=3)
    with pytest.raises(gpu.MarsError) as e:
        m.classify_results(1)
    assert e.value.code == gpu.MARS_ERR_INVALID_TENSOR
    nb = m.input_view(0).shape[1]
    for f in range(3):
        m.input_view(0)[f] = lcg_frame(0xC1A60000 + 16 * C_ + f, nb)
    m.run()
    bytes_ = frames_of(m, out, 3)
    want, want_sums = classify_np(bytes_, C_, 8, 8, not nchw, 0.37, 8, False)
    for k in (1, 8, 1):
        top, sums = m.classify(top_k=k, output_index=0)
        same(sums, want_sums, ("growth", k, "sums"))
        same(top, np.ascontiguousarray(want[:, :k]), ("growth", k))
    m.close()


# ---- the chain ---------------------------------------------------------------------------------------------------------------------------
def out_geometry(d2, tout):
    """-> (C, H, W, nhwc, scale) of the second stage's output tensor"""
    _, tensors, _ = marsfile.parse(d2)
    t = tensors[tout]
    nhwc = t["fmt"] == marsfile.NHWC
    _, a, b, c = t["shape"]
    return ((c, a, b) if nhwc else (a, b, c)) + (nhwc, t["scale"])


def one_pass(c, dst, buf, wait):
    """detector -> crops -> classifier -> labels of one batch of frames; wait: a host wait after every step"""
    c.detect(buf)
    if wait:
        c.det.detect_results()
    dst.crop_detections(c.det, buf.ptr, c.opts(), device=True)
    if wait:
        dst.roi_results()
    dst.run_device(sync=wait)
    dst.classify_device(top_k=3)
    if wait:
        dst.classify_results(3)
    c.det.label_detections(dst)


def fetch(c, dst):
    dets = c.det.detect_results()
    rois, dropped = dst.roi_results()
    top, sums = dst.classify_results(3)
    return dets, rois, dropped, top, sums, c.det.label_results()


def check_pass(dst, tout, geo, dets, rois, top, sums, labels):
    C, H, W, nhwc, scale = geo
    out = frames_of(dst, tout, dst.batch)
    want, want_sums = classify_np(out, C, H, W, nhwc, scale, 3, False)
    same(sums, want_sums, "chain sums")
    same(top, want, "chain top")
    same(labels, label_np(rois, top[:, 0], [len(x) for x in dets]), "labels")


def test_chain_end_to_end(gpu):
    """preprocess_nv12_device -> run_device -> detect_heads_device -> crop_detections(device) -> run_device -> classify_device ->
    label_detections, nothing waiting in between; then the detections, the ROI table, the entries and the labels are fetched"""
    d2, tin, tout, nhwc = second_stage(gpu, "shipped")
    geo = out_geometry(d2, tout)
    c = Chain(gpu)
    dst = gpu.Model(d2, batch=8)
    nv, buf = c.frames(FRAME_SEED)
    one_pass(c, dst, buf, wait=False)
    dets, rois, dropped, top, sums, labels = fetch(c, dst)
    assert len(rois) == 8 and dropped > 0 and sum(len(x) for x in dets) > 8
    check_pass(dst, tout, geo, dets, rois, top, sums, labels)
    labelled = int((labels["cls"] >= 0).sum())
    assert labelled == 8
    # detections without a crop carry {-1, 0}: the boxes dropped for want of a frame, every list's unused tail
    without = [(f, i) for f, x in enumerate(dets) for i in range(len(x)) if labels[f, i]["cls"] < 0]
    assert len(without) >= 1 and all(labels[f, i]["score"] == 0 for f, i in without)
    for k, r in enumerate(rois):
        assert labels[r["frame"], r["det"]].tobytes() == top[k, 0].tobytes()
    assert len({s.tobytes() for s in sums}) > 1
    dst.close()
    c.close()


def test_chain_repeats_without_a_host_wait(gpu):
    """two passes on different frames, no host wait between the first label_detections and the second pass's front-end: the second pass's
    results equal a pass on those frames that waits after every step"""
    d2, tin, tout, nhwc = second_stage(gpu, "shipped")
    geo = out_geometry(d2, tout)
    c = Chain(gpu)
    dst = gpu.Model(d2, batch=8)
    (nv_a, buf_a), (nv_b, buf_b) = c.frames(FRAME_SEED), c.frames(FRAME_SEED + 32)
    one_pass(c, dst, buf_b, wait=True)
    ref = fetch(c, dst)
    check_pass(dst, tout, geo, ref[0], ref[1], ref[3], ref[4], ref[5])
    for _ in range(2):  # (the second stage's plan runs launch by launch, is captured, is replayed)
        one_pass(c, dst, buf_a, wait=False)
        one_pass(c, dst, buf_b, wait=False)
        got = fetch(c, dst)
        for g, w in zip(got[0], ref[0]):
            assert g.tobytes() == w.tobytes()
        assert got[1].tobytes() == ref[1].tobytes() and got[2] == ref[2]
        same(got[3], ref[3], "top")
        same(got[4], ref[4], "sums")
        same(got[5], ref[5], "labels")
    one_pass(c, dst, buf_a, wait=True)
    assert fetch(c, dst)[4].tobytes() != ref[4].tobytes()  # other frames, other sums
    dst.close()
    c.close()


def test_classify_is_deterministic(gpu):
    """the shipped second stage's output map (64 channels; its three unpadded 3 x 3 convolutions leave 154 x 154 of the 160 x 160 input),
    frames split over several workgroups: the same bytes twice, and the restatement's"""
    d2, tin, tout, nhwc = second_stage(gpu, "shipped")
    geo = out_geometry(d2, tout)
    assert geo[0] == 64 and geo[1] * geo[2] > 16384
    dst = gpu.Model(d2, batch=2)
    for f in range(2):
        dst.write_tensor(tin, lcg_frame(0xC1A70000 + f, 160 * 160 * 3), frame=f)
    dst.run_device()
    a = dst.classify(top_k=8, softmax=True)
    b = dst.classify(top_k=8, softmax=True)
    assert a[1].tobytes() == b[1].tobytes() and a[0].tobytes() == b[0].tobytes()
    want, want_sums = classify_np(frames_of(dst, tout, 2), *geo[:3], geo[3], geo[4], 8, True)
    same(a[1], want_sums, "sums")
    same(a[0], want, "top")
    dst.close()


def test_classify_refusals_that_need_a_device(gpu):
    BAD_TENSOR = gpu.MARS_ERR_INVALID_TENSOR

    def refused(fn, *a, **kw):
        with pytest.raises(gpu.MarsError) as ei:
            fn(*a, **kw)
        assert ei.value.code == BAD_TENSOR

    f32 = gpu.Model(gpu.synth_model(tiny=True, input_hw=32, float32=True, seed=5))
    refused(f32.classify_device)  # a float32 tensor
    f32.close()
    d2, tin, tout, nhwc = second_stage(gpu, "shipped")
    dst = gpu.Model(d2, batch=8)
    refused(dst.classify_results, 1)  # nothing pending
    refused(dst.classify_device, output_index=1)
    refused(dst.classify_device, tensor=10 ** 6)
    refused(dst.classify_device, tensor=tin if tin > 0 else 10 ** 6)  # a graph input
    hdr, tensors, _ = marsfile.parse(d2)
    weights = [i for i, t in enumerate(tensors) if t["size"] and t["dtype"] == marsfile.I8]
    refused(dst.classify_device, tensor=weights[0])  # a weight
    dst.pipe_open()
    refused(dst.classify_device)  # an open pipe
    dst.pipe_close()
    c, other = Chain(gpu), Chain(gpu)
    nv, buf = c.frames(FRAME_SEED)
    refused(c.det.label_results)  # nothing pending
    c.detect(buf)
    other.detect(buf)
    dst.run_device()
    dst.classify_device(top_k=3)
    refused(c.det.label_detections, dst)  # no crop call into dst yet
    refused(dst.label_detections, dst)
    dst.crop_detections(c.det, buf.ptr, c.opts(), device=True)
    dst.run_device(sync=False)
    dst.classify_device(top_k=3)
    refused(other.det.label_detections, dst)  # the crops came out of another detector
    c.det.label_detections(dst)
    assert (c.det.label_results()["cls"] >= 0).sum() == 8
    fresh = gpu.Model(d2, batch=8)
    fresh.crop_detections(c.det, buf.ptr, c.opts(), device=True)
    refused(c.det.label_detections, fresh)  # crops, but no classify results
    fresh.close()
    dst.close()
    c.close()
    other.close()
