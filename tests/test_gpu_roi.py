"""ROI crops on the device (include/mars_hip.h, "ROI crops"): mars_yolo_crop_boxes, the device chain detector -> crops -> second model, the
selection rules and the ROI table.  The expected bytes come from the numpy restatement of tests/test_roi_cpu.py (checked there by hand);
every comparison is bit-exact."""
import os

import numpy as np
import pytest

import marsfile
from conftest import lcg_frame
from test_roi_cpu import box, nv12_to_rgb_np, roi_crop_np, roi_rect_np, roi_select_np

pytestmark = pytest.mark.gpu

MODELS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "models")
FULL, VU = 1, 2
SOURCES = [("rgb", 0), ("nv12", 0), ("nv12", FULL), ("nv12", VU), ("nv12", FULL | VU)]
SOURCE_IDS = ["rgb", "nv12_limited_uv", "nv12_full_uv", "nv12_limited_vu", "nv12_full_vu"]
SIZES = [(98, 62), (1280, 720)]  # w % 4 == 2; the camera size
# (tw, th, nhwc): one strip; the second stage's size in both layouts; rows of 99 bytes and a last strip of one row
TARGETS = [(16, 16, 1), (160, 160, 1), (160, 160, 0), (33, 17, 1), (33, 17, 0)]

_frames = {}


def source(kind, flags, w, h):
    """-> (the frame's bytes as the library takes them, the same frame as uint8 RGB [h][w][3]); made once per size and flag set"""
    key = (kind, flags, w, h)
    if key not in _frames:
        if kind == "rgb":
            raw = lcg_frame(0x201000 + w, w * h * 3)
            _frames[key] = (raw, raw.reshape(h, w, 3))
        else:
            raw = lcg_frame(0x202000 + w, w * h * 3 // 2)
            _frames[key] = (raw, nv12_to_rgb_np(raw, w, h, flags))
    return _frames[key]


def geometry_boxes(W, H, tw):
    """the boxes the crop kernel can go wrong on, for a W x H frame and a target tw wide"""
    cx, cy = W / 2, H / 2
    b = [box(10.5, 20, 1, 20),                    # a band one pixel wide: refused by the default min_size
         box(21, 31, 2, 2),                       # 2 x 2
         box(cx, cy, W, H),                       # the whole frame
         box(3, cy, 20, 30), box(W - 3, cy, 20, 30), box(cx, 2, 30, 20), box(cx, H - 2, 30, 20),  # over each edge
         box(W - 4, H - 5, 24, 26), box(2, 3, 24, 26),                                             # over two corners
         box(W + 50, cy, 20, 20), box(cx, -40, 20, 20), box(-1e30, cy, 20, 20), box(cx, 3e38, 3e38, 20),  # outside: skipped
         box(float("nan"), cy, 20, 20), box(cx, cy, 0, 20), box(cx, cy, 20, float("inf")),           # skipped
         box(30.0, 25.0, 11, 9), box(30.5, 25.5, 11, 9), box(30.999, 25.999, 11, 9),                  # fractional centres
         box(40, 21, 14, 11),                     # x0 = 33, y0 = 15: odd, the chroma pair is shared across the crop's edge
         box(cx, cy, max(tw // 7, 2), max(tw // 7, 2) + 1),   # up-scale x 7
         box(cx, cy, min(tw * 5, W), min(tw * 5, H))]          # down-scale x 5 (as far as the frame allows)
    return np.array(b)


def expected_crops(rgb, boxes, W, H, tw, th, nhwc, keep, expand=0.0, min_size=0):
    rects = [roi_rect_np(b, W, H, expand, min_size) for b in boxes]
    return rects, np.stack([roi_crop_np(rgb, r, tw, th, nhwc, keep) for r in rects])


def check_rois(rois, rects, frame=0):
    for i, r in enumerate(rects):
        assert rois[i]["frame"] == frame and rois[i]["det"] == -1
        if r is None:
            assert rois[i]["x1"] == rois[i]["x0"], i
        else:
            assert (rois[i]["x0"], rois[i]["y0"], rois[i]["x1"], rois[i]["y1"]) == r, i


@pytest.mark.parametrize("size", SIZES, ids=["98x62", "1280x720"])
@pytest.mark.parametrize("src", SOURCES, ids=SOURCE_IDS)
def test_crop_boxes_geometries(gpu, src, size):
    kind, flags = src
    W, H = size
    raw, rgb = source(kind, flags, W, H)
    fmt = gpu.CAMERA_NV12 if kind == "nv12" else gpu.CAMERA_RGB
    for tw, th, nhwc in TARGETS:
        boxes = geometry_boxes(W, H, tw)
        for keep in (False, True):
            for expand in (0.0, 1.25):  # 0 = the default, 1.0
                o = gpu.roi_opts(W, H, fmt=fmt, src_flags=flags, expand=expand, keep_aspect=keep)
                got, rois = gpu.crop_boxes(raw, boxes, np.zeros(len(boxes), dtype=np.int32), o, tw, th, nhwc)
                rects, want = expected_crops(rgb, boxes, W, H, tw, th, nhwc, keep, expand)
                assert (rects[0] is None) == (expand == 0.0) and sum(r is None for r in rects) == (8 if expand == 0.0 else 7)
                check_rois(rois, rects)
                bad = [i for i in range(len(boxes)) if not np.array_equal(got[i], want[i])]
                assert not bad, (tw, th, nhwc, keep, expand, bad, int((got != want).sum()))


@pytest.mark.parametrize("src", [SOURCES[0], SOURCES[4]], ids=[SOURCE_IDS[0], SOURCE_IDS[4]])
def test_crop_boxes_min_size_and_expand_one(gpu, src):
    """the one-pixel band is a crop once min_size = 1 allows it (every output column then blends one source column with itself); expand = 1.0
    given explicitly equals the default"""
    kind, flags = src
    W, H = 98, 62
    raw, rgb = source(kind, flags, W, H)
    fmt = gpu.CAMERA_NV12 if kind == "nv12" else gpu.CAMERA_RGB
    boxes = np.array([box(10.5, 20, 1, 20), box(20, 10.5, 20, 1), box(33.5, 33.5, 1, 1), box(21, 31, 2, 2)])
    fo = np.zeros(len(boxes), dtype=np.int32)
    for tw, th, nhwc in [(16, 16, 1), (33, 17, 0)]:
        for keep in (False, True):
            got, rois = gpu.crop_boxes(raw, boxes, fo, gpu.roi_opts(W, H, fmt=fmt, src_flags=flags, min_size=1, expand=1.0, keep_aspect=keep), tw, th, nhwc)
            rects, want = expected_crops(rgb, boxes, W, H, tw, th, nhwc, keep, 1.0, 1)
            assert rects == [(10, 10, 11, 30), (10, 10, 30, 11), (33, 33, 34, 34), (20, 30, 22, 32)]
            check_rois(rois, rects)
            assert np.array_equal(got, want), (tw, th, nhwc, keep)
            got2, rois2 = gpu.crop_boxes(raw, boxes, fo, gpu.roi_opts(W, H, fmt=fmt, src_flags=flags, keep_aspect=keep), tw, th, nhwc)
            assert (rois2["x1"] == rois2["x0"]).tolist() == [True, True, True, False] and np.array_equal(got2[3], want[3])
            assert (got2[:3] == -17).all()


@pytest.mark.parametrize("flags", [0, FULL, VU, FULL | VU], ids=SOURCE_IDS[1:])
def test_nv12_crop_equals_rgb_crop_of_the_converted_frame(gpu, flags):
    """two frames per call (the second starts at an odd multiple of 2 bytes), boxes in both: the NV12 crops are the RGB crops of the
    library's own nv12_to_rgb of those frames"""
    W, H = 98, 62
    nv = np.stack([lcg_frame(0x203000 + 7 * flags + f, W * H * 3 // 2) for f in range(2)])
    rgb = np.stack([gpu.nv12_to_rgb(nv[f], W, H, flags) for f in range(2)])
    boxes = np.concatenate([geometry_boxes(W, H, 160), geometry_boxes(W, H, 16)])
    fo = (np.arange(len(boxes)) % 2).astype(np.int32)
    for tw, th, nhwc, keep in [(160, 160, 0, False), (33, 17, 1, True)]:
        a, ra = gpu.crop_boxes(nv, boxes, fo, gpu.roi_opts(W, H, fmt=gpu.CAMERA_NV12, src_flags=flags, keep_aspect=keep), tw, th, nhwc)
        b, rb = gpu.crop_boxes(rgb, boxes, fo, gpu.roi_opts(W, H, keep_aspect=keep), tw, th, nhwc)
        assert ra.tobytes() == rb.tobytes() and (ra["frame"] == fo).all()
        assert np.array_equal(a, b), int((a != b).sum())
        want = np.stack([roi_crop_np(rgb[fo[i]], roi_rect_np(boxes[i], W, H), tw, th, nhwc, keep) for i in range(len(boxes))])
        assert np.array_equal(b, want)


def test_crop_boxes_frame_index_out_of_range_is_skipped(gpu):
    W, H = 98, 62
    raw, rgb = source("rgb", 0, W, H)
    boxes = np.array([box(40, 30, 20, 20)] * 3)
    got, rois = gpu.crop_boxes(raw, boxes, np.array([0, 1, -1], dtype=np.int32), gpu.roi_opts(W, H), 16, 16)
    assert (rois["x1"] == rois["x0"]).tolist() == [False, True, True] and (got[1:] == -17).all()
    assert np.array_equal(got[0], roi_crop_np(rgb, (30, 20, 50, 40), 16, 16))


# ---- the device chain ----------------------------------------------------------------------------------------------------------------------
CW, CH, DET_B, DET_CONF = 320, 240, 3, 0.25
# chosen on the CPU oracle: the reference decode of these frames keeps about 200 boxes each (at least 9 overall: test_chain_end_to_end asserts it)
DET_SEED, FRAME_SEED = 3, 0x5EC0000


def second_stage(gpu, which):
    """-> (file bytes, input tensor, output tensor, nhwc)"""
    if which == "shipped":
        with open(os.path.join(MODELS, "tiny_160_int8.mars"), "rb") as fh:
            d = fh.read()
    else:
        d = gpu.synth_model(tiny=True, input_hw=160, seed=5)
    hdr, tensors, _ = marsfile.parse(d)
    tin, tout = hdr["inputs"][0], hdr["outputs"][0]
    nhwc = tensors[tin]["fmt"] == marsfile.NHWC
    shp = tensors[tin]["shape"]
    assert (shp[1:] == (160, 160, 3)) if nhwc else (shp[1:] == (3, 160, 160))
    return d, tin, tout, nhwc


class Chain:
    """the detector (anchor twin, 320 x 320, batch 3) with its NV12 frames in HBM"""

    def __init__(self, gpu, flags=0):
        self.gpu, self.flags = gpu, flags
        self.det = gpu.Model(gpu.synth_model(width_x16=4, input_hw=320, seed=DET_SEED), batch=DET_B)
        self.bufs = []

    def frames(self, seed, order=(0, 1, 2)):
        nv = np.stack([lcg_frame(seed + f, CW * CH * 3 // 2) for f in order])
        buf = self.gpu.DeviceBuffer(nv)
        self.bufs.append(buf)
        return nv, buf

    def detect(self, buf):
        """front-end -> graph -> raw-head tail; nothing here waits"""
        self.det.preprocess_nv12_device(buf.ptr, CW, CH, DET_B, flags=self.flags)
        self.det.run_device(sync=False)
        self.det.detect_heads_device(conf=DET_CONF, src=(CW, CH))

    def opts(self, **kw):
        return self.gpu.roi_opts(CW, CH, fmt=self.gpu.CAMERA_NV12, src_flags=self.flags, **kw)

    def close(self):
        self.det.close()
        for b in self.bufs:
            b.free()


_rgb = {}


def expected_input(nv, flags, dets, slots, nhwc, **kw):
    """-> (ROI records, dropped, [slots][160 * 160 * 3] bytes) of the numpy selection + crops over the fetched detections"""
    kw = dict(kw)
    keep = kw.pop("keep_aspect", False)
    kept, dropped = roi_select_np(dets, CW, CH, slots, **kw)
    key = (nv.tobytes(), flags)
    if key not in _rgb:
        _rgb[key] = [nv12_to_rgb_np(nv[f], CW, CH, flags) for f in range(len(nv))]
    rgb = _rgb[key]
    x = np.full((slots, 160 * 160 * 3), -17, dtype=np.int8)
    for k, (f, i, x0, y0, x1, y1) in enumerate(kept):
        x[k] = roi_crop_np(rgb[f], (x0, y0, x1, y1), 160, 160, nhwc, keep)
    return kept, dropped, x


def check_slots(gpu, dst, tin, kept, dropped, want):
    rois, got_dropped = dst.roi_results()
    assert [tuple(int(v) for v in r) for r in rois] == kept and got_dropped == dropped
    for k in range(dst.batch):
        got = dst.read_tensor(tin, frame=k)[:want[k].size].view(np.int8)
        assert np.array_equal(got, want[k]), (k, int((got != want[k]).sum()))


@pytest.mark.parametrize("which", ["shipped", "nhwc_twin"])
def test_chain_end_to_end(gpu, which):
    """preprocess_nv12_device -> run_device -> detect_heads_device -> crop_detections(device) -> second model's run, nothing waiting in
    between; then the detections, the ROI table, the second model's input and output are fetched"""
    d2, tin, tout, nhwc = second_stage(gpu, which)
    c = Chain(gpu)
    dst = gpu.Model(d2, batch=8)
    nv, buf = c.frames(FRAME_SEED)
    c.detect(buf)
    dst.crop_detections(c.det, buf.ptr, c.opts(), device=True)
    dst.run_device(sync=False)
    dets = c.det.detect_results()
    assert sum(len(x) for x in dets) >= 9  # more boxes than the second stage has frames: the drop path runs
    kept, dropped, want = expected_input(nv, 0, dets, 8, nhwc)
    assert len(kept) == 8 and 0 < dropped <= sum(len(x) for x in dets) - 8  # (the rectangle rule skips a few)
    check_slots(gpu, dst, tin, kept, dropped, want)
    out = [dst.read_tensor(tout, frame=k) for k in range(8)]
    # the same model on the expected bytes, written from the host
    for k in range(8):
        dst.write_tensor(tin, want[k], frame=k)
    dst.run_device()
    for k in range(8):
        assert np.array_equal(dst.read_tensor(tout, frame=k), out[k]), k
    assert len({o.tobytes() for o in out}) > 1
    dst.close()
    c.close()


def test_chain_selection_rules(gpu):
    """one detection pass, many option sets (the detections stay in HBM between the crop calls)"""
    d2, tin, tout, nhwc = second_stage(gpu, "shipped")
    c = Chain(gpu, flags=FULL | VU)
    nv, buf = c.frames(FRAME_SEED)
    c.detect(buf)
    best = [float(x["conf"].max()) for x in c.det.detect_results()]
    mid = int(np.argmin(best))  # a frame's boxes depend on that frame alone: the frame whose best box is weakest goes in the middle
    nv, buf = c.frames(FRAME_SEED, order=[f for f in range(3) if f != mid][:1] + [mid] + [f for f in range(3) if f != mid][1:])
    c.detect(buf)
    dets = c.det.detect_results()
    n = [len(x) for x in dets]
    assert min(n) >= 2 and sum(n) >= 9
    classes = sorted({int(v) for x in dets for v in x["cls"]})
    confs = np.sort(np.concatenate([x["conf"] for x in dets]))
    # a threshold no box of frame 1 passes while frames 0 and 2 keep some: a frame with zero boxes between two frames with boxes
    gap = float(np.nextafter(dets[1]["conf"].max(), np.float32(2)))
    assert (dets[0]["conf"] >= gap).any() and (dets[2]["conf"] >= gap).any()
    sets = [dict(), dict(keep_aspect=True), dict(expand=1.25), dict(min_size=24),
            dict(classes=(classes[0], 1)), dict(classes=(classes[len(classes) // 2], max(classes) + 1)), dict(classes=(max(classes) + 1, 3)),
            dict(min_conf=float(confs[len(confs) // 2])), dict(min_conf=gap, max_per_frame=1),
            dict(max_per_frame=1), dict(max_per_frame=4), dict(max_per_frame=0, min_conf=float(confs[0]))]
    seen_short = seen_drop = False
    for batch in (8, 2):
        dst = gpu.Model(d2, batch=batch)
        for kw in sets:
            dst.crop_detections(c.det, buf.ptr, c.opts(**kw), device=True)
            kept, dropped, want = expected_input(nv, FULL | VU, dets, batch, nhwc, **kw)
            check_slots(gpu, dst, tin, kept, dropped, want)
            seen_short |= 0 < len(kept) < batch  # fewer crops than frames: the tail slots are all -17 (compared above)
            seen_drop |= dropped > 0
            if kw == dict(min_conf=gap, max_per_frame=1):
                assert [k[0] for k in kept] == [0, 2] and dropped == 0
            if kw == dict(max_per_frame=4):
                assert ([k[0] for k in kept], dropped) == (([0] * 4 + [1] * 4, 4) if batch == 8 else ([0, 0], 10))
            if kw == dict(classes=(max(classes) + 1, 3)):
                assert kept == [] and (want == -17).all()
        dst.close()
    assert seen_short and seen_drop
    c.close()


def test_chain_repeats_on_new_frames(gpu):
    """three rounds of detect -> crop -> run on different frames, nothing waiting inside a round: every round's input and output are its own
    (the crop overwrites the input only after the earlier run -- plain, captured, replayed -- has read it, and before the next reads it)"""
    d2, tin, tout, nhwc = second_stage(gpu, "nhwc_twin")
    c = Chain(gpu)
    dst = gpu.Model(d2, batch=4)
    ref = gpu.Model(d2, batch=4)
    rounds = [c.frames(FRAME_SEED + 16 * r) for r in range(3)]
    outs = []
    for r, (nv, buf) in enumerate(rounds):  # (the second model's plan runs launch by launch, is captured into a graph, is replayed)
        c.detect(buf)
        dst.crop_detections(c.det, buf.ptr, c.opts(max_per_frame=2), device=True)
        dst.run_device(sync=False)
        dets = c.det.detect_results()
        outs.append([dst.read_tensor(tout, frame=k) for k in range(4)])
        kept, dropped, want = expected_input(nv, 0, dets, 4, nhwc, max_per_frame=2)
        assert [k[0] for k in kept] == [0, 0, 1, 1] and dropped == 2
        check_slots(gpu, dst, tin, kept, dropped, want)
        for k in range(4):
            ref.write_tensor(tin, want[k], frame=k)
        ref.run_device()
        for k in range(4):
            assert np.array_equal(ref.read_tensor(tout, frame=k), outs[r][k]), (r, k)
    assert outs[0][0].tobytes() != outs[1][0].tobytes()
    # two rounds queued with no wait in between: the second crop must not reach the input before the first run has read it
    (nv_a, buf_a), (nv_b, buf_b) = rounds[0], rounds[2]
    c.detect(buf_a)
    dst.crop_detections(c.det, buf_a.ptr, c.opts(max_per_frame=2), device=True)
    dst.run_device(sync=False)
    c.detect(buf_b)
    dst.crop_detections(c.det, buf_b.ptr, c.opts(max_per_frame=2), device=True)
    dets_b = c.det.detect_results()
    _, _, want_b = expected_input(nv_b, 0, dets_b, 4, nhwc, max_per_frame=2)
    for k in range(4):
        assert np.array_equal(dst.read_tensor(tin, frame=k)[:want_b[k].size].view(np.int8), want_b[k]), k
        assert np.array_equal(dst.read_tensor(tout, frame=k), outs[0][k]), k  # the output is still round a's
    dst.close()
    ref.close()
    c.close()


def test_crop_detections_host_frames_and_refusals(gpu):
    d2, tin, tout, nhwc = second_stage(gpu, "shipped")
    c = Chain(gpu)
    dst = gpu.Model(d2, batch=8)
    nv, buf = c.frames(FRAME_SEED)
    BAD_FILE, BAD_TENSOR = gpu.MARS_ERR_INVALID_FILE, gpu.MARS_ERR_INVALID_TENSOR

    def refused(code, det, frames, into, opts, **kw):
        with pytest.raises(gpu.MarsError) as ei:
            into.crop_detections(det, frames, opts, **kw)
        assert ei.value.code == code

    with pytest.raises(gpu.MarsError) as ei:
        dst.roi_results()  # no crop call yet
    assert ei.value.code == BAD_TENSOR
    refused(BAD_TENSOR, c.det, buf.ptr, dst, c.opts(), device=True)  # no detections in HBM yet
    c.detect(buf)
    refused(BAD_TENSOR, c.det, buf.ptr, c.det, c.opts(), device=True)  # det_model == dst_model
    refused(BAD_TENSOR, c.det, buf.ptr, dst, c.opts(), device=True, input_index=1)
    f32 = gpu.Model(gpu.synth_model(tiny=True, input_hw=32, float32=True, seed=5))
    refused(BAD_TENSOR, c.det, buf.ptr, f32, c.opts(), device=True)  # an input that is not int8
    f32.close()
    refused(BAD_FILE, c.det, buf.ptr, dst, gpu.roi_opts(CW + 1, CH, fmt=gpu.CAMERA_NV12), device=True)
    refused(BAD_FILE, c.det, buf.ptr, dst, gpu.roi_opts(CW, CH, fmt=gpu.CAMERA_NV12, src_flags=8), device=True)
    refused(BAD_FILE, c.det, buf.ptr, dst, gpu.roi_opts(CW, CH, fmt=3), device=True)
    # the host-frame form equals the device form
    dst.crop_detections(c.det, nv, c.opts(keep_aspect=True))
    dets = c.det.detect_results()
    kept, dropped, want = expected_input(nv, 0, dets, 8, nhwc, keep_aspect=True)
    check_slots(gpu, dst, tin, kept, dropped, want)
    dst.close()
    c.close()
