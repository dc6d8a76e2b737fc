"""Rotated crops on the device (include/mars_hip.h, "Rotated crops"): mars_yolo_crop_obb, the device chain obb detector -> rotated crops ->
second model, the selection rules, the ROI table and the label join.  The expected bytes come from the numpy restatement of tests/rotref.py
(checked by hand in tests/test_rot_cpu.py); every comparison is bit-exact."""
import os

import numpy as np
import pytest

import marsfile
from conftest import lcg_frame
from rotref import nv12_to_rgb_np, obb, rot_crop_np, rot_rect_np, rot_select_np

pytestmark = pytest.mark.gpu

F = np.float32
MODELS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "models")
FULL, VU = 1, 2
SOURCES = [("rgb", 0), ("nv12", 0), ("nv12", FULL), ("nv12", VU), ("nv12", FULL | VU)]
SOURCE_IDS = ["rgb", "nv12_limited_uv", "nv12_full_uv", "nv12_limited_vu", "nv12_full_vu"]
W, H = 98, 62


def lcg_angles(n, seed=0x0B0B):
    """n angles of the obb rule's interval [-pi / 4, 3 pi / 4), drawn by the suite's LCG"""
    raw = lcg_frame(seed, 2 * n).astype(np.uint32)
    u = (raw[0::2] * 256 + raw[1::2]).astype(np.float64) / 65536.0
    return [float(F(-np.pi / 4 + u[k] * np.pi)) for k in range(n)]


QUARTER = float(F(np.pi / 4))
ANGLES = [0.0, float(F(np.pi / 2)), -QUARTER, float(np.nextafter(F(3 * np.pi / 4), F(0))), QUARTER] + lcg_angles(12)
# (x, y, w, h) of the boxes that are kept at every angle
KEPT = [(49, 31, 30, 14),                                                     # inside the frame
        (3, 31, 20, 12), (95, 31, 20, 12), (49, 2, 20, 12), (49, 60, 20, 12),  # over each edge
        (4, 4, 24, 16), (94, 4, 24, 16), (4, 58, 24, 16), (94, 58, 24, 16),    # over each corner
        (0, 0, 16, 10), (98, 62, 16, 10),                                      # centred on a corner
        (21.3, 31.7, 2, 2),                                                    # the smallest kept
        (49, 31, 150, 20),                                                     # wider than the frame
        (30.5, 25.25, 11.5, 9.25)]                                             # fractional centre and sides
NAN, INF = float("nan"), float("inf")
SKIPPED = [obb(NAN, 31, 20, 20, 0.3), obb(49, 31, 0, 20, 0.3), obb(49, 31, 20, INF, 0.3), obb(49, 31, 20, 20, NAN),
           obb(120, 31, 20, 20, 0.3), obb(49, -3, 20, 20, 0.3), obb(49, 31, 1.5, 10, 0.3), obb(49, 31, 40000, 10, 0.3)]

_frames = {}


def source(kind, flags, w, h, n=1):
    """-> (n frames' bytes as the library takes them, the same frames as uint8 RGB [n][h][w][3]); made once per size and flag set"""
    key = (kind, flags, w, h, n)
    if key not in _frames:
        if kind == "rgb":
            raw = np.stack([lcg_frame(0x301000 + w + f, w * h * 3) for f in range(n)])
            _frames[key] = (raw, raw.reshape(n, h, w, 3))
        else:
            raw = np.stack([lcg_frame(0x302000 + w + f, w * h * 3 // 2) for f in range(n)])
            _frames[key] = (raw, np.stack([nv12_to_rgb_np(raw[f], w, h, flags) for f in range(n)]))
    return _frames[key]


def geometry_boxes():
    return np.array([obb(x, y, w, h, a) for (x, y, w, h) in KEPT for a in ANGLES] + SKIPPED)


def check_rois(rois, boxes, fo, w, h, expand=0.0, min_size=0):
    kept = 0
    for i, b in enumerate(boxes):
        r = rot_rect_np(b, w, h, expand, min_size)
        assert rois[i]["frame"] == fo[i] and rois[i]["det"] == -1
        if r is None:
            assert rois[i]["x1"] == rois[i]["x0"], i
        else:
            assert (rois[i]["x0"], rois[i]["y0"], rois[i]["x1"], rois[i]["y1"]) == r and r[2] > r[0] and r[3] > r[1], i
            kept += 1
    return kept


@pytest.mark.parametrize("src", SOURCES, ids=SOURCE_IDS)
def test_crop_obb_geometries(gpu, src):
    kind, flags = src
    raw, rgb = source(kind, flags, W, H, 2)
    fmt = gpu.CAMERA_NV12 if kind == "nv12" else gpu.CAMERA_RGB
    boxes = geometry_boxes()
    fo = (np.arange(len(boxes)) % 2).astype(np.int32)
    for tw, th in [(32, 32), (40, 24)]:
        for keep, expand in [(False, 0.0), (True, 1.25)]:
            want = np.stack([rot_crop_np(rgb[fo[i]], boxes[i], tw, th, True, keep, expand) for i in range(len(boxes))])
            for nhwc in (1, 0):
                o = gpu.roi_opts(W, H, fmt=fmt, src_flags=flags, expand=expand, keep_aspect=keep)
                got, rois = gpu.crop_obb(raw, boxes, fo, o, tw, th, nhwc)
                # nothing is left out silently: every box of KEPT at every angle is a crop, every box of SKIPPED is not
                assert check_rois(rois, boxes, fo, W, H, expand) == len(KEPT) * len(ANGLES) == len(boxes) - 8
                w = want if nhwc else want.reshape(-1, th, tw, 3).transpose(0, 3, 1, 2).reshape(len(boxes), -1)
                bad = [i for i in range(len(boxes)) if not np.array_equal(got[i], w[i])]
                assert not bad, (tw, th, nhwc, keep, expand, bad[:8], int((got != w).sum()))
                assert (got[-8:] == -17).all() and not (got[0] == -17).all()


@pytest.mark.parametrize("src", [SOURCES[0], SOURCES[4]], ids=[SOURCE_IDS[0], SOURCE_IDS[4]])
def test_crop_obb_scale_limits(gpu, src):
    """a 13 x down-scale along the diagonal (the staged chunk must shrink to a few columns), and a 4 x / 8 x up-scale into the second stage's size"""
    kind, flags = src
    BW, BH = 640, 360
    raw, rgb = source(kind, flags, BW, BH)
    fmt = gpu.CAMERA_NV12 if kind == "nv12" else gpu.CAMERA_RGB
    down = np.array([obb(320, 180, 600, 300, QUARTER), obb(320, 180, 600, 300, float(F(np.pi / 6))), obb(300.5, 170.25, 600, 300, 0.0),
                     obb(320, 180, 300, 600, -QUARTER)])
    up = np.array([obb(320, 180, 40, 20, 0.3), obb(5, 355, 40, 20, QUARTER), obb(100.5, 99.5, 20, 40, float(F(np.pi / 2)))])
    for boxes, tw, th in [(down, 32, 32), (up, 160, 160)]:
        fo = np.zeros(len(boxes), dtype=np.int32)
        for nhwc, keep in [(1, False), (0, True)]:
            got, rois = gpu.crop_obb(raw, boxes, fo, gpu.roi_opts(BW, BH, fmt=fmt, src_flags=flags, keep_aspect=keep), tw, th, nhwc)
            assert check_rois(rois, boxes, fo, BW, BH) == len(boxes)
            for i, b in enumerate(boxes):
                want = rot_crop_np(rgb[0], b, tw, th, nhwc, keep)
                assert np.array_equal(got[i], want), (tw, th, nhwc, keep, i, int((got[i] != want).sum()))


@pytest.mark.parametrize("flags", [0, FULL, VU, FULL | VU], ids=SOURCE_IDS[1:])
def test_rotated_nv12_crop_equals_rgb_crop_of_the_converted_frame(gpu, flags):
    nv = np.stack([lcg_frame(0x303000 + 7 * flags + f, W * H * 3 // 2) for f in range(2)])
    rgb = np.stack([gpu.nv12_to_rgb(nv[f], W, H, flags) for f in range(2)])
    boxes = geometry_boxes()
    fo = (np.arange(len(boxes)) % 2).astype(np.int32)
    for tw, th, nhwc, keep in [(32, 32, 0, False), (40, 24, 1, True)]:
        a, ra = gpu.crop_obb(nv, boxes, fo, gpu.roi_opts(W, H, fmt=gpu.CAMERA_NV12, src_flags=flags, keep_aspect=keep), tw, th, nhwc)
        b, rb = gpu.crop_obb(rgb, boxes, fo, gpu.roi_opts(W, H, keep_aspect=keep), tw, th, nhwc)
        assert ra.tobytes() == rb.tobytes() and (ra["frame"] == fo).all()
        assert np.array_equal(a, b), int((a != b).sum())


def test_crop_obb_min_size_and_frame_index(gpu):
    raw, rgb = source("rgb", 0, W, H, 2)
    boxes = np.array([obb(40, 30, 1.5, 10, 0.4), obb(40, 30, 20, 12, 0.4), obb(40, 30, 20, 12, 0.4), obb(40, 30, 20, 12, 0.4)])
    fo = np.array([0, 1, 2, -1], dtype=np.int32)
    got, rois = gpu.crop_obb(raw, boxes, fo, gpu.roi_opts(W, H, min_size=1, expand=1.0), 32, 32)
    assert (rois["x1"] == rois["x0"]).tolist() == [False, False, True, True] and (got[2:] == -17).all()
    assert np.array_equal(got[0], rot_crop_np(rgb[0], boxes[0], 32, 32, min_size=1)) and np.array_equal(got[1], rot_crop_np(rgb[1], boxes[1], 32, 32))
    got, rois = gpu.crop_obb(raw, boxes, fo, gpu.roi_opts(W, H), 32, 32)
    assert (rois["x1"] == rois["x0"]).tolist() == [True, False, True, True] and (got[0] == -17).all()


# ---- the device chain ----------------------------------------------------------------------------------------------------------------------
# The obb twin's random weights give boxes a thousand pixels long, most of them centred outside the frame.  At its smallest input (32 x 32: 21
# predictions) one box per frame has its centre inside, so the selection rules need the next size (64 x 64: 84 predictions, two to five such
# boxes per frame, several classes and angles); `expand` of a twentieth brings the crops to the size of the second stage's input.
CW, CH, DET_B, DET_CONF = 320, 240, 4, 0.01
DET_HW_MIN, DET_HW = 32, 64
BASE = dict(expand=0.05)
FRAME_SEED = 0x0BBC0000


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
    """the obb twin, batch 4, with its NV12 frames in HBM"""

    def __init__(self, gpu, flags=0, hw=DET_HW):
        self.gpu, self.flags = gpu, flags
        d = gpu.synth_model(width_x16=1, input_hw=hw, seed=1, head="obb")
        self.angs = gpu.obb_twin_tensors(d)
        self.det = gpu.Model(d, batch=DET_B)
        self.bufs = []

    def frames(self, seed):
        nv = np.stack([lcg_frame(seed + f, CW * CH * 3 // 2) for f in range(DET_B)])
        buf = self.gpu.DeviceBuffer(nv)
        self.bufs.append(buf)
        return nv, buf

    def detect(self, buf):
        """front-end -> graph -> oriented tail; nothing here waits"""
        self.det.preprocess_nv12_device(buf.ptr, CW, CH, DET_B, flags=self.flags)
        self.det.run_device(sync=False)
        self.det.detect_obb_device(self.gpu.obb_opts(self.angs), conf=DET_CONF, src=(CW, CH))

    def opts(self, **kw):
        return self.gpu.roi_opts(CW, CH, fmt=self.gpu.CAMERA_NV12, src_flags=self.flags, **{**BASE, **kw})

    def close(self):
        self.det.close()
        for b in self.bufs:
            b.free()


_rgb = {}


def expected_input(nv, flags, boxes, slots, nhwc, **kw):
    """-> (ROI records, dropped, [slots][160 * 160 * 3] bytes) of the numpy selection + rotated crops over the fetched obb records"""
    kw = {**BASE, **kw}
    keep = kw.pop("keep_aspect", False)
    kept, dropped = rot_select_np(boxes, CW, CH, slots, **kw)
    key = (nv.tobytes(), flags)
    if key not in _rgb:
        _rgb[key] = [nv12_to_rgb_np(nv[f], CW, CH, flags) for f in range(len(nv))]
    rgb = _rgb[key]
    x = np.full((slots, 160 * 160 * 3), -17, dtype=np.int8)
    for k, (f, i, *_r) in enumerate(kept):
        x[k] = rot_crop_np(rgb[f], boxes[f][i], 160, 160, nhwc, keep, kw.get("expand", 0.0), kw.get("min_size", 0))
    return kept, dropped, x


def check_slots(dst, tin, kept, dropped, want):
    rois, got_dropped = dst.roi_results()
    assert [tuple(int(v) for v in r) for r in rois] == kept and got_dropped == dropped
    for k in range(dst.batch):
        got = dst.read_tensor(tin, frame=k)[:want[k].size].view(np.int8)
        assert np.array_equal(got, want[k]), (k, int((got != want[k]).sum()))


@pytest.mark.parametrize("hw", [DET_HW_MIN, DET_HW])
@pytest.mark.parametrize("which", ["shipped", "nhwc_twin"])
def test_chain_end_to_end(gpu, which, hw):
    """preprocess_nv12_device -> run_device -> detect_obb_device -> crop_obb_detections_device -> run -> classify -> label_detections, nothing
    waiting in between; then the lists, the ROI table, the second model's input and the labels are fetched"""
    d2, tin, tout, nhwc = second_stage(gpu, which)
    c = Chain(gpu, hw=hw)
    dst = gpu.Model(d2, batch=8)
    nv, buf = c.frames(FRAME_SEED)
    c.detect(buf)
    before = ([x.tobytes() for x in c.det.detect_results()], [x.tobytes() for x in c.det.obb_results()])
    c.detect(buf)
    dst.crop_obb_detections_device(c.det, buf.ptr, c.opts())
    dst.run_device(sync=False)
    dst.classify_device(top_k=3)
    c.det.label_detections(dst)
    dets, boxes = c.det.detect_results(), c.det.obb_results()
    assert ([x.tobytes() for x in dets], [x.tobytes() for x in boxes]) == before  # the crop call leaves both lists alone
    assert all(len(a) == len(b) for a, b in zip(dets, boxes)) and sum(len(x) for x in boxes) >= 9
    assert len({float(b["angle"]) for x in boxes for b in x}) > 3
    kept, dropped, want = expected_input(nv, 0, boxes, 8, nhwc)
    if hw == DET_HW_MIN:  # one box per frame or so: the slots behind the last crop are -17
        assert 4 <= len(kept) < 8 and dropped == 0 and (want[len(kept):] == -17).all() and not (want[:len(kept)] == -17).all()
    else:  # more boxes than the second stage has frames: the drop path runs
        assert len(kept) == 8 and dropped > 0
    assert sum(len(x) for x in boxes) > len(kept) + dropped  # the centre rule skips boxes of the lists
    check_slots(dst, tin, kept, dropped, want)
    top, _ = dst.classify_results(3)
    labels = c.det.label_results()
    assert int((labels["cls"] >= 0).sum()) == len(kept)
    for k, (f, i, *_r) in enumerate(kept):  # the join is on det, which indexes the detection list and the obb records alike
        assert labels[f, i].tobytes() == top[k, 0].tobytes()
    # a short destination: slots behind the last crop are -17
    big = gpu.Model(d2, batch=32)
    big.crop_obb_detections_device(c.det, buf.ptr, c.opts(max_per_frame=3))
    kept, dropped, want = expected_input(nv, 0, boxes, 32, nhwc, max_per_frame=3)
    assert 0 < len(kept) <= 12 and dropped == 0 and (want[len(kept):] == -17).all()
    check_slots(big, tin, kept, dropped, want)
    big.close()
    dst.close()
    c.close()


def test_chain_selection_rules(gpu):
    """one detection pass, many option sets (the obb records stay in HBM between the crop calls)"""
    d2, tin, tout, nhwc = second_stage(gpu, "shipped")
    c = Chain(gpu, flags=FULL | VU)
    nv, buf = c.frames(FRAME_SEED)
    c.detect(buf)
    boxes = c.det.obb_results()
    n = [len(x) for x in boxes]
    assert sum(n) >= 9
    classes = sorted({int(v) for x in boxes for v in x["cls"]})
    confs = np.sort(np.concatenate([x["conf"] for x in boxes]))
    sets = [dict(), dict(keep_aspect=True), dict(expand=0.08), dict(expand=1.0), dict(min_size=24), dict(min_size=100000),
            dict(classes=(classes[0], 1)), dict(classes=(classes[len(classes) // 2], max(classes) + 1)), dict(classes=(max(classes) + 1, 3)),
            dict(min_conf=float(confs[len(confs) // 2])), dict(max_per_frame=1), dict(max_per_frame=2, min_conf=float(confs[1]))]
    seen_short = seen_drop = False
    for batch in (8, 2):
        dst = gpu.Model(d2, batch=batch)
        for kw in sets:
            dst.crop_obb_detections_device(c.det, buf.ptr, c.opts(**kw))
            kept, dropped, want = expected_input(nv, FULL | VU, boxes, batch, nhwc, **kw)
            check_slots(dst, tin, kept, dropped, want)
            seen_short |= 0 < len(kept) < batch
            seen_drop |= dropped > 0
            if kw in (dict(classes=(max(classes) + 1, 3)), dict(min_size=100000)):
                assert kept == [] and dropped == 0 and (want == -17).all()
            if kw == dict(max_per_frame=1):
                assert len({k[0] for k in kept}) == len(kept)
        dst.close()
    assert seen_short and seen_drop
    c.close()


def test_chain_repeats_on_new_frames(gpu):
    """three rounds of detect -> rotated crop -> run on different frames, nothing waiting inside a round: every round's input is its own"""
    d2, tin, tout, nhwc = second_stage(gpu, "nhwc_twin")
    c = Chain(gpu)
    dst = gpu.Model(d2, batch=4)
    ref = gpu.Model(d2, batch=4)
    outs = []
    for r in range(3):
        nv, buf = c.frames(FRAME_SEED + 16 * (r + 1))
        c.detect(buf)
        dst.crop_obb_detections_device(c.det, buf.ptr, c.opts(max_per_frame=2))
        dst.run_device(sync=False)
        boxes = c.det.obb_results()
        outs.append([dst.read_tensor(tout, frame=k) for k in range(4)])
        kept, dropped, want = expected_input(nv, 0, boxes, 4, nhwc, max_per_frame=2)
        assert len(kept) == 4
        check_slots(dst, tin, kept, dropped, want)
        for k in range(4):
            ref.write_tensor(tin, want[k], frame=k)
        ref.run_device()
        for k in range(4):
            assert np.array_equal(ref.read_tensor(tout, frame=k), outs[r][k]), (r, k)
    assert outs[0][0].tobytes() != outs[1][0].tobytes()
    dst.close()
    ref.close()
    c.close()


def test_crop_obb_host_frames_and_refusals(gpu):
    d2, tin, tout, nhwc = second_stage(gpu, "shipped")
    c = Chain(gpu)
    dst = gpu.Model(d2, batch=8)
    nv, buf = c.frames(FRAME_SEED)
    BAD_FILE, BAD_TENSOR = gpu.MARS_ERR_INVALID_FILE, gpu.MARS_ERR_INVALID_TENSOR

    def refused(code, det, frames, into, opts, **kw):
        with pytest.raises(gpu.MarsError) as ei:
            into.crop_obb_detections_device(det, frames, opts, **kw)
        assert ei.value.code == code

    refused(BAD_TENSOR, c.det, buf.ptr, dst, c.opts())  # no obb results in HBM yet
    # an upright DFL decode leaves detections, not obb results
    c.det.preprocess_nv12_device(buf.ptr, CW, CH, DET_B)
    c.det.run_device(sync=False)
    c.det.detect_dfl_device(conf=DET_CONF, src=(CW, CH))
    refused(BAD_TENSOR, c.det, buf.ptr, dst, c.opts())
    dst.crop_detections(c.det, buf.ptr, c.opts(), device=True)  # (the upright call takes them)
    c.detect(buf)
    refused(BAD_TENSOR, c.det, buf.ptr, c.det, c.opts())  # det_model == dst_model
    refused(BAD_TENSOR, c.det, buf.ptr, dst, c.opts(), input_index=1)
    refused(BAD_FILE, c.det, buf.ptr, dst, gpu.roi_opts(CW + 1, CH, fmt=gpu.CAMERA_NV12))  # odd NV12 sizes
    refused(BAD_FILE, c.det, buf.ptr, dst, gpu.roi_opts(CW, CH + 1, fmt=gpu.CAMERA_NV12))
    refused(BAD_FILE, c.det, buf.ptr, dst, gpu.roi_opts(CW, CH, fmt=gpu.CAMERA_NV12, src_flags=8))
    dst.pipe_open()
    refused(BAD_TENSOR, c.det, buf.ptr, dst, c.opts())  # an open pipe
    dst.pipe_close()
    # the host-frame form equals the device form
    dst.crop_obb_detections(c.det, nv, c.opts(keep_aspect=True))
    boxes = c.det.obb_results()
    kept, dropped, want = expected_input(nv, 0, boxes, 8, nhwc, keep_aspect=True)
    assert len(kept) > 0
    check_slots(dst, tin, kept, dropped, want)
    dst.close()
    c.close()
