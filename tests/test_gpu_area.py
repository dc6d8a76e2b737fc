"""Area averaging on the device (include/mars_hip.h, "Area averaging"): MARS_ROI_AREA through mars_yolo_crop_boxes and the device chain,
MARS_TILE_AREA through the tile front-end, and the rotated calls' refusal.  The expected bytes come from the numpy restatement of
tests/arearef.py (checked by hand in tests/test_area_cpu.py); every comparison is for equal bytes."""
import numpy as np
import pytest

import test_gpu_rot as rot
import tileref
from arearef import area_crop_np, roi_rect_np
from conftest import lcg_frame
from test_gpu_roi import (CH, CW, FRAME_SEED, FULL, SIZES, SOURCE_IDS, SOURCES, VU, Chain, check_rois, check_slots, geometry_boxes, second_stage,
                          source)
from test_gpu_tile import tile_graph
from test_roi_cpu import box, nv12_to_rgb_np, roi_select_np

pytestmark = pytest.mark.gpu

# (tw, th, nhwc): less than a strip; one strip; rows of 99 bytes and a last strip of one row, both layouts; the second stage's size, planar
TARGETS = [(5, 3, 1), (16, 16, 1), (33, 17, 1), (33, 17, 0), (160, 160, 0)]


def rect_box(x0, y0, x1, y1):
    """the box whose rectangle is (x0, y0, x1, y1) under the default expand"""
    return box((x0 + x1) / 2, (y0 + y1) / 2, x1 - x0, y1 - y0)


def area_boxes(W, H, tw, th):
    """geometry_boxes of tests/test_gpu_roi.py (the whole frame, the edges and corners, the skipped boxes, fractional centres, x 7 up and x 5
    down) and the sizes at which the area taps can go wrong, as far as the frame holds them"""
    def at(x0, y0, w, h):
        w, h = min(w, W - x0), min(h, H - y0)
        return rect_box(x0, y0, x0 + w, y0 + h)
    b = [at(4, 2, 2 * tw, 2 * th), at(2, 4, 3 * tw, 3 * th),      # exact ratios: block means
         at(6, 6, tw + 1, th + 1), at(8, 2, 2 * tw - 1, 2 * th - 1),  # every output has two taps; the taps' weights run through every value
         at(0, 10, 2 * tw + 3, max(th // 2, 2)),                   # wide and flat: averaged along x, interpolated along y
         at(10, 0, max(tw // 2, 2), 2 * th + 3),                   # tall and thin
         at(33, 15, 2 * tw, 2 * th), at(33, 15, tw + 2, 3 * th)]   # odd x0, y0: the chroma pair is shared across the crop's edge
    return np.concatenate([geometry_boxes(W, H, tw), np.array(b)])


_want = {}


def want_crop(key, rgb, rect, tw, th, nhwc, keep):
    """area_crop_np, the resize computed once per (frame, rectangle, target) and laid out for both layouts"""
    k = (key, rect, tw, th, keep)
    if k not in _want:
        _want[k] = area_crop_np(rgb, rect, tw, th, True, keep).reshape(th, tw, 3)
    a = _want[k]
    return (a if nhwc else a.transpose(2, 0, 1)).reshape(-1)


@pytest.mark.parametrize("size", SIZES, ids=["98x62", "1280x720"])
@pytest.mark.parametrize("src", SOURCES, ids=SOURCE_IDS)
def test_area_crop_boxes_geometries(gpu, src, size):
    kind, flags = src
    W, H = size
    raw, rgb = source(kind, flags, W, H)
    fmt = gpu.CAMERA_NV12 if kind == "nv12" else gpu.CAMERA_RGB
    averaged = 0
    for tw, th, nhwc in TARGETS:
        boxes = area_boxes(W, H, tw, th)
        rects = [roi_rect_np(b, W, H) for b in boxes]
        assert sum(r is None for r in rects) == 8  # those of geometry_boxes
        averaged += sum(r is not None and (r[2] - r[0] > tw or r[3] - r[1] > th) for r in rects)
        for keep in (False, True):
            o = gpu.roi_opts(W, H, fmt=fmt, src_flags=flags, keep_aspect=keep, area=True)
            got, rois = gpu.crop_boxes(raw, boxes, np.zeros(len(boxes), dtype=np.int32), o, tw, th, nhwc)
            check_rois(rois, rects)
            want = [want_crop((kind, flags, W, H), rgb, r, tw, th, nhwc, keep) for r in rects]
            bad = [i for i in range(len(boxes)) if not np.array_equal(got[i], want[i])]
            assert not bad, (tw, th, nhwc, keep, bad, [int((got[i] != want[i]).sum()) for i in bad])
    assert averaged >= 5 * 8


@pytest.mark.parametrize("src", [SOURCES[0], SOURCES[1]], ids=[SOURCE_IDS[0], SOURCE_IDS[1]])
def test_area_wide_targets(gpu, src):
    """the launcher's other paths: more (column, channel) pairs per thread above 170 and above 682 columns, strips of 4 rows above 640
    columns; few rows, so that the wide targets stay small"""
    kind, flags = src
    W, H = 1280, 720
    raw, rgb = source(kind, flags, W, H)
    fmt = gpu.CAMERA_NV12 if kind == "nv12" else gpu.CAMERA_RGB
    boxes = np.array([rect_box(0, 0, W, H), rect_box(33, 15, 1233, 36), rect_box(101, 201, 1100, 212), rect_box(640, 300, 700, 304),
                      rect_box(7, 9, 7 + 701, 9 + 10)])
    rects = [roi_rect_np(b, W, H) for b in boxes]
    fo = np.zeros(len(boxes), dtype=np.int32)
    for tw, th, nhwc in [(171, 10, 0), (640, 9, 1), (641, 5, 1), (683, 9, 0), (700, 10, 1)]:
        for keep in (False, True):
            got, rois = gpu.crop_boxes(raw, boxes, fo, gpu.roi_opts(W, H, fmt=fmt, src_flags=flags, keep_aspect=keep, area=True), tw, th, nhwc)
            check_rois(rois, rects)
            want = np.stack([area_crop_np(rgb, r, tw, th, nhwc, keep) for r in rects])
            bad = [i for i in range(len(boxes)) if not np.array_equal(got[i], want[i])]
            assert not bad, (tw, th, nhwc, keep, bad)
            plain, _ = gpu.crop_boxes(raw, boxes, fo, gpu.roi_opts(W, H, fmt=fmt, src_flags=flags, keep_aspect=keep), tw, th, nhwc)
            assert np.array_equal(plain[3], got[3]) and not np.array_equal(plain[0], got[0])  # the 60 x 4 box has nothing to average


@pytest.mark.parametrize("src", [SOURCES[0], SOURCES[4]], ids=[SOURCE_IDS[0], SOURCE_IDS[4]])
def test_area_band_one_pixel_wide(gpu, src):
    """min_size = 1 lets a 1 x 20 band through: every output column blends the one source column with itself, the rows are averaged"""
    kind, flags = src
    W, H = 98, 62
    raw, rgb = source(kind, flags, W, H)
    fmt = gpu.CAMERA_NV12 if kind == "nv12" else gpu.CAMERA_RGB
    boxes = np.array([box(10.5, 20, 1, 20), box(20, 10.5, 20, 1), box(33.5, 33.5, 1, 1), box(21, 31, 2, 2)])
    fo = np.zeros(len(boxes), dtype=np.int32)
    for tw, th, nhwc in [(5, 3, 1), (16, 16, 1), (33, 17, 0)]:
        for keep in (False, True):
            got, rois = gpu.crop_boxes(raw, boxes, fo, gpu.roi_opts(W, H, fmt=fmt, src_flags=flags, min_size=1, keep_aspect=keep, area=True), tw, th, nhwc)
            rects = [roi_rect_np(b, W, H, 0.0, 1) for b in boxes]
            assert rects == [(10, 10, 11, 30), (10, 10, 30, 11), (33, 33, 34, 34), (20, 30, 22, 32)]
            check_rois(rois, rects)
            want = np.stack([area_crop_np(rgb, r, tw, th, nhwc, keep) for r in rects])
            assert np.array_equal(got, want), (tw, th, nhwc, keep)


@pytest.mark.parametrize("src", [SOURCES[0], SOURCES[2]], ids=[SOURCE_IDS[0], SOURCE_IDS[2]])
def test_area_flag_with_nothing_to_average_changes_no_byte(gpu, src):
    kind, flags = src
    fmt = gpu.CAMERA_NV12 if kind == "nv12" else gpu.CAMERA_RGB
    for (W, H) in SIZES:
        raw, rgb = source(kind, flags, W, H)
        for tw, th, nhwc in TARGETS:
            b = [rect_box(7, 5, 7 + min(tw, W - 7), 5 + min(th, H - 5)), rect_box(33, 15, 33 + min(max(tw // 2, 2), W - 33), 15 + min(th, H - 15)),
                 rect_box(0, 0, min(tw, W), max(th // 3, 2)), rect_box(40, 20, 40 + max(tw // 7, 2), 20 + max(th // 7, 2)), box(21, 31, 2, 2),
                 box(W - 1, H - 1, min(tw, 40), min(th, 40)), box(W + 50, H / 2, 20, 20)]
            boxes = np.array(b)
            rects = [roi_rect_np(x, W, H) for x in boxes]
            assert all(r is None or (r[2] - r[0] <= tw and r[3] - r[1] <= th) for r in rects) and sum(r is None for r in rects) == 1
            fo = np.zeros(len(boxes), dtype=np.int32)
            for keep in (False, True):
                kw = dict(fmt=fmt, src_flags=flags, keep_aspect=keep)
                a, ra = gpu.crop_boxes(raw, boxes, fo, gpu.roi_opts(W, H, area=True, **kw), tw, th, nhwc)
                u, ru = gpu.crop_boxes(raw, boxes, fo, gpu.roi_opts(W, H, **kw), tw, th, nhwc)
                assert ra.tobytes() == ru.tobytes() and np.array_equal(a, u), (W, tw, th, nhwc, keep, int((a != u).sum()))


@pytest.mark.parametrize("flags", [0, FULL, VU, FULL | VU], ids=SOURCE_IDS[1:])
def test_nv12_area_crop_equals_rgb_area_crop_of_the_converted_frame(gpu, flags):
    """two frames per call (the second starts at an odd multiple of 2 bytes), boxes in both: the NV12 crops are the RGB crops of the
    library's own nv12_to_rgb of those frames"""
    W, H = 98, 62
    nv = np.stack([lcg_frame(0x204000 + 7 * flags + f, W * H * 3 // 2) for f in range(2)])
    assert (W * H * 3 // 2) % 4 == 2
    rgb = np.stack([gpu.nv12_to_rgb(nv[f], W, H, flags) for f in range(2)])
    boxes = np.concatenate([area_boxes(W, H, 16, 16), area_boxes(W, H, 5, 3)])
    fo = (np.arange(len(boxes)) % 2).astype(np.int32)
    for tw, th, nhwc, keep in [(16, 16, 0, False), (33, 17, 1, True), (5, 3, 1, False)]:
        a, ra = gpu.crop_boxes(nv, boxes, fo, gpu.roi_opts(W, H, fmt=gpu.CAMERA_NV12, src_flags=flags, keep_aspect=keep, area=True), tw, th, nhwc)
        b, rb = gpu.crop_boxes(rgb, boxes, fo, gpu.roi_opts(W, H, keep_aspect=keep, area=True), tw, th, nhwc)
        assert ra.tobytes() == rb.tobytes() and (ra["frame"] == fo).all()
        assert np.array_equal(a, b), int((a != b).sum())
        want = np.stack([area_crop_np(rgb[fo[i]], roi_rect_np(boxes[i], W, H), tw, th, nhwc, keep) for i in range(len(boxes))])
        assert np.array_equal(b, want)


def test_area_wide_accumulators(gpu):
    """cw * ch = 3840 * 4400 = 16 896 000 > 16 843 009: S passes 2^32 in every output pixel, the sums need 64 bits.  The frame is all 255 but
    for its first and last pixel: every one of the 16 x 16 outputs is the rounded mean of a 240 x 275 block (the single zero in the two corner
    blocks moves their means by 255 / 66 000, which rounds away: the restatement gives 127 there too)"""
    W, H = 3840, 4400
    assert W * H > 16843009 and 255 * W * H > 1 << 32
    frame = np.full((H, W, 3), 255, dtype=np.uint8)
    frame[0, 0] = 0
    frame[-1, -1] = 0
    got, rois = gpu.crop_boxes(frame, np.array([box(W / 2, H / 2, W, H)]), np.zeros(1, dtype=np.int32), gpu.roi_opts(W, H, area=True), 16, 16, True)
    assert tuple(rois[0])[2:] == (0, 0, W, H)
    want = area_crop_np(frame, (0, 0, W, H), 16, 16)
    assert np.array_equal(got[0], want), int((got[0] != want).sum())
    assert (want == 127).all()


# ---- tiles -------------------------------------------------------------------------------------------------------------------------------
TILES = tileref.grid(98, 62, 56, 36, 14, 10) + [(0, 0, 98, 62)]  # 2 x 2 tiles of 56 x 36 and the whole frame


@pytest.mark.parametrize("src", [SOURCES[0], SOURCES[3]], ids=[SOURCE_IDS[0], SOURCE_IDS[3]])
def test_area_tiles_equal_area_crops(gpu, src):
    kind, flags = src
    W, H = 98, 62
    assert len(TILES) == 5 and TILES[0] == (0, 0, 56, 36) and TILES[3] == (42, 26, 98, 62)
    fmt = dict(fmt=gpu.CAMERA_NV12, src_flags=flags) if kind == "nv12" else {}
    nb = W * H * 3 // 2 if kind == "nv12" else W * H * 3
    frames = np.stack([lcg_frame(0x205000 + f, nb) for f in range(2)])
    boxes = np.array([rect_box(*t) for t in TILES] * 2)
    fo = np.repeat(np.arange(2, dtype=np.int32), len(TILES))
    for tw, th, nhwc in [(16, 16, 1), (33, 17, 0), (56, 36, 1)]:
        for keep in (False, True):
            got = gpu.tile_frames(frames, gpu.tile_opts(W, H, TILES, keep_aspect=keep, area=True, **fmt), tw, th, nhwc)
            want, rois = gpu.crop_boxes(frames, boxes, fo, gpu.roi_opts(W, H, min_size=1, keep_aspect=keep, area=True, **fmt), tw, th, nhwc)
            assert [tuple(r)[2:] for r in rois] == TILES * 2
            assert got.shape == want.shape and np.array_equal(got, want), (tw, th, nhwc, keep, int((got != want).sum()))
            plain = gpu.tile_frames(frames, gpu.tile_opts(W, H, TILES, keep_aspect=keep, **fmt), tw, th, nhwc)
            assert (tw, th) == (56, 36) or not np.array_equal(plain, got)  # the flag does something
            if (tw, th) == (56, 36):  # the grid's tiles have the target's size: still the exact copy, whole frame beside them or not
                rgb = [frames[f].reshape(H, W, 3) if kind == "rgb" else nv12_to_rgb_np(frames[f], W, H, flags) for f in range(2)]
                for f in range(2):
                    for t, (x0, y0, x1, y1) in enumerate(TILES[:4]):
                        assert np.array_equal(got[f * 5 + t].reshape(36, 56, 3), (rgb[f][y0:y1, x0:x1].astype(np.int16) - 128).astype(np.int8))
                        assert np.array_equal(got[f * 5 + t], plain[f * 5 + t])


@pytest.mark.parametrize("nchw", [False, True])
def test_area_tiles_into_a_graph_input(gpu, nchw):
    """Model.preprocess_tiles under MARS_TILE_AREA, host and device frames: the graph input holds the bytes of the host form, which are those
    of the restatement: the whole 96 x 64 frame into 64 x 64 (x averaged, y copied) and a 64 x 64 tile (copied)"""
    W, H, S = 96, 64, 64
    tiles = [(0, 0, W, H), (16, 0, 80, 64)]
    d, tin, _ = tile_graph(nchw)
    m = gpu.Model(d, batch=4)
    frames = np.stack([lcg_frame(0x206000 + f, W * H * 3) for f in range(2)]).reshape(2, H, W, 3)
    o = gpu.tile_opts(W, H, tiles, flags=gpu.TILE_AREA)
    assert o.flags == 16
    host = gpu.tile_frames(frames, o, S, S, not nchw)
    want = np.stack([area_crop_np(frames[f], t, S, S, not nchw) for f in range(2) for t in tiles])
    assert np.array_equal(host, want)
    assert not np.array_equal(host, gpu.tile_frames(frames, gpu.tile_opts(W, H, tiles), S, S, not nchw))
    buf = gpu.DeviceBuffer(frames)
    for device in (False, True):
        for f in range(4):
            m.write_tensor(tin, np.full(S * S * 3, 5, dtype=np.int8), frame=f)
        m.preprocess_tiles(buf.ptr if device else frames, o, device=device)
        for f in range(4):
            assert np.array_equal(m.read_tensor(tin, frame=f)[:S * S * 3].view(np.int8), host[f]), (device, f)
    m.close()
    buf.free()


# ---- the device chain ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["shipped", "nhwc_twin"])
def test_area_chain_end_to_end(gpu, which):
    """test_chain_end_to_end of tests/test_gpu_roi.py with the flag: the second model's input holds the area crops of the ROI table, and the
    table is the one of the unflagged call.  The detector's boxes in its 320 x 240 frames are smaller than the 160 x 160 input, so the chain
    runs a second time with expand = 3: rectangles up to the whole frame, which the flag averages"""
    d2, tin, tout, nhwc = second_stage(gpu, which)
    c = Chain(gpu)
    dst = gpu.Model(d2, batch=8)
    nv, buf = c.frames(FRAME_SEED)
    c.detect(buf)
    dets = c.det.detect_results()
    rgb = [nv12_to_rgb_np(nv[f], CW, CH, 0) for f in range(len(nv))]
    averaged = 0
    for kw in ({}, {"expand": 3.0}):
        dst.crop_detections(c.det, buf.ptr, c.opts(**kw), device=True)
        plain_rois, plain_dropped = dst.roi_results()
        plain = [dst.read_tensor(tin, frame=k).tobytes() for k in range(8)]
        dst.crop_detections(c.det, buf.ptr, c.opts(area=True, **kw), device=True)
        dst.run_device(sync=False)
        kept, dropped = roi_select_np(dets, CW, CH, 8, **kw)
        assert len(kept) == 8 and dropped > 0
        rois, got_dropped = dst.roi_results()
        assert rois.tobytes() == plain_rois.tobytes() and got_dropped == plain_dropped
        want = np.stack([area_crop_np(rgb[f], (x0, y0, x1, y1), 160, 160, nhwc) for (f, i, x0, y0, x1, y1) in kept])
        check_slots(gpu, dst, tin, kept, dropped, want)
        down = [k for k, r in enumerate(kept) if r[4] - r[2] > 160 or r[5] - r[3] > 160]
        averaged += len(down)
        for k in range(8):  # the flag changes the crops of the larger boxes, and only those
            assert (dst.read_tensor(tin, frame=k).tobytes() != plain[k]) == (k in down), k
        out = [dst.read_tensor(tout, frame=k) for k in range(8)]
        for k in range(8):
            dst.write_tensor(tin, want[k], frame=k)
        dst.run_device()
        for k in range(8):
            assert np.array_equal(dst.read_tensor(tout, frame=k), out[k]), k
    assert averaged > 0, "no kept box is larger than the second model's input: the flag shows nothing here"
    dst.close()
    c.close()


# ---- the rotated calls -----------------------------------------------------------------------------------------------------------------------
def test_rotated_calls_refuse_the_flag_on_a_live_model(gpu):
    d2, tin, tout, nhwc = rot.second_stage(gpu, "shipped")
    c = rot.Chain(gpu)
    dst = gpu.Model(d2, batch=8)
    nv, buf = c.frames(rot.FRAME_SEED)
    c.detect(buf)
    mark = [lcg_frame(0x207000 + k, 160 * 160 * 3).view(np.int8) for k in range(8)]
    for k in range(8):
        dst.write_tensor(tin, mark[k], frame=k)
    for keep in (False, True):
        for call in (lambda o: dst.crop_obb_detections_device(c.det, buf.ptr, o), lambda o: dst.crop_obb_detections(c.det, nv, o)):
            with pytest.raises(gpu.MarsError) as ei:
                call(c.opts(area=True, keep_aspect=keep))
            assert ei.value.code == gpu.MARS_ERR_INVALID_FILE
    boxes = np.array([rot.obb(49, 31, 30, 14, 0.3)])
    with pytest.raises(gpu.MarsError) as ei:
        gpu.crop_obb(rot.source("rgb", 0, rot.W, rot.H)[0], boxes, np.zeros(1, dtype=np.int32), gpu.roi_opts(rot.W, rot.H, area=True), 16, 16)
    assert ei.value.code == gpu.MARS_ERR_INVALID_FILE
    for k in range(8):
        assert np.array_equal(dst.read_tensor(tin, frame=k)[:mark[k].size].view(np.int8), mark[k]), k
    dst.crop_obb_detections_device(c.det, buf.ptr, c.opts())  # (without the flag the same call goes through)
    assert any(not np.array_equal(dst.read_tensor(tin, frame=k)[:mark[k].size].view(np.int8), mark[k]) for k in range(8))
    dst.close()
    c.close()
