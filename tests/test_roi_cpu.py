"""ROI crops (include/mars_hip.h, "ROI crops"), the part that needs no GPU: the new entry points are exported, mars_roi_t is 24 bytes, arguments
that can never be valid are refused up front, and the numpy restatement of the arithmetic that tests/test_gpu_roi.py compares the device
against is itself checked on cases worked out by hand."""
import ctypes as C

import numpy as np

F = np.float32
NEW = ["mars_yolo_crop_boxes", "mars_hip_crop_detections_device", "mars_hip_crop_detections", "mars_hip_roi_results"]


# ---- the numpy restatement (int64 positions, np.float32 scalar steps for the rectangle) ----------------------------------------------
def roi_rect_np(box, W, H, expand=0.0, min_size=0):
    """box -> (x0, y0, x1, y1), or None if the box is skipped"""
    e = F(expand) if expand else F(1.0)
    ms = int(min_size) if min_size else 2
    x, y, w, h, conf = F(box["x"]), F(box["y"]), F(box["w"]), F(box["h"]), F(box["conf"])
    if not all(np.isfinite(v) for v in (x, y, w, h, conf)) or not w > 0 or not h > 0:
        return None
    with np.errstate(over="ignore"):
        hw, hh = F(F(w * e) * F(0.5)), F(F(h * e) * F(0.5))
        x0f, x1f = max(F(x - hw), F(0)), min(F(x + hw), F(W))
        y0f, y1f = max(F(y - hh), F(0)), min(F(y + hh), F(H))
    # (the conversions of far-away boxes: limited first, which changes no decision)
    x0, x1 = int(np.floor(min(x0f, F(W + 1)))), int(np.ceil(max(x1f, F(-1))))
    y0, y1 = int(np.floor(min(y0f, F(H + 1)))), int(np.ceil(max(y1f, F(-1))))
    if x1 - x0 < ms or y1 - y0 < ms:
        return None
    return x0, y0, x1, y1


def roi_target_np(cw, ch, tw, th, keep_aspect):
    """-> (nw, nh, px, py)"""
    nw, nh = tw, th
    if keep_aspect:
        if cw * th >= ch * tw:
            nh = max(1, (ch * tw + cw // 2) // cw)
        else:
            nw = max(1, (cw * th + ch // 2) // ch)
    return nw, nh, (tw - nw) // 2, (th - nh) // 2


def roi_axis_np(n_in, n_out):
    """-> (i0, i1, f) of every output sample"""
    i = np.arange(n_out, dtype=np.int64)
    pos = ((2 * i + 1) * n_in * 256) // (2 * n_out) - 128
    pos = np.clip(pos, 0, (n_in - 1) * 256)
    i0 = pos >> 8
    return i0, np.minimum(i0 + 1, n_in - 1), pos & 255


def roi_resize_np(crop, nw, nh):
    """uint8 [ch][cw][3] -> int8 [nh][nw][3]"""
    ch, cw = crop.shape[:2]
    i0, i1, fx = roi_axis_np(cw, nw)
    j0, j1, fy = roi_axis_np(ch, nh)
    p = crop.astype(np.int64)
    fx, fy = fx[None, :, None], fy[:, None, None]
    top = p[j0][:, i0] * (256 - fx) + p[j0][:, i1] * fx
    bot = p[j1][:, i0] * (256 - fx) + p[j1][:, i1] * fx
    v = (top * (256 - fy) + bot * fy + 32768) >> 16
    assert v.min() >= 0 and v.max() <= 255
    return (v - 128).astype(np.int8)


def roi_crop_np(rgb, rect, tw, th, nhwc=True, keep_aspect=False):
    """uint8 RGB frame [H][W][3] + rectangle (None: skipped) -> the int8 bytes of one destination frame"""
    out = np.full((th, tw, 3), -17, dtype=np.int8)
    if rect is not None:
        x0, y0, x1, y1 = rect
        nw, nh, px, py = roi_target_np(x1 - x0, y1 - y0, tw, th, keep_aspect)
        out[py:py + nh, px:px + nw] = roi_resize_np(rgb[y0:y1, x0:x1], nw, nh)
    return (out if nhwc else out.transpose(2, 0, 1)).reshape(-1).copy()


def roi_select_np(dets, W, H, slots, expand=0.0, min_conf=0.0, min_size=0, classes=None, max_per_frame=0):
    """dets: one record array per frame, in the tail's order -> ([(frame, det, x0, y0, x1, y1)] of the kept boxes, dropped)"""
    kept = []
    for f, d in enumerate(dets):
        n = 0
        for i in range(len(d)):
            if not F(d[i]["conf"]) >= F(min_conf):
                continue
            if classes is not None and classes[1] and not classes[0] <= int(d[i]["cls"]) < classes[0] + classes[1]:
                continue
            r = roi_rect_np(d[i], W, H, expand, min_size)
            if r is None or (max_per_frame and n >= max_per_frame):
                continue
            n += 1
            kept.append((f, i) + r)
    return kept[:slots], max(len(kept) - slots, 0)


def nv12_to_rgb_np(buf, w, h, flags):
    """"NV12 camera frames" of the header: Y plane [h][w], chroma plane [h/2][w/2][2] behind it, nearest chroma, integer BT.601"""
    buf = np.asarray(buf, dtype=np.uint8).reshape(-1)
    assert buf.size == w * h * 3 // 2 and w % 2 == 0 and h % 2 == 0
    y = buf[:w * h].reshape(h, w).astype(np.int32)
    c = buf[w * h:].reshape(h // 2, w // 2, 2).astype(np.int32)
    u, v = (c[..., 1], c[..., 0]) if flags & 2 else (c[..., 0], c[..., 1])
    d = np.repeat(np.repeat(u - 128, 2, axis=0), 2, axis=1)
    e = np.repeat(np.repeat(v - 128, 2, axis=0), 2, axis=1)
    if flags & 1:
        r, g, b = (256 * y + 359 * e + 128) >> 8, (256 * y - 88 * d - 183 * e + 128) >> 8, (256 * y + 454 * d + 128) >> 8
    else:
        cc = y - 16
        r, g, b = (298 * cc + 409 * e + 128) >> 8, (298 * cc - 100 * d - 208 * e + 128) >> 8, (298 * cc + 516 * d + 128) >> 8
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


def box(x, y, w, h, conf=0.9, cls=0):
    """one mars_det_t record (the layout restated, so that the helper needs no library)"""
    b = np.zeros((), dtype=np.dtype([("x", "<f4"), ("y", "<f4"), ("w", "<f4"), ("h", "<f4"), ("conf", "<f4"), ("cls", "<i4")]))
    b["x"], b["y"], b["w"], b["h"], b["conf"], b["cls"] = x, y, w, h, conf, cls
    return b


# ---- exports and refusals -------------------------------------------------------------------------------------------------------------
def test_roi_symbols_are_exported(marsrt):
    L = marsrt.lib()
    for n in NEW:
        assert n in marsrt.EXPORTS["mars_hip.h"], n
        assert hasattr(L, n), n
    assert marsrt.ROI_KEEP_ASPECT == 1
    assert callable(marsrt.crop_boxes) and callable(marsrt.Model.crop_detections) and callable(marsrt.Model.roi_results)


def test_roi_record_sizes(marsrt, tmp_path):
    import os
    import subprocess
    assert marsrt.ROI_DTYPE.itemsize == 24
    assert [f[0] for f in marsrt.RoiOpts._fields_] == ["src_w", "src_h", "src_format", "src_flags", "expand", "min_conf", "min_size", "cls_first",
                                                       "cls_count", "max_per_frame", "flags"]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "roi_abi.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mars_hip.h"\n'
                   'int main(void){ printf("%zu %zu %zu %zu %u", sizeof(mars_roi_t), sizeof(mars_hip_roi_opts_t), offsetof(mars_roi_t, x0),\n'
                   ' offsetof(mars_hip_roi_opts_t, flags), MARS_ROI_KEEP_ASPECT); return 0; }\n')
    exe = tmp_path / "roi_abi"
    subprocess.run(["gcc", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)], check=True)
    got = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert got == ["24", str(C.sizeof(marsrt.RoiOpts)), "8", str(marsrt.RoiOpts.flags.offset), "1"]


def test_roi_bad_arguments_are_refused_up_front(marsrt):
    L = marsrt.lib()
    BAD_FILE, BAD_TENSOR = marsrt.MARS_ERR_INVALID_FILE, marsrt.MARS_ERR_INVALID_TENSOR
    frames = np.zeros(6 * 4 * 3 + 64, dtype=np.uint8)
    boxes = np.zeros(2, dtype=marsrt.DET_DTYPE)
    boxes["x"], boxes["y"], boxes["w"], boxes["h"] = 3, 2, 4, 3
    fo = np.zeros(2, dtype=np.int32)
    out = np.full(2 * 8 * 8 * 3, 77, dtype=np.int8)
    rois = np.full(2, 77, dtype=marsrt.ROI_DTYPE)

    def crop(o, n_frames=1, n_boxes=2, tw=8, th=8, fr=frames, bx=boxes):
        return L.mars_yolo_crop_boxes(None if fr is None else fr.ctypes.data, n_frames, None if bx is None else bx.ctypes.data, fo.ctypes.data, n_boxes,
                                      None if o is None else C.byref(o), tw, th, 1, out.ctypes.data, rois.ctypes.data)

    good = marsrt.roi_opts(6, 4)
    bad = [marsrt.roi_opts(0, 4), marsrt.roi_opts(6, -4),                                   # non-positive sizes
           marsrt.roi_opts(6, 4, fmt=2), marsrt.roi_opts(6, 4, fmt=-1),                     # an unknown format
           marsrt.roi_opts(6, 4, src_flags=1),                                              # an NV12 flag on RGB frames
           marsrt.roi_opts(6, 4, fmt=marsrt.CAMERA_NV12, src_flags=4),                      # an unknown NV12 flag bit
           marsrt.roi_opts(5, 4, fmt=marsrt.CAMERA_NV12), marsrt.roi_opts(6, 3, fmt=marsrt.CAMERA_NV12),  # odd NV12 sizes
           marsrt.roi_opts(6, 4, expand=-1.0), marsrt.roi_opts(6, 4, expand=float("nan")), marsrt.roi_opts(6, 4, min_size=-1),
           marsrt.roi_opts(6, 4, max_per_frame=-1), marsrt.roi_opts(6, 4, classes=(0, -1))]
    o = marsrt.roi_opts(6, 4)
    o.flags = 2                                                                             # an unknown ROI flag bit
    bad.append(o)
    P = C.POINTER(marsrt.MarsModel)
    a, b = marsrt.MarsModel(), marsrt.MarsModel()  # never looked into: the refusals come first
    for o in bad:
        assert crop(o) == BAD_FILE
        for f in (L.mars_hip_crop_detections_device, L.mars_hip_crop_detections):
            assert f(C.pointer(a), frames.ctypes.data, C.pointer(b), 0, C.byref(o)) == BAD_FILE
    assert crop(None) == BAD_FILE
    for kw in (dict(tw=0), dict(th=-8), dict(n_frames=0), dict(n_boxes=0), dict(fr=None), dict(bx=None)):
        assert crop(good, **kw) == BAD_FILE, kw
    assert (out == 77).all() and rois.tobytes() == np.full(2, 77, dtype=marsrt.ROI_DTYPE).tobytes()  # nothing was written
    for f in (L.mars_hip_crop_detections_device, L.mars_hip_crop_detections):
        assert f(P(), frames.ctypes.data, C.pointer(b), 0, C.byref(good)) == BAD_FILE       # no model
        assert f(C.pointer(a), None, C.pointer(b), 0, C.byref(good)) == BAD_FILE            # no frames
        assert f(C.pointer(a), frames.ctypes.data, C.pointer(b), 0, None) == BAD_FILE       # no options
        assert f(C.pointer(a), frames.ctypes.data, C.pointer(a), 0, C.byref(good)) == BAD_TENSOR  # det_model == dst_model
    assert L.mars_hip_roi_results(P(), None, 0, None, None) == BAD_FILE


# ---- the restatement itself -----------------------------------------------------------------------------------------------------------
def _image(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(h, w, 3), dtype=np.uint8)


def test_restated_rectangle():
    assert roi_rect_np(box(10.5, 20, 4, 6), 98, 62) == (8, 17, 13, 23)
    assert roi_rect_np(box(10, 20, 4, 6), 98, 62) == (8, 17, 12, 23)
    assert roi_rect_np(box(10.5, 20, 1, 6), 98, 62) is None and roi_rect_np(box(10.5, 20, 1, 6), 98, 62, min_size=1) == (10, 17, 11, 23)
    assert roi_rect_np(box(1, 1, 10, 10), 98, 62) == (0, 0, 6, 6)          # over the top left corner
    assert roi_rect_np(box(97, 61, 10, 10), 98, 62) == (92, 56, 98, 62)     # over the bottom right corner
    assert roi_rect_np(box(49, 31, 98, 62), 98, 62) == (0, 0, 98, 62)       # the whole frame
    assert roi_rect_np(box(49, 31, 98, 62), 98, 62, expand=1.25) == (0, 0, 98, 62)
    assert roi_rect_np(box(40, 30, 8, 8), 98, 62, expand=1.25) == (35, 25, 45, 35)
    for b in (box(200, 31, 10, 10), box(-50, 31, 10, 10), box(49, 1e30, 10, 10), box(-1e30, 31, 10, 10)):  # outside
        assert roi_rect_np(b, 98, 62) is None
    for b in (box(float("nan"), 31, 10, 10), box(49, 31, 0, 10), box(49, 31, 10, -1), box(49, 31, float("inf"), 10),
              box(49, 31, 10, 10, conf=float("nan"))):
        assert roi_rect_np(b, 98, 62) is None


def test_restated_identity_crop_returns_the_source():
    img = _image(62, 98, 1)
    for rect in [(0, 0, 98, 62), (7, 5, 40, 22), (97, 61, 98, 62)]:
        x0, y0, x1, y1 = rect
        want = (img[y0:y1, x0:x1].astype(np.int16) - 128).astype(np.int8)
        assert np.array_equal(roi_crop_np(img, rect, x1 - x0, y1 - y0).reshape(y1 - y0, x1 - x0, 3), want)
        assert np.array_equal(roi_crop_np(img, rect, x1 - x0, y1 - y0, nhwc=False).reshape(3, y1 - y0, x1 - x0), want.transpose(2, 0, 1))


def test_restated_constant_image_stays_constant():
    for v in (0, 1, 127, 200, 255):
        img = np.full((40, 50, 3), v, dtype=np.uint8)
        for tw, th in [(16, 16), (33, 17), (160, 160), (350, 7)]:
            got = roi_crop_np(img, (3, 4, 45, 37), tw, th)
            assert (got == np.int8(v - 128)).all(), (v, tw, th)


def test_restated_axis_by_hand():
    # 2 -> 4: centres at 0.25, 0.75, 1.25, 1.75 source pixels minus the half pixel: -0.25 (clamped), 0.25, 0.75, 1.25 (clamped)
    i0, i1, f = roi_axis_np(2, 4)
    assert i0.tolist() == [0, 0, 0, 1] and i1.tolist() == [1, 1, 1, 1] and f.tolist() == [0, 64, 192, 0]
    # 4 -> 2: 0.5 and 2.5
    i0, i1, f = roi_axis_np(4, 2)
    assert i0.tolist() == [0, 2] and i1.tolist() == [1, 3] and f.tolist() == [128, 128]
    # 5 -> 1: the middle pixel
    i0, i1, f = roi_axis_np(5, 1)
    assert (i0.tolist(), i1.tolist(), f.tolist()) == ([2], [3], [0])
    row = np.array([[[0, 0, 0], [100, 100, 100], [200, 200, 200], [255, 255, 255]]], dtype=np.uint8)
    assert roi_resize_np(row, 2, 1)[0, :, 0].tolist() == [50 - 128, 228 - 128]  # 50.0 and 227.5, rounded half up


def test_restated_keep_aspect_geometry_by_hand():
    assert roi_target_np(40, 20, 160, 160, False) == (160, 160, 0, 0)
    assert roi_target_np(40, 20, 160, 160, True) == (160, 80, 0, 40)        # wide box: full width, bands above and below
    assert roi_target_np(20, 40, 160, 160, True) == (80, 160, 40, 0)        # tall box
    assert roi_target_np(30, 30, 33, 17, True) == (17, 17, 8, 0)            # 30 * 17 < 30 * 33: height-bound
    assert roi_target_np(100, 7, 33, 17, True) == (33, 2, 0, 7)             # (7 * 33 + 50) / 100 = 2
    assert roi_target_np(1000, 2, 16, 16, True) == (16, 1, 0, 7)            # (2 * 16 + 500) / 1000 = 0 -> 1
    assert roi_target_np(2, 1000, 16, 16, True) == (1, 16, 7, 0)
    assert roi_target_np(3, 2, 16, 16, True) == (16, 11, 0, 2)              # (2 * 16 + 1) / 3 = 11
    img = _image(30, 120, 2)
    out = roi_crop_np(img, (10, 4, 110, 11), 33, 17, keep_aspect=True).reshape(17, 33, 3)
    assert (out[:7] == -17).all() and (out[9:] == -17).all() and not (out[7:9] == -17).all()


def test_restated_selection():
    d0 = np.array([box(20, 20, 10, 10, 0.9, 1), box(30, 30, 10, 10, 0.8, 2), box(300, 30, 10, 10, 0.7, 1), box(40, 30, 10, 10, 0.2, 1)])
    d1 = np.zeros(0, dtype=d0.dtype)
    d2 = np.array([box(50, 20, 10, 10, 0.6, 3), box(60, 20, 10, 10, 0.5, 1)])
    k, dropped = roi_select_np([d0, d1, d2], 98, 62, 8)
    assert [(f, i) for f, i, *_ in k] == [(0, 0), (0, 1), (0, 3), (2, 0), (2, 1)] and dropped == 0
    k, dropped = roi_select_np([d0, d1, d2], 98, 62, 3)
    assert [(f, i) for f, i, *_ in k] == [(0, 0), (0, 1), (0, 3)] and dropped == 2
    k, dropped = roi_select_np([d0, d1, d2], 98, 62, 8, min_conf=0.5, classes=(1, 1))
    assert [(f, i) for f, i, *_ in k] == [(0, 0), (2, 1)] and dropped == 0
    k, dropped = roi_select_np([d0, d1, d2], 98, 62, 8, max_per_frame=1)
    assert [(f, i) for f, i, *_ in k] == [(0, 0), (2, 0)]
