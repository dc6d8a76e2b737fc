"""Rotated crops (include/mars_hip.h, "Rotated crops"), the part that needs no GPU: the new entry points are exported, the records and the
options keep their layout, arguments that can never be valid are refused before any device work, and the numpy restatement that
tests/test_gpu_rot.py compares the device against (tests/rotref.py) is itself checked on cases worked out by hand."""
import ctypes as C

import numpy as np

import rotref
from rotref import obb, rot_crop_np, rot_geom_np, rot_rect_np, rot_sample_np, rot_select_np, rot_sides_np

F = np.float32
NEW = ["mars_yolo_crop_obb", "mars_hip_crop_obb_device", "mars_hip_crop_obb"]
HALF_PI = float(F(np.pi / 2))


def _image(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(h, w, 3), dtype=np.uint8)


# ---- exports, layouts, refusals ---------------------------------------------------------------------------------------------------------
def test_rot_symbols_are_exported(marsrt):
    L = marsrt.lib()
    for n in NEW:
        assert n in marsrt.EXPORTS["mars_hip.h"], n
        assert hasattr(L, n), n
    assert callable(marsrt.crop_obb) and callable(marsrt.Model.crop_obb_detections) and callable(marsrt.Model.crop_obb_detections_device)


def test_rot_record_sizes_are_unchanged(marsrt, tmp_path):
    import os
    import subprocess
    assert marsrt.ROI_DTYPE.itemsize == 24 and marsrt.OBB_DTYPE.itemsize == 32
    assert [f[0] for f in marsrt.RoiOpts._fields_] == ["src_w", "src_h", "src_format", "src_flags", "expand", "min_conf", "min_size", "cls_first",
                                                       "cls_count", "max_per_frame", "flags"]
    assert C.sizeof(marsrt.RoiOpts) == 44
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    inc = os.path.join(root, "include")
    src = tmp_path / "rot_abi.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mars_hip.h"\n'
                   'int main(void){ printf("%zu %zu %zu %zu %zu", sizeof(mars_roi_t), sizeof(mars_hip_roi_opts_t), offsetof(mars_hip_roi_opts_t, flags),\n'
                   ' sizeof(mars_obb_t), offsetof(mars_obb_t, angle)); return 0; }\n')
    exe = tmp_path / "rot_abi"
    subprocess.run(["gcc", "-I", inc, str(src), "-o", str(exe)], check=True)
    got = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    # the declared prototypes, compiled only: an assignment to a pointer of the stated type does not compile against another declaration
    proto = tmp_path / "rot_proto.c"
    proto.write_text('#include "mars_hip.h"\n'
                     'mars_error_t (*a)(const unsigned char *, int, const mars_obb_t *, const int *, int, const mars_hip_roi_opts_t *, int, int, int,\n'
                     ' signed char *, mars_roi_t *) = mars_yolo_crop_obb;\n'
                     'mars_error_t (*b)(mars_model_t *, const void *, mars_model_t *, int, const mars_hip_roi_opts_t *) = mars_hip_crop_obb_device;\n'
                     'mars_error_t (*c)(mars_model_t *, const unsigned char *, mars_model_t *, int, const mars_hip_roi_opts_t *) = mars_hip_crop_obb;\n')
    subprocess.run(["gcc", "-Werror", "-I", inc, "-c", str(proto), "-o", str(tmp_path / "rot_proto.o")], check=True)
    assert got == ["24", "44", "40", "32", "24"]


def test_rot_bad_arguments_are_refused_up_front(marsrt):
    L = marsrt.lib()
    BAD_FILE, BAD_TENSOR = marsrt.MARS_ERR_INVALID_FILE, marsrt.MARS_ERR_INVALID_TENSOR
    frames = np.zeros(6 * 4 * 3 + 64, dtype=np.uint8)
    boxes = np.zeros(2, dtype=marsrt.OBB_DTYPE)
    boxes["x"], boxes["y"], boxes["w"], boxes["h"], boxes["angle"] = 3, 2, 4, 3, 0.5
    fo = np.zeros(2, dtype=np.int32)
    out = np.full(2 * 8 * 8 * 3, 77, dtype=np.int8)
    rois = np.full(2, 77, dtype=marsrt.ROI_DTYPE)

    def crop(o, n_frames=1, n_boxes=2, tw=8, th=8, fr=frames, bx=boxes):
        return L.mars_yolo_crop_obb(None if fr is None else fr.ctypes.data, n_frames, None if bx is None else bx.ctypes.data, fo.ctypes.data, n_boxes,
                                    None if o is None else C.byref(o), tw, th, 1, out.ctypes.data, rois.ctypes.data)

    good = marsrt.roi_opts(6, 4)
    bad = [marsrt.roi_opts(0, 4), marsrt.roi_opts(6, -4),                                   # non-positive sizes
           marsrt.roi_opts(6, 4, fmt=2), marsrt.roi_opts(6, 4, fmt=-1),                     # an unknown format
           marsrt.roi_opts(6, 4, src_flags=1),                                              # an NV12 flag on RGB frames
           marsrt.roi_opts(6, 4, fmt=marsrt.CAMERA_NV12, src_flags=4),                      # an unknown NV12 flag bit
           marsrt.roi_opts(5, 4, fmt=marsrt.CAMERA_NV12), marsrt.roi_opts(6, 3, fmt=marsrt.CAMERA_NV12),  # odd NV12 sizes
           marsrt.roi_opts(6, 4, expand=-1.0), marsrt.roi_opts(6, 4, expand=float("nan")), marsrt.roi_opts(6, 4, min_size=-1),
           marsrt.roi_opts(6, 4, max_per_frame=-1), marsrt.roi_opts(6, 4, classes=(0, -1)),
           marsrt.roi_opts(6, 32768)]                                                       # positions would leave the Q16 integers
    o = marsrt.roi_opts(6, 4)
    o.flags = 2                                                                             # an unknown ROI flag bit
    bad.append(o)
    P = C.POINTER(marsrt.MarsModel)
    a, b = marsrt.MarsModel(), marsrt.MarsModel()  # never looked into: the refusals come first
    for o in bad:
        assert crop(o) == BAD_FILE
        for f in (L.mars_hip_crop_obb_device, L.mars_hip_crop_obb):
            assert f(C.pointer(a), frames.ctypes.data, C.pointer(b), 0, C.byref(o)) == BAD_FILE
    assert crop(None) == BAD_FILE
    for kw in (dict(tw=0), dict(th=-8), dict(n_frames=0), dict(n_boxes=0), dict(n_boxes=65536), dict(fr=None), dict(bx=None)):
        assert crop(good, **kw) == BAD_FILE, kw
    assert (out == 77).all() and rois.tobytes() == np.full(2, 77, dtype=marsrt.ROI_DTYPE).tobytes()  # nothing was written
    for f in (L.mars_hip_crop_obb_device, L.mars_hip_crop_obb):
        assert f(P(), frames.ctypes.data, C.pointer(b), 0, C.byref(good)) == BAD_FILE       # no model
        assert f(C.pointer(a), None, C.pointer(b), 0, C.byref(good)) == BAD_FILE            # no frames
        assert f(C.pointer(a), frames.ctypes.data, C.pointer(b), 0, None) == BAD_FILE       # no options
        assert f(C.pointer(a), frames.ctypes.data, C.pointer(a), 0, C.byref(good)) == BAD_TENSOR  # det_model == dst_model


# ---- the restatement itself -----------------------------------------------------------------------------------------------------------
def test_restated_angle_zero_is_an_exact_copy():
    """nw == we, we and x - we / 2 integers: Ux = Vy = 32768, Uy = Vx = 0, no fraction anywhere"""
    img = _image(62, 98, 1)
    for x0, y0, w, h in [(7, 5, 33, 17), (0, 0, 98, 62), (40, 30, 2, 2), (96, 60, 2, 2)]:
        b = obb(x0 + w / 2, y0 + h / 2, w, h, 0.0)
        we, he = rot_sides_np(b, 98, 62)
        g = rot_geom_np(b, we, he, F(1), F(0), w, h)
        assert (g["Ux"], g["Uy"], g["Vx"], g["Vy"]) == (32768, 0, 0, 32768)
        want = (img[y0:y0 + h, x0:x0 + w].astype(np.int16) - 128).astype(np.int8)
        got, outside = rot_sample_np(img, g)
        # fx = fy = 0: the right / lower taps carry no weight, inside or not.  A crop that ends at the frame's right and lower edge has the right
        # taps of its last column (h), the lower taps of its last row (w) and the diagonal taps of both (h + w - 1) outside
        assert np.array_equal(got, want) and outside == (2 * (h + w) - 1 if (x0 + w, y0 + h) == (98, 62) else 0)
        assert np.array_equal(rot_crop_np(img, b, w, h).reshape(h, w, 3), want)
        assert np.array_equal(rot_crop_np(img, b, w, h, nhwc=False).reshape(3, h, w), want.transpose(2, 0, 1))
        assert rot_rect_np(b, 98, 62) == (x0, y0, x0 + w, y0 + h)


def test_restated_quarter_turn_is_an_exact_transpose():
    """cs, sn of (float)(pi / 2): cs = -4.4e-8, so Ux and Vy round to 0; column i walks down the frame, row j walks left"""
    img = _image(62, 98, 2)
    cs, sn = rotref.csn_of(obb(0, 0, 1, 1, HALF_PI))
    assert sn == F(1) and cs != 0 and abs(cs) < 1e-7
    w, h = 20, 12  # along the box's own axes: w runs down the frame, h runs across it
    b = obb(40.0, 31.0, w, h, HALF_PI)
    we, he = rot_sides_np(b, 98, 62)
    g = rot_geom_np(b, we, he, cs, sn, w, h)
    assert (g["Ux"], g["Uy"], g["Vx"], g["Vy"]) == (0, 32768, -32768, 0)
    got, outside = rot_sample_np(img, g)
    # out[j][i] = frame[y - w / 2 + i][x + h / 2 - 1 - j]
    want = (img[21:41, 34:46].astype(np.int16) - 128).astype(np.int8)[:, ::-1].transpose(1, 0, 2)
    assert outside == 0 and np.array_equal(got, want)
    assert rot_rect_np(b, 98, 62) == (34, 21, 46, 41)


def test_restated_corner_box_counts_its_grey_taps():
    """an upright 8 x 8 box centred on the frame's corner (0, 0): columns / rows 0 .. 3 of the 8 x 8 crop lie outside"""
    img = np.full((62, 98, 3), 200, dtype=np.uint8)
    b = obb(0.0, 0.0, 8, 8, 0.0)
    we, he = rot_sides_np(b, 98, 62)
    g = rot_geom_np(b, we, he, F(1), F(0), 8, 8)
    assert (g["X0"], g["Ux"]) == (-32768, 32768)  # PX = (i - 4) * 65536: ix = i - 4
    got, outside = rot_sample_np(img, g)
    # per axis: ix = -4 .. 3 and ix + 1 = -3 .. 4; outside: 4 of the left taps, 3 of the right.  A tap is inside when both its axes are
    inside_taps = (4 * 4) + (5 * 4) + (4 * 5) + (5 * 5)
    assert outside == 4 * 64 - inside_taps
    assert (got[4:, 4:] == 200 - 128).all() and (got[:4] == -17).all() and (got[:, :4] == -17).all()
    assert rot_rect_np(b, 98, 62) == (0, 0, 4, 4)
    # 45 degrees over the bottom right corner: some taps grey, some not, and the centre pixel is the frame's
    b = obb(96.0, 60.0, 16, 6, float(F(np.pi / 4)))
    out = rot_crop_np(img, b, 16, 6).reshape(6, 16, 3)
    assert (out == -17).any() and (out == 72).any() and (out[:, :6] == 72).all()


def test_restated_half_pixel_blend_by_hand():
    """a 1 x 1 box at (1.0, 1.0) into one pixel: X0 = Y0 = 32768, a = b = 0: ix = iy = 0, fx = fy = 128: the mean of pixels (0..1, 0..1)"""
    img = np.zeros((4, 4, 3), dtype=np.uint8)
    img[0, 0], img[0, 1], img[1, 0], img[1, 1] = 10, 20, 40, 81
    b = obb(1.0, 1.0, 1, 1, 0.0)
    we, he = rot_sides_np(b, 4, 4, min_size=1)
    g = rot_geom_np(b, we, he, F(1), F(0), 1, 1)
    assert (g["X0"], g["Y0"], g["Ux"], g["Vy"]) == (32768, 32768, 32768, 32768)
    got, outside = rot_sample_np(img, g)
    # top = 10 * 128 + 20 * 128 = 3840, bot = 40 * 128 + 81 * 128 = 15488, v = (3840 * 128 + 15488 * 128 + 32768) >> 16 = 2506752 >> 16 = 38
    assert outside == 0 and got.reshape(3).tolist() == [38 - 128] * 3
    # two columns from a 1-wide box: sx = 0.25, a = -1, +1: PX = 32768 -+ 16384: fx = 64, 192 between columns 0 and 1
    g = rot_geom_np(b, we, he, F(1), F(0), 2, 1)
    got, _ = rot_sample_np(img, g)
    # column 0: top = 10 * 192 + 20 * 64 = 3200, bot = 40 * 192 + 81 * 64 = 12864 -> (3200 * 128 + 12864 * 128 + 32768) >> 16 = 31
    # column 1: top = 10 * 64 + 20 * 192 = 4480, bot = 40 * 64 + 81 * 192 = 18112 -> (4480 * 128 + 18112 * 128 + 32768) >> 16 = 44
    assert got[0, :, 0].tolist() == [31 - 128, 44 - 128]


def test_restated_skip_rule_every_branch():
    W, H = 98, 62
    assert rot_sides_np(obb(49, 31, 10, 10, 0.3), W, H) == (F(10), F(10))
    nan, inf = float("nan"), float("inf")
    for b in (obb(nan, 31, 10, 10, 0), obb(49, inf, 10, 10, 0), obb(49, 31, nan, 10, 0), obb(49, 31, 10, inf, 0), obb(49, 31, 10, 10, nan),
              obb(49, 31, 10, 10, 0, conf=nan), obb(49, 31, 10, 10, -inf)):                # a float field that is not finite
        assert rot_sides_np(b, W, H) is None
    for b in (obb(49, 31, 0, 10, 0), obb(49, 31, 10, -1, 0)):                              # w <= 0, h <= 0
        assert rot_sides_np(b, W, H) is None
    assert rot_sides_np(obb(49, 31, 1.9, 10, 0), W, H) is None and rot_sides_np(obb(49, 31, 10, 1.9, 0), W, H) is None  # below min_size 2
    assert rot_sides_np(obb(49, 31, 2, 2, 0), W, H) == (F(2), F(2))
    assert rot_sides_np(obb(49, 31, 1.9, 10, 0), W, H, min_size=1) is not None and rot_sides_np(obb(49, 31, 1.9, 10, 0), W, H, expand=1.25) is not None
    assert rot_sides_np(obb(49, 31, 23, 23, 0), W, H, min_size=24) is None and rot_sides_np(obb(49, 31, 24, 24, 0), W, H, min_size=24) is not None
    assert rot_sides_np(obb(49, 31, 32768, 10, 0), W, H) is not None                       # the largest side kept
    assert rot_sides_np(obb(49, 31, 32770, 10, 0), W, H) is None and rot_sides_np(obb(49, 31, 10, 30000, 0), W, H, expand=1.25) is None
    assert rot_sides_np(obb(49, 31, 3e38, 10, 0), W, H, expand=2.0) is None                # we overflows to infinity
    for b in (obb(-0.001, 31, 10, 10, 0), obb(98.001, 31, 10, 10, 0), obb(49, -0.001, 10, 10, 0), obb(49, 62.001, 10, 10, 0)):  # the centre
        assert rot_sides_np(b, W, H) is None
    for b in (obb(0, 0, 10, 10, 0), obb(98, 62, 10, 10, 0), obb(0, 62, 10, 10, 1.0)):      # on the frame's edge: kept
        assert rot_sides_np(b, W, H) is not None
    assert rot_rect_np(obb(49, 31, 0, 10, 0), W, H) is None
    assert (rot_crop_np(_image(H, W, 3), obb(49, 70, 10, 10, 0), 8, 8) == -17).all()


def test_restated_keep_aspect_targets():
    img = _image(62, 98, 4)
    for b, tw, th, want in [(obb(49, 31, 40, 20, 0.3), 32, 32, (32, 16, 0, 8)),            # wide: bands above and below
                            (obb(49, 31, 20, 40, 0.3), 32, 32, (16, 32, 8, 0)),            # tall
                            (obb(49, 31, 2, 90, 0.3), 16, 16, (1, 16, 7, 0)),              # (2 * 16 + 45) / 90 = 0 -> nw = 1
                            (obb(49, 31, 20.5, 10.4, 0.3), 40, 24, (40, 20, 0, 2)),        # cw = rint(20.5) = 20 (to even), ch = 10
                            (obb(49, 31, 21.5, 10.5, 0.3), 40, 24, (40, 18, 0, 3))]:       # cw = 22, ch = 10: (10 * 40 + 11) / 22 = 18
        we, he = rot_sides_np(b, 98, 62)
        cs, sn = rotref.csn_of(b)
        g = rot_geom_np(b, we, he, cs, sn, tw, th, keep_aspect=True)
        assert (g["nw"], g["nh"], g["px"], g["py"]) == want, (b, g)
        out = rot_crop_np(img, b, tw, th, keep_aspect=True).reshape(th, tw, 3)
        inner = np.zeros((th, tw), dtype=bool)
        inner[g["py"]:g["py"] + g["nh"], g["px"]:g["px"] + g["nw"]] = True
        assert (out[~inner] == -17).all() and not (out[inner] == -17).all()


def test_restated_selection():
    W, H = 98, 62
    d0 = np.array([obb(20, 20, 10, 10, 0.1, 0.9, 1), obb(30, 30, 10, 10, 0.2, 0.8, 2), obb(300, 30, 10, 10, 0.3, 0.7, 1), obb(40, 30, 10, 10, 0.4, 0.2, 1)])
    d1 = np.zeros(0, dtype=d0.dtype)
    d2 = np.array([obb(50, 20, 10, 10, 0.5, 0.6, 3), obb(60, 20, 10, 10, 0.6, 0.5, 1)])
    k, dropped = rot_select_np([d0, d1, d2], W, H, 8)
    assert [(f, i) for f, i, *_ in k] == [(0, 0), (0, 1), (0, 3), (2, 0), (2, 1)] and dropped == 0
    k, dropped = rot_select_np([d0, d1, d2], W, H, 3)
    assert [(f, i) for f, i, *_ in k] == [(0, 0), (0, 1), (0, 3)] and dropped == 2
    k, dropped = rot_select_np([d0, d1, d2], W, H, 8, min_conf=0.5, classes=(1, 1))
    assert [(f, i) for f, i, *_ in k] == [(0, 0), (2, 1)] and dropped == 0
    k, dropped = rot_select_np([d0, d1, d2], W, H, 8, max_per_frame=1)
    assert [(f, i) for f, i, *_ in k] == [(0, 0), (2, 0)]
