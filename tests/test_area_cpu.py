"""Area averaging (include/mars_hip.h, "Area averaging" inside "ROI crops"), the part that needs no GPU: the two flag values, what the calls
refuse and what they no longer refuse, and the numpy restatement of tests/arearef.py -- the one tests/test_gpu_area.py compares the device
against -- on cases worked by hand."""
import ctypes as C
import os
import subprocess

import numpy as np

from arearef import area_axis_np, area_resize_np
from test_roi_cpu import roi_resize_np


# ---- constants ------------------------------------------------------------------------------------------------------------------------
def test_area_flag_values_and_record_sizes(marsrt, tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "area_abi.c"
    src.write_text('#include <stdio.h>\n#include "mars_hip.h"\n'
                   'int main(void){ printf("%u %u %zu %zu", MARS_ROI_AREA, MARS_TILE_AREA, sizeof(mars_hip_roi_opts_t), sizeof(mars_hip_tile_opts_t));\n'
                   ' return 0; }\n')
    exe = tmp_path / "area_abi"
    subprocess.run(["gcc", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)], check=True)
    got = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert got == ["4", "16", "44", "48"]  # the option structs are what they were
    assert marsrt.ROI_AREA == 4 and marsrt.TILE_AREA == 16
    assert C.sizeof(marsrt.RoiOpts) == 44 and C.sizeof(marsrt.TileOpts) == 48
    assert marsrt.roi_opts(6, 4, area=True).flags == 4 and marsrt.roi_opts(6, 4, area=True, keep_aspect=True).flags == 5
    assert marsrt.roi_opts(6, 4).flags == 0
    t = [(0, 0, 6, 4)]
    assert marsrt.tile_opts(6, 4, t, area=True).flags == 16 and marsrt.tile_opts(6, 4, t, area=True, keep_aspect=True, agnostic=True).flags == 21
    assert marsrt.tile_opts(6, 4, t).flags == 0


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_area_flag_is_accepted_by_the_upright_calls_and_unknown_bits_stay_refused(marsrt):
    L = marsrt.lib()
    BAD_FILE = marsrt.MARS_ERR_INVALID_FILE
    ACCEPTED = (marsrt.MARS_OK, marsrt.MARS_ERR_NNA_INIT_FAILED)  # with and without a device
    frames = np.zeros(12 * 8 * 3 + 64, dtype=np.uint8)
    boxes = np.zeros(2, dtype=marsrt.DET_DTYPE)
    boxes["x"], boxes["y"], boxes["w"], boxes["h"] = 6, 4, 10, 7
    fo = np.zeros(2, dtype=np.int32)
    out = np.full(2 * 4 * 4 * 3, 77, dtype=np.int8)

    def crop(o):
        return L.mars_yolo_crop_boxes(frames.ctypes.data, 1, boxes.ctypes.data, fo.ctypes.data, 2, C.byref(o), 4, 4, 1, out.ctypes.data, None)

    def tile(o):
        return L.mars_yolo_tile_frames(frames.ctypes.data, 1, C.byref(o), 4, 4, 1, out.ctypes.data)

    for keep in (False, True):
        assert crop(marsrt.roi_opts(12, 8, area=True, keep_aspect=keep)) in ACCEPTED
        assert crop(marsrt.roi_opts(12, 8, fmt=marsrt.CAMERA_NV12, src_flags=3, area=True, keep_aspect=keep)) in ACCEPTED
        assert tile(marsrt.tile_opts(12, 8, [(0, 0, 12, 8), (2, 0, 12, 8)], area=True, keep_aspect=keep)) in ACCEPTED
    assert tile(marsrt.tile_opts(12, 8, [(0, 0, 12, 8)], fmt=marsrt.CAMERA_NV12, area=True, ios=True)) in ACCEPTED
    # the flag does not narrow the limits: up to frames 3840 wide and targets 1280 wide it passes wherever the unflagged call does
    # (frames two rows high, one box; the bilinear kernel's own buffers refuse the widest pairs)
    wide = np.zeros(3840 * 2 * 3, dtype=np.uint8)
    big = np.zeros(1280 * 2 * 3, dtype=np.int8)
    passed = 0
    for fmt in (marsrt.CAMERA_RGB, marsrt.CAMERA_NV12):
        for w in (500, 1920, 3840):
            for tw in (160, 640, 1000, 1280):
                rc = [L.mars_yolo_crop_boxes(wide.ctypes.data, 1, boxes.ctypes.data, fo.ctypes.data, 1, C.byref(marsrt.roi_opts(w, 2, fmt=fmt, area=a)),
                                             tw, 2, 1, big.ctypes.data, None) for a in (False, True)]
                assert rc[0] in ACCEPTED + (BAD_FILE,) and (rc[1] in ACCEPTED) == (rc[0] in ACCEPTED), (fmt, w, tw, rc)
                passed += rc[1] in ACCEPTED
    assert passed >= 2 * 10  # 3840 -> 1000 and 500 -> 1280 among them
    out[:] = 77
    for bits in (2, 8, 4 | 8, 4 | 2, 32):
        o = marsrt.roi_opts(12, 8)
        o.flags = bits
        assert crop(o) == BAD_FILE, bits
    for bits in (8, 32, 16 | 8, 16 | 32):
        o = marsrt.tile_opts(12, 8, [(0, 0, 12, 8)], flags=bits)
        assert tile(o) == BAD_FILE, bits
    assert (out == 77).all()
    # the merge accepts the bit (and ignores it): the argument checks pass
    dets = np.zeros((1, 4), dtype=marsrt.DET_DTYPE)
    counts = np.zeros(1, dtype=np.int32)
    mo, mc = np.zeros(1000, dtype=marsrt.DET_DTYPE), np.zeros(1, dtype=np.int32)
    o = marsrt.tile_opts(12, 8, [(0, 0, 12, 8)], area=True)
    assert L.mars_yolo_merge_tiles(dets.ctypes.data, counts.ctypes.data, 1, 4, C.byref(o), 4, 4, mo.ctypes.data, mc.ctypes.data, None, None) in ACCEPTED


def test_rotated_calls_refuse_the_area_flag(marsrt):
    L = marsrt.lib()
    BAD_FILE = marsrt.MARS_ERR_INVALID_FILE
    frames = np.zeros(12 * 8 * 3 + 64, dtype=np.uint8)
    boxes = np.zeros(2, dtype=marsrt.OBB_DTYPE)
    boxes["x"], boxes["y"], boxes["w"], boxes["h"], boxes["angle"] = 6, 4, 10, 7, 0.5
    fo = np.zeros(2, dtype=np.int32)
    out = np.full(2 * 4 * 4 * 3, 77, dtype=np.int8)
    rois = np.full(2, 77, dtype=marsrt.ROI_DTYPE)
    a, b = marsrt.MarsModel(), marsrt.MarsModel()  # never looked into: the refusal comes first
    for keep in (False, True):
        o = marsrt.roi_opts(12, 8, area=True, keep_aspect=keep)
        assert L.mars_yolo_crop_obb(frames.ctypes.data, 1, boxes.ctypes.data, fo.ctypes.data, 2, C.byref(o), 4, 4, 1, out.ctypes.data,
                                    rois.ctypes.data) == BAD_FILE
        for f in (L.mars_hip_crop_obb_device, L.mars_hip_crop_obb):
            assert f(C.pointer(a), frames.ctypes.data, C.pointer(b), 0, C.byref(o)) == BAD_FILE
    assert (out == 77).all() and rois.tobytes() == np.full(2, 77, dtype=marsrt.ROI_DTYPE).tobytes()  # nothing was written


# ---- the restatement, by hand ---------------------------------------------------------------------------------------------------------
def _image(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(h, w, 3), dtype=np.uint8)


def test_restated_weights_7_to_3():
    D, W = area_axis_np(7, 3, True)
    assert D == 7
    assert W.tolist() == [[3, 3, 1, 0, 0, 0, 0], [0, 0, 2, 3, 2, 0, 0], [0, 0, 0, 0, 1, 3, 3]]
    # the flag clear, or nothing to average: the bilinear taps, D = 256
    D, W = area_axis_np(7, 3, False)
    assert D == 256 and (W.sum(axis=1) == 256).all() and ((W != 0).sum(axis=1) <= 2).all()
    D, W = area_axis_np(3, 3, True)
    assert D == 256 and W.tolist() == [[256, 0, 0], [0, 256, 0], [0, 0, 256]]
    D, W = area_axis_np(2, 4, True)  # pos = 0, 0.25, 0.75, 1 (clamped)
    assert D == 256 and W.tolist() == [[256, 0], [192, 64], [64, 192], [0, 256]]


def test_restated_tap_counts_and_sums():
    for (n_in, n_out), most in [((7, 3), 3), ((1280, 160), 8), ((1081, 360), 4), ((5, 4), 2)]:
        D, W = area_axis_np(n_in, n_out, True)
        assert D == n_in and (W >= 0).all() and (W.sum(axis=1) == n_in).all()
        taps = (W != 0).sum(axis=1)
        assert taps.max() == most and most <= (n_in + n_out - 1) // n_out + 1
        # the taps of one output are a run from (i * n_in) / n_out to ((i + 1) * n_in + n_out - 1) / n_out - 1
        for i in (0, n_out // 2, n_out - 1):
            nz = np.flatnonzero(W[i])
            assert nz[0] == (i * n_in) // n_out and nz[-1] == ((i + 1) * n_in + n_out - 1) // n_out - 1 and len(nz) == nz[-1] - nz[0] + 1
        assert (W.sum(axis=0) == n_out).all()  # every source sample is used exactly once in all


def test_restated_a_source_sample_feeds_one_or_two_outputs():
    for n_in, n_out in [(7, 3), (5, 4), (100, 99), (9, 4)]:
        _, W = area_axis_np(n_in, n_out, True)
        feeds = (W != 0).sum(axis=0)
        assert feeds.min() >= 1 and feeds.max() <= 2, (n_in, n_out)


def test_restated_integer_ratio_is_the_rounded_block_mean():
    img = _image(6, 9, 1)
    got = area_resize_np(img, 3, 2)
    blocks = img.astype(np.int64).reshape(2, 3, 3, 3, 3).sum(axis=(1, 3))  # [2][3][channel]: sums of 3 x 3 blocks
    assert np.array_equal(got, ((blocks + 4) // 9 - 128).astype(np.int8))
    assert got.shape == (2, 3, 3) and got.dtype == np.int8


def test_restated_constant_crop_stays_constant():
    for (cw, ch), (nw, nh) in [((7, 5), (3, 2)), ((9, 3), (4, 8)), ((4, 9), (8, 4)), ((64, 64), (1, 1)), ((5, 5), (4, 4)), ((17, 3), (16, 3))]:
        got = area_resize_np(np.full((ch, cw, 3), 200, dtype=np.uint8), nw, nh)
        assert got.shape == (nh, nw, 3) and (got == 72).all(), (cw, ch, nw, nh)


def test_restated_nothing_to_average_is_the_bilinear_resize():
    for k, ((cw, ch), (nw, nh)) in enumerate([((3, 4), (3, 4)), ((3, 4), (7, 9)), ((5, 2), (5, 8)), ((1, 1), (4, 4))]):
        img = _image(ch, cw, 10 + k)
        assert np.array_equal(area_resize_np(img, nw, nh), roi_resize_np(img, nw, nh)), (cw, ch, nw, nh)
    # ... and so is every size with the flag clear
    img = _image(9, 14, 20)
    assert np.array_equal(area_resize_np(img, 4, 3, area=False), roi_resize_np(img, 4, 3))
    assert not np.array_equal(area_resize_np(img, 4, 3), roi_resize_np(img, 4, 3))


def test_restated_mixed_axes_by_hand():
    """7 x 2 -> 3 x 4: x is averaged with the 7 -> 3 weights, y interpolates 2 -> 4 (fy = 0, 64, 192, 0 of rows (0, 0), (0, 1), (0, 1), (1, 1))"""
    img = _image(2, 7, 30)
    p = img.astype(np.int64)
    wx = [(0, (3, 3, 1)), (2, (2, 3, 2)), (4, (1, 3, 3))]
    wy = [(256, 0), (192, 64), (64, 192), (0, 256)]
    want = np.zeros((4, 3, 3), dtype=np.int64)
    for j, (a, b) in enumerate(wy):
        for i, (s, w) in enumerate(wx):
            for c in range(3):
                S = sum(wy_ * sum(w[t] * p[row, s + t, c] for t in range(3)) for row, wy_ in ((0, a), (1, b)))
                want[j, i, c] = (S + (7 * 256) // 2) // (7 * 256)
    assert np.array_equal(area_resize_np(img, 3, 4), (want - 128).astype(np.int8))
