"""Motion maps (include/mars_hip.h, "Motion"), the part that needs no GPU: the numpy restatement tests/test_gpu_motion.py compares the device
against (tests/motionref.py) is pinned on cases worked out by hand, the record sizes are the header's, arguments that can never be valid are
refused up front, and every case the GPU file uses is shown not to be vacuous."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import motionref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mars_hip_motion_create", "mars_hip_motion_reset", "mars_hip_motion_free", "mars_hip_motion_grid", "mars_hip_motion_read",
       "mars_yolo_motion_frames", "mars_hip_motion_device", "mars_hip_motion_results", "mars_hip_motion_detections_device",
       "mars_hip_motion_det_results", "mars_yolo_motion_boxes", "mars_hip_motion_ms"]


def nv12(y):
    """a luma plane [H][W] -> one NV12 frame with grey chroma"""
    y = np.asarray(y, dtype=np.uint8)
    return np.concatenate([y.reshape(-1), np.full(y.size // 2, 128, dtype=np.uint8)])


def const_frames(W, H, levels):
    return np.stack([nv12(np.full((H, W), v)) for v in levels])


# ---- the library's side that needs no device ------------------------------------------------------------------------------------------------
def test_symbols_and_record_sizes(marsrt, tmp_path):
    L = marsrt.lib()
    for n in NEW:
        assert n in marsrt.EXPORTS["mars_hip.h"] and hasattr(L, n), n
    assert marsrt.MOTION_STATS_DTYPE.itemsize == R.STATS.itemsize == 24 and marsrt.MOTION_DET_DTYPE.itemsize == R.DET.itemsize == 8
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "mars_hip.h"\nint main(void){printf("%zu %zu %zu %d", sizeof(mars_motion_stats_t), '
                   'sizeof(mars_motion_det_t), sizeof(mars_hip_motion_opts_t), MARS_MOTION_MAX_ZONES);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert subprocess.check_output([str(exe)]).decode().split() == ["24", "8", str(C.sizeof(marsrt.MotionOpts)), str(R.MAX_ZONES)]


def test_grid_and_refusals_without_a_device(marsrt):
    FILE, TENSOR = marsrt.MARS_ERR_INVALID_FILE, marsrt.MARS_ERR_INVALID_TENSOR
    for W, H in R.RGB_SIZES + [(8192, 8192), (64, 128)]:
        for B in (4, 8, 16, 32, 64):
            assert marsrt.motion_grid(W, H, B) == R.grid(W, H, B)
    assert marsrt.motion_grid(100, 50) == R.grid(100, 50, 16)
    L = marsrt.lib()
    assert L.mars_hip_motion_grid(100, 50, 4, None, None, None) == marsrt.MARS_OK
    p = C.c_void_p()
    bad = [((1, 0, 8, 0, 16), FILE), ((1, 8, -1, 0, 16), FILE), ((0, 8, 8, 0, 16), FILE), ((1, 8, 8, 2, 16), FILE), ((1, 8, 8, 0, 2), FILE),
           ((1, 8, 8, 0, 24), FILE), ((1, 8, 8, 0, 128), FILE), ((1, 9, 8, 1, 16), FILE), ((1, 8, 9, 1, 16), FILE), ((1, 8193, 8, 0, 16), TENSOR),
           ((1, 8, 8194, 1, 16), TENSOR), ((65536, 8, 8, 0, 16), TENSOR),
           # two faults of different codes: the format before the grid, the grid before the evenness, the evenness before the stream count
           ((1, 8195, 8, 1, 16), TENSOR), ((1, 8193, 8, 2, 16), FILE), ((65536, 9, 8, 1, 16), FILE)]
    for args, code in bad:
        assert L.mars_hip_motion_create(*args, C.byref(p)) == code and not p.value, args
    assert L.mars_hip_motion_create(1, 8, 8, 0, 16, None) == FILE
    o = marsrt.motion_opts()
    assert L.mars_hip_motion_reset(None, 0) == FILE and L.mars_hip_motion_read(None, 0, None, None) == FILE
    assert L.mars_hip_motion_device(None, None, 1, C.byref(o)) == FILE and L.mars_hip_motion_results(None, None, None, None) == FILE
    assert L.mars_yolo_motion_frames(None, None, 1, C.byref(o), None, None, None) == FILE
    assert L.mars_hip_motion_detections_device(None, None, 1.0) == FILE and L.mars_hip_motion_det_results(None, None) == FILE
    assert L.mars_yolo_motion_boxes(None, None, None, 0, 1.0, None) == FILE and L.mars_hip_motion_ms(None) < 0
    L.mars_hip_motion_free(None)


# ---- the restatement on hand-computed cases -------------------------------------------------------------------------------------------------
def test_luma_weights():
    px = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 255], [0, 0, 0], [1, 1, 1]], dtype=np.uint8)
    # 19635 + 128 = 19763 -> 77; 38250 + 128 = 38378 = 149 * 256 + 234 -> 149 (the formula is the rule: pure green is not 150); 7395 + 128 = 7523
    # -> 29; white: 65280 + 128 -> 255
    assert R.luma_np(px, 6, 1, R.RGB).tolist() == [[77, 149, 29, 255, 0, 1]]
    y = np.arange(8, dtype=np.uint8).reshape(2, 4)
    assert np.array_equal(R.luma_np(nv12(y), 4, 2, R.NV12), y)  # the Y byte; the chroma is not looked at


def test_cell_mean_rounding_and_a_clipped_edge_cell():
    # a 4 x 4 cell of fifteen 0s and one 1: S = 1, n = 16, m = (256 + 8) / 16 = 16
    y = np.zeros((4, 4), dtype=np.int64)
    y[2, 1] = 1
    assert R.cell_means_np(y, 4).tolist() == [[16]]
    # 6 x 5 at B = 4: cells of 16, 8 (clipped right), 4 (clipped below) and 2 pixels
    y = np.zeros((5, 6), dtype=np.int64)
    y[0, 0], y[0, 5], y[4, 0], y[4, 4], y[4, 5] = 3, 3, 1, 1, 2
    assert R.cell_count_np(6, 5, 4).tolist() == [[16, 8], [4, 2]]
    # (256 * 3 + 8) / 16 = 48; (768 + 4) / 8 = 96; (256 + 2) / 4 = 64; (768 + 1) / 2 = 384
    assert R.cell_means_np(y, 4).tolist() == [[48, 96], [64, 384]]
    # n = 3 (a 3 x 1 frame): S = 1 -> (256 + 1) / 3 = 85; S = 2 -> 513 / 3 = 171: rounded to nearest, floor of the quotient
    assert R.cell_means_np(np.array([[1, 0, 0]]), 4).tolist() == [[85]] and R.cell_means_np(np.array([[1, 1, 0]]), 4).tolist() == [[171]]
    assert R.cell_means_np(np.full((64, 64), 255), 64).tolist() == [[65280]]
    assert R.grid(6, 5, 4) == (2, 2, 1) and R.grid(8192, 8192, 4) == (2048, 2048, 64) and R.grid(33, 1, 4) == (9, 1, 1)


@pytest.mark.parametrize("threshold", [0, 1, 8, 255])
def test_threshold_edge(threshold):
    """constant NV12 cells that differ from bg by exactly `threshold` levels are not active, by threshold + 1 they are"""
    thr = threshold or 8
    for base, sign in ((0, 1), (255, -1)):
        for d, want in ((thr, 0), (thr + 1, 1)):
            if not 0 <= base + sign * d <= 255:
                continue
            det = R.Detector(1, 8, 8, R.NV12, 4)
            _, st, _ = det.run(const_frames(8, 8, [base, base + sign * d]), threshold=threshold)
            assert st["active"].tolist() == [0, 4 * want] and st["first"].tolist() == [1, 0], (threshold, base, d)


def test_filter_at_a_grid_corner():
    raw = np.zeros((3, 4), dtype=bool)
    raw[0, 0] = raw[0, 1] = raw[1, 1] = True
    for k, want in ((0, True), (2, True), (3, False), (8, False)):  # the corner has 3 neighbours, 2 of them raw
        assert R.filter_np(raw, k)[0, 0] == want
    assert R.filter_np(np.ones((3, 3), dtype=bool), 8).tolist() == [[False] * 3, [False, True, False], [False] * 3]
    assert R.filter_np(np.ones((1, 1), dtype=bool), 1).tolist() == [[False]] and R.filter_np(np.ones((1, 1), dtype=bool), 0).tolist() == [[True]]
    lone = np.zeros((3, 3), dtype=bool)
    lone[2, 2] = True
    assert not R.filter_np(lone, 1).any()


def test_stall_bound_freeze_and_frame_diff():
    # a step from 0 to 255 with k = 4 (never raw: threshold 255) ends 15 short of 65280
    det = R.Detector(1, 4, 4, R.NV12, 4)
    det.run(const_frames(4, 4, [0] + [255] * 400), threshold=255, learn=4)
    assert det.bg[0, 0, 0] == 65280 - 15
    for k in (1, 8):
        det = R.Detector(1, 4, 4, R.NV12, 4)
        det.run(const_frames(4, 4, [255] + [0] * 6000), threshold=255, learn=k)
        assert 0 < det.bg[0, 0, 0] <= 2 ** k - 1, k  # from above alike: truncation toward zero
    # learn_active = 16 freezes an active cell; learn = 16 an inactive one
    det = R.Detector(1, 4, 4, R.NV12, 4)
    _, st, _ = det.run(const_frames(4, 4, [10, 200, 200, 200]), learn_active=16)
    assert det.bg[0, 0, 0] == 2560 and st["active"].tolist() == [0, 1, 1, 1]
    det = R.Detector(1, 4, 4, R.NV12, 4)
    det.run(const_frames(4, 4, [10, 13, 13]), learn=16)
    assert det.bg[0, 0, 0] == 2560
    # one update by hand: bg 2560, m 51200 (200), raw, k = 8: bg += 48640 >> 8 = 190; downwards: delta -2560 + ..., k = 4
    raw, bg = R.step_np(np.array([[2560]]), True, np.array([[51200]]))
    assert raw.tolist() == [[True]] and bg.tolist() == [[2750]]
    raw, bg = R.step_np(np.array([[2560]]), True, np.array([[2560 - 33]]))
    assert raw.tolist() == [[False]] and bg.tolist() == [[2558]]  # -(33 >> 4): toward zero, not floor(-33 / 16) = -3
    # FRAME_DIFF: bg = m after the comparison, whatever the shifts
    det = R.Detector(1, 4, 4, R.NV12, 4)
    _, st, _ = det.run(const_frames(4, 4, [10, 200, 200, 100]), flags=R.FRAME_DIFF, learn=16, learn_active=16)
    assert st["active"].tolist() == [0, 1, 0, 1] and det.bg[0, 0, 0] == 25600


def test_first_and_reset():
    det = R.Detector(2, 4, 4, R.NV12, 4)
    f = const_frames(4, 4, [10, 200, 10, 200])  # default order: stream 0 sees 10, 10 and stream 1 sees 200, 200
    _, st, _ = det.run(f)
    assert st["first"].tolist() == [1, 1, 0, 0] and st["active"].tolist() == [0, 0, 0, 0] and det.init.all()
    assert det.bg[:, 0, 0].tolist() == [2560, 51200]
    det.reset(1)
    assert det.bg[:, 0, 0].tolist() == [2560, 0] and det.init.tolist() == [True, False]
    _, st, _ = det.run(const_frames(4, 4, [110, 60]))
    assert st["first"].tolist() == [0, 1] and st["active"].tolist() == [1, 0] and det.bg[1, 0, 0] == 60 * 256


@pytest.mark.parametrize("stream_major", [False, True])
def test_two_calls_of_T_steps_equal_one_of_2T(stream_major):
    S, T, W, H, B = 3, 2, 33, 45, 16
    sc = R.scene(11, S, 2 * T, W, H, R.RGB, B)
    flags = R.STREAM_MAJOR if stream_major else 0
    one, two = R.Detector(S, W, H, R.RGB, B), R.Detector(S, W, H, R.RGB, B)
    m1, s1, _ = one.run(R.in_order(sc, stream_major), min_neighbors=1, flags=flags)
    parts = [two.run(R.in_order(sc[h * T:(h + 1) * T], stream_major), min_neighbors=1, flags=flags) for h in (0, 1)]
    assert np.array_equal(one.bg, two.bg) and s1["active"].sum() > 0
    # frame (s, t) of the long call is frame (s, t % T) of call t / T
    F = S * 2 * T
    for f in range(F):
        s, t = R.stream_step(f, F, S, stream_major)
        g = s * T + t % T if stream_major else (t % T) * S + s
        assert np.array_equal(m1[f], parts[t // T][0][g]) and s1[f] == parts[t // T][1][g], (f, s, t)
    # and the two orders describe the same streams
    other = R.Detector(S, W, H, R.RGB, B)
    other.run(R.in_order(sc, not stream_major), min_neighbors=1, flags=R.STREAM_MAJOR - flags)
    assert np.array_equal(one.bg, other.bg)


def test_zone_rule_is_the_cells_whose_pixels_meet_the_zone():
    rng = np.random.default_rng(3)
    for W, H, B in ((33, 45, 4), (65, 66, 16), (257, 130, 64), (2, 2, 4)):
        gw, gh, _ = R.grid(W, H, B)
        act = rng.integers(0, 2, (gh, gw)).astype(bool)
        for x0, y0, x1, y1 in R.case_zones(W, H, B):
            brute = sum(act[cy, cx] for cy in range(gh) for cx in range(gw)
                        if cx * B < x1 and min(W, (cx + 1) * B) > x0 and cy * B < y1 and min(H, (cy + 1) * B) > y0)
            assert R.rect_count_np(act, (x0, y0, x1, y1), B)[0] == brute, (W, H, B, x0, y0, x1, y1)
    z = R.case_zones(65, 66, 16)
    assert len(z) == R.MAX_ZONES and tuple(z[0]) == (64, 65, 65, 66) and tuple(z[1]) == (0, 0, 65, 66) and tuple(z[2]) == (0, 0, 16, 16)
    act = np.ones((5, 5), dtype=bool)
    assert [R.rect_count_np(act, r, 16) for r in z[:3]] == [(1, 1), (25, 25), (1, 1)]  # a zone ending on a cell border takes no cell behind it
    assert R.rect_count_np(act, (0, 0, 17, 16), 16) == (2, 2)


def test_map_words_padding_and_statistics():
    act = np.zeros((2, 33), dtype=bool)
    act[0, 0] = act[0, 31] = act[1, 32] = True
    w = R.pack_np(act)
    assert w.dtype == np.uint32 and w.tolist() == [[0x80000001, 0], [0, 1]]  # bits at cx >= gw stay zero
    assert np.array_equal(R.unpack_np(w, 33), act)
    full = R.pack_np(np.ones((1, 35), dtype=bool))
    assert full.tolist() == [[0xFFFFFFFF, 7]]
    # 130 x 20 at B = 4: gw = 33 (the last column 2 pixels wide), gh = 5
    assert R.stats_np(act[:1].repeat(5, axis=0), 130, 20, 4, True) == (10, 0, 0, 128, 20, 1)
    a = np.zeros((5, 33), dtype=bool)
    a[1, 32] = a[3, 30] = True
    assert R.stats_np(a, 130, 20, 4, False) == (2, 120, 4, 130, 16, 0)
    assert R.stats_np(np.zeros((5, 33), dtype=bool), 130, 20, 4, False) == (0, 0, 0, 0, 0, 0)


def test_detections_use_the_rectangle_rule_with_min_size_1():
    from test_roi_cpu import box
    act = np.zeros((5, 5), dtype=bool)
    act[1, 1] = act[1, 2] = True
    W = H = 65
    assert R.det_np(act, box(24, 24, 16, 16), W, H, 16) == (1, 1)         # [16, 32) x [16, 32): cell (1, 1) alone
    assert R.det_np(act, box(24.5, 24, 16, 16), W, H, 16) == (2, 2)       # [16, 33): floor and ceil reach into cell 2
    assert R.det_np(act, box(24, 24, 16, 16), W, H, 16, expand=2.0) == (2, 9)
    assert R.det_np(act, box(64.6, 64.6, 0.5, 0.5), W, H, 16) == (0, 1)   # one pixel: min_size is 1 here, not the crops' 2
    for b in (box(float("nan"), 1, 2, 2), box(5, 5, 0, 2), box(200, 5, 4, 4), box(5, 5, 2, 2, conf=float("inf"))):
        assert R.det_np(act, b, W, H, 16) == (0, 0)


# ---- no GPU case passes empty -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [R.RGB, R.NV12])
def test_gpu_cases_are_not_vacuous(fmt):
    seen_block = seen_small = 0
    for W, H in (R.NV12_SIZES if fmt else R.RGB_SIZES):
        for B in R.CELLS:
            for S, T, flags in R.STREAMS_STEPS:
                det = R.Detector(S, W, H, fmt, B)
                sc = R.scene(W * 100 + B, S, T, W, H, fmt, B)
                _, st, _ = det.run(R.in_order(sc, bool(flags)), min_neighbors=R.case_min_neighbors(W, H, B), flags=flags)
                if T == 1:  # the first step of a stream only initialises
                    assert st["first"].all() and not st["active"].any()
                    continue
                assert R.not_vacuous(det, W, H, B, T), (W, H, B, S, T, flags)
                seen_block += R.has_block(W, H, B)
                seen_small += not R.has_block(W, H, B)
    assert seen_block >= 15 and seen_small >= 9
