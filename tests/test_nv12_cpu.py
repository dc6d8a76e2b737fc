"""NV12 camera frames, the part that needs no GPU: the new entry points are exported, the frame size is right, and arguments that can
never be valid (odd sizes, unknown flag bits, NULL pointers) are refused up front -- with or without a device."""
import ctypes as C

import numpy as np

NEW = ["mars_hip_nv12_frame_bytes", "mars_yolo_nv12_to_rgb", "mars_yolo_letterbox_nv12", "mars_hip_preprocess_nv12",
       "mars_hip_preprocess_nv12_device"]


def test_nv12_symbols_are_exported(marsrt):
    L = marsrt.lib()
    for n in NEW:
        assert n in marsrt.EXPORTS["mars_hip.h"], n
        assert hasattr(L, n), n
    assert (marsrt.CAMERA_RGB, marsrt.CAMERA_NV12) == (0, 1) and (marsrt.NV12_FULL_RANGE, marsrt.NV12_VU) == (1, 2)
    names = [f[0] for f in marsrt.PipeOpts._fields_]
    assert names[-2:] == ["camera_format", "camera_flags"] and names[-3] == "dfl_heads"  # appended: zero still means RGB
    for n in ("nv12_to_rgb", "letterbox_nv12"):
        assert callable(getattr(marsrt, n))
    assert callable(marsrt.Model.preprocess_nv12)


def test_nv12_frame_bytes(marsrt):
    fb = marsrt.lib().mars_hip_nv12_frame_bytes
    assert fb(6, 4) == 36
    assert fb(1280, 720) == 1382400
    assert fb(2, 2) == 6
    assert fb(4096, 4096) == 4096 * 4096 * 3 // 2
    for w, h in [(5, 4), (6, 3), (7, 7), (0, 4), (6, 0), (-2, 4), (6, -4), (0, 0)]:
        assert fb(w, h) == 0, (w, h)


def test_nv12_bad_arguments_are_refused_up_front(marsrt):
    L = marsrt.lib()
    src = np.zeros(6 * 4 * 3 // 2 + 64, dtype=np.uint8)
    rgb = np.full(6 * 4 * 3 + 64, 77, dtype=np.uint8)
    out = np.full(8 * 8 * 3, 77, dtype=np.int8)
    s, r, o = src.ctypes.data, rgb.ctypes.data, out.ctypes.data
    # odd or non-positive sizes
    for w, h in [(5, 4), (6, 3), (0, 4), (6, -2)]:
        assert L.mars_yolo_nv12_to_rgb(s, w, h, 0, r) == -1, (w, h)
        assert L.mars_yolo_letterbox_nv12(s, w, h, 8, 8, 1, 0, o) == -1, (w, h)
    # unknown flag bits (bit 2 and above)
    for flags in (4, 5, 8, 0x80000000):
        assert L.mars_yolo_nv12_to_rgb(s, 6, 4, flags, r) == -1, flags
        assert L.mars_yolo_letterbox_nv12(s, 6, 4, 8, 8, 1, flags, o) == -1, flags
    # NULL pointers
    assert L.mars_yolo_nv12_to_rgb(None, 6, 4, 0, r) == -1
    assert L.mars_yolo_nv12_to_rgb(s, 6, 4, 0, None) == -1
    assert L.mars_yolo_letterbox_nv12(None, 6, 4, 8, 8, 1, 0, o) == -1
    assert L.mars_yolo_letterbox_nv12(s, 6, 4, 8, 8, 1, 0, None) == -1
    assert L.mars_yolo_letterbox_nv12(s, 6, 4, 0, 8, 1, 0, o) == -1
    assert (rgb == 77).all() and (out == 77).all()  # nothing was written
    # the model forms: no model, NULL frames, odd sizes, unknown flags
    P = C.POINTER(marsrt.MarsModel)
    for f in (L.mars_hip_preprocess_nv12, L.mars_hip_preprocess_nv12_device):
        assert f(P(), 0, s, 6, 4, 0, 0, 1) == marsrt.MARS_ERR_INVALID_FILE
        assert f(P(), 0, None, 6, 4, 0, 0, 1) == marsrt.MARS_ERR_INVALID_FILE
        assert f(P(), 0, s, 5, 4, 0, 0, 1) == marsrt.MARS_ERR_INVALID_FILE
        assert f(P(), 0, s, 6, 4, 4, 0, 1) == marsrt.MARS_ERR_INVALID_FILE
