"""The numpy restatement of "Area averaging" (include/mars_hip.h, "ROI crops"), vectorised: per axis a weight matrix and a denominator, per
channel Wy @ crop @ Wx.T over int64, then the rounding.  tests/test_area_cpu.py checks it on cases worked by hand, tests/test_gpu_area.py
compares the device against it.  The rectangle and target rules are those of tests/test_roi_cpu.py, imported unchanged."""
import numpy as np

from test_roi_cpu import roi_axis_np, roi_rect_np, roi_target_np  # noqa: F401  (roi_rect_np: for the callers)


def area_axis_np(n_in, n_out, area):
    """-> (D, int64 weight matrix [n_out][n_in]): row i holds the taps of output sample i"""
    W = np.zeros((n_out, n_in), dtype=np.int64)
    if not area or n_in <= n_out:
        i0, i1, f = roi_axis_np(n_in, n_out)
        i = np.arange(n_out)
        np.add.at(W, (i, i0), 256 - f)
        np.add.at(W, (i, i1), f)
        return 256, W
    i = np.arange(n_out, dtype=np.int64)[:, None]
    s = np.arange(n_in, dtype=np.int64)[None, :]
    W[:] = np.maximum(np.minimum((s + 1) * n_out, (i + 1) * n_in) - np.maximum(s * n_out, i * n_in), 0)
    return n_in, W


def _taps_matmul(W, a):
    """W @ a over int64 for a weight matrix whose rows are runs of taps: the zeros outside a row's run are not multiplied (a whole-frame
    crop would cost seconds otherwise); a: [n_in][m], any integer type"""
    out = np.empty((W.shape[0], a.shape[1]), dtype=np.int64)
    for i in range(W.shape[0]):
        nz = np.flatnonzero(W[i])
        lo, hi = nz[0], nz[-1] + 1
        out[i] = W[i, lo:hi] @ a[lo:hi].astype(np.int64)
    return out


def area_resize_np(crop, nw, nh, area=True):
    """uint8 [ch][cw][3] -> int8 [nh][nw][3]: S = Wy @ crop @ Wx.T per channel"""
    ch, cw = crop.shape[:2]
    Dx, Wx = area_axis_np(cw, nw, area)
    Dy, Wy = area_axis_np(ch, nh, area)
    D = Dx * Dy
    rows = _taps_matmul(Wy, crop.reshape(ch, cw * 3)).reshape(nh, cw, 3)                    # [nh][cw][3]
    S = _taps_matmul(Wx, rows.transpose(1, 0, 2).reshape(cw, nh * 3)).reshape(nw, nh, 3).transpose(1, 0, 2)
    v = (S + D // 2) // D
    assert v.min() >= 0 and v.max() <= 255
    return (v - 128).astype(np.int8)


def area_crop_np(rgb, rect, tw, th, nhwc=True, keep_aspect=False, area=True):
    """uint8 RGB frame [H][W][3] + rectangle (None: skipped) -> the int8 bytes of one destination frame"""
    out = np.full((th, tw, 3), -17, dtype=np.int8)
    if rect is not None:
        x0, y0, x1, y1 = rect
        nw, nh, px, py = roi_target_np(x1 - x0, y1 - y0, tw, th, keep_aspect)
        out[py:py + nh, px:px + nw] = area_resize_np(rgb[y0:y1, x0:x1], nw, nh, area)
    return (out if nhwc else out.transpose(2, 0, 1)).reshape(-1).copy()
