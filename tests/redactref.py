"""The numpy restatement of "Redaction" (include/mars_hip.h) for RGB and NV12 frames: regions, their union, the cells, mosaic and fill, the
selection of the device form and the statistics.  tests/test_redact_cpu.py pins it against a per-pixel loop and cases worked by hand,
tests/test_gpu_redact.py compares the device against it.  The rectangle rule is that of tests/test_roi_cpu.py, imported unchanged."""
import numpy as np

from test_roi_cpu import roi_rect_np

F = np.float32
MOSAIC, FILL = 0, 1
RGB, NV12 = 0, 1
NV12_VU = 2
CELLS = (2, 4, 8, 16, 32, 64)
STATS = np.dtype([("regions", "<i4"), ("masked", "<i4"), ("skipped", "<i4"), ("pixels", "<i4")])


def frame_bytes(W, H, fmt):
    return W * H * 3 // 2 if fmt == NV12 else W * H * 3


def unpack_words(words, W):
    """uint32 [H][(W + 31) / 32] -> bool [H][W]: pixel x is bit x & 31 of word x >> 5"""
    words = np.asarray(words, dtype=np.uint32)
    x = np.arange(W)
    return ((words[:, x >> 5] >> (x & 31).astype(np.uint32)) & 1).astype(bool)


def union_np(boxes, W, H, expand=0.0, masks=None):
    """every box is a selected detection -> (U bool [H][W], (regions, masked, skipped, pixels)); masks: None, or per box None / bool [H][W]"""
    U = np.zeros((H, W), dtype=bool)
    regions = masked = skipped = 0
    for i in range(len(boxes)):
        r = roi_rect_np(boxes[i], W, H, expand, 1)
        if r is None:
            skipped += 1
            continue
        regions += 1
        x0, y0, x1, y1 = r
        if masks is not None and masks[i] is not None:
            masked += 1
            U[y0:y1, x0:x1] |= masks[i][y0:y1, x0:x1]
        else:
            U[y0:y1, x0:x1] = True
    return U, (regions, masked, skipped, int(U.sum()))


def cell_means_np(plane, B):
    """[h][w][c] uint8 -> the same shape: at every sample the rounded mean (S + n / 2) / n of its cell, cells of B x B anchored at the origin
    and clipped at the far edges"""
    h, w = plane.shape[:2]
    ys, xs = np.arange(0, h, B), np.arange(0, w, B)
    S = np.add.reduceat(np.add.reduceat(plane.astype(np.int64), ys, axis=0), xs, axis=1)
    n = (np.minimum(ys + B, h) - ys)[:, None, None] * (np.minimum(xs + B, w) - xs)[None, :, None]
    v = (S + n // 2) // n
    return np.repeat(np.repeat(v, B, axis=0), B, axis=1)[:h, :w].astype(np.uint8)


def redact_plane_np(plane, cov, mode, B, fill):
    """[h][w][c] uint8, cov bool [h][w], fill [c] -> the redacted plane (a new array)"""
    out = plane.copy()
    if mode == FILL:
        out[cov] = np.asarray(fill, dtype=np.uint8)
    else:
        out[cov] = cell_means_np(plane, B)[cov]
    return out


def redact_frame_np(buf, W, H, fmt, U, mode=MOSAIC, cell=0, fill=(0, 0, 0), src_flags=0):
    """one frame's bytes + the union -> the redacted frame's bytes"""
    B = cell or 16
    assert B in CELLS and mode in (MOSAIC, FILL)
    buf = np.asarray(buf, dtype=np.uint8).reshape(-1)
    assert buf.size == frame_bytes(W, H, fmt)
    if fmt == RGB:
        return redact_plane_np(buf.reshape(H, W, 3), U, mode, B, fill).reshape(-1)
    assert W % 2 == 0 and H % 2 == 0
    y = redact_plane_np(buf[:W * H].reshape(H, W, 1), U, mode, B, fill[:1])
    cu = U.reshape(H // 2, 2, W // 2, 2).any(axis=(1, 3))  # any of the four pixels
    cf = (fill[2], fill[1]) if src_flags & NV12_VU else (fill[1], fill[2])
    c = redact_plane_np(buf[W * H:].reshape(H // 2, W // 2, 2), cu, mode, B // 2, cf)
    return np.concatenate([y.reshape(-1), c.reshape(-1)])


def redact_frames_np(frames, boxes, frame_of_box, W, H, fmt=RGB, mode=MOSAIC, cell=0, fill=(0, 0, 0), expand=0.0, src_flags=0, mask_words=None,
                     mask_of_box=None):
    """the host-pointer form: -> (uint8 [F][frame bytes], STATS [F], [U of every frame])"""
    fb = frame_bytes(W, H, fmt)
    frames = np.asarray(frames, dtype=np.uint8).reshape(-1, fb)
    fo = np.asarray(frame_of_box, dtype=np.int64).reshape(-1)
    out = np.empty_like(frames)
    stats = np.zeros(len(frames), dtype=STATS)
    unions = []
    for f in range(len(frames)):
        idx = np.flatnonzero(fo == f)
        masks = None
        if mask_of_box is not None:
            masks = [unpack_words(mask_words[mask_of_box[i]], W) if mask_of_box[i] >= 0 else None for i in idx]
        U, st = union_np(boxes[idx], W, H, expand, masks)
        out[f] = redact_frame_np(frames[f], W, H, fmt, U, mode, cell, fill, src_flags)
        stats[f] = st
        unions.append(U)
    return out, stats, unions


def select_np(dets, min_conf=0.0, classes=None, idents=None, ident_min=0.0):
    """the device form's selection over one frame's list -> the indices of the selected detections, in list order"""
    keep = []
    for i in range(len(dets)):
        if not F(dets[i]["conf"]) >= F(min_conf):
            continue
        if classes is not None and classes[1] and not classes[0] <= int(dets[i]["cls"]) < classes[0] + classes[1]:
            continue
        if idents is not None and int(idents[i]["cls"]) >= 0 and F(idents[i]["score"]) >= F(ident_min):
            continue
        keep.append(i)
    return keep
