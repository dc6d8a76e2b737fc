"""numpy restatement of include/mars_hip.h "Pose keypoints" (shared by tests/test_pose_cpu.py and tests/test_gpu_pose.py) in float32 scalar
steps, every operation rounded on its own: one keypoint (point), one detection's K keypoints (keypoints), the selection, one frame
(pose_frame).  The visibility table and the letterbox geometry are the detection tail's (tests/test_gpu_yolo_heads.py)."""
import functools

import numpy as np

from test_gpu_yolo_heads import letterbox_map, sig_table

F32 = np.float32
POSE_DTYPE = np.dtype([("det", "<i4"), ("head", "<i4"), ("cell", "<i4")])
KPT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("v", "<f4")])


@functools.lru_cache(maxsize=None)
def _vis(s_bits):
    return sig_table(np.uint32(s_bits).view(F32))


def visibility(s):
    """v[q + 128] = 1.0f / (1.0f + expf((-(float)q) * s)): the class confidence's table (built once per scale)"""
    return _vis(int(F32(s).view(np.uint32)))


def point(q, g, stride, s):
    """((float)q * s * 2 + g) * stride, one rounding per operation"""
    ax = F32(int(q)) * F32(s)
    return (ax * F32(2.0) + F32(int(g))) * F32(int(stride))


def keypoints(row, K, D, gx, gy, stride, s, src=None, in_hw=None):
    """row: the K * D int8 bytes of one cell -> KPT_DTYPE [K]; src = (src_w, src_h) with in_hw = (in_w, in_h): mapped as the boxes are"""
    assert D in (2, 3) and len(row) == K * D
    out = np.zeros(K, dtype=KPT_DTYPE)
    vis = visibility(s) if D == 3 else None
    for j in range(K):
        out[j]["x"] = point(row[D * j], gx, stride, s)
        out[j]["y"] = point(row[D * j + 1], gy, stride, s)
        out[j]["v"] = vis[int(row[D * j + 2]) + 128] if D == 3 else F32(1.0)
    if src is not None:
        # the boxes' rule through the boxes' own restatement: x' = (x - px) * rx, y' = (y - py) * ry (w and h are not used)
        d = np.zeros(K, dtype=[("x", "<f4"), ("y", "<f4"), ("w", "<f4"), ("h", "<f4")])
        d["x"], d["y"] = out["x"], out["y"]
        d = letterbox_map(d, src[0], src[1], in_hw[0], in_hw[1])
        out["x"], out["y"] = d["x"], d["y"]
    return out


def select(confs, min_conf, max_per_frame, take_all=False):
    """indices of the list taken, in list order"""
    out = []
    for i, c in enumerate(confs):
        if len(out) >= max_per_frame:
            break
        if take_all or F32(c) >= F32(min_conf):
            out.append(i)
    return out


def pose_frame(confs, origins, kpt_arrs, scales, strides, K, D, min_conf=0.0, max_per_frame=32, src=None, in_hw=None):
    """one frame.  confs: the kept list's confidences; origins[i]: the prediction index of kept detection i; kpt_arrs[k]: int8
    [K * D][H_k][W_k] of head k; scales[k], strides[k] -> (records POSE_DTYPE [max_per_frame], keypoints KPT_DTYPE [max_per_frame][K])"""
    cells = np.cumsum([0] + [a.shape[1] * a.shape[2] for a in kpt_arrs])
    recs = np.zeros(max_per_frame, dtype=POSE_DTYPE)
    recs[:] = (-1, -1, -1)
    kpts = np.zeros((max_per_frame, K), dtype=KPT_DTYPE)
    for t, i in enumerate(select(confs, min_conf, max_per_frame)):
        o = int(origins[i])
        k = int(np.searchsorted(cells, o, side="right")) - 1
        cell, W = o - int(cells[k]), kpt_arrs[k].shape[2]
        row = kpt_arrs[k].reshape(K * D, -1)[:, cell]
        recs[t] = (i, k, cell)
        kpts[t] = keypoints(row, K, D, cell % W, cell // W, strides[k], scales[k], src, in_hw)
    return recs, kpts
