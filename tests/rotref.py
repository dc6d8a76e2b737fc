"""numpy restatement of include/mars_hip.h "Rotated crops" (shared by tests/test_rot_cpu.py and tests/test_gpu_rot.py): np.float32 scalar steps,
every operation rounded on its own (np.rint is round-to-nearest-even), int64 positions, integer blend.  cosf and sinf are the host libm's
(tests/obbref.py).  Written from the header, not from the C."""
import numpy as np

import obbref
from test_roi_cpu import nv12_to_rgb_np, roi_target_np  # noqa: F401  (nv12_to_rgb_np: for the callers)

F = np.float32
OBB_DTYPE = obbref.OBB_DTYPE
GREY = 111


def obb(x, y, w, h, angle, conf=0.9, cls=0, pred=0):
    """one mars_obb_t record"""
    b = np.zeros((), dtype=OBB_DTYPE)
    b["x"], b["y"], b["w"], b["h"], b["angle"], b["conf"], b["cls"], b["pred"] = x, y, w, h, angle, conf, cls, pred
    return b


def csn_of(box):
    """cosf(angle), sinf(angle) of the host libm, as float32 scalars (a non-finite angle gives NaNs: the skip rule comes first)"""
    with np.errstate(invalid="ignore"):
        a = np.array([box["angle"]], dtype=F)
        return obbref.cosf(a)[0], obbref.sinf(a)[0]


def rot_sides_np(box, W, H, expand=0.0, min_size=0):
    """the skip rule -> (we, he), or None if the box is skipped"""
    e = F(expand) if expand else F(1.0)
    ms = int(min_size) if min_size else 2
    x, y, w, h = F(box["x"]), F(box["y"]), F(box["w"]), F(box["h"])
    if not all(np.isfinite(v) for v in (x, y, w, h, F(box["conf"]), F(box["angle"]))):
        return None
    if not w > 0 or not h > 0:
        return None
    with np.errstate(over="ignore"):
        we, he = F(w * e), F(h * e)
    if we < F(ms) or he < F(ms) or we > F(32768) or he > F(32768):
        return None
    if x < 0 or x > F(W) or y < 0 or y > F(H):
        return None
    return we, he


def rot_rect_np(box, W, H, expand=0.0, min_size=0, cs=None, sn=None):
    """the ROI table's x0 .. y1: the enclosing rectangle of the expanded box, clipped to the frame; None if the box is skipped"""
    s = rot_sides_np(box, W, H, expand, min_size)
    if s is None:
        return None
    we, he = s
    if cs is None:
        cs, sn = csn_of(box)
    ac, as_ = np.abs(F(cs)), np.abs(F(sn))
    x, y = F(box["x"]), F(box["y"])
    ex = F(F(F(we * ac) + F(he * as_)) * F(0.5))
    ey = F(F(F(we * as_) + F(he * ac)) * F(0.5))
    return (int(np.floor(max(F(x - ex), F(0)))), int(np.floor(max(F(y - ey), F(0)))),
            int(np.ceil(min(F(x + ex), F(W)))), int(np.ceil(min(F(y + ey), F(H)))))


def _q16(v):
    return int(np.rint(F(F(v) * F(65536.0))))


def rot_geom_np(box, we, he, cs, sn, tw, th, keep_aspect=False):
    """-> dict(nw, nh, px, py, X0, Y0, Ux, Uy, Vx, Vy)"""
    nw, nh, px, py = tw, th, 0, 0
    if keep_aspect:
        nw, nh, px, py = roi_target_np(max(1, int(np.rint(we))), max(1, int(np.rint(he))), tw, th, True)
    cs, sn = F(cs), F(sn)
    sx, sy = F(we / F(2 * nw)), F(he / F(2 * nh))
    g = dict(nw=nw, nh=nh, px=px, py=py)
    g["Ux"], g["Uy"] = _q16(F(sx * cs)), _q16(F(sx * sn))
    g["Vx"], g["Vy"] = _q16(-F(sy * sn)), _q16(F(sy * cs))
    g["X0"], g["Y0"] = _q16(F(F(box["x"]) - F(0.5))), _q16(F(F(box["y"]) - F(0.5)))
    assert all(-2 ** 31 <= g[k] < 2 ** 31 for k in ("Ux", "Uy", "Vx", "Vy", "X0", "Y0"))
    return g


def rot_sample_np(rgb, g):
    """uint8 RGB frame [H][W][3] + geometry -> (int8 [nh][nw][3], the number of taps outside the frame)"""
    H, W = rgb.shape[:2]
    a = (2 * np.arange(g["nw"], dtype=np.int64) + 1 - g["nw"])[None, :]
    b = (2 * np.arange(g["nh"], dtype=np.int64) + 1 - g["nh"])[:, None]
    PX = g["X0"] + a * g["Ux"] + b * g["Vx"]
    PY = g["Y0"] + a * g["Uy"] + b * g["Vy"]
    qx, qy = PX >> 8, PY >> 8
    ix, fx, iy, fy = qx >> 8, (qx & 255)[..., None], qy >> 8, (qy & 255)[..., None]
    p = rgb.astype(np.int64)
    outside = 0

    def tap(xx, yy):
        nonlocal outside
        ok = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
        outside += int((~ok).sum())
        v = p[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)]
        return np.where(ok[..., None], v, GREY)

    top = tap(ix, iy) * (256 - fx) + tap(ix + 1, iy) * fx
    bot = tap(ix, iy + 1) * (256 - fx) + tap(ix + 1, iy + 1) * fx
    v = (top * (256 - fy) + bot * fy + 32768) >> 16
    assert v.min() >= 0 and v.max() <= 255
    return (v - 128).astype(np.int8), outside


def rot_crop_np(rgb, box, tw, th, nhwc=True, keep_aspect=False, expand=0.0, min_size=0, cs=None, sn=None):
    """uint8 RGB frame [H][W][3] + one oriented box (None: an empty slot) -> the int8 bytes of one destination frame"""
    out = np.full((th, tw, 3), -17, dtype=np.int8)
    s = None if box is None else rot_sides_np(box, rgb.shape[1], rgb.shape[0], expand, min_size)
    if s is not None:
        if cs is None:
            cs, sn = csn_of(box)
        g = rot_geom_np(box, s[0], s[1], cs, sn, tw, th, keep_aspect)
        out[g["py"]:g["py"] + g["nh"], g["px"]:g["px"] + g["nw"]] = rot_sample_np(rgb, g)[0]
    return (out if nhwc else out.transpose(2, 0, 1)).reshape(-1).copy()


def rot_select_np(boxes, W, H, slots, expand=0.0, min_conf=0.0, min_size=0, classes=None, max_per_frame=0):
    """boxes: one OBB_DTYPE array per frame, in list order -> ([(frame, det, x0, y0, x1, y1)] of the kept boxes, dropped)"""
    kept = []
    for f, d in enumerate(boxes):
        n = 0
        for i in range(len(d)):
            if not F(d[i]["conf"]) >= F(min_conf):
                continue
            if classes is not None and classes[1] and not classes[0] <= int(d[i]["cls"]) < classes[0] + classes[1]:
                continue
            r = rot_rect_np(d[i], W, H, expand, min_size)
            if r is None or (max_per_frame and n >= max_per_frame):
                continue
            n += 1
            kept.append((f, i) + r)
    return kept[:slots], max(len(kept) - slots, 0)
