"""numpy restatement of include/mars_hip.h "Oriented boxes" (shared by tests/test_obb_cpu.py and tests/test_gpu_obb.py) in float32 steps, every
operation rounded on its own (numpy's float32 +, -, *, / and sqrt are single correctly rounded operations, element by element): the angle
tables, the decode, the covariance, the pair relation, sort + greedy NMS carrying indices, the letterbox mapping, the enclosing rectangle and
the corners.  expf, cosf and sinf are the host libm's, through the route tests/test_gpu_yolo_heads.py uses."""
import ctypes as C
import functools

import numpy as np

from test_gpu_yolo_dfl import e_table
from test_gpu_yolo_heads import _libm, sig_table

F32 = np.float32
OBB_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("w", "<f4"), ("h", "<f4"), ("conf", "<f4"), ("cls", "<i4"), ("angle", "<f4"), ("pred", "<i4")])
DET_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("w", "<f4"), ("h", "<f4"), ("conf", "<f4"), ("cls", "<i4")])
PI = F32(3.14159265)

for _n in ("cosf", "sinf"):
    getattr(_libm, _n).restype = C.c_float
    getattr(_libm, _n).argtypes = [C.c_float]


def _map(fn, x):
    """a libm float function over an array, one call per element"""
    a = np.asarray(x, dtype=F32)
    return np.array([fn(float(v)) for v in a.reshape(-1)], dtype=F32).reshape(a.shape)


def expf(x):
    return _map(_libm.expf, x)


def cosf(x):
    return _map(_libm.cosf, x)


def sinf(x):
    return _map(_libm.sinf, x)


@functools.lru_cache(maxsize=None)
def _tables(s_bits):
    sg = sig_table(np.uint32(s_bits).view(F32))  # 1.0f / (1.0f + expf((-(float)q) * s))
    ang = (sg - F32(0.25)) * PI
    return sg, ang, cosf(ang), sinf(ang)


def tables(s):
    """(sg, ang, cs, sn), each float32 [256] indexed by q + 128 (built once per scale)"""
    return _tables(int(F32(s).view(np.uint32)))


def decode(heads, conf=0.25):
    """heads: [(box int8 [4 R][H][W], cls int8 [nc][H][W], angle int8 [H][W] (or [1][H][W]), box scale, class scale, angle scale, stride)]
    in prediction order -> (the candidate records, the first 1000, in prediction order; their cs; their sn; the number of candidates)"""
    conf = F32(conf)
    out, css, sns, pred0 = [], [], [], 0
    for box, cls, ang, bs, cs_, as_, stride in heads:
        nc, H, W = cls.shape
        R = box.shape[0] // 4
        sg, E = sig_table(cs_), e_table(bs)
        _, at, ct, st = tables(as_)
        cl = cls.reshape(nc, H * W).astype(np.int32)
        best = np.argmax(cl, axis=0)  # the first class of largest byte
        c = sg[cl[best, np.arange(H * W)] + 128]
        idx = np.nonzero(c >= conf)[0]
        q = box.reshape(4, R, H * W)[:, :, idx].astype(np.int32)
        e = E[q.max(axis=1)[:, None, :] - q]
        den, num = e[:, 0].copy(), np.zeros((4, len(idx)), dtype=F32)
        for i in range(1, R):
            den = den + e[:, i]
        for i in range(R):
            num = num + F32(i) * e[:, i]
        dist = num / den  # left, top, right, bottom
        assert dist.dtype == F32
        qa = ang.reshape(H * W)[idx].astype(np.int32) + 128
        cs, sn = ct[qa], st[qa]
        xf, yf = (dist[2] - dist[0]) * F32(0.5), (dist[3] - dist[1]) * F32(0.5)
        ax, ay = (idx % W).astype(F32) + F32(0.5), (idx // W).astype(F32) + F32(0.5)
        rec = np.zeros(len(idx), dtype=OBB_DTYPE)
        rec["x"] = (((xf * cs) - (yf * sn)) + ax) * F32(stride)
        rec["y"] = (((xf * sn) + (yf * cs)) + ay) * F32(stride)
        rec["w"] = (dist[0] + dist[2]) * F32(stride)
        rec["h"] = (dist[1] + dist[3]) * F32(stride)
        rec["conf"] = c[idx]
        rec["cls"] = best[idx]
        rec["angle"] = at[qa]
        rec["pred"] = pred0 + idx
        pred0 += H * W
        out.append(rec)
        css.append(cs)
        sns.append(sn)
    all_ = np.concatenate(out)
    return all_[:1000], np.concatenate(css)[:1000], np.concatenate(sns)[:1000], len(all_)


def covariance(w, h, cs, sn):
    """-> (a, b, c, d) of boxes w x h whose angle has cosine cs and sine sn"""
    w, h, cs, sn = (np.asarray(v, dtype=F32) for v in (w, h, cs, sn))
    A, B = (w * w) / F32(12.0), (h * h) / F32(12.0)
    cc, ss = cs * cs, sn * sn
    a = (A * cc) + (B * ss)
    b = (A * ss) + (B * cc)
    c = (A - B) * (cs * sn)
    with np.errstate(all="ignore"):
        v = (a * b) - (c * c)
        d = np.where(v > 0, v, F32(0.0)).astype(F32)  # a NaN gives 0
    return a, b, c, d


def e_of(T):
    """E = (float)(1 - (1 - T)^2), in double from the float threshold"""
    t = float(F32(T))
    return F32(1.0 - (1.0 - t) * (1.0 - t))


def suppresses(bi, bj, T):
    """box i = (x, y, a, b, c, d) against boxes j (scalars or arrays, broadcast) -> bool: i suppresses j at nms_thresh T"""
    xi, yi, ai, bi_, ci, di = (np.asarray(v, dtype=F32) for v in bi)
    xj, yj, aj, bj_, cj, dj = (np.asarray(v, dtype=F32) for v in bj)
    with np.errstate(all="ignore"):
        sa, sb, sc = ai + aj, bi_ + bj_, ci + cj
        dx, dy = xi - xj, yi - yj
        den = (sa * sb) - (sc * sc)
        t1 = (((sa * (dy * dy)) + (sb * (dx * dx))) / den) * F32(0.25)
        t2 = (((sc * (-dx)) * dy) / den) * F32(0.5)
        X = den / (F32(4.0) * np.sqrt(di * dj))
        lhs = expf(-(t1 + t2))
        rhs = e_of(T) * np.sqrt(X)
        assert lhs.dtype == F32 and rhs.dtype == F32
        return lhs > rhs  # a NaN on either side: False


def sort_nms(boxes, cs, sn, T=0.45, agnostic=False):
    """indices into boxes of the kept ones, in order: confidence descending then index ascending; greedy, suppressed boxes suppress nothing"""
    n = len(boxes)
    conf = boxes["conf"]
    assert not (np.isnan(conf).any() or (conf < 0).any())
    order = np.argsort(-conf.astype(np.float64), kind="stable")  # stable: equal confidences keep ascending index
    d = boxes[order]
    a, b, c, dd = covariance(d["w"], d["h"], np.asarray(cs, dtype=F32)[order], np.asarray(sn, dtype=F32)[order])
    x, y, cls = d["x"], d["y"], d["cls"]
    removed, keep = np.zeros(n, dtype=bool), []
    for i in range(n):
        if removed[i]:
            continue
        keep.append(int(order[i]))
        js = np.nonzero(~removed[i + 1:] & (agnostic | (cls[i + 1:] == cls[i])))[0] + i + 1  # (a removed box stays removed: skip it)
        if len(js):
            hit = suppresses((x[i], y[i], a[i], b[i], c[i], dd[i]), (x[js], y[js], a[js], b[js], c[js], dd[js]), T)
            removed[js[hit]] = True
    return np.array(keep, dtype=np.int64)


def letterbox(src_w, src_h, tw, th):
    """mars_preproc.c's letterbox geometry -> (px, py, rx, ry) as float32 (the boxes': tests/test_gpu_yolo_heads.py letterbox_map)"""
    scale = min(F32(tw) / F32(src_w), F32(th) / F32(src_h))
    nw, nh = int(F32(src_w) * scale), int(F32(src_h) * scale)
    return F32((tw - nw) // 2), F32((th - nh) // 2), F32(src_w) / F32(nw), F32(src_h) / F32(nh)


def mapped(boxes, src, in_hw):
    """x' = (x - px) * rx, y' = (y - py) * ry, w' = w * rx, h' = h * rx (both sides by rx); the angle stays"""
    px, py, rx, ry = letterbox(src[0], src[1], in_hw[0], in_hw[1])
    d = boxes.copy()
    d["x"] = (d["x"] - px) * rx
    d["y"] = (d["y"] - py) * ry
    d["w"] = d["w"] * rx
    d["h"] = d["h"] * rx
    return d


def enclosing(boxes, cs, sn):
    """the upright rectangle around every box: same centre, conf, cls; w_e = w |cs| + h |sn|, h_e = w |sn| + h |cs|"""
    ac, as_ = np.abs(np.asarray(cs, dtype=F32)), np.abs(np.asarray(sn, dtype=F32))
    d = np.zeros(len(boxes), dtype=DET_DTYPE)
    for k in ("x", "y", "conf", "cls"):
        d[k] = boxes[k]
    d["w"] = (boxes["w"] * ac) + (boxes["h"] * as_)
    d["h"] = (boxes["w"] * as_) + (boxes["h"] * ac)
    return d


def frame(heads, conf=0.25, T=0.45, agnostic=False, src=None, in_hw=None):
    """one frame of mars_hip_detect_obb -> (obb records, enclosing rectangles, number of candidates)"""
    cand, cs, sn, raw = decode(heads, conf)
    keep = sort_nms(cand, cs, sn, T, agnostic)
    kept = cand[keep]
    if src is not None:
        kept = mapped(kept, src, in_hw)
    return kept, enclosing(kept, cs[keep], sn[keep]), raw


def nms_list(boxes, T=0.45, agnostic=False):
    """mars_yolo_obb_nms: cs, sn = cosf(angle), sinf(angle)"""
    b = np.asarray(boxes, dtype=OBB_DTYPE)
    return b[sort_nms(b, cosf(b["angle"]), sinf(b["angle"]), T, agnostic)]


def corners(box):
    """mars_yolo_obb_corners -> float32 [4][2]"""
    x, y, w, h = (F32(box[k]) for k in ("x", "y", "w", "h"))
    cs, sn = cosf(box["angle"]).reshape(())[()], sinf(box["angle"]).reshape(())[()]
    hw, hh = w * F32(0.5), h * F32(0.5)
    ux, uy, vx, vy = hw * cs, hw * sn, hh * sn, hh * cs
    return np.array([[(x - ux) + vx, (y - uy) - vy], [(x + ux) + vx, (y + uy) - vy], [(x + ux) - vx, (y + uy) + vy], [(x - ux) - vx, (y - uy) + vy]],
                    dtype=F32)
