"""numpy restatement of include/mars_hip.h "Aligned crops" (shared by tests/test_align_cpu.py and tests/test_gpu_align.py): np.float32 scalar
steps, every operation rounded on its own, sums in ascending j from 0.0f.  The sampler, q16 and the NV12 conversion are those of
tests/rotref.py ("Rotated crops"); nothing of them is restated here.  Written from the header, not from the C."""
import numpy as np

from rotref import _q16, nv12_to_rgb_np, rot_sample_np  # noqa: F401  (nv12_to_rgb_np: for the callers)

F = np.float32
KPT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("v", "<f4")])  # mars_kpt_t
FIT_KEYS = ("X0", "Y0", "Ux", "Uy", "Vx", "Vy", "used", "n_used")
ZERO_FIT = dict.fromkeys(FIT_KEYS, 0)
# why a box is skipped, in the order the header states the rules
FEW, NOT_FINITE, DEGENERATE, FIT_NOT_FINITE, SMALL, LARGE, OFF_FRAME = "few", "not_finite", "degenerate", "fit_not_finite", "small", "large", "off_frame"


def kpts(xy, v=1.0):
    """[K][2] positions (+ one visibility, or K of them) -> KPT_DTYPE [K]"""
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    k = np.zeros(len(xy), dtype=KPT_DTYPE)
    k["x"], k["y"], k["v"] = xy[:, 0], xy[:, 1], v
    return k


def align_fit_np(kp, tmpl, tw, th, W, H, use=0, min_vis=0.0, expand=0.0, min_size=0):
    """-> (fit dict of the eight integers, (x0, y0, x1, y1), None) of a kept box, (ZERO_FIT, (0, 0, 0, 0), reason) of a skipped one;
    the float32 a, b, cx, cy of a kept box ride along under "abc" for the tests that look at them"""
    tmpl = np.asarray(tmpl, dtype=F).reshape(-1, 2)
    K = len(tmpl)
    e = F(expand) if expand else F(1.0)
    ms = int(min_size) if min_size else 2
    use = int(use) if use else (1 << K) - 1
    skipped = lambda why: (dict(ZERO_FIT), (0, 0, 0, 0), why)  # noqa: E731
    with np.errstate(all="ignore"):
        P = [j for j in range(K) if (use >> j) & 1 and F(kp[j]["v"]) >= F(min_vis)]
        if any(not np.isfinite(F(kp[j][c])) for j in P for c in ("x", "y", "v")):
            return skipped(NOT_FINITE)
        if len(P) < 2:
            return skipped(FEW)
        n = F(len(P))
        sqx = sqy = spx = spy = F(0)
        for j in P:
            sqx, sqy = F(sqx + tmpl[j, 0]), F(sqy + tmpl[j, 1])
            spx, spy = F(spx + F(kp[j]["x"])), F(spy + F(kp[j]["y"]))
        qmx, qmy, pmx, pmy = F(sqx / n), F(sqy / n), F(spx / n), F(spy / n)
        A = B = D = F(0)
        for j in P:
            dqx, dqy = F(tmpl[j, 0] - qmx), F(tmpl[j, 1] - qmy)
            dpx, dpy = F(F(kp[j]["x"]) - pmx), F(F(kp[j]["y"]) - pmy)
            A = F(A + F(F(dqx * dpx) + F(dqy * dpy)))
            B = F(B + F(F(dqx * dpy) - F(dqy * dpx)))
            D = F(D + F(F(dqx * dqx) + F(dqy * dqy)))
        if not D > 0:
            return skipped(DEGENERATE)
        a, b = F(A / D), F(B / D)
        if not (np.isfinite(a) and np.isfinite(b)):
            return skipped(FIT_NOT_FINITE)
        ux, uy = F(F(F(tw) * F(0.5)) - qmx), F(F(F(th) * F(0.5)) - qmy)
        cx = F(pmx + F(F(a * ux) - F(b * uy)))
        cy = F(pmy + F(F(b * ux) + F(a * uy)))
        ae, be = F(a * e), F(b * e)
        s = F(np.sqrt(F(F(ae * ae) + F(be * be))))
        we, he = F(s * F(tw)), F(s * F(th))
        if we < F(ms) or he < F(ms):
            return skipped(SMALL)
        if we > F(32768) or he > F(32768):
            return skipped(LARGE)
        if not (cx >= 0 and cx <= F(W) and cy >= 0 and cy <= F(H)):
            return skipped(OFF_FRAME)
        ha, hb = F(ae * F(0.5)), F(be * F(0.5))
        fit = dict(Ux=_q16(ha), Uy=_q16(hb), Vx=_q16(-hb), Vy=_q16(ha), X0=_q16(F(cx - F(0.5))), Y0=_q16(F(cy - F(0.5))),
                   used=sum(1 << j for j in P), n_used=len(P), abc=(a, b, cx, cy))
        assert all(-2 ** 31 <= fit[k] < 2 ** 31 for k in FIT_KEYS[:6])
        ca, sa = F(np.abs(ae) / s), F(np.abs(be) / s)
        ex = F(F(F(we * ca) + F(he * sa)) * F(0.5))
        ey = F(F(F(we * sa) + F(he * ca)) * F(0.5))
        rect = (int(np.floor(max(F(cx - ex), F(0)))), int(np.floor(max(F(cy - ey), F(0)))),
                int(np.ceil(min(F(cx + ex), F(W)))), int(np.ceil(min(F(cy + ey), F(H)))))
    return fit, rect, None


def fit_tuple(fit):
    return tuple(int(fit[k]) for k in FIT_KEYS)


def geom_of(fit, tw, th):
    """the geometry rot_sample_np takes"""
    return dict(nw=tw, nh=th, px=0, py=0, **{k: int(fit[k]) for k in FIT_KEYS[:6]})


def align_crop_np(rgb, kp, tmpl, tw, th, nhwc=True, **kw):
    """uint8 RGB frame [H][W][3] + one keypoint set (None: an empty slot) -> the int8 bytes of one destination frame"""
    out = np.full((th, tw, 3), -17, dtype=np.int8)
    if kp is not None:
        fit, _, why = align_fit_np(kp, tmpl, tw, th, rgb.shape[1], rgb.shape[0], **kw)
        if why is None:
            out[:] = rot_sample_np(rgb, geom_of(fit, tw, th))[0]
    return (out if nhwc else out.transpose(2, 0, 1)).reshape(-1).copy()


def align_select_np(dets, recs, kp, tmpl, tw, th, W, H, slots, min_conf=0.0, classes=None, max_per_frame=0, **kw):
    """dets: one record array per frame (conf, cls); recs [frames][max] (det) and kp [frames][max][K]: the pose block ->
    ([(frame, det, x0, y0, x1, y1)], [fit tuples], [(frame, slot)] of the kept boxes, dropped)"""
    kept, fits, where = [], [], []
    for f in range(len(recs)):
        n = 0
        for t in range(len(recs[f])):
            i = int(recs[f][t]["det"])
            if i == -1:
                break
            d = dets[f][i]
            if not F(d["conf"]) >= F(min_conf):
                continue
            if classes is not None and classes[1] and not classes[0] <= int(d["cls"]) < classes[0] + classes[1]:
                continue
            fit, rect, why = align_fit_np(kp[f][t], tmpl, tw, th, W, H, **kw)
            if why is not None or (max_per_frame and n >= max_per_frame):
                continue
            n += 1
            kept.append((f, i) + rect)
            fits.append(fit_tuple(fit))
            where.append((f, t))
    return kept[:slots], fits[:slots], where[:slots], max(len(kept) - slots, 0)
