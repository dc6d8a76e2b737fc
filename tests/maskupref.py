"""numpy / Python-int restatement of include/mars_hip.h "Instance masks in frame pixels" (shared by tests/test_maskup_cpu.py and
tests/test_gpu_maskup.py): the tap tables from the rational with Python's unbounded integers, the literal per-pixel loops of one detection
(mask_literal), the same rule on whole arrays (mask_array, mask_frame).  The rectangle's edge rule, the selection and the bit packing are
those of tests/segref.py."""
import collections

import numpy as np

import segref

F32 = np.float32
OUT_MAX, AXIS_MAX = 8192, 1 << 20
S16 = F32(1.52587890625e-05)  # 2^-16

Geom = collections.namedtuple("Geom", "in_w in_h nw nh px py base_w base_h out_w out_h")  # mars_mask_geom_t


def identity(in_w, in_h, out_w, out_h):
    """no letterbox: the content is the graph input, the boxes are in its pixels"""
    return Geom(in_w, in_h, in_w, in_h, 0, 0, in_w, in_h, out_w, out_h)


def letterbox(src_w, src_h, in_w, in_h, out_w=0, out_h=0):
    """the boxes' letterbox rule for src_w x src_h frames (float32, as the C states it); the boxes are in the frame's pixels"""
    scale = min(F32(in_w) / F32(src_w), F32(in_h) / F32(src_h))
    nw, nh = int(F32(src_w) * scale), int(F32(src_h) * scale)
    return Geom(in_w, in_h, nw, nh, (in_w - nw) // 2, (in_h - nh) // 2, src_w, src_h, out_w or src_w, out_h or src_h)


def taps(out_n, in_n, n_content, pad, P):
    """one axis -> (ia, ib, w1), lists of Python ints; ValueError where the rule refuses"""
    if not (1 <= out_n <= OUT_MAX and 1 <= in_n <= AXIS_MAX and 1 <= P <= AXIS_MAX and n_content >= 1 and pad >= 0 and pad + n_content <= in_n):
        raise ValueError("axis out of range")
    if out_n * in_n < n_content * P:
        raise ValueError("down-scaling")
    ia, ib, w1 = [], [], []
    D = 2 * out_n * in_n
    for X in range(out_n):
        N = (2 * X + 1) * n_content * P + 2 * out_n * pad * P - out_n * in_n
        i0 = N // D  # Python's // is a true floor
        r = N - i0 * D
        assert 0 <= r < D
        w = (r * 256) // D
        assert 0 <= w <= 255
        w1.append(w)
        ia.append(min(max(i0, 0), P - 1))
        ib.append(min(max(i0 + 1, 0), P - 1))
    return ia, ib, w1


def geom_taps(g, ph, pw):
    if not (g.base_w > 0 and g.base_h > 0 and 1 <= g.out_w <= OUT_MAX and 1 <= g.out_h <= OUT_MAX and g.out_h * ((g.out_w + 31) // 32) <= 1 << 24):
        raise ValueError("grid out of range")
    return taps(g.out_w, g.in_w, g.nw, g.px, pw), taps(g.out_h, g.in_h, g.nh, g.py, ph)


def rect(box, g):
    """box = (cx, cy, w, h) in pixels of the base grid -> (x0, y0, x1, y1) in output pixels"""
    return segref.rect(box, g.base_w, g.base_h, g.out_w, g.out_h)


def bit_of(S, s, logit_min):
    """(float)S * s16 > logit_min; S is below 2^53, so Python int -> double -> float32 rounds once, to nearest even"""
    return bool(F32(S) * (F32(s) * S16) > F32(logit_min))


def mask_literal(a, proto, box, g, s, logit_min=0.0):
    """one detection, the literal loops: a int8 [nm], proto int8 [nm][PH][PW] -> ((x0, y0, x1, y1, area), words uint32 [out_h][pitch])"""
    nm, ph, pw = proto.shape
    (xa, xb, xw), (ya, yb, yw) = geom_taps(g, ph, pw)
    x0, y0, x1, y1 = rect(box, g)
    words = np.zeros((g.out_h, (g.out_w + 31) // 32), dtype=np.uint32)
    area = 0

    def dot(x, y):
        d = sum(int(a[c]) * int(proto[c, y, x]) for c in range(nm))
        assert -(1 << 31) <= d < (1 << 31)
        return d
    for Y in range(max(y0, 0), min(y1, g.out_h)):
        wy1 = yw[Y]
        wy0 = 256 - wy1
        for X in range(max(x0, 0), min(x1, g.out_w)):
            wx1 = xw[X]
            wx0 = 256 - wx1
            S = wy0 * (wx0 * dot(xa[X], ya[Y]) + wx1 * dot(xb[X], ya[Y])) + wy1 * (wx0 * dot(xa[X], yb[Y]) + wx1 * dot(xb[X], yb[Y]))
            assert abs(S) <= 1 << 36
            if bit_of(S, s, logit_min):
                words[Y, X >> 5] |= np.uint32(1 << (X & 31))
                area += 1
    return (x0, y0, x1, y1, area), words


def blend(dots, tx, ty):
    """int64 [PH][PW] dots -> int64 [out_h][out_w] S"""
    (xa, xb, xw), (ya, yb, yw) = (tuple(np.asarray(v, dtype=np.int64) for v in t) for t in (tx, ty))
    d = np.asarray(dots, dtype=np.int64)
    h = (256 - xw)[None, :] * d[:, xa] + xw[None, :] * d[:, xb]
    return (256 - yw)[:, None] * h[ya] + yw[:, None] * h[yb]


def mask_array(a, proto, box, g, s, logit_min=0.0, tables=None):
    """mask_literal on whole arrays (the same integers; int64 -> float32 rounds to nearest even)"""
    nm, ph, pw = proto.shape
    tx, ty = tables or geom_taps(g, ph, pw)
    x0, y0, x1, y1 = rect(box, g)
    S = blend(np.tensordot(np.asarray(a, dtype=np.int64), proto.astype(np.int64), axes=1), tx, ty)
    bit = S.astype(F32) * (F32(s) * S16) > F32(logit_min)
    ys, xs = np.arange(g.out_h)[:, None], np.arange(g.out_w)[None, :]
    bit &= (xs >= x0) & (xs < x1) & (ys >= y0) & (ys < y1)
    return (x0, y0, x1, y1, int(bit.sum())), segref.pack(bit)


def mask_frame(boxes, rows, scales, proto, g, logit_min=0.0, min_conf=0.0, max_per_frame=16, take_all=False):
    """one frame, as segref.mask_frame: boxes are the records of the base grid (what the detection results hold) ->
    (records MASK_DTYPE [max_per_frame], words uint32 [max_per_frame][out_h][pitch])"""
    nm, ph, pw = proto.shape
    tables = geom_taps(g, ph, pw)
    recs = np.zeros(max_per_frame, dtype=segref.MASK_DTYPE)
    recs["det"] = -1
    words = np.zeros((max_per_frame, g.out_h, (g.out_w + 31) // 32), dtype=np.uint32)
    for j, i in enumerate(segref.select(boxes["conf"], min_conf, max_per_frame, take_all)):
        b = boxes[i]
        (x0, y0, x1, y1, area), words[j] = mask_array(rows[i], proto, (b["x"], b["y"], b["w"], b["h"]), g, scales[i], logit_min, tables)
        recs[j] = (i, x0, y0, x1, y1, area)
    return recs, words
