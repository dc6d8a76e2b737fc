"""numpy restatement of include/mars_hip.h "Instance masks" (shared by tests/test_seg_cpu.py and tests/test_gpu_yolo_seg.py): the literal
per-pixel loops (mask_literal), the same rule on whole arrays (mask_frame), the rectangle, the selection, and the bit packing."""
import numpy as np

F32 = np.float32
MASK_FIELDS = ("det", "x0", "y0", "x1", "y1", "area")
MASK_DTYPE = np.dtype([(n, "<i4") for n in MASK_FIELDS])


def _edge(v, hi, up):
    """clamp((int)floorf / ceilf(v), 0, hi), clamped before the conversion: beyond the int range -> the bound, NaN -> 0"""
    v = np.ceil(v) if up else np.floor(v)
    if v != v:
        return 0
    return int(min(max(v, F32(0)), F32(hi)))


def rect(box, in_w, in_h, pw, ph):
    """box = (cx, cy, w, h) in graph-input pixels -> (x0, y0, x1, y1); float32, every operation rounded on its own"""
    cx, cy, w, h = (F32(v) for v in box)
    fx, fy = F32(pw) / F32(in_w), F32(ph) / F32(in_h)
    hw, hh = w * F32(0.5), h * F32(0.5)
    with np.errstate(all="ignore"):
        return (_edge((cx - hw) * fx, pw, False), _edge((cy - hh) * fy, ph, False), _edge((cx + hw) * fx, pw, True), _edge((cy + hh) * fy, ph, True))


def mask_literal(a, proto, box, in_w, in_h, s, logit_min=0.0):
    """one detection, the literal loops: a int8 [nm], proto int8 [nm][PH][PW] -> ((x0, y0, x1, y1, area), words uint32 [PH][pitch])"""
    nm, ph, pw = proto.shape
    x0, y0, x1, y1 = rect(box, in_w, in_h, pw, ph)
    words = np.zeros((ph, (pw + 31) // 32), dtype=np.uint32)
    area = 0
    for y in range(ph):
        for x in range(pw):
            if not (x0 <= x < x1 and y0 <= y < y1):
                continue
            dot = 0
            for c in range(nm):
                dot += int(a[c]) * int(proto[c, y, x])
            assert -(1 << 31) <= dot < (1 << 31)
            if F32(dot) * F32(s) > F32(logit_min):
                words[y, x >> 5] |= np.uint32(1 << (x & 31))
                area += 1
    return (x0, y0, x1, y1, area), words


def pack(bits):
    """bool [..., PW] -> uint32 [..., pitch]: pixel x is bit x & 31 of word x >> 5, padding bits 0"""
    pw = bits.shape[-1]
    pitch = (pw + 31) // 32
    b = np.zeros(bits.shape[:-1] + (pitch * 32,), dtype=np.uint8)
    b[..., :pw] = bits
    return np.ascontiguousarray(np.packbits(b, axis=-1, bitorder="little")).view("<u4").reshape(bits.shape[:-1] + (pitch,))


def unpack(words, pw):
    w = np.ascontiguousarray(words, dtype="<u4")
    bits = np.unpackbits(w.view(np.uint8).reshape(w.shape[:-1] + (w.shape[-1] * 4,)), axis=-1, bitorder="little")
    return bits[..., :pw].astype(bool)


def mask_array(a, proto, box, in_w, in_h, s, logit_min=0.0):
    """mask_literal on whole arrays (the same int32 dots, the same float32 product and compare)"""
    nm, ph, pw = proto.shape
    x0, y0, x1, y1 = rect(box, in_w, in_h, pw, ph)
    dot = np.tensordot(np.asarray(a, dtype=np.int32), proto.astype(np.int32), axes=1)  # [PH][PW] int32, exact
    bit = dot.astype(F32) * F32(s) > F32(logit_min)
    ys, xs = np.arange(ph)[:, None], np.arange(pw)[None, :]
    bit &= (xs >= x0) & (xs < x1) & (ys >= y0) & (ys < y1)
    return (x0, y0, x1, y1, int(bit.sum())), pack(bit)


def select(confs, min_conf, max_per_frame, take_all=False):
    """indices of the list taken, in list order"""
    out = []
    for i, c in enumerate(confs):
        if len(out) >= max_per_frame:
            break
        if take_all or F32(c) >= F32(min_conf):
            out.append(i)
    return out


def mask_frame(boxes, rows, scales, proto, in_w, in_h, logit_min=0.0, min_conf=0.0, max_per_frame=16, take_all=False):
    """one frame.  boxes: records with x, y, w, h, conf in graph-input pixels (the kept list); rows[i]: int8 [nm] coefficient row of
    detection i; scales[i]: its product scale -> (records MASK_DTYPE [max_per_frame], words uint32 [max_per_frame][PH][pitch])"""
    nm, ph, pw = proto.shape
    recs = np.zeros(max_per_frame, dtype=MASK_DTYPE)
    recs["det"] = -1
    words = np.zeros((max_per_frame, ph, (pw + 31) // 32), dtype=np.uint32)
    for j, i in enumerate(select(boxes["conf"], min_conf, max_per_frame, take_all)):
        b = boxes[i]
        (x0, y0, x1, y1, area), words[j] = mask_array(rows[i], proto, (b["x"], b["y"], b["w"], b["h"]), in_w, in_h, scales[i], logit_min)
        recs[j] = (i, x0, y0, x1, y1, area)
    return recs, words
