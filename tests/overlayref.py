"""The numpy restatement of "Overlay" (include/mars_hip.h) for RGB and NV12 frames: elements, colours, texts, the four layers and their
owners, the NV12 rule and the statistics.  pixel_np is the rule for ONE pixel, a loop over the elements in list order; overlay_frame_np
builds an owner map per layer instead (elements written in reverse order, so the lowest index stays on top) and
tests/test_overlay_cpu.py pins it against pixel_np and cases worked by hand; tests/test_gpu_overlay.py compares the device against it.
Neither is the kernel's algorithm (bit masks and minima per thread).  The rectangle rule is that of tests/test_roi_cpu.py, imported
unchanged; the glyph rows and the built-in palette come from the library's host functions (bind)."""
import functools

import numpy as np

from redactref import frame_bytes, unpack_words
from test_roi_cpu import roi_rect_np

F = np.float32
RGB, NV12 = 0, 1
NV12_FULL_RANGE, NV12_VU = 1, 2
MASKS, BOXES, KEYPOINTS, LABELS = 1, 2, 4, 8
BY_CLASS, BY_TRACK, FIXED = 0, 1, 2
TEXT_CLASS, TEXT_TRACK, TEXT_CONF = 1, 2, 4
TEXT_MAX, NAME_LEN = 24, 16
STATS = np.dtype([("boxes", "<i4"), ("masked", "<i4"), ("labels", "<i4"), ("markers", "<i4"), ("skipped", "<i4"), ("pixels", "<i4")])
NONE = 1 << 30

FONT = None     # uint8 [256][7]: the rows of the glyph every byte shows as
PALETTE = None  # uint8 [16][3]


def bind(rt):
    """the glyph rows and the built-in palette through the library's host functions (no device)"""
    global FONT, PALETTE
    if FONT is None:
        FONT = np.stack([rt.overlay_glyph(b) for b in range(256)])
        PALETTE = rt.overlay_default_palette()


def rgb_to_yuv_np(rgb, flags=0):
    """(R, G, B) -> (Y, first stored chroma byte, second); >> on a Python int is an arithmetic shift"""
    r, g, b = (int(v) for v in rgb)
    if flags & NV12_FULL_RANGE:
        y, u, v = (77 * r + 150 * g + 29 * b + 128) >> 8, ((-43 * r - 85 * g + 128 * b + 128) >> 8) + 128, ((128 * r - 107 * g - 21 * b + 128) >> 8) + 128
    else:
        y, u, v = ((66 * r + 129 * g + 25 * b + 128) >> 8) + 16, ((-38 * r - 74 * g + 112 * b + 128) >> 8) + 128, ((112 * r - 94 * g - 18 * b + 128) >> 8) + 128
    y, u, v = (min(max(c, 0), 255) for c in (y, u, v))
    return (y, v, u) if flags & NV12_VU else (y, u, v)


def text_white(rgb):
    return ((77 * int(rgb[0]) + 150 * int(rgb[1]) + 29 * int(rgb[2]) + 128) >> 8) < 128


def text_np(cls, conf, track_id=-1, text=0, names=None):
    """the label bytes of a detection; names: None or uint8 [n][NAME_LEN]"""
    text = text or (TEXT_CLASS | TEXT_CONF)
    parts = []
    if text & TEXT_CLASS:
        nm = b""
        if names is not None and 0 <= cls < len(names):
            nm = bytes(names[cls]).split(b"\0")[0]
        parts.append(nm if nm else b"%d" % cls)
    if text & TEXT_TRACK and track_id >= 0:
        parts.append(b"#%d" % track_id)
    if text & TEXT_CONF:
        v = F(F(F(conf) * F(100.0)) + F(0.5))
        p = 0 if not v > 0 else 100 if v >= 100 else int(v)
        parts.append(b"%d%%" % p)
    return b" ".join(parts)[:TEXT_MAX]


@functools.lru_cache(maxsize=None)
def label_np(text, s):
    """the strip of a text (bytes) at scale s, not cut: bool [9 s][s (6 n + 1)], True = a text pixel; shared, so left unchanged by its users"""
    n = len(text)
    out = np.zeros((9 * s, s * (6 * n + 1)), dtype=bool)
    for y in range(9 * s):
        for x in range(out.shape[1]):
            u, v = x - s, y - s
            if u >= 0 and 0 <= v < 7 * s and u // (6 * s) < n and u % (6 * s) < 5 * s:
                out[y, x] = (int(FONT[text[u // (6 * s)]][v // s]) >> (4 - (u % (6 * s)) // s)) & 1
    return out


class Opts:
    """the options with their defaults resolved"""

    def __init__(self, layers=0, color_by=BY_CLASS, text=0, thickness=0, radius=0, scale=0, alpha=0, no_key=(0, 0, 0), kpt_min_v=0.0,
                 palette=None, names=None, src_flags=0):
        self.layers = layers or (BOXES | LABELS)
        self.color_by, self.text = color_by, text or (TEXT_CLASS | TEXT_CONF)
        self.t, self.r, self.s, self.a = thickness or 2, radius or 2, scale or 2, alpha or 96
        self.no_key, self.kpt_min_v = tuple(int(v) for v in no_key), F(kpt_min_v) if kpt_min_v else F(0.5)
        self.palette = np.asarray(PALETTE if palette is None else palette, dtype=np.uint8).reshape(-1, 3)
        self.names, self.src_flags = names, src_flags


def elements_np(boxes, W, H, o, keys=None, texts=None, masks=None, kpts=None, tracks=None):
    """the selected detections of one frame, in list order -> (elements, markers, skipped).  An element is a dict {rect, rgb, text, mask};
    a marker is (element index, keypoint index, cx, cy).  keys / texts / masks (bool [H][W] or None) / kpts ([K] records or None) /
    tracks (records with id) are per box, each list may be None"""
    P = len(o.palette)
    elems, marks, skipped = [], [], 0
    for i in range(len(boxes)):
        r = roi_rect_np(boxes[i], W, H, 0.0, 1)
        if r is None:
            skipped += 1
            continue
        cls, tid = int(boxes[i]["cls"]), int(tracks[i]["id"]) if tracks is not None else -1
        key = int(keys[i]) if keys is not None else cls if o.color_by == BY_CLASS else tid if o.color_by == BY_TRACK else 0
        rgb = tuple(int(v) for v in o.palette[key % P]) if key >= 0 else o.no_key
        text = b""
        if o.layers & LABELS:
            text = bytes(texts[i]).split(b"\0")[0][:TEXT_MAX] if texts is not None else text_np(cls, boxes[i]["conf"], tid, o.text, o.names)
        mask = masks[i] if masks is not None and o.layers & MASKS else None
        e = len(elems)
        elems.append(dict(rect=r, rgb=rgb, text=text, mask=mask))
        if o.layers & KEYPOINTS and kpts is not None and kpts[i] is not None:
            for j, k in enumerate(kpts[i]):
                x, y, v = F(k["x"]), F(k["y"]), F(k["v"])
                if not (np.isfinite(x) and np.isfinite(y)) or not v >= o.kpt_min_v:
                    continue
                cx, cy = np.floor(x), np.floor(y)
                if cx < F(-8.0) or cx > F(W + 8) or cy < F(-8.0) or cy > F(H + 8):
                    continue
                marks.append((e, j, int(cx), int(cy)))
    return elems, marks, skipped


def strip_rect(e, o):
    """(lx, ly, Wl, Hl) of an element's label strip, not cut"""
    x0, y0 = e["rect"][:2]
    Hl = 9 * o.s
    return x0, (y0 - Hl if y0 - Hl >= 0 else y0), o.s * (6 * len(e["text"]) + 1), Hl


def pixel_np(x, y, W, H, elems, marks, o):
    """the rule for one pixel: -> (kind, rgb) with kind None (the source pixel stays), "opaque" or "tint"; loops in list order, so the first
    element found in a layer is its owner"""
    if o.layers & LABELS:
        for e in elems:
            if e["text"]:
                lx, ly, Wl, Hl = strip_rect(e, o)
                if lx <= x < lx + Wl and ly <= y < ly + Hl:
                    u, v, s = x - lx - o.s, y - ly - o.s, o.s
                    on = u >= 0 and 0 <= v < 7 * s and u // (6 * s) < len(e["text"]) and u % (6 * s) < 5 * s and \
                        (int(FONT[e["text"][u // (6 * s)]][v // s]) >> (4 - (u % (6 * s)) // s)) & 1
                    return "opaque", ((255, 255, 255) if text_white(e["rgb"]) else (0, 0, 0)) if on else e["rgb"]
    for ei, j, cx, cy in sorted(marks):
        if abs(x - cx) <= o.r and abs(y - cy) <= o.r:
            return "opaque", tuple(int(v) for v in o.palette[j % len(o.palette)])
    if o.layers & BOXES:
        for e in elems:
            x0, y0, x1, y1 = e["rect"]
            if x0 <= x < x1 and y0 <= y < y1 and not (x0 + o.t <= x < x1 - o.t and y0 + o.t <= y < y1 - o.t):
                return "opaque", e["rgb"]
    for e in elems:
        x0, y0, x1, y1 = e["rect"]
        if e["mask"] is not None and x0 <= x < x1 and y0 <= y < y1 and e["mask"][y, x]:
            return "tint", e["rgb"]
    return None, None


def cut(lo, hi, n):
    return max(lo, 0), min(hi, n)


def owners_np(W, H, elems, marks, o):
    """per layer the owner map int32 [H][W] (NONE: nobody; markers: element * 32 + keypoint), the label's text pixels, how many elements
    of each layer cover every pixel, and the pixels any element's rectangle, strip or marker square touches"""
    own = {k: np.full((H, W), NONE, dtype=np.int32) for k in (LABELS, KEYPOINTS, BOXES, MASKS)}
    cnt = {k: np.zeros((H, W), dtype=np.int32) for k in own}
    on = np.zeros((H, W), dtype=bool)
    touched = np.zeros((H, W), dtype=bool)
    for ei in reversed(range(len(elems))):
        e = elems[ei]
        x0, y0, x1, y1 = e["rect"]
        touched[y0:y1, x0:x1] = True
        if e["mask"] is not None:
            m = e["mask"][y0:y1, x0:x1]
            own[MASKS][y0:y1, x0:x1][m] = ei
            cnt[MASKS][y0:y1, x0:x1] += m
        if o.layers & BOXES:
            ring = np.ones((y1 - y0, x1 - x0), dtype=bool)
            if x0 + o.t < x1 - o.t and y0 + o.t < y1 - o.t:
                ring[o.t:y1 - y0 - o.t, o.t:x1 - x0 - o.t] = False
            own[BOXES][y0:y1, x0:x1][ring] = ei
            cnt[BOXES][y0:y1, x0:x1] += ring
        if o.layers & LABELS and e["text"]:
            lx, ly, Wl, Hl = strip_rect(e, o)
            bm = label_np(e["text"], o.s)
            (ax, bx), (ay, by) = cut(lx, lx + Wl, W), cut(ly, ly + Hl, H)
            if bx > ax and by > ay:
                own[LABELS][ay:by, ax:bx] = ei
                cnt[LABELS][ay:by, ax:bx] += 1
                on[ay:by, ax:bx] = bm[ay - ly:by - ly, ax - lx:bx - lx]
                touched[ay:by, ax:bx] = True
    for ei, j, cx, cy in sorted(marks, reverse=True):
        (ax, bx), (ay, by) = cut(cx - o.r, cx + o.r + 1, W), cut(cy - o.r, cy + o.r + 1, H)
        if bx > ax and by > ay:
            own[KEYPOINTS][ay:by, ax:bx] = ei * 32 + j
            cnt[KEYPOINTS][ay:by, ax:bx] += 1
            touched[ay:by, ax:bx] = True
    return own, on, cnt, touched


def colour_bytes(rgb, fmt, flags):
    return rgb_to_yuv_np(rgb, flags) if fmt == NV12 else tuple(int(v) for v in rgb)


def overlay_frame_np(buf, W, H, fmt, elems, marks, o):
    """one frame's bytes -> (the painted frame's bytes, the covered pixels, the owner maps' record for the vacuity checks)"""
    buf = np.asarray(buf, dtype=np.uint8).reshape(-1)
    assert buf.size == frame_bytes(W, H, fmt)
    own, on, cnt, touched = owners_np(W, H, elems, marks, o)
    col = np.zeros((H, W, 3), dtype=np.int64)  # the colour over every pixel, in the frame format's bytes
    opaque = np.zeros((H, W), dtype=bool)
    P = len(o.palette)
    ecol = [colour_bytes(e["rgb"], fmt, o.src_flags) for e in elems]
    tcol = [colour_bytes((255, 255, 255) if text_white(e["rgb"]) else (0, 0, 0), fmt, o.src_flags) for e in elems]
    pcol = [colour_bytes(c, fmt, o.src_flags) for c in o.palette]
    visible = {}
    for layer in (MASKS, BOXES, KEYPOINTS, LABELS):  # upwards: each layer overwrites the ones below it
        m = own[layer] != NONE
        visible[layer] = m.copy()
        for lo in (MASKS, BOXES, KEYPOINTS):
            if lo < layer:
                visible[lo] &= ~m
        for v in np.unique(own[layer][m]):
            sel = own[layer] == v
            if layer == KEYPOINTS:
                col[sel] = pcol[(int(v) & 31) % P]
            elif layer == LABELS:
                col[sel & on] = tcol[v]
                col[sel & ~on] = ecol[v]
            else:
                col[sel] = ecol[v]
        if layer != MASKS:
            opaque |= m
    tint = (own[MASKS] != NONE) & ~opaque
    covered = opaque | tint

    def paint(plane, colours, opq, tnt):
        src = plane.astype(np.int64)
        out = np.where(opq[..., None], colours, np.where(tnt[..., None], (src * (256 - o.a) + colours * o.a + 128) >> 8, src))
        return out.astype(np.uint8)

    if fmt == RGB:
        out = paint(buf.reshape(H, W, 3), col, opaque, tint).reshape(-1)
    else:
        y = paint(buf[:W * H].reshape(H, W, 1), col[..., :1], opaque, tint)
        c = paint(buf[W * H:].reshape(H // 2, W // 2, 2), col[::2, ::2, 1:], opaque[::2, ::2], tint[::2, ::2])  # sample (i, j) follows pixel (2i, 2j)
        out = np.concatenate([y.reshape(-1), c.reshape(-1)])
    info = dict(visible=visible, cnt=cnt, opaque_over_tint=bool((opaque & (own[MASKS] != NONE)).any()), touched=touched, covered=covered)
    return out, covered, info


def overlay_frames_np(frames, boxes, frame_of_box, W, H, fmt=RGB, keys=None, texts=None, mask_words=None, mask_of_box=None, kpts=None,
                      tracks=None, **opts):
    """the host-pointer form (tracks = None) and, with per-box tracks, what the device form paints for pre-selected lists:
    -> (uint8 [F][frame bytes], STATS [F], [info of every frame])"""
    o = Opts(**opts)
    fb = frame_bytes(W, H, fmt)
    frames = np.asarray(frames, dtype=np.uint8).reshape(-1, fb)
    fo = np.asarray(frame_of_box, dtype=np.int64).reshape(-1)
    out = np.empty_like(frames)
    stats = np.zeros(len(frames), dtype=STATS)
    infos = []
    for f in range(len(frames)):
        idx = np.flatnonzero(fo == f)
        masks = None
        if mask_of_box is not None:
            masks = [unpack_words(mask_words[mask_of_box[i]], W) if mask_of_box[i] >= 0 else None for i in idx]
        elems, marks, skipped = elements_np(boxes[idx], W, H, o, None if keys is None else [keys[i] for i in idx],
                                            None if texts is None else [texts[i] for i in idx], masks, None if kpts is None else [kpts[i] for i in idx],
                                            None if tracks is None else [tracks[i] for i in idx])
        out[f], covered, info = overlay_frame_np(frames[f], W, H, fmt, elems, marks, o)
        stats[f] = (len(elems), sum(e["mask"] is not None for e in elems), sum(bool(e["text"]) for e in elems), len(marks), skipped,
                    int(covered.sum()))
        info["elems"], info["marks"] = elems, marks
        infos.append(info)
    return out, stats, infos


def not_vacuous(infos, layers, W, H):
    """the four conditions a case must meet (tests/test_overlay_cpu.py checks every generator of tests/test_gpu_overlay.py): every enabled
    layer owns a pixel; two elements of one layer overlap; an opaque layer lies over a tint (where MASKS is on with another layer);
    some 64 x 64 tile of some frame is touched by no element -> a list of what is missing"""
    layers = layers or (BOXES | LABELS)
    missing = []
    for k, name in ((MASKS, "masks"), (BOXES, "boxes"), (KEYPOINTS, "keypoints"), (LABELS, "labels")):
        if layers & k and not any((i["cnt"][k] > 0).any() for i in infos):
            missing.append("no pixel of " + name)
    if not any((i["cnt"][k] >= 2).any() for i in infos for k in i["cnt"]):
        missing.append("no two elements of a layer overlap")
    if layers & MASKS and layers & ~MASKS and not any(i["opaque_over_tint"] for i in infos):
        missing.append("no opaque pixel over a tint")
    if not any(not i["touched"][y:y + 64, x:x + 64].any() for i in infos for y in range(0, H, 64) for x in range(0, W, 64)):
        missing.append("no tile without an element")
    return missing
